"""Arias intensity, Husid curve and significant duration of waveform batches (libtqdne_duration.so, include/tqdne_duration.h): the
shaking-duration comparison of the reference's scripts/seismo_evaluations/arias_intensity_duration.ipynb, whose functions keep their
names here and are batched over leading dimensions, and its ``compute_time_derivative`` (numpy's gradient).

What the GPU route is: the float64 evaluation of the formula on the float32 inputs.  One launch (tqd_arias, one wave per row) forms
s = x^2 (+ y^2) from the widened samples, the cumulative trapezoid sum ``cum`` of s in float64, its total, the largest s and the first
index at which ``cum`` reaches each requested fraction of the total; the Husid curve cum / total is written from the same sequence when
asked for.  The reference takes the resultant sqrt(x^2 + y^2) and its peak normalisation in float32 before it squares again; those
intermediates move the total by about 1e-7 of itself (measured on the CPU on decaying-noise pairs, T = 2 ... 4097: 1.18e-7, with all
5 / 75 / 95 % crossings identical).  Results are bit-reproducible and a row's result does not depend on the rest of the batch.  A row of
zero energy or with a non-finite sample has no crossings: its times are NaN.

Dispatch (the rule of ``conditioning``): a GPU tensor takes the kernels and comes back as GPU tensors; evenly strided views such as
``w[:, 0]`` and ``w[:, 1]`` of one (N, 3, T) tensor go in without a copy; calls enqueue on the current stream and do not synchronise.  A
numpy array or a CPU tensor takes numpy / scipy with the reference's own arithmetic: float32 resultant, float32 normalisation,
``cumulative_trapezoid`` on the given time array.

The time axis: ``dt`` means t0 = 0 and step = dt.  ``time`` is a 1-D array of length T; the notebook's ``np.linspace(0, 0.01 * T, T)``
has the step 0.01 T / (T - 1), not 0.01.  The GPU route takes t0 = time[0] and step = (time[-1] - time[0]) / (T - 1) and refuses a time
array whose differences leave that step by more than 1e-9 of it; the host path keeps scipy's general rule."""

from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib_duration
from ._lib_duration import check
from .conditioning import _host_array, _is_gpu, _rows, _stream

__all__ = ["compute_time_derivative", "calculate_resultant_horizontal", "calculate_arias_intensity", "calculate_signal_duration",
           "significant_duration", "husid", "shaking_duration", "max_fractions"]

UNIFORM_RTOL = 1e-9   # a time array on the GPU route: every difference within this of the mean step


def max_fractions() -> int:
    return _lib_duration.TQD_MAX_FRACTIONS


# ---- argument checks --------------------------------------------------------------------------------------------------

def _check_rows(x, name="x"):
    shape = tuple(x.shape) if hasattr(x, "shape") else tuple(np.shape(x))
    if len(shape) < 1 or shape[-1] < 2:
        raise ValueError(f"{name}: expected (..., T) series with T >= 2, got shape {shape}")
    return shape


def _check_pair(x, y):
    shape = _check_rows(x)
    if y is None:
        return shape
    if _check_rows(y, "y") != shape:
        raise ValueError(f"x and y: shapes {shape} and {tuple(y.shape)} differ")
    if _is_gpu(x) != _is_gpu(y) or (_is_gpu(x) and x.device != y.device):
        raise ValueError("x and y: one is on the GPU and the other is not, or they are on different devices")
    return shape


def _positive(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not (value > 0 and math.isfinite(value)):
        raise ValueError(f"{name} = {value!r} must be positive and finite")
    return float(value)


def _fraction(percent, name):
    if isinstance(percent, bool) or not isinstance(percent, (int, float, np.integer, np.floating)) or not 0 <= percent <= 100:
        raise ValueError(f"{name} = {percent!r} must be a number in [0, 100]")
    return percent / 100


def _like(x, y):
    """a host result in the container of the host input (a 0-d result stays 0-d)"""
    return torch.from_numpy(np.array(y)) if isinstance(x, torch.Tensor) else y


def _time_array(time, T):
    t = np.asarray(time.detach().cpu() if isinstance(time, torch.Tensor) else time, dtype=np.float64)
    if t.ndim != 1 or t.shape[0] != T:
        raise ValueError(f"time: expected a 1-D array of the series' length {T}, got shape {t.shape}")
    return t


def _axis(time, dt, T, uniform):
    """-> (time array or None, t0, step).  ``uniform``: the GPU route's rule for a time array."""
    if (time is None) == (dt is None):
        raise ValueError("exactly one of time and dt is required")
    if dt is not None:
        return None, 0.0, _positive(dt, "dt")
    t = _time_array(time, T)
    t0, step = float(t[0]), float((t[-1] - t[0]) / (T - 1))
    if uniform:
        if not (step > 0 and math.isfinite(step)) or not (np.abs(np.diff(t) - step) <= UNIFORM_RTOL * step).all():
            raise ValueError("time: the GPU route takes a uniform, increasing time axis (differences within 1e-9 of their mean step)")
    return t, t0, step


# ---- the launch -------------------------------------------------------------------------------------------------------

def _arias_gpu(x, y, step, fractions, want_husid):
    """one tqd_arias call -> (energy, peak2 float64 (...), index int32 (..., F), husid float32 (..., T) or None)"""
    if not 1 <= len(fractions) <= max_fractions():
        raise ValueError(f"{len(fractions)} fractions; the kernel takes 1 to {max_fractions()}")
    lead, T = tuple(x.shape[:-1]), x.shape[-1]
    dev = x.device
    xg, R, _, ldx = _rows(x if x.dtype == torch.float32 else x.float())
    yg, ldy = None, 0
    if y is not None:
        yg, _, _, ldy = _rows(y if y.dtype == torch.float32 else y.float())
    F = len(fractions)
    energy, peak2 = torch.empty((2,) + lead, device=dev, dtype=torch.float64).unbind(0)   # (one allocation)
    index = torch.empty(lead + (F,), device=dev, dtype=torch.int32)
    curve = torch.empty(lead + (T,), device=dev, dtype=torch.float32) if want_husid else None
    if R:
        fr = (ctypes.c_double * F)(*[float(f) for f in fractions])   # read during the call, passed to the kernel by value
        check(_lib_duration.load().tqd_arias(xg.data_ptr(), yg.data_ptr() if yg is not None else None, energy.data_ptr(),
                                             peak2.data_ptr(), index.data_ptr(), curve.data_ptr() if want_husid else None, R, T, ldx,
                                             ldy, float(step), fr, F, _stream(xg)), "arias")
    return energy, peak2, index, curve


def _times_of(index, t0, step):
    """t0 + index * step in float64, NaN where the index is -1"""
    t = index.to(torch.float64).mul_(step)
    if t0 != 0.0:
        t.add_(t0)
    return t.masked_fill_(index < 0, float("nan"))


# ---- host paths: the reference's arithmetic ---------------------------------------------------------------------------------

def _arias_host(acc: np.ndarray, time, gravity):
    from scipy.integrate import cumulative_trapezoid
    acc_squared = acc ** 2
    integral = cumulative_trapezoid(acc_squared, time, initial=0)
    cumulative = (np.pi / (2 * gravity)) * integral
    return cumulative[..., -1], cumulative


def _first_reached(cumulative: np.ndarray, threshold):
    """first index along the last axis with cumulative >= threshold, -1 where there is none"""
    mask = cumulative >= np.asarray(threshold)[..., None]
    return np.where(mask.any(-1), mask.argmax(-1), -1)


def _acceleration_host(x, y, normalize):
    a = _host_array(x)
    if y is not None:
        a = calculate_resultant_horizontal(a, _host_array(y))
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore"):
            a = a / np.abs(a).max(-1, keepdims=True)
    return a


# ---- the notebook's functions -----------------------------------------------------------------------------------------------

def compute_time_derivative(waveform, sampling_rate=100):
    """The reference's ``compute_time_derivative``: ``np.gradient(waveform, 1 / sampling_rate, axis=-1)``, same shape out.  GPU
    tensors: one launch in numpy's float32 arithmetic (a true division, one rounding per operation).  numpy arrays / CPU tensors:
    numpy."""
    dt = 1.0 / _positive(sampling_rate, "sampling_rate")
    _check_rows(waveform, "waveform")
    if not _is_gpu(waveform):
        return _like(waveform, np.gradient(_host_array(waveform), dt, axis=-1))
    xg = waveform if waveform.dtype == torch.float32 else waveform.float()
    g = torch.empty(tuple(xg.shape), device=xg.device, dtype=torch.float32)
    xg, R, T, ld = _rows(xg)
    if R:
        check(_lib_duration.load().tqd_gradient(xg.data_ptr(), g.data_ptr(), R, T, ld, T, dt, _stream(xg)), "gradient")
    return g


def calculate_resultant_horizontal(acc_x, acc_y):
    """sqrt(acc_x^2 + acc_y^2) in the inputs' own arithmetic"""
    if isinstance(acc_x, torch.Tensor):
        return torch.sqrt(acc_x ** 2 + acc_y ** 2)
    return np.sqrt(acc_x ** 2 + acc_y ** 2)


def calculate_arias_intensity(time, acceleration, gravity=9.81):
    """The reference's ``calculate_arias_intensity`` along the last axis -> (Ia (...), cumulative Ia (..., T)).  GPU tensors: one
    launch; the curve comes back as float64, the kernel's float32 Husid curve times Ia."""
    gravity = _positive(gravity, "gravity")
    shape = _check_rows(acceleration, "acceleration")
    if not _is_gpu(acceleration):
        t = _time_array(time, shape[-1])
        Ia, cumulative = _arias_host(_host_array(acceleration), t, gravity)
        return _like(acceleration, Ia), _like(acceleration, cumulative)
    _, _, step = _axis(time, None, shape[-1], True)
    energy, _, _, curve = _arias_gpu(acceleration, None, step, [1.0], True)
    Ia = (math.pi / (2 * gravity)) * energy
    return Ia, curve.to(torch.float64) * Ia[..., None]


def calculate_signal_duration(time, cumulative_arias, arias_intensity, lower_percent=5, upper_percent=95):
    """The reference's ``calculate_signal_duration`` along the last axis -> (t_start, t_end, duration): the times at which the curve
    first reaches the two percentages of ``arias_intensity``.  Where the reference raises because a threshold is never reached (a NaN
    row), the times are NaN.  Plain array arithmetic on either route; the one-launch route is ``significant_duration``."""
    lo, hi = _fraction(lower_percent, "lower_percent"), _fraction(upper_percent, "upper_percent")
    shape = _check_rows(cumulative_arias, "cumulative_arias")
    t = _time_array(time, shape[-1])
    if _is_gpu(cumulative_arias):
        tg = torch.from_numpy(t).to(cumulative_arias.device)
        total = torch.as_tensor(arias_intensity, device=cumulative_arias.device)
        out = []
        for f in (lo, hi):
            mask = cumulative_arias >= (f * total)[..., None]
            found = tg[mask.to(torch.int8).argmax(-1)]
            out.append(torch.where(mask.any(-1), found, torch.full_like(found, float("nan"))))
        return out[0], out[1], out[1] - out[0]
    cumulative, total = _host_array(cumulative_arias), np.asarray(_host_array(arias_intensity))
    out = []
    for f in (lo, hi):
        idx = _first_reached(cumulative, f * total)
        out.append(np.where(idx >= 0, t[idx], np.nan)[()])
    res = (out[0], out[1], out[1] - out[0])
    return tuple(_like(cumulative_arias, r) for r in res)


# ---- the fused route ----------------------------------------------------------------------------------------------------

def significant_duration(x, y=None, *, time=None, dt=None, lower_percent=5, upper_percent=95, normalize=False, gravity=9.81):
    """Arias intensity and significant duration of every series (two components: of their resultant) -> (Ia, t_start, t_end, duration),
    each of the leading shape, float64.  ``normalize``: of the series divided by its peak, as the notebook's loop does.  GPU tensors:
    ONE tqd_arias launch, no Husid curve written; Ia = pi / (2 g) * energy (/ peak^2), the times t0 + index * step, NaN where a row
    has no crossing.  numpy arrays / CPU tensors: the reference's functions, one after the other."""
    lo, hi = _fraction(lower_percent, "lower_percent"), _fraction(upper_percent, "upper_percent")
    gravity = _positive(gravity, "gravity")
    shape = _check_pair(x, y)
    t, t0, step = _axis(time, dt, shape[-1], _is_gpu(x))
    if _is_gpu(x):
        energy, peak2, index, _ = _arias_gpu(x, y, step, [lo, hi], False)
        Ia = (math.pi / (2 * gravity)) * energy
        if normalize:
            Ia = Ia / peak2
        t_start, t_end = _times_of(index, t0, step).unbind(-1)
        return Ia, t_start, t_end, t_end - t_start
    acc = _acceleration_host(x, y, normalize)
    axis = t if t is not None else step * np.arange(shape[-1])   # (dt: the time axis in float64, as the notebook's is)
    Ia, cumulative = _arias_host(acc, axis, gravity)
    res = (Ia,) + tuple(calculate_signal_duration(axis, cumulative, Ia, lower_percent, upper_percent))
    return tuple(_like(x, r) for r in res)


def husid(x, y=None, *, time=None, dt=None):
    """The normalised cumulative curve cum / cum[-1] of every series (two components: of their resultant), same shape as ``x``.  GPU
    tensors: one launch, float32.  numpy arrays / CPU tensors: the reference's cumulative trapezoid sum over its last value."""
    shape = _check_pair(x, y)
    t, _, step = _axis(time, dt, shape[-1], _is_gpu(x))
    if _is_gpu(x):
        return _arias_gpu(x, y, step, [1.0], True)[3]
    total, cumulative = _arias_host(_acceleration_host(x, y, False), t if t is not None else step * np.arange(shape[-1]), 9.81)
    with np.errstate(invalid="ignore", divide="ignore"):
        return _like(x, cumulative / np.asarray(total)[..., None])


def shaking_duration(target, predicted, dt=0.01, lower_percent=5, upper_percent=95):
    """The notebook's loop over both sets of (n, C >= 2, T) waveforms: the duration between ``lower_percent`` and ``upper_percent`` of
    the Arias intensity of the peak-normalised resultant of channels 1 and 0, on the notebook's time axis
    ``np.linspace(0, dt * T, T)`` -> (durations of target, durations of predicted).  One launch per set on the GPU."""
    dt = _positive(dt, "dt")
    out = []
    for name, w in (("target", target), ("predicted", predicted)):
        shape = _check_rows(w, name)
        if len(shape) != 3 or shape[1] < 2:
            raise ValueError(f"{name}: expected (n, C, T) waveforms with at least two channels, got shape {shape}")
        time = np.linspace(0, dt * shape[-1], shape[-1])
        out.append(significant_duration(w[:, 1], w[:, 0], time=time, lower_percent=lower_percent, upper_percent=upper_percent,
                                        normalize=True)[3])
    return out[0], out[1]
