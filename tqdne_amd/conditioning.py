"""Time-domain conditioning of waveform batches on the GPU (libtqdne_series.so, include/tqdne_series.h): what the reference applies
to every stream before its intensity measures -- the causal Butterworth high-pass of scripts/seismo_evaluations/utils.py
(``highpass_filter``), the detrend + causal band-pass chain of scripts/preprocessing/04_filter_waveforms.py (obspy's ``detrend`` and
``filter("bandpass", zerophase=False)``) and the hold-and-recompute envelope ``moving_average_envelope_adaptive``.

Every function is ONE launch in which one lane walks one series (tqs_sosfilt, tqs_hold_envelope; csrc_series/series.hip).  The
filter is a cascade of second-order sections whose state, coefficients and intermediate signals are fp64; samples are widened once and
results rounded to fp32 once.  Results are bit-reproducible and a series' result does not depend on the rest of the batch.  A series
with a non-finite sample comes out all NaN.

Dispatch: a GPU tensor takes the kernels and comes back as a float32 GPU tensor; a view whose series are contiguous and evenly
strided (``w[:, c]`` or ``w[..., :T]`` of a (B, C, T') tensor) goes in without a copy.  Calls enqueue on the current stream and do not
synchronise.  A numpy array or a CPU tensor takes a host path with the reference's arithmetic -- scipy's ``lfilter(b, a)`` for
``highpass_filter``, ``sosfilt`` for ``bandpass``, numpy's float32 decisions and slice means for the envelope -- and returns the
reference's values and dtypes.  The filter tables are designed on the host in float64 by scipy and cached per (order, Wn, btype,
device)."""

from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _lib_series
from ._lib_series import TQS_DETREND_DEMEAN, TQS_DETREND_LINEAR, TQS_DETREND_NONE, check

__all__ = ["sosfilt", "butter_sos", "highpass_filter", "bandpass", "detrend", "condition_stream", "moving_average_envelope_adaptive",
           "max_sections", "JUMP"]

JUMP = 5            # the reference's envelope recomputes where |x[i]| > 5 |x[i-1]|
_DETREND = {None: TQS_DETREND_NONE, "demean": TQS_DETREND_DEMEAN, "constant": TQS_DETREND_DEMEAN, "linear": TQS_DETREND_LINEAR}
_IDENTITY = np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]])
_SOS = {}           # (order, Wn, btype) -> host table (n_sections, 6)
_DEVICE_SOS = {}    # (order, Wn, btype, device) -> device table


def max_sections() -> int:
    return _lib_series.TQS_SOSFILT_MAX_SECTIONS


def _is_gpu(x) -> bool:
    return isinstance(x, torch.Tensor) and x.is_cuda


def _host_array(x) -> np.ndarray:
    return x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _like(x, y: np.ndarray):
    """a host result in the container of the host input"""
    return torch.from_numpy(np.ascontiguousarray(y)) if isinstance(x, torch.Tensor) else y


def _detrend_mode(name):
    if not (name is None or isinstance(name, str)) or name not in _DETREND:
        raise ValueError(f"detrend = {name!r} must be None, 'demean', 'constant' or 'linear'")
    return _DETREND[name]


def _check_sos(sos) -> np.ndarray:
    sos = np.array(sos, dtype=np.float64, ndmin=2)
    if sos.ndim != 2 or sos.shape[1] != 6 or sos.shape[0] < 1 or not np.isfinite(sos).all():
        raise ValueError(f"sos: expected a finite (n_sections, 6) table, got shape {sos.shape}")
    if sos.shape[0] > max_sections():
        raise ValueError(f"sos: {sos.shape[0]} sections; the filter kernel carries at most {max_sections()} sections")
    if (sos[:, 3] == 0).any():
        raise ValueError("sos: a section has a0 == 0")
    return np.ascontiguousarray(sos / sos[:, 3:4])   # a0 == 1 (a division by 1.0 where it already is)


def _check_series(x, name="x"):
    shape = tuple(x.shape) if hasattr(x, "shape") else tuple(np.shape(x))
    if len(shape) < 1 or shape[-1] < 1:
        raise ValueError(f"{name}: expected (..., T) series with T >= 1, got shape {shape}")
    return shape


def _rows(xg):
    """float32 GPU tensor (..., T) -> (tensor that owns the memory, R, T, ld): R rows, row r at data_ptr + r * ld.  No copy when the
    samples are contiguous and the leading axes collapse to one even row stride."""
    T = xg.shape[-1]
    lead = [(n, s) for n, s in zip(xg.shape[:-1], xg.stride()[:-1]) if n != 1]
    R = 1
    for n in xg.shape[:-1]:
        R *= n
    even = (xg.stride(-1) == 1 or T == 1) and all(a[1] == b[0] * b[1] for a, b in zip(lead, lead[1:]))
    if even and (not lead or lead[-1][1] >= T):
        return xg, R, T, (lead[-1][1] if lead else T)
    return xg.contiguous(), R, T, T


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _sosfilt_gpu(x, sos_dev, n_sections, mode):
    xg = x if x.dtype == torch.float32 else x.float()
    y = torch.empty(tuple(xg.shape), device=xg.device, dtype=torch.float32)
    xg, R, T, ld = _rows(xg)
    if R:
        check(_lib_series.load().tqs_sosfilt(xg.data_ptr(), y.data_ptr(), sos_dev.data_ptr(), R, T, ld, T, n_sections, mode,
                                             _stream(xg)), "sosfilt")
    return y


def _sosfilt_host(x, sos, mode):
    """float64 scipy on a numpy array / CPU tensor: scipy.signal.detrend (constant, then linear: the reference's order), then sosfilt"""
    import scipy.signal
    a = _host_array(x)
    if mode != TQS_DETREND_NONE:
        a = scipy.signal.detrend(a.astype(np.float64), axis=-1, type="constant")   # (scipy would detrend float32 in float32)
    if mode == TQS_DETREND_LINEAR:
        a = scipy.signal.detrend(a, axis=-1, type="linear")
    return _like(x, scipy.signal.sosfilt(sos, a, axis=-1) if sos is not None else a)


def sosfilt(sos, x, detrend=None):
    """scipy.signal.sosfilt(sos, x, axis=-1) from a zero state, after ``detrend`` (None, "demean" = "constant", or "linear") of every
    series.  ``sos``: array-like float64 (n_sections, 6), at most ``max_sections()`` = 8 sections."""
    sos = _check_sos(sos)
    mode = _detrend_mode(detrend)
    _check_series(x)
    if not _is_gpu(x):
        return _sosfilt_host(x, sos, mode)
    return _sosfilt_gpu(x, torch.from_numpy(sos).to(x.device), len(sos), mode)


def _design_key(order, Wn, btype):
    return int(order), tuple(float(w) for w in np.atleast_1d(Wn)), str(btype)


def butter_sos(order, Wn, btype):
    """The Butterworth design as second-order sections, on the host in float64: scipy.signal.butter(order, Wn, btype, output="sos"),
    which is iirfilter's zeros and poles through zpk2sos (obspy's construction).  Returns a (n_sections, 6) array (a copy)."""
    import scipy.signal
    key = _design_key(order, Wn, btype)
    if key not in _SOS:
        wn = key[1][0] if len(key[1]) == 1 else list(key[1])
        _SOS[key] = scipy.signal.butter(key[0], wn, btype=key[2], output="sos")
    return _SOS[key].copy()


def _butter_device(order, Wn, btype, device):
    sos = _check_sos(butter_sos(order, Wn, btype))
    key = _design_key(order, Wn, btype) + (str(device),)
    if key not in _DEVICE_SOS:
        _DEVICE_SOS[key] = torch.from_numpy(sos).to(device)
    return _DEVICE_SOS[key], len(sos)


def highpass_filter(data, cutoff_freq=0.1, sampling_rate=100):
    """The reference's ``highpass_filter``: the causal 4th-order Butterworth high-pass of waveforms (n, C, T), same shape out.
    GPU tensors: two fp64 sections in one launch.  numpy arrays / CPU tensors: the reference's transfer-function form, scipy's
    ``lfilter(b, a)`` in float64 along the last axis, returned in the input's dtype."""
    wn = cutoff_freq / (0.5 * sampling_rate)
    _check_series(data, "data")
    if _is_gpu(data):
        sos_dev, n = _butter_device(4, wn, "high", data.device)
        return _sosfilt_gpu(data, sos_dev, n, TQS_DETREND_NONE)
    import scipy.signal
    x = _host_array(data)
    if x.ndim != 3:
        raise ValueError(f"data: expected (n, C, T) waveforms, got shape {x.shape}")
    b, a = scipy.signal.butter(4, wn, btype="high")
    return _like(data, scipy.signal.lfilter(b, a, x, axis=-1).astype(x.dtype))


def _bandpass_design(freqmin, freqmax, df, corners, zerophase):
    """obspy.signal.filter.bandpass's rules -> (order, Wn, btype) of the Butterworth design"""
    if zerophase:
        raise NotImplementedError("zerophase=True is not supported: the backward pass needs the forward pass's result in fp64; "
                                  "only the causal form (zerophase=False) is implemented")
    nyquist = 0.5 * df
    lo, hi = freqmin / nyquist, freqmax / nyquist
    if lo > 1:
        raise ValueError(f"freqmin = {freqmin} is above Nyquist ({nyquist})")
    if hi - 1.0 > -1e-6:
        warnings.warn(f"freqmax = {freqmax} of the band-pass is at or above Nyquist ({nyquist}): applying a high-pass at {freqmin} instead")
        return int(corners), lo, "highpass"
    return int(corners), (lo, hi), "band"


def _filter_after_detrend(data, design, mode):
    _check_series(data, "data")
    if _is_gpu(data):
        sos_dev, n = _butter_device(*design, data.device)
        return _sosfilt_gpu(data, sos_dev, n, mode)
    return _sosfilt_host(data, _check_sos(butter_sos(*design)), mode)


def bandpass(data, freqmin, freqmax, df, corners=4, zerophase=False):
    """obspy's causal Butterworth band-pass along the last axis: ``corners`` corners = ``corners`` second-order sections, designed as
    iirfilter(corners, [freqmin, freqmax] / Nyquist, "band", "butter", "zpk") through zpk2sos and applied by sosfilt.  As in obspy, a
    ``freqmax`` at or above Nyquist falls back to the high-pass at ``freqmin`` with a warning.  ``zerophase=True`` is refused."""
    return _filter_after_detrend(data, _bandpass_design(freqmin, freqmax, df, corners, zerophase), TQS_DETREND_NONE)


def detrend(data, type="linear"):
    """Remove the mean ("demean" or "constant") or the least-squares line ("linear") of every series along the last axis.  GPU
    tensors: the filter launch with a one-section identity table.  numpy arrays / CPU tensors: scipy.signal.detrend in float64."""
    if type is None:
        raise ValueError("type = None must be 'demean', 'constant' or 'linear'")
    mode = _detrend_mode(type)
    _check_series(data, "data")
    if not _is_gpu(data):
        return _sosfilt_host(data, None, mode)
    key = ("identity", str(data.device))
    if key not in _DEVICE_SOS:
        _DEVICE_SOS[key] = torch.from_numpy(_IDENTITY).to(data.device)
    return _sosfilt_gpu(data, _DEVICE_SOS[key], 1, mode)


def condition_stream(data, df=100, freqmin=0.1, freqmax=30):
    """The reference's preprocessing chain, detrend("demean"), detrend("linear"), filter("bandpass", freqmin, freqmax,
    zerophase=False) with obspy's 4 corners, in one launch: the least-squares line contains the mean."""
    return _filter_after_detrend(data, _bandpass_design(freqmin, freqmax, df, 4, False), TQS_DETREND_LINEAR)


def _envelope_host(x: np.ndarray, window: int, eps) -> np.ndarray:
    """The recurrence with numpy's own arithmetic in the input's dtype: the decisions |x[i]| > 5 |x[i-1]| for all samples at once,
    a slice ``.mean()`` at each jump only, and the held values by a forward fill from the last jump."""
    a = np.abs(x)
    T = a.shape[-1]
    rows = a.reshape(-1, T)
    out = np.empty_like(rows)
    jumps = np.zeros(rows.shape, bool)
    jumps[:, 1:] = rows[:, 1:] > JUMP * rows[:, :-1]
    idx = np.arange(T)
    for r, (row, jump) in enumerate(zip(rows, jumps)):
        value = np.empty_like(row)
        value[0] = row[0]
        for i in np.flatnonzero(jump):
            value[i] = row[max(0, i - window + 1): i + 1].mean()
        last = np.maximum.accumulate(np.where(jump, idx, 0))   # the latest jump at or before each sample, 0 before the first
        out[r] = value[last]
    return out.reshape(a.shape) + eps


def moving_average_envelope_adaptive(waveform, window_size: int = 128, log_eps: float = 1e-6):
    """The reference's envelope along the last axis: the mean of the last ``window_size`` amplitudes, recomputed only where the
    amplitude jumps above 5 x the previous one and held otherwise, plus ``log_eps`` (no logarithm is taken, as in the reference).
    GPU tensors: one launch, the jump decisions those of numpy on the float32 amplitudes.  numpy arrays / CPU tensors: numpy."""
    if not (isinstance(window_size, (int, np.integer)) and not isinstance(window_size, bool) and 1 <= window_size < 2 ** 31):
        raise ValueError(f"window_size = {window_size!r} must be an integer >= 1")
    if not np.isfinite(np.float32(log_eps)):
        raise ValueError(f"log_eps = {log_eps!r} must be finite")
    _check_series(waveform, "waveform")
    if not _is_gpu(waveform):
        return _like(waveform, _envelope_host(_host_array(waveform), int(window_size), log_eps))
    xg = waveform if waveform.dtype == torch.float32 else waveform.float()
    env = torch.empty(tuple(xg.shape), device=xg.device, dtype=torch.float32)
    xg, R, T, ld = _rows(xg)
    if R:
        check(_lib_series.load().tqs_hold_envelope(xg.data_ptr(), env.data_ptr(), R, T, ld, T, int(window_size), float(JUMP),
                                                   float(log_eps), _stream(xg)), "hold_envelope")
    return env
