"""Ground-motion intensity measures of generated waveforms on the GPU (the reference's scripts/seismo_evaluations:
``gmrotdpp_withPG`` and ``parallel_processing_sa`` of example_GMM.py; ``evaluate_ratio`` of utils.py with its ``calculate_gmrotd50``
and ``process_kanno`` reductions, on the frequency-domain integration / high-pass of ``spectra.py``).

The reference judges a waveform set against ground-motion models by PGA, PGV, PGD and the 5 %-damped spectral acceleration SA(T),
each combined over the two horizontal components as GMRotDpp.  It computes them with smtk on ten host processes, one waveform at a
time: a Nigam-Jennings time stepping per period, then 90 rotations of the whole response series.  Here the directional peaks of a
whole batch -- ground acceleration, velocity, displacement and every oscillator response, at 180 whole degrees -- are ONE HIP launch
(tq_rotd_peaks, csrc/intensity.hip) on waveforms that already live on the GPU; the percentile over the angles is a sort and a
lerp in torch on the device.  smtk's semantics are restated (include/tqdne_hip.h), not run.

Inputs may be torch tensors on a GPU (returned as GPU tensors) or numpy arrays / CPU tensors (uploaded, computed on the GPU, returned
as numpy / CPU tensors), with any leading dimensions: the conventions of ``representation.py``.  Results are fp32.  There is no host
fallback: without a GPU the calls raise.  Calls on GPU tensors enqueue on the current stream and do not synchronise; the per-period
tables are computed on the host in double on first use and cached by (periods, dt, damping, device)."""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import check

__all__ = ["rotd_peaks", "gmrotdpp_with_pg", "response_spectrum", "parallel_processing_sa", "calculate_gmrotd50", "process_kanno",
           "evaluate_ratio", "N_ANGLES"]

N_ANGLES = 180
_TABLES = {}   # (periods, dt, damping, device) -> device tensor of tq_oscillator_tables


def _to_gpu(x):
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.contiguous().float(), "cuda"
    if not torch.cuda.is_available():
        raise RuntimeError("tqdne_amd.ground_motion runs on the GPU (no CPU fallback): no GPU is visible")
    kind = "torch" if isinstance(x, torch.Tensor) else "numpy"
    t = torch.as_tensor(np.asarray(x) if kind == "numpy" else x, dtype=torch.float32)
    return t.contiguous().to("cuda"), kind


def _back(y, kind):
    if kind == "cuda":
        return y
    return y.cpu() if kind == "torch" else y.cpu().numpy()


def _shape_of(a, name):
    shape = tuple(a.shape) if hasattr(a, "shape") else tuple(np.shape(a))
    if len(shape) < 1:
        raise ValueError(f"{name}: expected (..., T) samples, got a scalar")
    return shape


def _check(x, y, dt, periods, damping, percentile=None):
    """every argument check, before anything is uploaded; returns the periods as a tuple of floats"""
    sx = _shape_of(x, "x")
    if y is not None and _shape_of(y, "y") != sx:
        raise ValueError(f"x and y: the two components must have equal shapes, got {sx} and {_shape_of(y, 'y')}")
    if sx[-1] < 2:
        raise ValueError(f"x: T = {sx[-1]} samples; the series have T - 1 samples, so T >= 2 is needed")
    if not (isinstance(dt, (int, float, np.floating, np.integer)) and math.isfinite(dt) and dt > 0):
        raise ValueError(f"dt = {dt!r} must be a positive, finite number")
    per = np.atleast_1d(np.asarray(periods.detach().cpu().numpy() if isinstance(periods, torch.Tensor) else periods, dtype=np.float64))
    if per.ndim != 1 or not (np.isfinite(per).all() and (per > 0).all()):
        raise ValueError(f"periods = {periods!r} must be a flat sequence of positive, finite numbers")
    if not (isinstance(damping, (int, float, np.floating, np.integer)) and 0.0 <= damping < 1.0):
        raise ValueError(f"damping = {damping!r} must lie in [0, 1)")
    if percentile is not None and not (isinstance(percentile, (int, float, np.floating, np.integer)) and 0.0 <= percentile <= 100.0):
        raise ValueError(f"percentile = {percentile!r} must lie in [0, 100]")
    return tuple(float(p) for p in per)


def oscillator_tables(periods, dt, damping=0.05):
    """what tq_oscillator_tables writes, as a host array: cos | sin of the 180 angles, then 12 floats per period (the step of the
    scaled state (w^2 u, w u'): A11 A12 A21 A22 B0 B0 B1 B1 2xi 0 0 0)"""
    lib = _lib.load()
    per = np.ascontiguousarray(periods, dtype=np.float64)
    buf = np.empty(lib.tq_oscillator_table_floats(len(per)), np.float32)
    check(lib.tq_oscillator_tables(per.ctypes.data, len(per), float(dt), float(damping), buf.ctypes.data), "oscillator_tables")
    return buf


def _tables(per, dt, damping, device):
    key = (per, float(dt), float(damping), str(device))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(oscillator_tables(per, dt, damping)).to(device)
    return _TABLES[key]


def _peaks(xg, yg, dt, per, damping):
    """GPU tensors (..., T) -> (..., 3 + P, 180)"""
    T = xg.shape[-1]
    N = xg.numel() // T
    out = torch.empty(tuple(xg.shape[:-1]) + (3 + len(per), N_ANGLES), device=xg.device, dtype=torch.float32)
    if N:
        tables = _tables(per, dt, damping, xg.device)
        check(_lib.load().tq_rotd_peaks(xg.data_ptr(), yg.data_ptr(), tables.data_ptr(), out.data_ptr(), N, T, len(per), float(dt),
                                        torch.cuda.current_stream(xg.device).cuda_stream), "rotd_peaks")
    return out


def _percentile(v, percentile):
    """numpy.percentile(v, percentile, axis=-1) with linear interpolation, on the tensor's device and without a host sync"""
    n = v.shape[-1]
    s = torch.sort(v, dim=-1).values
    pos = float(percentile) / 100.0 * (n - 1)
    lo = min(int(math.floor(pos)), n - 1)
    hi = min(lo + 1, n - 1)
    return torch.lerp(s[..., lo], s[..., hi], pos - lo)


def rotd_peaks(x, y, dt, periods, damping=0.05):
    """max_t |sx(t) cos phi + sy(t) sin phi| at phi = 0 .. 179 degrees for the 3 + P series pairs of every waveform: ground
    acceleration, velocity, displacement, then the oscillator responses.  x, y (..., T) -> (..., 3 + P, 180)."""
    per = _check(x, y, dt, periods, damping)
    xg, kind = _to_gpu(x)
    yg, _ = _to_gpu(y)
    if yg.device != xg.device:
        yg = yg.to(xg.device)
    return _back(_peaks(xg, yg, dt, per, damping), kind)


def gmrotdpp_with_pg(x, y, dt, periods, percentile=50, damping=0.05, kind="gmrotd"):
    """The reference's ``gmrotdpp_withPG`` for a batch: {"PGA", "PGV", "PGD"} of shape (...,) and "Acceleration" of shape (..., P).
    kind="gmrotd": the percentile over theta = 0 .. 89 of sqrt(m[theta] m[theta + 90]) (smtk's rotate_horizontal form, as the
    reference); kind="rotd": the percentile of m over all 180 angles (Boore 2010)."""
    if kind not in ("gmrotd", "rotd"):
        raise ValueError(f"kind = {kind!r} must be 'gmrotd' or 'rotd'")
    per = _check(x, y, dt, periods, damping, percentile)
    xg, back = _to_gpu(x)
    yg, _ = _to_gpu(y)
    if yg.device != xg.device:
        yg = yg.to(xg.device)
    m = _peaks(xg, yg, dt, per, damping)
    if kind == "gmrotd":
        m = torch.sqrt(m[..., :N_ANGLES // 2] * m[..., N_ANGLES // 2:])
    g = _percentile(m, percentile)
    return {"PGA": _back(g[..., 0], back), "PGV": _back(g[..., 1], back), "PGD": _back(g[..., 2], back),
            "Acceleration": _back(g[..., 3:], back)}


def response_spectrum(a, dt, periods, damping=0.05):
    """Spectral acceleration of one component: a (..., T) -> (..., P), the peak absolute acceleration of every oscillator (the same
    launch with a zero second component, read at angle 0)."""
    per = _check(a, None, dt, periods, damping)
    ag, kind = _to_gpu(a)
    m = _peaks(ag, torch.zeros_like(ag), dt, per, damping)
    return _back(m[..., 3:, 0], kind)


def parallel_processing_sa(wf_NS, wf_EW, dt, periods, percentile):
    """The reference's call: GMRotDpp spectral accelerations (N, P) of N waveform pairs (no process pool: one launch)."""
    return gmrotdpp_with_pg(wf_NS, wf_EW, dt, periods, percentile)["Acceleration"]


def calculate_gmrotd50(c1, c2):
    """The reference's ``calculate_gmrotd50`` for batches (..., T) of equal length: max over time of the median over 180 rotation
    angles of sqrt(r1^2 + r2^2).  The rotation (r1, r2) = (c1 cos + c2 sin, -c1 sin + c2 cos) is orthogonal, so r1^2 + r2^2 =
    c1^2 + c2^2 at every angle: the median over the angles does not depend on the angle and is sqrt(c1^2 + c2^2) itself."""
    return torch.sqrt(c1 * c1 + c2 * c2).amax(dim=-1)


def process_kanno(EW, NS):
    """The reference's ``process_kanno`` for batches (..., T): sqrt(max|EW|^2 + max|NS|^2), the two peaks at their own times"""
    a, b = EW.abs().amax(dim=-1), NS.abs().amax(dim=-1)
    return torch.sqrt(a * a + b * b)


def evaluate_ratio(target, predicted, dt=0.01, n_worker=4, evaluate_obs=True, PGV=True, kanno=False):
    """The reference's ``evaluate_ratio`` (scripts/seismo_evaluations/utils.py): peak values of observed (``target``) and generated
    (``predicted``) two-component waveforms (n, 2, T), component 0 = NS, 1 = EW.  ``PGV``: the series are integrated in the frequency
    domain and reduced by ``calculate_gmrotd50`` (``kanno``: by ``process_kanno``); otherwise they are high-passed and reduced by
    ``calculate_gmrotd50`` (``kanno`` is not read, as in the reference).  Returns {"PGV_geom_mean_obs", "PGV_geom_mean_gwm"} (or
    "PGA_..."), each (n,), or the generated set's values alone with ``evaluate_obs=False``.  ``n_worker`` is accepted and ignored: the
    whole batch is two launches per set, no chunks and no process pool."""
    from . import spectra
    for name, a in (("target", target), ("predicted", predicted)):
        shape = _shape_of(a, name)
        if len(shape) != 3 or shape[1] < 2:
            raise ValueError(f"{name}: expected (n, 2, T) waveforms, got {shape}")
        spectra._check_length(a, name)
    transform = spectra.integrate_frequency_domain if PGV else spectra.filter_frequency_domain
    reduce_ = process_kanno if (PGV and kanno) else calculate_gmrotd50

    def peaks(w):
        wg, kind = spectra._to_gpu(w)
        s = transform(wg[:, :2], dt)
        return _back(reduce_(s[:, 1], s[:, 0]), kind)

    gwm = peaks(predicted)
    if not evaluate_obs:
        return gwm
    q = "PGV" if PGV else "PGA"
    return {f"{q}_geom_mean_obs": peaks(target), f"{q}_geom_mean_gwm": gwm}
