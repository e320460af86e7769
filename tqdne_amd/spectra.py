"""Fourier transforms of waveforms at their own length on the GPU (libtqdne_eval.so, include/tqdne_eval.h): the real DFT behind
``metric.AmplitudeSpectralDensity`` and the frequency-domain half of the reference's scripts/seismo_evaluations/utils.py
(``integrate_frequency_domain``, ``filter_frequency_domain``, ``fft``), batched over leading axes.

Every transform is ONE launch of one workgroup per row (tqe_rdft, tqe_spectral_filter; csrc_eval/spectra.hip), for any length from 2
to ``max_length()`` = 4096 samples; ``column_moments`` is the float64 mean / population std over the rows that the metric's
isotropic Frechet distance needs.  Results are bit-reproducible and a row's result does not depend on the rest of the batch.

Inputs may be torch tensors on a GPU (returned as GPU tensors) or numpy arrays / CPU tensors (uploaded, computed on the GPU, returned
as numpy / CPU tensors): the conventions of ``ground_motion.py``.  A GPU tensor whose rows are a strided view with contiguous samples
(``pred[:, c]`` of a (B, C, T) tensor) goes in without a copy.  There is no host fallback: without a GPU the calls raise.  Calls on
GPU tensors enqueue on the current stream and do not synchronise; tables are computed on the host in double on first use and cached
by (length, device)."""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib_eval
from ._lib_eval import TQE_RDFT_ABS, TQE_RDFT_COMPLEX, TQE_RDFT_LOG, check

__all__ = ["rdft", "amplitude_spectrum", "log_amplitude_spectrum", "spectral_filter", "column_moments", "integrate_frequency_domain",
           "filter_frequency_domain", "fft", "max_length", "HIGHPASS_HZ"]

HIGHPASS_HZ = 0.1   # the reference's mask: |f| >= 0.1 Hz
_TABLES = {}        # (N, device) -> device tensor of tqe_rdft_tables
_MULTIPLIERS = {}   # (kind, N, dt, device) -> device tensor (N/2+1, 2)


def max_length() -> int:
    return _lib_eval.load().tqe_rdft_max_length()


def rdft_tables(N: int) -> np.ndarray:
    """what tqe_rdft_tables writes for length N, as a host array (layout: include/tqdne_eval.h)"""
    lib = _lib_eval.load()
    buf = np.empty(lib.tqe_rdft_table_floats(int(N)), np.float32)
    check(lib.tqe_rdft_tables(int(N), buf.ctypes.data), "rdft_tables")
    return buf


def _check_length(x, name="x"):
    shape = tuple(x.shape) if hasattr(x, "shape") else tuple(np.shape(x))
    if len(shape) < 1:
        raise ValueError(f"{name}: expected (..., N) samples, got a scalar")
    N, limit = shape[-1], max_length()
    if N < 2:
        raise ValueError(f"{name}: N = {N} samples; the transform needs N >= 2")
    if N > limit:
        raise ValueError(f"{name}: N = {N} samples is above the limit of {limit} samples of the one-workgroup transform")
    return shape


def _to_gpu(x):
    """-> (float32 GPU tensor with contiguous samples, kind).  GPU tensors are not copied unless their samples are strided."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        x = x if x.dtype == torch.float32 else x.float()
        return (x if x.stride(-1) == 1 or x.shape[-1] == 1 else x.contiguous()), "cuda"
    if not torch.cuda.is_available():
        raise RuntimeError("tqdne_amd.spectra runs on the GPU (no CPU fallback): no GPU is visible")
    kind = "torch" if isinstance(x, torch.Tensor) else "numpy"
    t = torch.from_numpy(np.array(x, dtype=np.float32)) if kind == "numpy" else x.to(torch.float32)
    return t.contiguous().to("cuda"), kind


def _back(y, kind):
    if kind == "cuda":
        return y
    return y.cpu() if kind == "torch" else y.cpu().numpy()


def _rows(xg):
    """GPU tensor (..., N) with contiguous samples -> (tensor that owns the memory, R, N, ld): R rows, row r at data_ptr + r * ld"""
    N = xg.shape[-1]
    if xg.dim() == 1:
        return xg, 1, N, N
    if xg.dim() == 2 and (xg.shape[0] == 1 or xg.stride(0) >= N):
        return xg, xg.shape[0], N, (N if xg.shape[0] == 1 else xg.stride(0))
    xg = xg.contiguous()
    return xg, xg.numel() // N, N, N


def _tables(N, device):
    key = (int(N), str(device))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(rdft_tables(N)).to(device)
    return _TABLES[key]


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _rdft(xg, mode, log_eps=1.0):
    """GPU tensor (..., N) -> (..., N/2+1[, 2]) float32 on its device"""
    lead = tuple(xg.shape[:-1])
    xg, R, N, ld = _rows(xg)
    K = N // 2 + 1
    out = torch.empty(lead + ((K, 2) if mode == TQE_RDFT_COMPLEX else (K,)), device=xg.device, dtype=torch.float32)
    if R:
        check(_lib_eval.load().tqe_rdft(xg.data_ptr(), out.data_ptr(), _tables(N, xg.device).data_ptr(), R, N, ld, mode, float(log_eps),
                                        _stream(xg)), "rdft")
    return out


def rdft(x):
    """numpy.fft.rfft(x, axis=-1) in fp32: (..., N) real -> (..., N/2+1) complex64"""
    _check_length(x)
    xg, kind = _to_gpu(x)
    return _back(torch.view_as_complex(_rdft(xg, TQE_RDFT_COMPLEX)), kind)


def amplitude_spectrum(x):
    """|numpy.fft.rfft(x, axis=-1)|: (..., N) -> (..., N/2+1)"""
    _check_length(x)
    xg, kind = _to_gpu(x)
    return _back(_rdft(xg, TQE_RDFT_ABS), kind)


def log_amplitude_spectrum(x, log_eps=1e-8):
    """log(max(|rfft(x)|, log_eps)), the ``spectral_density`` of ``metric.AmplitudeSpectralDensity``, written by the transform's launch"""
    _check_length(x)
    if not (isinstance(log_eps, (int, float, np.floating)) and log_eps > 0 and np.float32(log_eps) > 0):
        raise ValueError(f"log_eps = {log_eps!r} must be a positive number (in float32)")
    xg, kind = _to_gpu(x)
    return _back(_rdft(xg, TQE_RDFT_LOG, log_eps), kind)


def _filter(xg, hg):
    lead = tuple(xg.shape[:-1])
    xg, R, N, ld = _rows(xg)
    y = torch.empty(lead + (N,), device=xg.device, dtype=torch.float32)
    if R:
        check(_lib_eval.load().tqe_spectral_filter(xg.data_ptr(), hg.data_ptr(), y.data_ptr(), _tables(N, xg.device).data_ptr(), R, N, ld,
                                                   _stream(xg)), "spectral_filter")
    return y


def spectral_filter(x, h):
    """Re IDFT(H . DFT(x)) along the last axis for a Hermitian multiplier given on the N/2 + 1 non-negative bins: ``h`` complex
    (N/2+1,) or real pairs (N/2+1, 2), shared by all rows.  The imaginary part of H X at DC and at the Nyquist bin contributes nothing."""
    shape = _check_length(x)
    K = shape[-1] // 2 + 1
    hh = h.detach().cpu().numpy() if isinstance(h, torch.Tensor) else np.asarray(h)
    if np.iscomplexobj(hh):
        hh = np.stack([hh.real, hh.imag], axis=-1)
    if hh.shape != (K, 2):
        raise ValueError(f"h: expected the {K} non-negative bins of a length-{shape[-1]} transform, complex ({K},) or real ({K}, 2); got {hh.shape}")
    xg, kind = _to_gpu(x)
    hg = torch.from_numpy(np.ascontiguousarray(hh, dtype=np.float32)).to(xg.device)
    return _back(_filter(xg, hg), kind)


def multiplier(kind: str, N: int, dt: float) -> np.ndarray:
    """The reference's frequency-domain multipliers on the bins k = 0 .. N/2 of numpy.fft.fftfreq(N, dt), complex128:
    "filter": the mask |f| >= 0.1 Hz (which also zeroes DC); "integrate": the mask over i 2 pi f, DC zero."""
    if kind not in ("filter", "integrate"):
        raise ValueError(f"kind = {kind!r} must be 'filter' or 'integrate'")
    f = np.fft.rfftfreq(N, float(dt))   # k * (1 / (N dt)): bit for bit the non-negative entries of fftfreq, so the mask's edge agrees
    h = (np.abs(f) >= HIGHPASS_HZ).astype(np.complex128)
    if kind == "integrate":
        h[1:] = h[1:] / (1j * 2 * np.pi * f[1:])
        h[0] = 0
    return h


def _multiplier(kind, N, dt, device):
    key = (kind, int(N), float(dt), str(device))
    if key not in _MULTIPLIERS:
        h = multiplier(kind, N, dt)
        _MULTIPLIERS[key] = torch.from_numpy(np.stack([h.real, h.imag], axis=-1).astype(np.float32)).to(device)
    return _MULTIPLIERS[key]


def _check_dt(dt):
    if not (isinstance(dt, (int, float, np.floating, np.integer)) and math.isfinite(dt) and dt > 0):
        raise ValueError(f"dt = {dt!r} must be a positive, finite number")


def _reference_filter(kind, signal, dt):
    shape = _check_length(signal, "signal")
    _check_dt(dt)
    xg, back = _to_gpu(signal)
    return _back(_filter(xg, _multiplier(kind, shape[-1], dt, xg.device)), back)


def integrate_frequency_domain(signal, dt):
    """The reference's integration (velocity from acceleration): the spectrum above 0.1 Hz divided by i 2 pi f, DC removed, back to
    the time domain.  (..., N) -> (..., N)."""
    return _reference_filter("integrate", signal, dt)


def filter_frequency_domain(signal, dt):
    """The reference's high-pass: bins with |f| < 0.1 Hz zeroed.  (..., N) -> (..., N)."""
    return _reference_filter("filter", signal, dt)


def fft(signal, dt=0.01):
    """The reference's ``fft``: (the first N // 2 frequencies of fftfreq(N, dt), the amplitude spectrum on them)"""
    shape = _check_length(signal, "signal")
    _check_dt(dt)
    N = shape[-1]
    xg, kind = _to_gpu(signal)
    amp = _rdft(xg, TQE_RDFT_ABS)[..., :N // 2]
    freqs = np.fft.fftfreq(N, dt)[:N // 2]
    if kind == "numpy":
        return freqs, amp.cpu().numpy()
    return torch.from_numpy(freqs).to(amp.device if kind == "cuda" else "cpu"), _back(amp, kind)


def _moments(ag):
    """contiguous float32 GPU tensor (R, F) -> float64 GPU tensors mean (F), std (F)"""
    R, F = ag.shape
    mean = torch.empty(F, device=ag.device, dtype=torch.float64)
    std = torch.empty(F, device=ag.device, dtype=torch.float64)
    check(_lib_eval.load().tqe_column_moments(ag.data_ptr(), mean.data_ptr(), std.data_ptr(), R, F, _stream(ag)), "column_moments")
    return mean, std


def column_moments(a):
    """a (R, F) -> (mean, std) over the rows in float64, std with ddof = 0 (numpy's ``a.mean(0), a.std(0)``)"""
    shape = tuple(a.shape) if hasattr(a, "shape") else tuple(np.shape(a))
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"a: expected (R, F) with R, F >= 1, got {shape}")
    ag, kind = _to_gpu(a)
    mean, std = _moments(ag.contiguous())
    return _back(mean, kind), _back(std, kind)
