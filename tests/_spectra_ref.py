"""float64 restatement of the frequency-domain half of the reference's scripts/seismo_evaluations/utils.py (integrate_frequency_domain,
filter_frequency_domain, fft, evaluate_ratio with calculate_gmrotd50 / process_kanno) and of metric.AmplitudeSpectralDensity, in
this project's words: the reference's script imports openquake and is not run.  Everything is numpy float64 and batched over leading
axes; ``fftmod`` is the transform package (numpy.fft by default; scipy.fft keeps single precision and so gives the fp32 yardstick of
the GPU tests).  tests/test_spectra_host.py pins the restatement against an explicit DFT matrix and the analytic integral of on-bin
sinusoids."""

import numpy as np

HIGHPASS_HZ = 0.1


def make_rows(R, N, seed=0):
    """float32 rows (R, N): decaying noise whose scale runs over four decades, row 1 (if any) with an offset, the last row of three
    or more all zero"""
    rng = np.random.default_rng(seed + 1000 * N + R)
    t = np.arange(N, dtype=np.float64)
    scale = 10.0 ** np.linspace(-2.0, 2.0, R)[:, None]
    x = scale * rng.standard_normal((R, N)) * np.exp(-t / max(N / 3.0, 1.0))
    if R > 1:
        x[1] += 3.0 * scale[1]
    if R > 2:
        x[-1] = 0.0
    return x.astype(np.float32)


def full_multiplier(kind, N, dt, dtype=np.complex128):
    """the factor the reference applies to numpy.fft.fft(signal) on all N bins: the mask |f| >= 0.1 Hz ("filter"); the mask over
    i 2 pi f with the DC bin set to zero ("integrate")"""
    f = np.fft.fftfreq(N, dt)
    h = (np.abs(f) >= HIGHPASS_HZ).astype(np.complex128)
    if kind == "integrate":
        h[1:] = h[1:] / (1j * 2 * np.pi * f[1:])
        h[0] = 0
    else:
        assert kind == "filter"
    return h.astype(dtype)


def apply_multiplier(kind, signal, dt, fftmod=np.fft):
    """real part of the inverse transform of (multiplier x transform) along the last axis, in the precision ``fftmod`` keeps"""
    signal = np.asarray(signal)
    X = fftmod.fft(signal, axis=-1)
    return fftmod.ifft(X * full_multiplier(kind, signal.shape[-1], dt, X.dtype), axis=-1).real


def integrate_frequency_domain(signal, dt, fftmod=np.fft):
    return apply_multiplier("integrate", signal, dt, fftmod)


def filter_frequency_domain(signal, dt, fftmod=np.fft):
    return apply_multiplier("filter", signal, dt, fftmod)


def fft(signal, dt=0.01):
    signal = np.asarray(signal, np.float64)
    N = signal.shape[-1]
    return np.fft.fftfreq(N, dt)[:N // 2], np.abs(np.fft.fft(signal, axis=-1))[..., :N // 2]


def gmrotd50_by_rotation(c1, c2):
    """calculate_gmrotd50 as the reference writes it, for ONE pair: 180 rotations, the median over them per sample, the largest"""
    c1, c2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)
    th = np.deg2rad(np.arange(180))[:, None]
    r1 = c1 * np.cos(th) + c2 * np.sin(th)
    r2 = -c1 * np.sin(th) + c2 * np.cos(th)
    return np.max(np.percentile(np.sqrt(r1 ** 2 + r2 ** 2), 50, axis=0))


def gmrotd50(c1, c2):
    """the same without the rotations (r1^2 + r2^2 = c1^2 + c2^2 at every angle), batched"""
    return np.sqrt(np.asarray(c1, np.float64) ** 2 + np.asarray(c2, np.float64) ** 2).max(axis=-1)


def kanno(EW, NS):
    return np.sqrt(np.abs(EW).max(axis=-1) ** 2 + np.abs(NS).max(axis=-1) ** 2)


def evaluate_ratio(target, predicted, dt=0.01, evaluate_obs=True, PGV=True, kanno_=False, fftmod=np.fft):
    """the reference's keys and shapes; ``kanno_`` is read with PGV only, as there"""
    kind = "integrate" if PGV else "filter"
    red = kanno if (PGV and kanno_) else gmrotd50

    def peaks(w):
        s = apply_multiplier(kind, np.asarray(w)[:, :2], dt, fftmod)
        return red(s[:, 1], s[:, 0])

    gwm = peaks(predicted)
    if not evaluate_obs:
        return gwm
    q = "PGV" if PGV else "PGA"
    return {f"{q}_geom_mean_obs": peaks(target), f"{q}_geom_mean_gwm": gwm}


def log_spectra(x, log_eps=1e-8, fftmod=np.fft):
    return np.log(np.clip(np.abs(fftmod.rfft(x, axis=-1)), log_eps, None))


def asd_isotropic(sp, st):
    """the isotropic Frechet distance of two sets of log spectra (rows), float64"""
    sp, st = np.asarray(sp, np.float64), np.asarray(st, np.float64)
    return np.sum((sp.mean(0) - st.mean(0)) ** 2) + np.sum((sp.std(0) - st.std(0)) ** 2)
