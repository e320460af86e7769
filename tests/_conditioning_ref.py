"""float64 restatement of the reference's time-domain conditioning (scripts/seismo_evaluations/utils.py highpass_filter and
moving_average_envelope_adaptive; the detrend + causal band-pass chain of scripts/preprocessing/04_filter_waveforms.py), in this
project's words: scipy.signal's sosfilt / lfilter / detrend / butter in float64, a plain loop of the section cascade in any numpy
float type (numpy.longdouble measures how far float64 is from the exact filter), and the envelope recurrence with its decisions taken
in float32 and its values in float64.  tests/test_conditioning_host.py pins each of them."""

import numpy as np
import scipy.signal

JUMP = 5
HIGHPASS_WN = 0.1 / 50.0   # the reference's 0.1 Hz corner at 100 Hz, over Nyquist


def make_series(R, T, seed=0, offset=True):
    """float32 rows (R, T): noise of unit scale decaying over the row, plus a row offset of at most 10 x the noise's standard
    deviation (so that a detrended, filtered row peaks near the input's scale)"""
    rng = np.random.default_rng(seed + 1000 * T + R)
    t = np.arange(T, dtype=np.float64)
    x = rng.standard_normal((R, T)) * np.exp(-t / max(T / 3.0, 1.0))
    if offset:
        x += rng.uniform(-10.0, 10.0, (R, 1))
    return x.astype(np.float32)


def butter_sos(order, Wn, btype):
    return scipy.signal.butter(order, Wn, btype=btype, output="sos")


def bandpass_sos(freqmin, freqmax, df, corners=4):
    """obspy's construction of its causal band-pass"""
    fe = 0.5 * df
    z, p, k = scipy.signal.iirfilter(corners, [freqmin / fe, freqmax / fe], btype="band", ftype="butter", output="zpk")
    return scipy.signal.zpk2sos(z, p, k)


def detrend64(x, mode):
    """scipy.signal.detrend in float64; mode None, "demean" / "constant" or "linear" (after "constant": the reference's order)"""
    x = np.asarray(x, np.float64)
    if mode is None:
        return x
    x = scipy.signal.detrend(x, axis=-1, type="constant")
    if mode == "linear":
        x = scipy.signal.detrend(x, axis=-1, type="linear")
    else:
        assert mode in ("demean", "constant")
    return x


def sosfilt64(sos, x, mode=None):
    return scipy.signal.sosfilt(sos, detrend64(x, mode), axis=-1)


def highpass_ba64(x, Wn=HIGHPASS_WN):
    """the reference's own form: the order-4 transfer function run by lfilter in float64"""
    b, a = scipy.signal.butter(4, Wn, btype="high")
    return scipy.signal.lfilter(b, a, np.asarray(x, np.float64), axis=-1)


def cascade(sos, x, dtype=np.longdouble):
    """the section cascade, direct form II transposed from a zero state, sample by sample in ``dtype`` (rows side by side)"""
    sos = np.asarray(sos, np.float64).astype(dtype)
    x = np.atleast_2d(np.asarray(x)).astype(dtype)
    y = np.empty_like(x)
    z = np.zeros((len(sos), 2, x.shape[0]), dtype)
    for t in range(x.shape[1]):
        u = x[:, t]
        for (b0, b1, b2, _, a1, a2), zs in zip(sos, z):
            w = b0 * u + zs[0]
            zs[0] = b1 * u - a1 * w + zs[1]
            zs[1] = b2 * u - a2 * w
            u = w
        y[:, t] = u
    return y


def hold_envelope(x, window, eps, jump=JUMP):
    """out[0] = a[0]; out[i] = mean(a[max(0, i - window + 1) .. i]) if a[i] > jump a[i-1] else out[i-1], on a = |x|.  The decision is
    float32's (product rounded, then compared), the values are float64.  Returns (out + eps in float64, the decisions as booleans)."""
    a32 = np.abs(np.atleast_2d(np.asarray(x, np.float32)))
    a64 = a32.astype(np.float64)
    out = np.empty_like(a64)
    jumps = np.zeros(a32.shape, bool)
    jumps[:, 1:] = a32[:, 1:] > np.float32(jump) * a32[:, :-1]
    for r in range(a32.shape[0]):
        for i in range(a32.shape[1]):
            if i == 0:
                out[r, 0] = a64[r, 0]
            elif jumps[r, i]:
                out[r, i] = a64[r, max(0, i - window + 1):i + 1].mean()
            else:
                out[r, i] = out[r, i - 1]
    return out + float(eps), jumps


def envelope_literal(x, window, eps, jump=JUMP):
    """the recurrence as written, one sample after the other in the input's own dtype (numpy scalars), for one row or a batch"""
    a = np.abs(np.asarray(x))
    out = np.zeros_like(a)
    for idx in np.ndindex(a.shape[:-1]):
        row, o = a[idx], out[idx]
        for i in range(len(row)):
            if i == 0:
                o[i] = row[0]
            elif row[i] > jump * row[i - 1]:
                o[i] = row[max(0, i - window + 1):i + 1].mean()
            else:
                o[i] = o[i - 1]
    return out + eps


def jump_margin_ulps(x, jump=JUMP):
    """the smallest distance, in float32 ulps of the threshold, between an amplitude and jump x its predecessor"""
    a = np.abs(np.atleast_2d(np.asarray(x, np.float32))).astype(np.float64)
    thr = float(jump) * a[:, :-1]
    ulp = np.spacing(np.maximum(thr, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return float((np.abs(a[:, 1:] - thr) / ulp).min()) if a.shape[1] > 1 else np.inf
