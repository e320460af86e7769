"""Ground-motion intensity measures restated in numpy: what smtk's ``get_response_spectrum(method="Nigam-Jennings")`` /
``rotate_horizontal`` and the reference's ``gmrotdpp_withPG`` (scripts/seismo_evaluations/example_GMM.py) compute, from their
definitions.  Neither smtk nor pyrotd is installed anywhere this suite runs, so nothing of them is run or copied; the oscillator
step is pinned against ``scipy.signal.lsim`` (exact for piecewise-linear input) in test_intensity_host.py.

float64 (the yardstick):
  nigam_jennings   the classic form on the state (u, u'): within a step the input is a0 + s tau, a particular solution is
                   -(a0 + s tau) / w^2 + 2 xi s / w^3, the homogeneous part exp(-xi w tau) (C1 cos wd tau + C2 sin wd tau)
  ground_series    a[:-1], dt * cumulative trapezoid of it, and of that
  rotd_peaks       max_t |sx cos phi + sy sin phi| for 180 whole degrees
  gmrotdpp_with_pg the percentile over sqrt(m[theta] m[theta + 90]) (GMRotD) or over m (RotD)
float32 (the emulation that sets the GPU test's bar; written from the recurrence, not from the kernel):
  emulate_peaks_f32  the scaled state (w^2 u, w u') advanced sample by sample with fp32 coefficients, every product and sum rounded to
                     fp32; the ground series accumulated in float64 and rounded; the rotation in fp32
"""

import numpy as np

N_ANGLES = 180
PERIODS7 = (0.03, 0.1, 0.3, 1.0, 2.0, 5.0, 10.0)


def periods_log(P):
    return np.array([1.0]) if P == 1 else np.geomspace(0.03, 10.0, P)


def make_waveforms(N, T, seed=0):
    """(x, y) float32 (N, T): smoothed Gaussian noise under a rise-and-decay envelope, amplitudes from 0.3 to 120 that differ per
    waveform and component.  Waveform 1 has y = 0, waveform 2 has x = y (every rotated series vanishes at 135 degrees)."""
    rng = np.random.default_rng(seed)
    ker = np.hanning(9)
    ker /= ker.sum()
    t = (np.arange(T) + 1.0) / T
    env = (t / 0.15) * np.exp(1.0 - t / 0.15)
    out = []
    for c in range(2):
        w = rng.standard_normal((N, T + 8))
        s = np.stack([np.convolve(r, ker, mode="valid") for r in w]) * env
        amp = 0.3 * 400.0 ** (((np.arange(N) * 2 + c) % 5) / 4.0)
        out.append(s * amp[:, None])
    x, y = out
    if N > 1:
        y[1] = 0.0
    if N > 2:
        y[2] = x[2]
    return x.astype(np.float32), y.astype(np.float32)


# ---------------------------------------------------------------- float64 ----------------------------------------------------------------

def _nj_step(u0, v0, a0, a1, w, xi, dt):
    """state (u, u') at the end of one step of the oscillator u'' + 2 xi w u' + w^2 u = -a, a linear from a0 to a1"""
    wd = w * np.sqrt(1.0 - xi * xi)
    s = (a1 - a0) / dt
    up0 = -a0 / w ** 2 + 2.0 * xi * s / w ** 3          # particular solution at tau = 0; its slope is -s / w^2 throughout
    c1 = u0 - up0
    c2 = (v0 + s / w ** 2 + xi * w * c1) / wd
    e, c, sn = np.exp(-xi * w * dt), np.cos(wd * dt), np.sin(wd * dt)
    u1 = -a1 / w ** 2 + 2.0 * xi * s / w ** 3 + e * (c1 * c + c2 * sn)
    v1 = -s / w ** 2 + e * ((wd * c2 - xi * w * c1) * c - (wd * c1 + xi * w * c2) * sn)
    return u1, v1


def nigam_jennings(a, dt, periods, damping=0.05):
    """a (..., T) -> absolute acceleration -(2 xi w u' + w^2 u) of every oscillator, (..., P, T - 1): sample k is the state at
    (k + 1) dt, from rest"""
    a = np.asarray(a, dtype=np.float64)
    w = 2.0 * np.pi / np.asarray(periods, dtype=np.float64)
    T = a.shape[-1]
    u = np.zeros(a.shape[:-1] + w.shape)
    v = np.zeros_like(u)
    out = np.empty(u.shape + (T - 1,))
    for k in range(T - 1):
        u, v = _nj_step(u, v, a[..., k, None], a[..., k + 1, None], w, damping, dt)
        out[..., k] = -(2.0 * damping * w * v + w * w * u)
    return out


def step_matrices(periods, dt, damping=0.05):
    """The step of the scaled state s = (w^2 u, w u'),  s' = A s + B0 a_k + B1 a_(k+1):  A (P, 2, 2), B0 (P, 2), B1 (P, 2), read off
    the step function above by linearity"""
    w = 2.0 * np.pi / np.asarray(periods, dtype=np.float64)
    z, one = np.zeros_like(w), np.ones_like(w)
    scale = np.stack([w * w, w], axis=-1)                # (P, 2): u -> w^2 u, u' -> w u'
    col = lambda u0, v0, a0, a1: np.stack(_nj_step(u0, v0, a0, a1, w, damping, dt), axis=-1) * scale
    A = np.stack([col(one / w ** 2, z, z, z), col(z, one / w, z, z)], axis=-1)
    return A, col(z, z, one, z), col(z, z, z, one)


def cumtrapz0(a, dt):
    """dt * scipy.integrate.cumulative_trapezoid(a, initial=0) along the last axis"""
    out = np.zeros_like(a)
    np.cumsum(0.5 * (a[..., 1:] + a[..., :-1]), axis=-1, out=out[..., 1:])
    return dt * out


def ground_series(a, dt):
    """(..., T) -> (..., 3, T - 1): acceleration a[:-1], velocity, displacement"""
    a = np.asarray(a, dtype=np.float64)[..., :-1]
    v = cumtrapz0(a, dt)
    return np.stack([a, v, cumtrapz0(v, dt)], axis=-2)


def series(a, dt, periods, damping=0.05):
    """(..., T) -> (..., 3 + P, T - 1)"""
    return np.concatenate([ground_series(a, dt), nigam_jennings(a, dt, periods, damping)], axis=-2)


def angle_table(dtype=np.float64):
    """cos and sin of 0 .. 179 degrees; 0 and 90 degrees leave the components exactly as they are"""
    phi = np.deg2rad(np.arange(N_ANGLES, dtype=np.float64))
    c, s = np.cos(phi), np.sin(phi)
    c[90] = 0.0
    return c.astype(dtype), s.astype(dtype)


def directional_peaks(sx, sy):
    """(..., L) pairs -> (..., 180) in the dtype of the series"""
    c, s = angle_table(sx.dtype)
    out = np.empty(sx.shape[:-1] + (N_ANGLES,), sx.dtype)
    for i in range(N_ANGLES):
        out[..., i] = np.abs(sx * c[i] + sy * s[i]).max(axis=-1)
    return out


def rotd_peaks(x, y, dt, periods, damping=0.05):
    return directional_peaks(series(x, dt, periods, damping), series(y, dt, periods, damping))


def rotate_literal(sx, sy, theta_deg):
    """the two rotated components of a literal rotation by theta"""
    th = np.deg2rad(theta_deg)
    return np.cos(th) * sx + np.sin(th) * sy, -np.sin(th) * sx + np.cos(th) * sy


def combine(peaks, percentile, kind="gmrotd"):
    """(..., K, 180) -> (..., K)"""
    if kind == "gmrotd":
        peaks = np.sqrt(peaks[..., :90] * peaks[..., 90:])
    elif kind != "rotd":
        raise ValueError(kind)
    return np.percentile(peaks, percentile, axis=-1)


def gmrotdpp_with_pg(x, y, dt, periods, percentile=50, damping=0.05, kind="gmrotd", peaks=None):
    g = combine(rotd_peaks(x, y, dt, periods, damping) if peaks is None else peaks, percentile, kind)
    return {"PGA": g[..., 0], "PGV": g[..., 1], "PGD": g[..., 2], "Acceleration": g[..., 3:]}


def response_spectrum(a, dt, periods, damping=0.05):
    """per-component SA (..., P): the peak of |absolute acceleration|"""
    return np.abs(nigam_jennings(a, dt, periods, damping)).max(axis=-1)


# ---------------------------------------------------------------- float32 ----------------------------------------------------------------

def _series_f32(a, dt, periods, damping):
    a = np.asarray(a, dtype=np.float32)
    f = np.float32
    A, B0, B1 = (m.astype(f) for m in step_matrices(periods, dt, damping))
    two_xi = f(2.0 * damping)
    T = a.shape[-1]
    p = np.zeros(a.shape[:-1] + (len(A),), f)
    q = np.zeros_like(p)
    out = np.empty(p.shape + (T - 1,), f)
    for k in range(T - 1):
        a0, a1 = a[..., k, None], a[..., k + 1, None]
        p, q = (((A[:, 0, 0] * p + A[:, 0, 1] * q) + B0[:, 0] * a0) + B1[:, 0] * a1,
                ((A[:, 1, 0] * p + A[:, 1, 1] * q) + B0[:, 1] * a0) + B1[:, 1] * a1)
        out[..., k] = -(two_xi * q + p)
    assert out.dtype == f
    return np.concatenate([ground_series(a.astype(np.float64), dt).astype(f), out], axis=-2)


def emulate_peaks_f32(x, y, dt, periods, damping=0.05):
    """(N, 3 + P, 180) float32: the sequential scaled-state recurrence and the rotation in fp32 arithmetic"""
    return directional_peaks(_series_f32(x, dt, periods, damping), _series_f32(y, dt, periods, damping))


def series_error(got, ref):
    """(..., K, 180) against float64: per series, max |got - ref| over the angles / that series' largest peak -> (..., K).  A series
    that is identically zero (velocity and displacement of a two-sample record, whose only sample is the initial 0) must come out
    as zeros: error 0 if it does, inf if not."""
    ref = np.asarray(ref, dtype=np.float64)
    d, top = np.abs(np.asarray(got, dtype=np.float64) - ref).max(axis=-1), ref.max(axis=-1)
    return np.where(top > 0.0, d / np.where(top > 0.0, top, 1.0), np.where(d == 0.0, 0.0, np.inf))
