"""float64 restatement of the reference's shaking-duration measures (scripts/seismo_evaluations/arias_intensity_duration.ipynb), in
this project's words: s = x^2 (+ y^2) on the widened float32 samples, the cumulative trapezoid recurrence
cum[0] = 0, cum[i] = cum[i-1] + 0.5 (s[i-1] + s[i]) step  one sample after the other, ``math.fsum`` for the exactly rounded total, the
first-crossing rule, and numpy's gradient formula in float64.  tests/test_duration_host.py pins each of them."""

import math

import numpy as np


def make_pairs(R, T, seed=0):
    """float32 (x, y), each (R, T): noise that rises over the first tenth of the row and decays after it, a row scale of 0.1 ... 10"""
    rng = np.random.default_rng(seed + 1000 * T + R)
    t = np.arange(T, dtype=np.float64) / max(T - 1, 1)
    env = (1.0 - np.exp(-t / 0.03)) * np.exp(-t / 0.3)
    scale = 10.0 ** rng.uniform(-1.0, 1.0, (R, 1))
    x = rng.standard_normal((R, T)) * (env + 1e-3) * scale
    y = rng.standard_normal((R, T)) * (env + 1e-3) * scale * 0.7
    return x.astype(np.float32), y.astype(np.float32)


def squares(x, y=None):
    s = np.atleast_2d(np.asarray(x, np.float32)).astype(np.float64) ** 2
    if y is not None:
        s = s + np.atleast_2d(np.asarray(y, np.float32)).astype(np.float64) ** 2
    return s


def terms(x, y=None, step=1.0):
    """(R, T - 1): the trapezoid term that ends at sample i, i = 1 ... T - 1"""
    s = squares(x, y)
    return 0.5 * (s[:, :-1] + s[:, 1:]) * step


def cumulative(x, y=None, step=1.0):
    """(R, T): the recurrence, one add per sample in sample order"""
    tm = terms(x, y, step)
    cum = np.zeros((tm.shape[0], tm.shape[1] + 1))
    for i in range(tm.shape[1]):
        cum[:, i + 1] = cum[:, i] + tm[:, i]
    return cum


def exact_total(x, y=None, step=1.0):
    """(R,): the correctly rounded sum of the float64 terms"""
    return np.array([math.fsum(row) for row in terms(x, y, step)])


def crossings(cum, fractions):
    """(R, F) int: the first i with cum[i] >= fl(f * cum[-1]); -1 for a row whose total is zero or not finite"""
    cum = np.atleast_2d(cum)
    out = np.full((cum.shape[0], len(fractions)), -1, np.int64)
    for r, row in enumerate(cum):
        if not (np.isfinite(row[-1]) and row[-1] > 0):
            continue
        for j, f in enumerate(fractions):
            out[r, j] = int(np.flatnonzero(row >= f * row[-1])[0])
    return out


def crossing_margin(cum, fractions):
    """the smallest distance, as a fraction of the total, that cum[n] and cum[n-1] keep from a threshold they decide (n: the crossing;
    n = 0 has no predecessor; a fraction of 0 or 1 is decided exactly and is left out)"""
    cum = np.atleast_2d(cum)
    idx = crossings(cum, fractions)
    worst = np.inf
    for r, row in enumerate(cum):
        for j, f in enumerate(fractions):
            n = idx[r, j]
            if n < 0 or f in (0.0, 1.0):
                continue
            thr = f * row[-1]
            worst = min(worst, (row[n] - thr) / row[-1])
            if n > 0:
                worst = min(worst, (thr - row[n - 1]) / row[-1])
    return worst


def husid(cum):
    cum = np.atleast_2d(cum)
    with np.errstate(invalid="ignore", divide="ignore"):
        return cum / cum[:, -1:]


def gradient(x, dt):
    """numpy.gradient's formula along the last axis on the widened samples, in float64, ``dt`` the float32 spacing widened"""
    x = np.asarray(x, np.float32).astype(np.float64)
    dt = float(np.float32(dt))
    g = np.empty_like(x)
    g[..., 1:-1] = (x[..., 2:] - x[..., :-2]) / (2.0 * dt)
    g[..., 0] = (x[..., 1] - x[..., 0]) / dt
    g[..., -1] = (x[..., -1] - x[..., -2]) / dt
    return g
