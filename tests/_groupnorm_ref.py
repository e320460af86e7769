"""GroupNorm32 forward fold and backward restated in float64 (numpy only, no GPU), and the yardstick the GPU tests measure the
kernels by: the same quantities formed from fp32 slot partials that are summed SEQUENTIALLY in float32 -- the least accurate order a
kernel may reasonably be compared with.  Shared by tests/test_groupnorm_host.py and tests/test_groupnorm_gpu.py.

Layouts as in include/tqdne_hip.h: activations (B, T, C) channels-last, the normalised tensor is the (virtual) channel concat of
``x_list`` (one or two sources), 32 groups of G = C / 32 adjacent channels of the concat; statistics (B, ceil(T / slot), C, 2).
``g`` is the gradient with respect to the OUTPUT u = scale x + shift of the norm (what the data-gradient epilogue hands on), see the
comment above gn_bwd_finalize_kernel (csrc/backward.hip)."""

import numpy as np

GROUPS = 32
EPS = 1e-5


def _cat(v_list):
    return np.concatenate([np.asarray(v, dtype=np.float64) for v in v_list if v is not None], axis=2)


def _split(v, like):
    out, c = [], 0
    for s in like:
        if s is None:
            continue
        out.append(v[:, :, c:c + np.shape(s)[2]])
        c += np.shape(s)[2]
    return out


def slot_sums(a, b=None, slot=128):
    """{sum a, sum a a} (b None) or {sum a, sum a b} per (sample, slot of ``slot`` positions, channel), in float64"""
    a = np.asarray(a, dtype=np.float64)
    b = a if b is None else np.asarray(b, dtype=np.float64)
    B, T, C = a.shape
    ns = (T + slot - 1) // slot
    out = np.empty((B, ns, C, 2))
    for s in range(ns):
        sa, sb = a[:, s * slot:(s + 1) * slot], b[:, s * slot:(s + 1) * slot]
        out[:, s, :, 0] = sa.sum(1)
        out[:, s, :, 1] = (sa * sb).sum(1)
    return out


def seq32_sum(v, axis):
    """column sums taken sequentially in float32 (numpy's cumsum has no pairwise tree), returned as float64"""
    return np.take(np.cumsum(np.asarray(v, dtype=np.float32), axis=axis, dtype=np.float32), -1, axis=axis).astype(np.float64)


def _per_channel(v, C):
    """(B, 32) group quantity -> (B, C)"""
    return np.repeat(v, C // GROUPS, axis=1)


def fold(x_list, gamma, beta, eps=EPS):
    """mean (B, 32), rstd (B, 32), scale (B, C), shift (B, C) with norm(x) = scale x + shift; two passes, no E[x^2]"""
    x = _cat(x_list)
    B, T, C = x.shape
    xg = x.reshape(B, T, GROUPS, C // GROUPS)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    rstd = 1.0 / np.sqrt(var + eps)
    scale = np.asarray(gamma, np.float64)[None] * _per_channel(rstd, C)
    shift = np.asarray(beta, np.float64)[None] - _per_channel(mean, C) * scale
    return dict(mean=mean, rstd=rstd, scale=scale, shift=shift)


def _coefficients(S1, S2c, gamma, mean, rstd, T):
    """S1 = sum_t g, S2c = sum_t g (x - mean) = S2 - mean S1, both (B, C) -> A, Bc, Cc (B, C), per-sample dgamma / dbeta terms"""
    B, C = S1.shape
    G = C // GROUPS
    gm = np.asarray(gamma, np.float64)[None]
    n = float(G * T)
    P1 = (gm * S1).reshape(B, GROUPS, G).sum(2)
    P2 = rstd * (gm * S2c).reshape(B, GROUPS, G).sum(2)
    A = gm * _per_channel(rstd, C)
    Bc = _per_channel(-rstd * rstd * P2 / n, C)
    Cc = _per_channel(rstd * rstd * P2 * mean / n - rstd * P1 / n, C)
    return A, Bc, Cc, _per_channel(rstd, C) * S2c, S1


def backward(x_list, g_list, gamma, mean, rstd):
    """float64 GroupNorm32 backward from the saved mean / rstd (B, 32): coefficients A, Bc, Cc (B, C) with dx = A g + Bc x + Cc,
    dx per source, dgamma / dbeta (C) summed over the batch and their per-sample contributions (B, C)"""
    x, g = _cat(x_list), _cat(g_list)
    B, T, C = x.shape
    mean, rstd = np.asarray(mean, np.float64), np.asarray(rstd, np.float64)
    S1 = g.sum(1)
    S2c = (g * (x - _per_channel(mean, C)[:, None])).sum(1)
    A, Bc, Cc, dg_b, db_b = _coefficients(S1, S2c, gamma, mean, rstd, T)
    dx = A[:, None] * g + Bc[:, None] * x + Cc[:, None]
    return dict(A=A, Bc=Bc, Cc=Cc, dx=_split(dx, x_list), dgamma=dg_b.sum(0), dbeta=db_b.sum(0), dgamma_b=dg_b, dbeta_b=db_b)


def _slot_partials(a, b, slot, dtype):
    """sequential slot sums {sum a, sum a b} in ``dtype`` (products in ``dtype`` too), combined over the slots in float64: (B, C) each"""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    T = a.shape[1]
    s1 = np.zeros((a.shape[0], a.shape[2]))
    s2 = np.zeros_like(s1)
    for s in range(0, T, slot):
        sa, sb = a[:, s:s + slot], b[:, s:s + slot]
        s1 += np.cumsum(sa, axis=1, dtype=dtype)[:, -1].astype(np.float64)
        s2 += np.cumsum(sa * sb, axis=1, dtype=dtype)[:, -1].astype(np.float64)
    return s1, s2


def emulate(x_list, g_list, gamma, beta, eps=EPS, slot=128, dtype=np.float32):
    """What ANY design with fp32 slot partials {sum x, sum x^2} / {sum g, sum g x} computes, at its least favourable summation order:
    the partials are sequential ``dtype`` sums, everything behind them is float64, and the saved mean / rstd and the coefficients are
    rounded to ``dtype``.  dx is then formed in float64 from the rounded coefficients (the rounding of the apply itself is a separate,
    derived term of the bars).  ``dtype`` = float64 is the control: the same algorithm without the fp32 partials."""
    x, g = _cat(x_list), _cat(g_list)
    B, T, C = x.shape
    G = C // GROUPS
    r = lambda v: np.asarray(v, dtype=dtype).astype(np.float64)
    gm, bt = np.asarray(gamma, np.float64)[None], np.asarray(beta, np.float64)[None]
    n = float(G * T)
    s1, s2 = _slot_partials(x, x, slot, dtype)
    mean = s1.reshape(B, GROUPS, G).sum(2) / n
    var = np.maximum(s2.reshape(B, GROUPS, G).sum(2) / n - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    mean, rstd = r(mean), r(rstd)   # (B, 32, 2) mean_rstd is an fp32 tensor
    scale = r(gm * _per_channel(rstd, C))
    shift = r(bt - _per_channel(mean, C) * scale)
    S1, S2 = _slot_partials(g, x, slot, dtype)
    A, Bc, Cc, dg_b, db_b = _coefficients(S1, S2 - _per_channel(mean, C) * S1, gamma, mean, rstd, T)
    A, Bc, Cc, dg_b, db_b = r(A), r(Bc), r(Cc), r(dg_b), r(db_b)
    dx = A[:, None] * g + Bc[:, None] * x + Cc[:, None]
    return dict(mean=mean, rstd=rstd, scale=scale, shift=shift, A=A, Bc=Bc, Cc=Cc, dx=_split(dx, x_list), dgamma=dg_b.sum(0),
                dbeta=db_b.sum(0))


def regime_input(B, T, c_list, ratio, seed):
    """x (float32 values, one (B, T, C_i) array per source) whose every group of the concat has |mean| = ratio x std, the sign of
    the offset alternating over the samples, and channel means spread inside a group by 0.5 std; plus g (same shapes), gamma, beta"""
    rng = np.random.default_rng(seed)
    C = sum(c_list)
    G = C // GROUPS
    z = rng.standard_normal((B, T, C))
    d = rng.standard_normal((1, 1, C))
    dg = d.reshape(GROUPS, G)
    dg = dg - dg.mean(1, keepdims=True)
    dg = 0.5 * dg / np.maximum(np.sqrt((dg ** 2).mean(1, keepdims=True)), 1e-30) if G > 1 else 0 * dg
    x = z + dg.reshape(1, 1, C)
    xg = x.reshape(B, T, GROUPS, G)
    xg = xg - xg.mean(axis=(1, 3), keepdims=True)
    std = np.sqrt((xg ** 2).mean(axis=(1, 3), keepdims=True))
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0).reshape(B, 1, 1, 1)
    x = (xg + sign * ratio * std).reshape(B, T, C).astype(np.float32)
    g = rng.standard_normal((B, T, C)).astype(np.float32)
    gamma = (1.0 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
    cut = np.cumsum([0] + list(c_list))
    sp = lambda v: [v[:, :, cut[i]:cut[i + 1]] for i in range(len(c_list)) if c_list[i]]
    return sp(x), sp(g), gamma, beta


def rel_max(a, b, floor=0.0):
    """max|a - b| / max(max|b|, floor)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-300))
