"""The GroupNorm chain against float64 (GPU): the slot statistics of every producer per entry, tq_gn_finalize on synthetic
statistics, the column-sum / apply kernels in every regime of their tiling, the dgamma / dbeta atomics over the batch, and the whole
chain producer -> tq_gn_finalize -> tq_conv1d_bwd_data -> tq_gn_bwd_finalize -> tq_gn_bwd_apply under group mean / std ratios of
0 ... 100.  The reference is tests/_groupnorm_ref.py (float64, numpy), never another kernel; the bit-for-bit pins between the kernels
stay where they are (tests/test_hip_bwd.py, tests/test_hip_ops.py, tests/test_wide_models_gpu.py).

As in tests/test_side_kernels_gpu.py every output is a slice out of the middle of a NaN-filled device tensor whose guard bands must
come back bit-unchanged, every input must equal the clone taken before the call, and a statistics / coefficient output the kernel
overwrites is NaN-prefilled so that an entry it forgets stays visible.  Every test prints what it measured.

Bars.  None is a measurement of the kernels:
  slot statistics   |err| <= (n + 1) 2^-24 sum|terms| per entry, n the rows of the slot: valid for ANY order of an fp32 sum of n
                    terms (n - 1 additions) whose terms carry one rounding of their own (the product y y or g x);
  tq_gn_finalize    BAR_FEW = 2e-6 relative per element on scale, mean, rstd (a handful of roundings behind an fp64 combine);
                    gshift to 2e-6 (|mean scale| + |beta|), because it cancels where beta ~ mean scale;
  dx                <= 4 2^-24 (|A g| + |Bc x| + |Cc| + |r| + |old|) per element: three products and four additions, contracted or not;
  column sums       <= 8 E per entry, E the largest error of a SEQUENTIAL fp32 sum of the same written values (the margin of
                    tests/test_intensity_gpu.py / tests/test_spectra_gpu.py; a dropped or doubled row misses it by orders of magnitude);
  max|dx|           bit-exact;
  dgamma / dbeta    <= (B + 2) 2^-24 (|prefill| + sum_b |contribution_b|): B + 1 atomic fp32 additions in any order, and the
                    rounding of each contribution to fp32;
  the chain         <= 8 x the error of _groupnorm_ref.emulate (fp32 slot partials summed sequentially) on the same input plus the
                    rounding floor of the fp32 outputs, at every ratio; and <= 1e-3 up to ratio 10."""

import ctypes

import numpy as np
import pytest
import torch

import _groupnorm_ref as R
from test_side_kernels_gpu import BAR_FEW, Case, Out, dev, lib, ok, p, stream

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64 = np.float64


def rng_of(*seed):
    return np.random.default_rng([int(s) & 0x7fffffff for s in seed] + [20261])


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def randn(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def host(o, *shape):
    """an Out (or a device tensor) as a float64 numpy array"""
    t = o.view if isinstance(o, Out) else o
    return t.detach().cpu().double().numpy().reshape(*shape)


def dview(o, *shape):
    return o.view.view(*shape)


def nslots(T, slot=128):
    return (T + slot - 1) // slot


# ============================================================================================================================
# (a) slot statistics of every producer, per entry
# ============================================================================================================================
def check_slot_stats(name, st, a, b=None, slot=128):
    """st (B, ns, C, 2) as the kernel left it in a NaN-prefilled tensor; a (and b): the tensor(s) the kernel itself wrote"""
    holes = int(np.isnan(st).sum())
    assert holes == 0, f"{name}: {holes} of {st.size} statistics entries were not written"
    ref = R.slot_sums(a, b, slot)
    mag = R.slot_sums(np.abs(a), None if b is None else np.abs(b), slot)
    assert st.shape == ref.shape, (st.shape, ref.shape)
    T, ns = a.shape[1], ref.shape[1]
    n = np.minimum(slot, T - slot * np.arange(ns)).reshape(1, ns, 1, 1)
    bar = (n + 1) * U * mag
    err = np.abs(st - ref)
    worst = float((err / np.maximum(bar, 1e-300)).max())
    print(f"{name}: worst statistics error {worst:.3f} of its bar ({st.shape[1]} slots of {slot}, last of {int(n.min())} rows)")
    assert (err <= bar).all(), f"{name}: {int((err > bar).sum())} entries beyond (n + 1) 2^-24 sum|terms|, worst {worst:.2f} x"


def conv_weights(rng, co, ci, k):
    return randn(rng, co, ci, k, scale=1.0 / np.sqrt(ci * k)), randn(rng, co)


def gn_coefs(c, rng, B, C):
    return c.inp(f32(1.0 + 0.3 * rng.standard_normal((B, C)))), c.inp(f32(0.3 * rng.standard_normal((B, C))))


def run_conv(c, rng, T_in, T_out, cins, co, k, *, act=False, slot=128, skip_c=0, **kw):
    """one tq_conv1d_fwd / tq_conv1d_fwd_skip launch with statistics through ops.conv1d into guarded outputs: (statistics, y)"""
    from tqdne_amd import ops
    B = 2
    xs = [c.inp(f32(randn(rng, B, T_in, ci))) for ci in cins]
    w, b = conv_weights(rng, co, sum(cins), k)
    wd, bd = c.inp(f32(w)), c.inp(f32(b))
    gs, gh = gn_coefs(c, rng, B, sum(cins)) if act else (None, None)
    skip = None
    if skip_c:
        ws, bs = conv_weights(rng, co, skip_c, 1)
        skip = (c.inp(f32(randn(rng, B, T_in, skip_c))), None, c.inp(f32(ws)), c.inp(f32(bs)))
    y, st = c.out(B * T_out * co), c.out(B * nslots(T_out, slot) * co * 2)
    ops.conv1d(xs[0], wd, bd, x1=xs[1] if len(xs) > 1 else None, gscale=gs, gshift=gh, silu=act, skip=skip,
               out=(dview(y, B, T_out, co), dview(st, B, nslots(T_out, slot), co, 2)), **kw)
    c.verify()
    return host(st, B, nslots(T_out, slot), co, 2), host(y, B, T_out, co)


def conv_producer(cins, co, k, **kw):
    def run(c, rng, T):
        return run_conv(c, rng, T, T, cins, co, k, **kw) + (None, kw.get("slot", 128))
    return run


def stride2_producer(c, rng, T):
    T_in = 2 * T - (T & 1)   # (both parities of the input length)
    return run_conv(c, rng, T_in, T, (64,), 64, 3, stride=2, wfmt=0) + (None, 128)


def upsample_producer(c, rng, T):
    return run_conv(c, rng, T // 2, T, (32,), 32, 5, upsample=True, wfmt=0) + (None, 128)


def poly2_producer(c, rng, T):
    """TQ_CONV_POLY2: the launch is a k = 3 conv to 2 C channels whose channel block p is row 2 t + p of a (B, 2 T, C) tensor; its
    statistics slot 2 tile + p holds the rows 2 t + p of the 128 t of that tile (the test compares each phase as a tensor of its own)."""
    from tqdne_amd import _lib, ops
    B, ci, co = 2, 64, 64
    x = c.inp(f32(randn(rng, B, T, ci)))
    w, b = conv_weights(rng, 2 * co, ci, 3)
    wp = ops.pack_conv_weight(c.inp(f32(w)), _lib.PACK_MODE[0])
    bd = c.inp(f32(b[:co]))
    ns = 2 * nslots(T)
    y, st = c.out(B * 2 * T * co), c.out(B * ns * co * 2)
    d = _lib.TqConvDesc()
    d.B, d.T_in, d.T_out, d.C_in0, d.C_in1, d.C_out = B, T, T, ci, 0, 2 * co
    d.ktaps, d.stride, d.pad, d.upsample = 3, 1, 1, 0
    d.flags, d.wfmt = _lib.TQ_CONV_STATS | _lib.TQ_CONV_POLY2, 0
    ok(lib().tq_conv1d_fwd(ctypes.byref(d), p(x), None, None, None, p(wp), p(bd), None, None, p(y), p(st), stream()))
    c.verify()
    return host(st, B, ns, co, 2), host(y, B, 2 * T, co), "poly2", 128


def stem_producer(ci, co):
    def run(c, rng, T):
        from tqdne_amd import ops
        B = 2
        x = c.inp(f32(randn(rng, B, ci, T)))
        w, b = conv_weights(rng, co, ci, 5)
        sc = c.inp(f32(rng.random(B) + 0.5))
        y, st = c.out(B * T * co), c.out(B * nslots(T) * co * 2)
        ops.stem_conv(x, c.inp(f32(w)), c.inp(f32(b)), in_scale=sc, out=(dview(y, B, T, co), dview(st, B, nslots(T), co, 2)))
        c.verify()
        return host(st, B, nslots(T), co, 2), host(y, B, T, co), None, 128
    return run


def resample_producer(up, C):
    def run(c, rng, T):
        from tqdne_amd import ops
        B = 2
        T_in = T // 2 if up else 2 * T + (T & 1)   # (avg_pool2 drops the last row of an odd length)
        x = c.inp(f32(randn(rng, B, T_in, C) + 0.5))
        y, st = c.out(B * T * C), c.out(B * nslots(T) * C * 2)
        (ops.nearest_up2 if up else ops.avg_pool2)(x, out=(dview(y, B, T, C), dview(st, B, nslots(T), C, 2)))
        c.verify()
        return host(st, B, nslots(T), C, 2), host(y, B, T, C), None, 128
    return run


def bwd_data(c, dy, w, xs, gs, gh, wfmt=0, flags=None):
    """tq_conv1d_bwd_data through the C ABI into guarded outputs: (g per source, statistics)"""
    from tqdne_amd import _lib, ops
    B, T, cdy = dy.shape
    cins = [x.shape[2] for x in xs]
    C = sum(cins)
    g = [c.out(B * T * ci) for ci in cins]
    st = c.out(B * nslots(T) * C * 2)
    d = _lib.TqConvBwdDesc()
    d.B, d.T, d.C_dy, d.C_dx0, d.C_dx1, d.ktaps = B, T, cdy, cins[0], cins[1] if len(cins) > 1 else 0, w.shape[2]
    d.flags = _lib.TQ_BWD_GN | _lib.TQ_BWD_SILU | _lib.TQ_BWD_STATS if flags is None else flags
    d.wfmt = wfmt
    amax = None
    if wfmt == _lib.TQ_WFMT_F16_MX6:
        amax = ops.amax_bits(dy)
        d.dy_amax = amax.data_ptr()
    wp = ops.pack_conv_weight(w, _lib.PACK_MODE_T[wfmt])
    rc = lib().tq_conv1d_bwd_data(ctypes.byref(d), p(dy), p(wp), p(xs[0]), p(xs[1]) if len(xs) > 1 else None, p(gs), p(gh), p(g[0]),
                                  p(g[1]) if len(g) > 1 else None, p(st), stream())
    torch.cuda.synchronize()
    del amax, wp
    return rc, g, st


def bwd_data_producer(cins, cdy, k, wfmt):
    def run(c, rng, T):
        B, C = 2, sum(cins)
        dy = c.inp(f32(randn(rng, B, T, cdy)))
        w = c.inp(f32(conv_weights(rng, cdy, C, k)[0]))
        xs_np = [randn(rng, B, T, ci) + 0.3 for ci in cins]
        xs = [c.inp(f32(x)) for x in xs_np]
        gs, gh = gn_coefs(c, rng, B, C)
        rc, g, st = bwd_data(c, dy, w, xs, gs, gh, wfmt)
        ok(rc)
        c.verify()
        gw = np.concatenate([host(gi, B, T, ci) for gi, ci in zip(g, cins)], axis=2)
        return host(st, B, nslots(T), C, 2), gw, np.concatenate(xs_np, axis=2).astype(F64), 128
    return run


def head_bwd_producer(ci):
    def run(c, rng, T):
        from tqdne_amd import ops
        B, co, k = 2, 3, 5
        x_np = randn(rng, B, T, ci) + 0.3
        x, dpred = c.inp(f32(x_np)), c.inp(f32(randn(rng, B, co, T)))
        w = c.inp(f32(conv_weights(rng, co, ci, k)[0]))
        gs, gh = gn_coefs(c, rng, B, ci)
        cout = c.inp(f32(rng.random(B) + 0.5))
        g, st = c.out(B * T * ci), c.out(B * nslots(T) * ci * 2)
        dw, db = c.out(co * ci * k, fill=np.zeros(co * ci * k)), c.out(co, fill=np.zeros(co))
        ops.head_conv_bwd(dpred, x, w, gs, gh, cout, out=(dview(g, B, T, ci), dview(st, B, nslots(T), ci, 2), dview(dw, co, ci, k), db.view))
        c.verify()
        return host(st, B, nslots(T), ci, 2), host(g, B, T, ci), x_np.astype(F64), 128
    return run


T_SLOTS = (128, 127, 129, 300)    # a full slot, a ragged one, a one-row last slot, three slots with a ragged last one
T_EVEN = (128, 126, 130, 300)     # outputs of a x2 upsampling have an even length: the shortest last slot is two rows
T_POLY2 = (128, 200, 256)         # the lengths TQ_CONV_POLY2's statistics are defined for (include/tqdne_hip.h)
MX6 = 2
PRODUCERS = {
    "conv_tile128_k3": (conv_producer((32,), 128, 3, wfmt=0), T_SLOTS),
    "conv_tile256_k1": (conv_producer((64,), 256, 1, wfmt=0), T_SLOTS),
    "conv_tile256_k5_concat": (conv_producer((64, 32), 256, 5, wfmt=0), T_SLOTS),
    "conv_tile64_k5": (conv_producer((32,), 64, 5, wfmt=0), T_SLOTS),
    "conv_tile32_k3": (conv_producer((32,), 96, 3, wfmt=0), T_SLOTS),
    "conv_tile128_mx6": (conv_producer((64,), 128, 3, wfmt=MX6), T_SLOTS),
    "conv_tile64_mx6_two_waves_per_slot": (conv_producer((64,), 64, 5, act=True, wfmt=MX6), T_SLOTS),
    "conv_t_tile32": (conv_producer((64,), 128, 5, act=True, wfmt=0, t_tile=32, slot=32), (128, 127, 129, 300, 97)),
    "conv_t_tile32_co64": (conv_producer((32,), 64, 5, act=True, wfmt=0, t_tile=32, slot=32), T_SLOTS),
    "conv_t_tile32_mx6": (conv_producer((64,), 128, 5, act=True, wfmt=MX6, t_tile=32, slot=32), T_SLOTS),
    "conv_poly2": (poly2_producer, T_POLY2),
    "conv_stride2": (stride2_producer, T_SLOTS),
    "conv_upsample": (upsample_producer, T_EVEN),
    "conv_skip": (conv_producer((64,), 128, 5, act=True, wfmt=0, skip_c=32), T_SLOTS),
    "conv_skip_co64_mx6": (conv_producer((64,), 64, 5, act=True, wfmt=MX6, skip_c=64), T_SLOTS),
    "stem_3": (stem_producer(3, 64), T_SLOTS),
    "stem_16": (stem_producer(16, 64), T_SLOTS),
    "stem_wide_160": (stem_producer(3, 160), T_SLOTS),
    "avg_pool2": (resample_producer(False, 96), T_SLOTS),
    "nearest_up2": (resample_producer(True, 96), T_EVEN),
    "bwd_data_single_bf16x3": (bwd_data_producer((128,), 64, 3, 0), T_SLOTS),
    "bwd_data_single_mx6": (bwd_data_producer((128,), 64, 3, MX6), T_SLOTS),
    "bwd_data_concat_64_32": (bwd_data_producer((64, 32), 64, 5, 0), T_SLOTS),
    "bwd_data_co64_bf16x3": (bwd_data_producer((64,), 128, 5, 0), T_SLOTS),
    "bwd_data_co64_mx6_two_waves_per_slot": (bwd_data_producer((64,), 128, 5, MX6), T_SLOTS),
    "head_bwd_64": (head_bwd_producer(64), T_SLOTS),
    "head_bwd_wide_160": (head_bwd_producer(160), T_SLOTS),
}


@pytest.mark.parametrize("name,T", [(n, T) for n, (_, ts) in PRODUCERS.items() for T in ts])
def test_producer_slot_statistics(name, T):
    """every (b, slot, c) pair of the statistics against slot_sums of the tensor the kernel wrote (read back: the contraction error of
    the conv is not part of this comparison)"""
    c = Case()
    st, a, b, slot = PRODUCERS[name][0](c, rng_of(T, len(name), sum(map(ord, name))), T)
    if isinstance(b, str):   # poly2: slot 2 tile + phase
        B, ns, C, _ = st.shape
        for ph in (0, 1):
            check_slot_stats(f"{name} T={T} phase {ph}", np.ascontiguousarray(st[:, ph::2]), a[:, ph::2], None, slot)
        return
    check_slot_stats(f"{name} T={T}", st, a, b, slot)


# ============================================================================================================================
# (b) tq_gn_finalize on synthetic statistics
# ============================================================================================================================
def synthetic_stats(rng, B, T, C, slot, m, v):
    """fp32 statistics (B, ceil(T / slot), C, 2) of a tensor whose channel c of sample b has mean m[b, c] and variance v[b, c]"""
    ns = nslots(T, slot)
    n = np.minimum(slot, T - slot * np.arange(ns)).reshape(1, ns, 1).astype(F64)
    s1 = n * m[:, None] + np.sqrt(n * v[:, None]) * rng.standard_normal((B, ns, C))
    s2 = n * (v + m * m)[:, None] * (1.0 + 0.02 * rng.standard_normal((B, ns, C)))
    return np.stack([s1, s2], axis=-1).astype(np.float32)


def finalize_ref(stats, C, T, gamma, beta):
    """float64 from the same fp32 statistics: (scale, shift, mean, rstd, |mean scale| + |beta|)"""
    s = np.concatenate([st.astype(F64).sum(1) for st in stats], axis=1)   # (B, C, 2)
    B, G = s.shape[0], C // 32
    n = float(G * T)
    mean = s[..., 0].reshape(B, 32, G).sum(2) / n
    var = np.maximum(s[..., 1].reshape(B, 32, G).sum(2) / n - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + float(np.float32(1e-5)))
    scale = gamma.astype(F64)[None] * np.repeat(rstd, G, axis=1)
    ms = np.repeat(mean, G, axis=1) * scale
    return scale, beta.astype(F64)[None] - ms, mean, rstd, np.abs(ms) + np.abs(beta.astype(F64))[None]


def run_finalize(c, stats, cs, B, T, gamma, beta, slots, with_mr):
    C = sum(cs)
    sd = [c.inp(f32(s)) for s in stats]
    gs, gh = c.out(B * C), c.out(B * C)
    mr = c.out(B * 64) if with_mr else None
    ok(lib().tq_gn_finalize(p(sd[0]), cs[0], p(sd[1]) if len(sd) > 1 else None, cs[1] if len(cs) > 1 else 0, B, T, p(c.inp(f32(gamma))),
                            p(c.inp(f32(beta))), p(gs), p(gh), p(mr), slots[0], slots[1], stream()))
    c.verify()
    return host(gs, B, C), host(gh, B, C), host(mr, B, 32, 2) if with_mr else None


FIN_CHANNELS = [(32,), (64, 32), (128,), (96, 64), (1024,), (1024, 32), (2048, 1792)]   # PARTS 4 / 2 / 2 / 1, pre-loaded affine up to 1024, then the general loop
FIN_SLOTS = [1, 7, 8, 9, 29, 33]
FIN_FORMS = [(1, (0, 0), True), (3, (128, 32), False), (3, (32, 128), True), (1, (32, 32), True)]   # B, slot arguments, mean_rstd given


@pytest.mark.parametrize("ns", FIN_SLOTS)
@pytest.mark.parametrize("cs", FIN_CHANNELS, ids=lambda cs: "+".join(map(str, cs)))
def test_gn_finalize_on_synthetic_statistics(cs, ns):
    C = sum(cs)
    worst = {}
    for B, slots, with_mr in FIN_FORMS:
        rng = rng_of(C, ns, B, slots[0], slots[1])
        s0 = slots[0] or 128
        T = max(1, ns * s0 - (s0 // 2 - 3) * (ns > 1) - 5 * (ns == 1))   # ns slots of source 0, the last one ragged
        assert nslots(T, s0) == ns
        m, v = rng.standard_normal((B, C)) * 1.5 + 0.5, rng.random((B, C)) * 1.5 + 0.5
        cut = np.cumsum((0,) + cs)
        stats = [synthetic_stats(rng, B, T, ci, slots[i] or 128, m[:, cut[i]:cut[i + 1]], v[:, cut[i]:cut[i + 1]]) for i, ci in enumerate(cs)]
        gamma, beta = randn(rng, C), randn(rng, C)
        c = Case()
        gs, gh, mr = run_finalize(c, stats, cs, B, T, gamma, beta, slots, with_mr)
        scale, shift, mean, rstd, shmag = finalize_ref(stats, C, T, gamma, beta)
        assert not np.isnan(gs).any() and not np.isnan(gh).any(), "coefficients left unwritten"
        e = dict(scale=float((np.abs(gs - scale) / np.abs(scale)).max()), shift=float((np.abs(gh - shift) / shmag).max()))
        if with_mr:
            assert not np.isnan(mr).any(), "mean_rstd left unwritten"
            e["mean"] = float((np.abs(mr[..., 0] - mean) / np.abs(mean)).max())
            e["rstd"] = float((np.abs(mr[..., 1] - rstd) / rstd).max())
        for k, x in e.items():
            worst[k] = max(worst.get(k, 0.0), x)
        assert max(e.values()) <= BAR_FEW, (B, slots, with_mr, e)
    print(f"gn_finalize C {cs} slots {ns}: " + " ".join(f"{k} {x:.1e}" for k, x in worst.items()))


@pytest.mark.parametrize("kind", ["constant", "inconsistent"])
def test_gn_finalize_degenerate_statistics(kind):
    """a constant group (sum y^2 = n mean^2 exactly) and statistics with sum y^2 / n < mean^2 (the clamp) both give rstd = 1 / sqrt(eps)"""
    B, T, cs = 2, 300, (64, 32)
    C = sum(cs)
    val = np.array([2.0, -0.5])[:, None] * np.ones((B, C))   # (powers of two: every sum below is exact in fp32)
    stats = []
    for ci, sl, c0 in ((64, 128, 0), (32, 32, 64)):
        n = np.minimum(sl, T - sl * np.arange(nslots(T, sl))).reshape(1, -1, 1).astype(F64)
        s1 = n * val[:, None, c0:c0 + ci]
        s2 = n * (val * val)[:, None, c0:c0 + ci] * (1.0 if kind == "constant" else 0.75)
        stats.append(np.stack([s1, s2], axis=-1).astype(np.float32))
    rng = rng_of(7, len(kind))
    gamma, beta = randn(rng, C), randn(rng, C)
    c = Case()
    gs, gh, mr = run_finalize(c, stats, cs, B, T, gamma, beta, (128, 32), True)
    top = 1.0 / np.sqrt(float(np.float32(1e-5)))
    e_r = float(np.abs(mr[..., 1] / top - 1).max())
    e_m = float(np.abs(mr[..., 0] - val[:, :1]).max())
    e_s = float((np.abs(gs - gamma.astype(F64)[None] * top) / np.abs(gamma.astype(F64) * top)[None]).max())
    print(f"gn_finalize {kind}: rstd {e_r:.1e} mean {e_m:.1e} scale {e_s:.1e} of 1 / sqrt(eps) = {top:.3f}")
    assert e_r <= BAR_FEW and e_m == 0.0 and e_s <= BAR_FEW


# ============================================================================================================================
# (c) tq_colsum, tq_gn_bwd_apply, tq_gn_bwd_apply_colsum against float64
# ============================================================================================================================
# The column-sum kernels give a workgroup `rows` rows of one sample: 128, doubled up to 4096 while B ceil(T / (2 rows)) >= 256
# workgroups remain (colsum_tiling, csrc/backward.hip); a thread owns one float4 column and every (256 / (C / 4))-th row, eight (apply:
# four) rows per trip of its unrolled body and a one-row remainder loop.  The plain apply is a grid-stride kernel of at most 4096
# workgroups of 256 float4.  The shapes below were chosen by that rule; the tests assert nothing about it.
CS_SHAPES = {
    "B2_T130_C36": (2, 130, 36),          # 9 float4 columns, 28 row lanes, 128 rows per workgroup and a two-row second one
    "B64_T1024_C64": (64, 1024, 64),      # 256 rows per workgroup
    "B64_T2100_C32": (64, 2100, 32),      # 512 rows, ragged last tile of 52
    "B256_T130_C32": (256, 130, 32),      # 4096 rows: one workgroup per sample
    "B5_T1153_C768": (5, 1153, 768),      # the plain apply's second grid-stride trip (above 4096 * 256 float4)
}
#            entry point     r      acc    c_offset  bc     c      c2     amax
CS_FORMS = {
    "fused_all": ("fused", True, True, 8, True, True, True, True),
    "fused_bc_amax": ("fused", False, False, 0, True, False, False, True),
    "fused_c_only": ("fused", True, False, 0, False, True, False, False),
    "fused_amax_only_acc": ("fused", False, True, 8, False, False, False, True),
    "plain_r_acc_offset": ("plain", True, True, 8, False, False, False, False),
    "plain_bare": ("plain", False, False, 0, False, False, False, False),
}


def check_sums(name, got, prefill, rows):
    """got, prefill (...,) and rows (n, ...) float64: the destination held ``prefill`` and the kernel added the n rows.  Error against
    the exact sum, bar 8 x the largest error of the sequential fp32 sum of the same numbers."""
    terms = np.concatenate([prefill[None], rows], axis=0)
    exact = terms.sum(0)
    E = float(np.abs(R.seq32_sum(terms, 0) - exact).max())
    err = float(np.abs(got - exact).max())
    print(f"  {name}: error {err:.2e}, sequential fp32 {E:.2e} ({err / max(E, 1e-300):.2f} x)")
    assert err <= 8 * E, f"{name}: {err:.3e} > 8 x {E:.3e}"


def amax_block(c):
    """a zeroed TQ_AMAX_WORDS block between guard bands (an fp32 Out: its NaN bands do not exist as integers; +0.0 is the zero word)"""
    from tqdne_amd import _lib
    return c.out(_lib.TQ_AMAX_WORDS, fill=np.zeros(_lib.TQ_AMAX_WORDS))


def amax_of(block):
    return int(block.view.view(torch.int32).cpu().max())


def bits_of_max_abs(a):
    return int(np.abs(a).max().astype(np.float32).view(np.int32))


@pytest.mark.parametrize("form", CS_FORMS)
@pytest.mark.parametrize("shape", CS_SHAPES)
def test_gn_bwd_apply_and_its_sums(shape, form):
    from tqdne_amd import _lib
    B, T, Cs = CS_SHAPES[shape]
    entry, with_r, acc, coff, with_bc, with_c, with_c2, with_amax = CS_FORMS[form]
    Ct = Cs + (12 if coff else 0)
    rng = rng_of(B, T, Cs, len(form), sum(map(ord, form)))
    tg = torch.Generator().manual_seed(B * 7 + T * 3 + Cs + len(form))
    tr = lambda *s: torch.randn(*s, generator=tg)
    g_t, x_t = tr(B, T, Cs), tr(B, T, Cs) + 0.5
    r_t = tr(B, T, Cs) if with_r else None
    old_t = tr(B, T, Cs) if acc else None
    A, Bc, Cc = randn(rng, B, Ct), randn(rng, B, Ct, scale=0.3), randn(rng, B, Ct, scale=0.3)
    c = Case()
    g, x, r = c.inp(g_t), c.inp(x_t), c.inp(r_t) if with_r else None
    Ad, Bd, Cd = c.inp(f32(A)), c.inp(f32(Bc)), c.inp(f32(Cc))
    dx = c.out(B * T * Cs, fill=old_t if acc else None)
    stride = Cs + 4
    pre_bc = np.full((B, stride), np.nan)
    pre_bc[:, :Cs] = rng.standard_normal((B, Cs)).astype(np.float32)
    pre_c, pre_c2 = randn(rng, Cs).astype(F64), randn(rng, Cs).astype(F64)
    obc = c.out(B * stride, fill=pre_bc) if with_bc else None
    oc = c.out(Cs, fill=pre_c) if with_c else None
    oc2 = c.out(Cs, fill=pre_c2) if with_c2 else None
    am = amax_block(c) if with_amax else None
    if entry == "plain":
        ok(lib().tq_gn_bwd_apply(p(g), p(x), p(r), p(Ad), p(Bd), p(Cd), p(dx), B, T, Cs, Ct, coff, int(acc), stream()))
    else:
        ok(lib().tq_gn_bwd_apply_colsum(p(g), p(x), p(r), p(Ad), p(Bd), p(Cd), p(dx), B, T, Cs, Ct, coff, int(acc), p(obc), stride, p(oc),
                                        p(oc2), p(am), stream()))
    c.verify()
    # dx per element
    gn, xn = g_t.double().numpy(), x_t.double().numpy()
    a64, b64, c64 = (k[:, None, coff:coff + Cs].astype(F64) for k in (A, Bc, Cc))
    ref = a64 * gn + b64 * xn + c64
    mag = np.abs(a64 * gn) + np.abs(b64 * xn) + np.abs(c64)
    for extra in (r_t, old_t):
        if extra is not None:
            ref = ref + extra.double().numpy()
            mag = mag + extra.double().abs().numpy()
    dxw = host(dx, B, T, Cs)
    assert not np.isnan(dxw).any(), "dx entries left unwritten"
    worst = float((np.abs(dxw - ref) / (4 * U * mag)).max())
    print(f"{shape} {form}: dx worst {worst:.3f} of 4 2^-24 (|A g| + |Bc x| + |Cc| + |r| + |old|)")
    assert worst <= 1.0
    # the sums of the tensor the kernel wrote
    if with_bc:
        got = host(obc, B, stride)
        assert np.isnan(got[:, Cs:]).all(), "per-sample sums written beyond C_src of a row"
        check_sums("colsum_bc", got[:, :Cs], pre_bc[:, :Cs], dxw.transpose(1, 0, 2))
    if with_c:
        check_sums("colsum_c", host(oc, Cs), pre_c, dxw.reshape(B * T, Cs))
    if with_c2:
        check_sums("colsum_c2", host(oc2, Cs), pre_c2, dxw.reshape(B * T, Cs))
    if with_amax:
        assert amax_of(am) == bits_of_max_abs(dxw), "amax is not the bit pattern of max|dx|"


@pytest.mark.parametrize("bscale", [False, True], ids=["plain", "bscale"])
@pytest.mark.parametrize("shape", CS_SHAPES)
def test_colsum(shape, bscale):
    from tqdne_amd import _lib
    B, T, C = CS_SHAPES[shape]
    rng = rng_of(B, T, C, int(bscale))
    dy_t = torch.randn(B, T, C, generator=torch.Generator().manual_seed(B + T + C)) + 0.25
    c = Case()
    dy = c.inp(dy_t)
    sc = (rng.random(B) + 0.5).astype(np.float32) if bscale else np.ones(B, dtype=np.float32)
    scd = c.inp(f32(sc)) if bscale else None
    stride = C + 8
    pre_bc = np.full((B, stride), np.nan)
    pre_bc[:, :C] = rng.standard_normal((B, C)).astype(np.float32)
    pre_c, pre_c2 = randn(rng, C).astype(F64), randn(rng, C).astype(F64)
    obc, oc = c.out(B * stride, fill=pre_bc), c.out(C, fill=pre_c)
    oc2 = None if bscale else c.out(C, fill=pre_c2)
    am = None if bscale else amax_block(c)
    ok(lib().tq_colsum(p(dy), B, T, C, p(obc), stride, p(oc), p(oc2), p(scd), p(am), stream()))
    c.verify()
    rows = dy_t.double().numpy() * sc.astype(F64)[:, None, None]   # (the scaled rows: the kernel scales each workgroup's partial sum once)
    got = host(obc, B, stride)
    print(f"colsum {shape} bscale {bscale}:")
    assert np.isnan(got[:, C:]).all()
    check_sums("out_bc", got[:, :C], pre_bc[:, :C], rows.transpose(1, 0, 2))
    check_sums("out_c", host(oc, C), pre_c, rows.reshape(B * T, C))
    if not bscale:
        check_sums("out_c2", host(oc2, C), pre_c2, rows.reshape(B * T, C))
        assert amax_of(am) == bits_of_max_abs(dy_t.numpy())


@pytest.mark.parametrize("entry", ["colsum", "fused"])
def test_a_nan_is_recorded_as_infinity(entry):
    from tqdne_amd import _lib
    B, T, C = 2, 130, 36
    tg = torch.Generator().manual_seed(3)
    v = torch.randn(B, T, C, generator=tg)
    v[1, 129, 35] = float("nan")
    c = Case()
    am = amax_block(c)
    if entry == "colsum":
        ok(lib().tq_colsum(p(c.inp(v)), B, T, C, None, 0, None, None, None, p(am), stream()))
    else:
        k = [c.inp(torch.randn(B, C, generator=tg)) for _ in range(3)]
        dx = c.out(B * T * C)
        ok(lib().tq_gn_bwd_apply_colsum(p(c.inp(torch.randn(B, T, C, generator=tg))), p(c.inp(torch.randn(B, T, C, generator=tg))), p(c.inp(v)),
                                        p(k[0]), p(k[1]), p(k[2]), p(dx), B, T, C, C, 0, 0, None, 0, None, None, p(am), stream()))
    c.verify()
    assert amax_of(am) == 0x7f800000


# ============================================================================================================================
# (d) dgamma / dbeta over the batch
# ============================================================================================================================
@pytest.mark.parametrize("C", [64, 768])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_gn_bwd_finalize_over_the_batch(B, C):
    T, G = 130, C // 32
    ns = nslots(T)
    rng = rng_of(B, C)
    gst = randn(rng, B, ns, C, 2)
    mr = np.stack([rng.standard_normal((B, 32)), rng.random((B, 32)) + 0.5], axis=-1).astype(np.float32)
    gamma = randn(rng, C)
    pre_g, pre_b = randn(rng, C).astype(F64), randn(rng, C).astype(F64)
    c = Case()
    A, Bc, Cc = c.out(B * C), c.out(B * C), c.out(B * C)
    dg, db = c.out(C, fill=pre_g), c.out(C, fill=pre_b)
    ok(lib().tq_gn_bwd_finalize(p(c.inp(f32(gst))), p(c.inp(f32(mr))), p(c.inp(f32(gamma))), B, C, T, p(A), p(Bc), p(Cc), p(dg), p(db), stream()))
    c.verify()
    s = gst.astype(F64).sum(1)
    S1, S2 = s[..., 0], s[..., 1]
    mean, rstd = mr[..., 0].astype(F64), mr[..., 1].astype(F64)
    S2c = S2 - np.repeat(mean, G, axis=1) * S1
    rA, rB, rC, dg_b, db_b = R._coefficients(S1, S2c, gamma, mean, rstd, T)
    n = float(G * T)
    gm = gamma.astype(F64)[None]
    P1 = np.repeat((gm * S1).reshape(B, 32, G).sum(2), G, axis=1)
    P2 = np.repeat(rstd * (gm * S2c).reshape(B, 32, G).sum(2), G, axis=1)
    r_c, m_c = np.repeat(rstd, G, axis=1), np.repeat(mean, G, axis=1)
    cmag = np.abs(r_c * r_c * P2 * m_c / n) + np.abs(r_c * P1 / n)   # (Cc is a difference of two terms)
    gA, gB, gC = host(A, B, C), host(Bc, B, C), host(Cc, B, C)
    assert not (np.isnan(gA).any() or np.isnan(gB).any() or np.isnan(gC).any()), "coefficients left unwritten"
    e = dict(A=float((np.abs(gA - rA) / np.abs(rA)).max()), Bc=float((np.abs(gB - rB) / np.abs(rB)).max()),
             Cc=float((np.abs(gC - rC) / cmag).max()))
    bar_g = (B + 2) * U * (np.abs(pre_g) + np.abs(dg_b).sum(0))
    bar_b = (B + 2) * U * (np.abs(pre_b) + np.abs(db_b).sum(0))
    e["dgamma"] = float((np.abs(host(dg, C) - (pre_g + dg_b.sum(0))) / bar_g).max())
    e["dbeta"] = float((np.abs(host(db, C) - (pre_b + db_b.sum(0))) / bar_b).max())
    print(f"gn_bwd_finalize B {B} C {C}: coefficients A {e['A']:.1e} Bc {e['Bc']:.1e} Cc {e['Cc']:.1e} (relative); "
          f"dgamma {e['dgamma']:.3f} dbeta {e['dbeta']:.3f} of (B + 2) 2^-24 (|prefill| + sum |contributions|)")
    assert max(e["A"], e["Bc"], e["Cc"]) <= BAR_FEW
    assert e["dgamma"] <= 1.0 and e["dbeta"] <= 1.0


# ============================================================================================================================
# (e) the chain under mean / std regimes, through the real kernels
# ============================================================================================================================
RATIOS = [0, 3, 10, 30, 100]
#                 C0   C1  T     wfmt of the data gradient
CHAIN_SHAPES = {
    "G1": (32, 0, 130, 0),
    "G3_straddling": (64, 32, 130, 0),
    "G6_T1153": (128, 64, 1153, 0),
    "G4_mx6": (128, 0, 130, MX6),
}


def produce(c, kind, x_np):
    """x through a real producer: (y as written (numpy), device y, device statistics)"""
    from tqdne_amd import ops
    B, T, C = x_np.shape
    y, st = c.out(B * T * C), c.out(B * nslots(T) * C * 2)
    outs = (dview(y, B, T, C), dview(st, B, nslots(T), C, 2))
    if kind == "nearest_up2":
        ops.nearest_up2(c.inp(f32(x_np[:, ::2])), out=outs)
    else:
        eye = np.eye(C, dtype=np.float32)[:, :, None]
        ops.conv1d(c.inp(f32(x_np)), c.inp(f32(eye)), None, wfmt=0, out=outs)
    torch.cuda.synchronize()
    yw = host(y, B, T, C)
    assert not np.isnan(yw).any() and not np.isnan(host(st, -1)).any()
    if kind == "nearest_up2":
        assert np.array_equal(yw, x_np.astype(F64)), "nearest x2 upsampling copies"
    return yw, y, st


def run_chain(kind, cs, T, wfmt, xs_np, gamma, beta, seed):
    """-> measured errors and their yardsticks, each max|a - b| / max|b| against the float64 restatement"""
    B = xs_np[0].shape[0]
    C = sum(cs)
    rng = rng_of(seed, 99)
    c = Case()
    made = [produce(c, kind, x) for x in xs_np]
    xw = [m[0] for m in made]
    gd, bd = c.inp(f32(gamma)), c.inp(f32(beta))
    gs, gh, mr = c.out(B * C), c.out(B * C), c.out(B * 64)
    ok(lib().tq_gn_finalize(p(made[0][2]), cs[0], p(made[1][2]) if len(cs) > 1 else None, cs[1] if len(cs) > 1 else 0, B, T, p(gd), p(bd),
                            p(gs), p(gh), p(mr), 0, 0, stream()))
    cdy = 64
    dy = c.inp(f32(randn(rng, B, T, cdy)))
    w = c.inp(f32(conv_weights(rng, cdy, C, 3)[0]))
    rc, g, gst = bwd_data(c, dy, w, [m[1].view.view(B, T, ci) for m, ci in zip(made, cs)], gs, gh, wfmt)
    ok(rc)
    A, Bc, Cc = c.out(B * C), c.out(B * C), c.out(B * C)
    dg, db = c.out(C, fill=np.zeros(C)), c.out(C, fill=np.zeros(C))
    ok(lib().tq_gn_bwd_finalize(p(gst), p(mr), p(gd), B, C, T, p(A), p(Bc), p(Cc), p(dg), p(db), stream()))
    dx, off = [], 0
    for m, gi, ci in zip(made, g, cs):
        o = c.out(B * T * ci)
        ok(lib().tq_gn_bwd_apply(p(gi), p(m[1]), None, p(A), p(Bc), p(Cc), p(o), B, T, ci, C, off, 0, stream()))
        dx.append(o)
        off += ci
    c.verify()
    for o in (gs, gh, mr, A, Bc, Cc, gst, *g, *dx):
        assert not np.isnan(host(o, -1)).any(), "an output of the chain was left unwritten"
    gw = [host(gi, B, T, ci) for gi, ci in zip(g, cs)]
    f = R.fold(xw, gamma, beta)
    bk = R.backward(xw, gw, gamma, f["mean"], f["rstd"])
    em = R.emulate(xw, gw, gamma, beta)
    x, gcat = np.concatenate(xw, axis=2), np.concatenate(gw, axis=2)
    y_ref = f["scale"][:, None] * x + f["shift"][:, None]
    dx_ref = np.concatenate(bk["dx"], axis=2)
    dx_k = np.concatenate([host(o, B, T, ci) for o, ci in zip(dx, cs)], axis=2)
    terms = np.abs(bk["A"][:, None] * gcat) + np.abs(bk["Bc"][:, None] * x) + np.abs(bk["Cc"][:, None])
    meas = dict(fwd=R.rel_max(host(gs, B, C)[:, None] * x + host(gh, B, C)[:, None], y_ref), dx=R.rel_max(dx_k, dx_ref),
                dgamma=R.rel_max(host(dg, C), bk["dgamma"]), dbeta=R.rel_max(host(db, C), bk["dbeta"]))
    emu = dict(fwd=R.rel_max(em["scale"][:, None] * x + em["shift"][:, None], y_ref), dx=R.rel_max(np.concatenate(em["dx"], axis=2), dx_ref),
               dgamma=R.rel_max(em["dgamma"], bk["dgamma"]), dbeta=R.rel_max(em["dbeta"], bk["dbeta"]))
    # rounding floor of the fp32 outputs (the derived bars of (c) and (d), and one rounding of each of gscale and gshift)
    top = lambda v: max(float(np.abs(v).max()), 1e-300)
    floor = dict(fwd=U * top(np.abs(f["scale"][:, None] * x) + np.abs(f["shift"][:, None])) / top(y_ref),
                 dx=4 * U * top(terms) / top(dx_ref),
                 dgamma=(B + 2) * U * top(np.abs(bk["dgamma_b"]).sum(0)) / top(bk["dgamma"]),
                 dbeta=(B + 2) * U * top(np.abs(bk["dbeta_b"]).sum(0)) / top(bk["dbeta"]))
    return meas, emu, floor, dict(dx=dx_k, Ag=float(np.abs(bk["A"][:, None] * gcat).max()))


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("kind", ["nearest_up2", "identity_conv"])
@pytest.mark.parametrize("shape", CHAIN_SHAPES)
def test_chain_under_mean_std_regimes(shape, kind, ratio):
    """nearest_up2 writes even lengths only: its T = 1153 case runs at 1154 (577 rows, doubled)"""
    C0, C1, T, wfmt = CHAIN_SHAPES[shape]
    cs = (C0, C1) if C1 else (C0,)
    seed = 1000 * ratio + T + C0 + C1
    if kind == "nearest_up2":
        xs, _, gamma, beta = R.regime_input(2, (T + 1) // 2, cs, float(ratio), seed)
        xs = [np.repeat(x, 2, axis=1) for x in xs]
        T = xs[0].shape[1]
    else:
        xs, _, gamma, beta = R.regime_input(2, T, cs, float(ratio), seed)
    meas, emu, floor, _ = run_chain(kind, cs, T, wfmt, xs, gamma, beta, seed)
    print(f"chain {shape} {kind} T {T} ratio {ratio}: " +
          "  ".join(f"{k} {meas[k]:.2e} (emulation {emu[k]:.2e}, floor {floor[k]:.1e})" for k in meas))
    for k in meas:
        assert meas[k] <= 8 * emu[k] + floor[k], f"{k}: {meas[k]:.3e} > 8 x {emu[k]:.3e} + {floor[k]:.1e}"
        if ratio <= 10:
            assert meas[k] <= 1e-3, f"{k}: {meas[k]:.3e} at ratio {ratio}"


def test_chain_group_of_one_element():
    """C = 32, T = 1: every group is one number, the normalised value is beta whatever x is, and dx is exactly zero"""
    rng = rng_of(1, 32)
    x = [randn(rng, 2, 1, 32)]
    gamma, beta = randn(rng, 32), randn(rng, 32)
    meas, emu, floor, more = run_chain("identity_conv", (32,), 1, 0, x, gamma, beta, 5)
    worst = float(np.abs(more["dx"]).max())
    print(f"chain group of one: max|dx| {worst:.2e}, max|A g| {more['Ag']:.2e}; fwd {meas['fwd']:.1e} dbeta {meas['dbeta']:.1e}")
    assert worst <= 8 * U * more["Ag"]
    for k in ("fwd", "dbeta"):   # (dgamma is exactly zero as well: no scale to hold an error against)
        assert meas[k] <= 8 * emu[k] + floor[k], f"{k}: {meas[k]:.3e} > 8 x {emu[k]:.3e} + {floor[k]:.1e}"


# ============================================================================================================================
# the refusal of TQ_BWD_ACCUM | TQ_BWD_STATS, through ops
# ============================================================================================================================
def test_ops_bwd_data_refuses_accumulate_with_stats():
    from tqdne_amd import ops
    from tqdne_amd._lib import TqError
    d = dev()
    dy, w, x = torch.randn(1, 40, 32, device=d), torch.randn(32, 32, 3, device=d), torch.randn(1, 40, 32, device=d)
    acc = torch.full((1, 40, 32), 7.0, device=d)
    with pytest.raises(TqError, match="conv1d_bwd_data failed with TQ_ERR_ARG"):
        ops.conv1d_bwd_data(dy, w, x0=x, stats=True, accumulate_into=(acc, None))
    torch.cuda.synchronize()
    assert bool((acc == 7.0).all()), "the refused call wrote"
    g0, _, _ = ops.conv1d_bwd_data(dy, w, accumulate_into=(acc, None))   # (each flag alone is served)
    _, _, st = ops.conv1d_bwd_data(dy, w, x0=x, stats=True)
    torch.cuda.synchronize()
    assert not bool((g0 == 7.0).all()) and bool(torch.isfinite(st).all())
