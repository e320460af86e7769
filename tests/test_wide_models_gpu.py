"""1-D UNets wider than the paper's on the GPU: tensors up to 1024 channels, up to 2048 concatenated channels into a conv, qkv
projections up to 3072 output channels.

Kernel level: the chunked column sums (tq_colsum / tq_gn_bwd_apply_colsum over more than 1024 channels) against fp64 sums; the forward
convs with the wide GroupNorm coefficient table (conv1d_fwd_wide*.hip) against an fp64 convolution, in both contraction schemes, and
bit for bit against the established kernels on narrow shapes; data and weight gradients at these widths against fp64 autograd.
Whole models ("paper x2": the paper architecture at model_channels = 128; "w1024": channel_mult (1, 2, 4, 8) at model_channels = 128,
k = 3) against the CPU oracle and its autograd.

Bars are the suite's: sums 1e-5 and forward convs 1e-4 (tests/test_hip_ops.py), conv gradients 2e-4 (tests/test_hip_bwd.py), whole path
1e-3 norm-wise and element-wise with conftest's grad_err / GRAD_OWN_TOL for gradients (tests/test_hip_unet.py).

Signal lengths of the whole-model tests: 512 and 504.  Both models down-sample three times, so a length must be a multiple of 8 -- at
T = 500 the reference itself fails in its skip concatenation (125 -> 63 -> 126 positions), which test_length_500_is_refused_like_the_
reference pins; 504 is the nearest length that is ragged against the 128- and 32-position tiles on every level (504, 252, 126, 63)."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import grad_err, rel_err
from test_head_sizes_gpu import cl, dev, guarded, ncw, perturbed_state
from test_wide_models_host import wide_cfg

pytestmark = pytest.mark.gpu

TOL_SUM, TOL_FWD, TOL_BWD, TOL_PATH = 1e-5, 1e-4, 2e-4, 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- column sums ---------------------------------------------------------------------------------------------------------------------

def _zeros_guarded(*shape):
    t, chk = guarded(*shape)
    t.zero_()
    return t, chk


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [64, 130, 4096])
@pytest.mark.parametrize("C", [1028, 1152, 1536, 2048, 3072])
def test_colsum_beyond_1024_channels_vs_fp64(C, T, B):
    """all four outputs of tq_colsum -- per-sample sums (scaled per sample), total sums, the second total, the max|.| block -- on a
    tensor wider than one float4 column per thread; sentinel-guarded destinations"""
    from tqdne_amd import _lib, ops
    g = torch.Generator().manual_seed(C + T + B)
    dy = torch.randn(B, T, C, generator=g) + 0.25
    dy[B - 1, T // 2, C - 2] = -37.5   # the maximum sits in the last chunk
    sc = torch.rand(B, generator=g) + 0.5
    obc, c0 = _zeros_guarded(B, C)
    oc, c1 = _zeros_guarded(C)
    oc2, c2 = _zeros_guarded(C)
    oc2.fill_(1.0)   # (accumulated into, like a second bias gradient)
    am = torch.zeros(_lib.TQ_AMAX_WORDS, dtype=torch.int32, device=dev())
    ops.colsum(dy.to(dev()), bscale=sc.to(dev()), amax=am, out=(obc, oc, oc2))
    torch.cuda.synchronize()
    c0(), c1(), c2()
    ref = dy.double().sum(1) * sc.double()[:, None]
    e = (rel_err(obc.cpu(), ref), rel_err(oc.cpu(), ref.sum(0)), rel_err(oc2.cpu(), ref.sum(0) + 1.0))
    print(f"colsum C={C} T={T} B={B}: per-sample {e[0]:.2e} total {e[1]:.2e} second total {e[2]:.2e}")
    assert max(e) < TOL_SUM
    assert ops.amax_value(am) == 37.5


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [64, 130, 4096])
@pytest.mark.parametrize("C", [1028, 1152, 1536, 2048, 3072])
def test_gn_bwd_apply_colsum_beyond_1024_channels_vs_fp64(C, T, B):
    """tq_gn_bwd_apply_colsum on a source wider than 1024 channels (a slice of a still wider GroupNorm): dx bit-identical to
    tq_gn_bwd_apply, its column sums vs fp64, exact maximum"""
    from tqdne_amd import _lib, ops
    g = torch.Generator().manual_seed(3 * C + T + B)
    d = dev()
    Ct, off = C + 64, 32
    G, x, r = (torch.randn(B, T, C, generator=g).to(d) for _ in range(3))
    coefs = tuple(torch.randn(B, Ct, generator=g).to(d) for _ in range(3))
    ref = ops.gn_bwd_apply(G, x, coefs, Ct, c_offset=off, r=r)
    dx, c0 = guarded(B, T, C)
    obc, c1 = _zeros_guarded(B, C)
    oc, c2 = _zeros_guarded(C)
    oc2, c3 = _zeros_guarded(C)
    am = torch.zeros(_lib.TQ_AMAX_WORDS, dtype=torch.int32, device=d)
    ops.gn_bwd_apply_colsum(G, x, coefs, Ct, c_offset=off, r=r, amax=am, out=(dx, obc, oc, oc2))
    torch.cuda.synchronize()
    c0(), c1(), c2(), c3()
    assert torch.equal(dx, ref)
    s = ref.double().sum(1).cpu()
    e = (rel_err(obc.cpu(), s), rel_err(oc.cpu(), s.sum(0)), rel_err(oc2.cpu(), s.sum(0)))
    print(f"gn_bwd_apply+colsum C={C} T={T} B={B}: per-sample {e[0]:.2e} total {e[1]:.2e} second total {e[2]:.2e}")
    assert max(e) < TOL_SUM
    assert ops.amax_value(am) == float(ref.abs().max())
    # accumulate form
    base = torch.randn(B, T, C, generator=g).to(d)
    ref2 = ops.gn_bwd_apply(G, x, coefs, Ct, c_offset=off, accumulate_into=base.clone())
    dx2, obc2, _ = ops.gn_bwd_apply_colsum(G, x, coefs, Ct, c_offset=off, accumulate_into=base.clone(), total=False)
    assert torch.equal(dx2, ref2) and rel_err(obc2.cpu(), ref2.double().sum(1).cpu()) < TOL_SUM


@pytest.mark.parametrize("C,chunk", [(256, 64), (1024, 256), (1024, 512), (1536, 768), (3072, 1024), (1028, 516)])
@pytest.mark.parametrize("T,B", [(130, 3), (4096, 1)])
def test_colsum_equals_a_chunk_by_chunk_call(C, chunk, T, B):
    """one call over C channels against one call per column slice (made contiguous): torch.equal.  The sums are accumulated with float
    atomics in an order that differs from run to run, so bit equality is only defined where every partial sum is exact: the data are
    multiples of 1/64 with |v| <= 16, and 3 x 4096 of them add up below 2^24 / 64 -- any association order gives the same bits.  What
    this pins is the indexing: every column, chunk offset and destination of the chunked launch (C > 1024) and of the established one."""
    from tqdne_amd import _lib, ops
    g = torch.Generator().manual_seed(C + chunk + T)
    dy = (torch.randint(-1024, 1025, (B, T, C), generator=g).float() / 64).to(dev())
    am = torch.zeros(_lib.TQ_AMAX_WORDS, dtype=torch.int32, device=dev())
    obc, oc = ops.colsum(dy, amax=am)
    parts = []
    for c0 in range(0, C, chunk):
        parts.append(ops.colsum(dy[:, :, c0:c0 + chunk].contiguous()))
    assert torch.equal(obc, torch.cat([p[0] for p in parts], 1)) and torch.equal(oc, torch.cat([p[1] for p in parts]))
    assert torch.equal(obc.double(), dy.double().sum(1)) and ops.amax_value(am) == float(dy.abs().max())


# ---- forward convs with the wide coefficient table ---------------------------------------------------------------------------------------

def ref_stats(y_nct, slot=128):
    B, C, T = y_nct.shape
    ns = (T + slot - 1) // slot
    out = torch.zeros(B, ns, C, 2, dtype=torch.float64)
    for s in range(ns):
        seg = y_nct[:, :, s * slot:(s + 1) * slot].double()
        out[:, s, :, 0] = seg.sum(-1)
        out[:, s, :, 1] = (seg * seg).sum(-1)
    return out


def _conv_case(C0, C1, Co, k, T, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    cin = C0 + C1
    x0 = torch.randn(B, C0, T, generator=g) * 1.5
    x1 = torch.randn(B, C1, T, generator=g) + 0.5 if C1 else None
    a, sh = torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g)
    w = torch.randn(Co, cin, k, generator=g) / math.sqrt(cin * k)
    b, emb, res = torch.randn(Co, generator=g), torch.randn(B, Co, generator=g), torch.randn(B, Co, T, generator=g)
    xin = (torch.cat([x0, x1], 1) if C1 else x0).double()
    ref = F.conv1d(F.silu(xin * a.double()[:, :, None] + sh.double()[:, :, None]), w.double(), b.double(), padding=k // 2)
    return x0, x1, a, sh, w, b, emb, res, ref + emb.double()[:, :, None]


WIDE_SOURCES = [(768, 512), (1024, 512), (1024, 1024), (2048, 0)]


@pytest.mark.parametrize("wfmt", [0, 2])
@pytest.mark.parametrize("k,t_tile", [(1, 0), (3, 0), (5, 0), (5, 32)])
@pytest.mark.parametrize("C0,C1,Co", [s + (256,) for s in WIDE_SOURCES] + [(1024, 512, 128), (1024, 1024, 1024)])
def test_wide_conv_vs_fp64(C0, C1, Co, k, t_tile, wfmt):
    """GroupNorm + SiLU prologue, embedding and residual epilogue, statistics, ragged T, over more than 1024 concatenated channels: the
    wide-table fp16 + MX-fp6 tiles (256- and 128-channel tile, small tile) and bf16x3 against an fp64 convolution"""
    from tqdne_amd import ops
    T = 200 if t_tile == 0 else 77
    x0, x1, a, sh, w, b, emb, res, ref = _conv_case(C0, C1, Co, k, T, C0 + C1 + Co + k + t_tile)
    ref = ref + res.double()
    d = dev()
    y, cy = guarded(2, T, Co)
    st, cs = guarded(2, (T + 31) // 32 if t_tile else (T + 127) // 128, Co, 2)
    ops.conv1d(cl(x0), w.to(d), b.to(d), x1=cl(x1) if C1 else None, gscale=a.to(d), gshift=sh.to(d), silu=True, emb=emb.to(d),
               residual=cl(res), wfmt=wfmt, t_tile=t_tile, out=(y, st))
    torch.cuda.synchronize()
    cy(), cs()
    e, es = rel_err(ncw(y), ref), rel_err(st.cpu(), ref_stats(ref, 32 if t_tile else 128))
    print(f"wide conv {C0}+{C1} -> {Co} k{k} t_tile={t_tile} wfmt={wfmt}: {e:.2e} (statistics {es:.2e})")
    assert e < TOL_FWD and es < TOL_FWD


@pytest.mark.parametrize("wfmt", [0, 2])
@pytest.mark.parametrize("p,Cm,skip", [(0.0, 1024, (1024, 1024)), (0.0, 1536, (1024, 512)), (0.2, 1536, (1024, 512))])
def test_wide_conv_with_the_fused_skip_conv(Cm, skip, p, wfmt):
    """ResBlock tail in one launch at width: conv5(SiLU(GN(h))) + emb + 1x1 conv of the concatenated 2048- / 1536-channel block input
    (what the output blocks of "w1024"-like models with k = 5 run), and the same with more than 1024 channels under the prologue
    (wide table + fused skip stages; with dropout against the two-launch form of the same seed)"""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(Cm + sum(skip) + int(10 * p))
    B, Co, T = 2, 1024, 150
    h = torch.randn(B, Cm, T, generator=g)
    s0, s1 = torch.randn(B, skip[0], T, generator=g), torch.randn(B, skip[1], T, generator=g) + 0.5
    a, sh = torch.rand(B, Cm, generator=g) + 0.5, torch.randn(B, Cm, generator=g)
    w = torch.randn(Co, Cm, 5, generator=g) / math.sqrt(5 * Cm)
    wsk = torch.randn(Co, sum(skip), 1, generator=g) / math.sqrt(sum(skip))
    b, bsk, emb = torch.randn(Co, generator=g), torch.randn(Co, generator=g), torch.randn(B, Co, generator=g)
    d = dev()
    kw = dict(gscale=a.to(d), gshift=sh.to(d), silu=True, emb=emb.to(d), dropout_p=p, dropout_seed=11, dropout_site=3, wfmt=wfmt)
    y, cy = guarded(B, T, Co)
    st, cs = guarded(B, 2, Co, 2)
    ops.conv1d(cl(h), w.to(d), b.to(d), skip=(cl(s0), cl(s1), wsk.to(d), bsk.to(d)), out=(y, st), **kw)
    torch.cuda.synchronize()
    cy(), cs()
    sx = torch.cat([s0, s1], 1)
    if p == 0.0:
        ref = (F.conv1d(F.silu(h.double() * a.double()[:, :, None] + sh.double()[:, :, None]), w.double(), b.double(), padding=2)
               + emb.double()[:, :, None] + F.conv1d(sx.double(), wsk.double(), bsk.double()))
    else:
        res = ops.conv1d(cl(sx), wsk.to(d), bsk.to(d), stats=False, wfmt=0)[0]
        ref = ncw(ops.conv1d(cl(h), w.to(d), b.to(d), residual=res, **dict(kw, wfmt=0))[0])
    e = rel_err(ncw(y), ref)
    print(f"wide fused skip {Cm} (+ {skip}) -> {Co} p={p} wfmt={wfmt}: {e:.2e}")
    assert e < TOL_FWD and rel_err(st.cpu(), ref_stats(ref.double())) < TOL_FWD


@pytest.mark.parametrize("wfmt", [0, 2])
@pytest.mark.parametrize("k", [3, 5])
def test_upsampling_conv_at_1024_channels(k, wfmt):
    """nearest x2 + conv on a 1024-channel tensor (no prologue: no table), both schemes"""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(k)
    B, Cn, T = 2, 1024, 100
    x = torch.randn(B, Cn, T, generator=g)
    w, b = torch.randn(Cn, Cn, k, generator=g) / math.sqrt(Cn * k), torch.randn(Cn, generator=g)
    y, st = ops.conv1d(cl(x), w.to(dev()), b.to(dev()), upsample=True, wfmt=wfmt)
    ref = F.conv1d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=k // 2)
    e = rel_err(ncw(y), ref)
    print(f"upsample conv 1024 -> 1024 k{k} wfmt={wfmt}: {e:.2e}")
    assert e < TOL_FWD and rel_err(st.cpu(), ref_stats(ref)) < TOL_FWD


@pytest.mark.parametrize("k,t_tile,p,skipc", [(5, 0, 0.0, 0), (5, 32, 0.0, 0), (3, 0, 0.0, 0), (1, 0, 0.0, 0), (5, 0, 0.3, 0), (5, 0, 0.0, 512), (5, 32, 0.2, 256)])
@pytest.mark.parametrize("C0,C1,Co", [(256, 256, 256), (512, 512, 256), (256, 128, 128)])
def test_wide_table_instantiation_is_bit_identical_on_narrow_shapes(C0, C1, Co, k, t_tile, p, skipc):
    """TQ_CONV_WIDE_TABLE forces the 2048-entry-table tile for a launch the established tile takes: y and the statistics are torch.equal
    (the table only changes where a thread finds its coefficients)"""
    from tqdne_amd import _lib, ops
    T = 300 if t_tile == 0 else 100
    x0, x1, a, sh, w, b, emb, res, _ = _conv_case(C0, C1, Co, k, T, C0 + Co + k + t_tile + skipc)
    d = dev()
    kw = dict(x1=cl(x1), gscale=a.to(d), gshift=sh.to(d), silu=True, emb=emb.to(d), wfmt=_lib.TQ_WFMT_F16_MX6, t_tile=t_tile,
              dropout_p=p, dropout_seed=5, dropout_site=2)
    if skipc:
        g = torch.Generator().manual_seed(skipc)
        kw["skip"] = (cl(torch.randn(2, skipc, T, generator=g)), None, (torch.randn(Co, skipc, 1, generator=g) / math.sqrt(skipc)).to(d), b.to(d))
    else:
        kw["residual"] = cl(res)
    y0, st0 = ops.conv1d(cl(x0), w.to(d), b.to(d), **kw)
    y1, st1 = ops.conv1d(cl(x0), w.to(d), b.to(d), wide_table=True, **kw)
    assert torch.isfinite(y0).all() and torch.equal(y0, y1) and torch.equal(st0, st1)


def test_wide_tiles_do_not_fold_and_refuse_what_they_are_not_built_for():
    """the consumer-side GroupNorm fold is not offered on the wide-table tiles (the engine emits tq_gn_finalize for them), a 64-channel
    output has no wide tile, and beyond 2048 concatenated channels the fp16-range scheme refuses while bf16x3 still runs"""
    from tqdne_amd import _lib, ops
    d = dev()
    B, T = 1, 64

    def run(C0, C1, Co, **kw):
        x0, x1 = torch.randn(B, T, C0, device=d), (torch.randn(B, T, C1, device=d) if C1 else None)
        gs, gh = torch.ones(B, C0 + C1, device=d), torch.zeros(B, C0 + C1, device=d)
        return ops.conv1d(x0, torch.randn(Co, C0 + C1, 5, device=d) / 100, None, x1=x1, gscale=gs, gshift=gh, silu=True, **kw)

    st = torch.ones(B, 2, 1024, 2, device=d)
    gam = torch.ones(2048, device=d)
    fold = (st, st, 32, 32, gam, gam, None)
    for t_tile in (32, 0):
        with pytest.raises(_lib.TqError, match="TQ_ERR_SHAPE"):
            run(1024, 1024, 128, wfmt=2, t_tile=t_tile, gn_fold=fold)
    with pytest.raises(_lib.TqError, match="TQ_ERR_SHAPE"):
        run(1024, 1024, 64, wfmt=2)
    with pytest.raises(_lib.TqError, match="TQ_ERR_SHAPE"):
        run(1024, 1088, 128, wfmt=2)
    y, _ = run(1024, 1088, 128, wfmt=0)
    assert torch.isfinite(y).all()


# ---- gradients at these widths ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wfmt", [0, 2])
@pytest.mark.parametrize("Cin,Cout,k,split", [(512, 1536, 1, None), (1024, 3072, 1, None), (2048, 1024, 3, 1024), (2048, 1024, 5, 1024),
                                              (1024, 1024, 5, None), (1536, 512, 5, 1024)])
def test_data_gradient_at_width_vs_fp64(Cin, Cout, k, split, wfmt):
    """plain, and through the forward prologue (GroupNorm for the qkv projections, GroupNorm + SiLU for the ResBlock convs) with the
    GroupNorm-backward sums and the split over two destinations; contraction over up to 3072 channels of dy; both schemes (dy at
    gradient scale)"""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(Cin + Cout + k)
    B, T = 2, 130
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)
    dy = torch.randn(B, Cout, T, generator=g) * 1e-4
    x = torch.randn(B, Cin, T, generator=g) + 0.3
    a, sh = torch.randn(B, Cin, generator=g), torch.randn(B, Cin, generator=g)
    silu = k != 1
    u = (x * a[:, :, None] + sh[:, :, None]).double().requires_grad_(True)
    F.conv1d(F.silu(u) if silu else u, w.double(), None, padding=k // 2).backward(dy.double())
    ref_plain = F.conv_transpose1d(dy.double(), w.double(), padding=k // 2)
    d = dev()
    C0 = split or Cin
    g0, c0 = guarded(B, T, C0)
    g1, c1 = guarded(B, T, Cin - C0) if split else (None, lambda: None)
    g0.zero_()
    if g1 is not None:
        g1.zero_()
    ops.conv1d_bwd_data(cl(dy), w.to(d), split=split, wfmt=wfmt, accumulate_into=(g0, g1))   # (accumulate into zeros: caller-owned buffers)
    torch.cuda.synchronize()
    c0(), c1()
    got = torch.cat([ncw(g0), ncw(g1)], 1) if split else ncw(g0)
    e_plain = rel_err(got, ref_plain)
    xs = (cl(x[:, :C0]), cl(x[:, C0:]) if split else None)
    h0, h1, st = ops.conv1d_bwd_data(cl(dy), w.to(d), x0=xs[0], x1=xs[1], gscale=a.to(d), gshift=sh.to(d), silu=silu, stats=True,
                                     split=split, wfmt=wfmt)
    got = torch.cat([ncw(h0), ncw(h1)], 1) if split else ncw(h0)
    e_chain = rel_err(got, u.grad)
    from test_hip_bwd import ref_slot_sums
    e_st = rel_err(st.cpu(), ref_slot_sums(u.grad.float(), x))
    print(f"dgrad {Cout} -> {Cin} k{k} split={split} wfmt={wfmt}: plain {e_plain:.2e} chain {e_chain:.2e} GN sums {e_st:.2e}")
    assert e_plain < TOL_BWD and e_chain < TOL_BWD and e_st < TOL_BWD


@pytest.mark.parametrize("B,T", [(2, 130), (3, 512)])
@pytest.mark.parametrize("Cin,Cout,k,split", [(512, 1536, 1, None), (1024, 3072, 1, None), (2048, 1024, 3, 1024), (2048, 1024, 5, 1024),
                                              (1024, 1024, 5, None)])
def test_weight_gradient_at_width_vs_fp64(Cin, Cout, k, split, B, T):
    """the weight-gradient plan, its workspace and the split reduction at these widths, with the forward prologue recomputed"""
    from tqdne_amd import ops
    if (B, T) == (3, 512) and Cin * Cout * k > 2048 * 1024 * 3:
        T = 256   # (keeps the fp64 reference of the widest k = 5 shape within a few seconds)
    g = torch.Generator().manual_seed(Cin + Cout + k + T)
    x = torch.randn(B, Cin, T, generator=g)
    a, sh = torch.randn(B, Cin, generator=g), torch.randn(B, Cin, generator=g)
    w = (torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)).double().requires_grad_(True)
    dy = torch.randn(B, Cout, T, generator=g)
    silu = k != 1
    u = x.double() * a.double()[:, :, None] + sh.double()[:, :, None]
    F.conv1d(F.silu(u) if silu else u, w, None, padding=k // 2).backward(dy.double())
    d = dev()
    C0 = split or Cin
    dw, chk = guarded(Cout, Cin, k)
    ops.conv1d_bwd_weight(cl(dy), cl(x[:, :C0]), (Cout, Cin, k), x1=cl(x[:, C0:]) if split else None, gscale=a.to(d), gshift=sh.to(d),
                          silu=silu, out=dw)
    torch.cuda.synchronize()
    chk()
    e = rel_err(dw.cpu(), w.grad)
    print(f"wgrad {Cin} -> {Cout} k{k} B={B} T={T}: {e:.2e}")
    assert e < TOL_BWD


# ---- whole models --------------------------------------------------------------------------------------------------------------------------

_MODELS = {}


def wide_model(which):
    """(cfg, perturbed state dict) -- built once per session"""
    if which not in _MODELS:
        from tqdne_amd import UNetModel
        cfg = wide_cfg(which)
        torch.manual_seed(0)
        _MODELS[which] = (cfg, perturbed_state(UNetModel(**cfg), 61))
    return _MODELS[which]


def _batch(B, T, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, T, generator=g), torch.randn(B, generator=g) * 0.5


_ORACLE = {}


def oracle_module_grads(which, T):
    """oracle forward and autograd of y.square().mean() w.r.t. every parameter and the input"""
    if (which, T) not in _ORACLE:
        from oracle import unet as OU
        cfg, sd = wide_model(which)
        x, t = _batch(2, T)
        params = {k: v.clone().requires_grad_(k != "time_embed.W") for k, v in sd.items()}
        xr = x.clone().requires_grad_(True)
        y = OU.unet_forward(params, cfg, xr, t, None)
        y.square().mean().backward()
        _ORACLE[(which, T)] = (y.detach(), {k: v.grad for k, v in params.items()}, xr.grad)
    return _ORACLE[(which, T)]


def _module_backward(which, T, ckpt=False):
    from tqdne_amd import UNetModel
    cfg, sd = wide_model(which)
    m = UNetModel(**dict(cfg, use_checkpoint=ckpt))
    m.load_state_dict(sd)
    m = m.to(dev()).train()
    x, t = _batch(2, T)
    xg = x.to(dev()).requires_grad_(True)
    y = m(xg, t.to(dev()), None)
    y.square().mean().backward()
    return m, y.detach().cpu(), xg.grad.cpu()


@pytest.mark.parametrize("T", [512, 504])
@pytest.mark.parametrize("which", ["paper_x2", "w1024"])
def test_forward_and_every_gradient_vs_oracle(which, T):
    """training-mode forward (dropout 0), then ALL parameter gradients and x.grad of y.square().mean() vs oracle autograd; the plan of
    "w1024" must hold wide-table launches in the fp16-range format (or bf16x3 when that scheme is requested)"""
    from tqdne_amd import _lib
    yo, gref, xref = oracle_module_grads(which, T)
    m, y, xgrad = _module_backward(which, T)
    e = rel_err(y, yo)
    gmax = max(float(v.abs().max()) for v in gref.values() if v is not None)
    worst, wname, n = 0.0, "", 0
    for name, p in m.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None, name
        ge = grad_err(p.grad, gref[name], gmax, name)
        n += 1
        if ge > worst:
            worst, wname = ge, name
    ex = rel_err(xgrad, xref)
    print(f"{which} T={T}: forward {e:.2e}; worst of {n} parameter gradients {worst:.2e} at {wname}; x.grad {ex:.2e}")
    assert e < TOL_PATH and worst < TOL_PATH and ex < TOL_PATH
    eng = m._engine(2, T, dev())
    wide = [d for d, _sites, _w in eng._wfmt_sites if d.C_in0 + d.C_in1 > 1024 and (d.flags & _lib.TQ_CONV_GN)]
    assert bool(wide) == (which == "w1024")
    if _lib.requested_scheme() == "f16mx6" and _lib.WIDE_MX6 and eng.scheme == "auto":
        assert all(d.wfmt == _lib.TQ_WFMT_F16_MX6 for d in wide if d.C_out % 128 == 0)
    assert not any(d.gn_fold for d in wide)


@pytest.mark.parametrize("which", ["paper_x2", "w1024"])
def test_checkpointed_plan_gives_the_gradients_of_the_plain_plan(which):
    """use_checkpoint=True re-runs each block's forward inside the backward: same kernels on the same data, so the gradients agree with
    the plain plan's to the rounding of the atomically accumulated sums (1e-5 of each tensor's largest entry), and hold the oracle's bar"""
    T = 512
    _, gref, xref = oracle_module_grads(which, T)
    m0, y0, x0 = _module_backward(which, T)
    m1, y1, x1 = _module_backward(which, T, ckpt=True)
    assert m1._engine(2, T, dev()).ckpt and not m0._engine(2, T, dev()).ckpt
    assert torch.equal(y0, y1)
    gmax = max(float(v.abs().max()) for v in gref.values() if v is not None)
    p0 = dict(m0.named_parameters())
    worst = 0.0
    for name, p in m1.named_parameters():
        if not p.requires_grad:
            continue
        a, b = p.grad.double().cpu(), p0[name].grad.double().cpu()
        worst = max(worst, float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)))
        assert grad_err(p.grad, gref[name], gmax, name) < TOL_PATH
    print(f"{which}: checkpointed vs plain plan, worst parameter gradient difference {worst:.2e}")
    assert worst < 1e-5 and rel_err(x1, x0) < 1e-5 and rel_err(x1, xref) < TOL_PATH


def _edm(which, steps=3):
    from tqdne_amd import LightningEDM
    cfg, sd = wide_model(which)
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}, num_sampling_steps=steps)
    edm.unet.load_state_dict(sd)
    return edm, cfg, sd


@pytest.mark.parametrize("which", ["paper_x2", "w1024"])
def test_edm_training_step_loss_vs_oracle(which):
    from oracle import edm as OE
    edm, cfg, sd = _edm(which)
    edm = edm.to(dev()).train()
    B, T = 2, 512
    g = torch.Generator().manual_seed(77)
    sig, eps, noise = 0.5 * torch.randn(B, 3, T, generator=g), torch.randn(B, generator=g), torch.randn(B, 3, T, generator=g)
    with torch.no_grad():
        lo = OE.loss_step(OE.EDMParams(), OE.make_net({("unet." + k): v for k, v in sd.items()}, cfg), sig, eps, noise, cond=None)
    loss = edm.step_with_noise(sig.to(dev()), eps.to(dev()), noise.to(dev()), cond=None)
    loss.backward()
    e = rel_err(loss.detach().cpu(), lo)
    print(f"{which}: EDM loss {float(loss.detach()):.6f} vs oracle {float(lo):.6f} ({e:.2e})")
    assert e < TOL_PATH
    assert all(torch.isfinite(p.grad).all() for p in edm.unet.parameters() if p.requires_grad)


@pytest.mark.parametrize("which", ["paper_x2", "w1024"])
def test_heun_sampler_3_steps_vs_oracle(which):
    from oracle import edm as OE
    edm, cfg, sd = _edm(which, 3)
    edm = edm.to(dev()).eval()
    g = torch.Generator().manual_seed(3)
    B, T = 2, 512
    start = torch.randn(B, 3, T, generator=g, dtype=torch.float64)
    sig = OE.sampling_sigmas(OE.EDMParams(), 3)
    out = edm.sample_deterministically((start * sig[0]).to(dev()), sig.to(dev()), None, None)
    with torch.no_grad():
        ref = OE.sample_deterministic(OE.EDMParams(), OE.make_net({("unet." + k): v for k, v in sd.items()}, cfg), start, 3, cond=None)
    e = rel_err(out.cpu(), ref)
    print(f"{which}: 3-step Heun sample (5 NFE): {e:.2e}")
    assert e < TOL_PATH


@pytest.mark.parametrize("which", ["paper_x2", "w1024"])
def test_forward_under_the_bf16x3_scheme_in_a_child_process(which, tmp_path):
    """TQDNE_CONV_SCHEME=bf16x3 is read once per process: the same eval forward there, against the oracle output computed here"""
    from oracle import unet as OU
    cfg, sd = wide_model(which)
    B, T = 2, 512
    x, t = _batch(B, T)
    with torch.no_grad():
        yo = OU.unet_forward(sd, cfg, x, t, None)
    f = tmp_path / "case.pt"
    torch.save({"cfg": cfg, "sd": sd, "x": x, "t": t, "y": yo}, f)
    code = r'''
import sys, torch
sys.path.insert(0, %r)
from tqdne_amd import UNetModel, _lib
z = torch.load(%r)
dev = torch.device("cuda:0")
m = UNetModel(**z["cfg"]); m.load_state_dict(z["sd"]); m = m.to(dev).eval()
with torch.no_grad():
    y = m(z["x"].to(dev), z["t"].to(dev), None).cpu().double()
eng = m._engine(2, z["x"].shape[2], dev)
assert all(d.wfmt == _lib.TQ_WFMT_BF16X3 for d, _s, _w in eng._wfmt_sites)
ref = z["y"].double()
e = float((y - ref).abs().max() / ref.abs().max())
ee = float(((y - ref).abs() / (ref.abs() + ref.pow(2).mean().sqrt())).max())
print("rel err", e, "element-wise", ee)
assert e < 1e-3 and ee <= 1e-3, (e, ee)
print("OK")
''' % (ROOT, str(f))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TQDNE_CONV_SCHEME="bf16x3"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:]


def test_length_500_is_refused_like_the_reference():
    """three stride-2 levels: 500 -> 250 -> 125 -> 63 positions, and 2 x 63 does not meet the 125 of the skip tensor (the reference
    raises in th.cat, unet.py:396); the plan says so when it is built"""
    from tqdne_amd import UNetModel
    cfg, sd = wide_model("paper_x2")
    m = UNetModel(**cfg).to(dev()).eval()
    x, t = _batch(1, 500)
    with pytest.raises(RuntimeError, match="Sizes of tensors must match"):
        with torch.no_grad():
            m(x.to(dev()), t.to(dev()), None)


def test_head_size_96_on_384_channels_gradients_vs_oracle():
    """the case the head-size change had to leave out (tests/test_head_sizes_gpu.py, ``wide_h96``): the qkv projection's output gradient
    has 3 x 384 = 1152 channels, one more chunk than tq_colsum used to take"""
    from test_head_sizes_gpu import _name, oracle_grads
    from tqdne_amd import LightningEDM
    B, T = 2, 512
    cfg, sd, (sig, eps, noise, cond), lo, ref = oracle_grads("wide_h96", B, T)
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0})
    edm.unet.load_state_dict(sd)
    edm = edm.to(dev()).train()
    loss = edm.step_with_noise(sig.to(dev()), eps.to(dev()), noise.to(dev()), cond=cond.to(dev()) if cond is not None else None)
    loss.backward()
    assert rel_err(loss.detach().cpu(), lo) < TOL_PATH
    eng = edm.unet._engine(B, T, dev())
    assert any(_name(op[0]) == "tq_attention_bwd_hd" for op in eng._bwd.ops)
    assert any(op[2].startswith("colsum:") and "qkv" in op[2] for op in eng._bwd.ops) or any("qkv" in op[2] for op in eng._bwd.ops)
    gmax = max(float(v.abs().max()) for v in ref.values() if v is not None)
    worst, wname = 0.0, ""
    for name, p in edm.unet.named_parameters():
        if not p.requires_grad:
            continue
        e = grad_err(p.grad, ref["unet." + name], gmax, name)
        if e > worst:
            worst, wname = e, name
    print(f"wide_h96: loss {float(loss):.6f}; worst gradient rel err {worst:.2e} at {wname}")
    assert worst < TOL_PATH


def test_a_model_beyond_the_limits_fails_when_its_plan_is_built():
    """1056-channel tensors (11 heads of 96 in the middle block; qkv 3168, 2112 concatenated): NotImplementedError naming the layer at the
    first forward's plan construction, not a launch error out of the middle of it.  The first layer beyond a limit is named: the middle
    block's qkv projection here, the first output block's conv in a model without attention there."""
    from tqdne_amd import UNetModel, tiny_1d_unet_config
    cfg = dict(tiny_1d_unet_config(), model_channels=96, channel_mult=(1, 11), num_res_blocks=1, num_heads=11, dropout=0.0)
    torch.manual_seed(0)
    m = UNetModel(**cfg).to(dev()).eval()
    x, t = _batch(1, 64)
    with pytest.raises(NotImplementedError, match=r"conv middle_block\.1\.qkv: 1056 -> 3168 channels"):
        with torch.no_grad():
            m(x.to(dev()), t.to(dev()), None)
    import tqdne_amd.engine as E
    with pytest.raises(NotImplementedError, match=r"conv output_blocks\.0\.0\.in_layers\.2: 2112 -> 1056 channels"):
        E._check_width_limits("output_blocks.0.0.in_layers.2", 2112, 1056)
