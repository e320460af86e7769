"""Kernel-level parity (GPU): each C-ABI entry point against the same op in plain PyTorch fp32 on the CPU.
Tolerance: the north-star bar is 1e-3 relative; single kernels are held to 1e-4 (bf16x3 products are ~2e-5)."""

import math
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4


def dev():
    return torch.device("cuda:0")


def cl(x):  # (B,C,T) -> channels-last (B,T,C) on device
    return x.permute(0, 2, 1).contiguous().to(dev())


def ncw(y):  # device (B,T,C) -> cpu (B,C,T)
    return y.permute(0, 2, 1).cpu()


def ref_stats(y_nct):
    B, C, T = y_nct.shape
    ns = (T + 127) // 128
    out = torch.zeros(B, ns, C, 2)
    for s in range(ns):
        seg = y_nct[:, :, s * 128:(s + 1) * 128].double()
        out[:, s, :, 0] = seg.sum(-1)
        out[:, s, :, 1] = (seg * seg).sum(-1)
    return out


@pytest.mark.parametrize("cin,cout,k,T", [
    (64, 64, 5, 256), (64, 128, 5, 384), (128, 256, 5, 200), (256, 256, 5, 127), (32, 32, 5, 300),
    (32, 96, 3, 130), (64, 64, 1, 256), (256, 768, 1, 512), (512, 256, 1, 100), (96, 64, 5, 508),
    (64, 64, 5, 64), (32, 32, 5, 62), (64, 32, 3, 31), (128, 64, 5, 129),
])
def test_conv_plain(cin, cout, k, T):
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(cin * 7 + cout + k + T)
    x = torch.randn(2, cin, T, generator=g)
    w = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k)
    b = torch.randn(cout, generator=g)
    y, st = ops.conv1d(cl(x), w.to(dev()), b.to(dev()))
    ref = F.conv1d(x, w, b, padding=k // 2)
    assert rel_err(ncw(y), ref) < TOL
    assert rel_err(st.cpu(), ref_stats(ref)) < TOL


@pytest.mark.parametrize("cin0,cin1,cout,k,T,gn", [
    (128, 0, 128, 5, 300, True), (256, 256, 256, 5, 200, True), (256, 128, 256, 1, 129, False), (64, 64, 256, 3, 260, True),
    (256, 0, 768, 1, 512, True), (512, 0, 128, 5, 64, False),
])
def test_conv_both_contraction_schemes(cin0, cin1, cout, k, T, gn):
    """shapes the fp16 + block-scaled-fp8 scheme serves (128 | C_out, 64 | sources): it and bf16x3 against fp32 PyTorch.
    Tolerance 1e-4 for both (measured: bf16x3 ~1e-5, f16+mx8 ~3e-5)."""
    from tqdne_amd import _lib, ops
    g = torch.Generator().manual_seed(cin0 + cin1 + cout + k + T)
    B = 2
    x0 = torch.randn(B, cin0, T, generator=g) * 1.5
    x1 = torch.randn(B, cin1, T, generator=g) if cin1 else None
    cin = cin0 + cin1
    w = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k)
    b = torch.randn(cout, generator=g)
    a, sh = (torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g)) if gn else (None, None)
    d = dev()
    assert _lib.forward_wfmt(cout, [cin0, cin1]) != _lib.TQ_WFMT_BF16X3 or os.environ.get("TQDNE_CONV_SCHEME") == "bf16x3"
    xin = torch.cat([x0, x1], 1) if cin1 else x0
    if gn:
        xin = F.silu(xin * a[:, :, None] + sh[:, :, None])
    ref = F.conv1d(xin, w, b, padding=k // 2)
    errs = {}
    for wfmt in (_lib.TQ_WFMT_BF16X3, _lib.TQ_WFMT_F16_MX8, _lib.TQ_WFMT_F16_MX6):
        y, st = ops.conv1d(cl(x0), w.to(d), b.to(d), x1=cl(x1) if cin1 else None, gscale=a.to(d) if gn else None,
                           gshift=sh.to(d) if gn else None, silu=gn, wfmt=wfmt)
        errs[wfmt] = rel_err(ncw(y), ref)
        assert errs[wfmt] < TOL, (wfmt, errs)
        assert rel_err(st.cpu(), ref_stats(ref)) < TOL, wfmt
    print("rel err bf16x3 / f16+mx8 / f16+mx6:", " / ".join(f"{errs[k]:.1e}" for k in sorted(errs)))
    # fp16 range of the activation operand: inputs beyond 65504 surface as inf / NaN (loud), NaN inputs stay NaN
    for wfmt in (_lib.TQ_WFMT_F16_MX8, _lib.TQ_WFMT_F16_MX6):
        big = cl(x0 * 1e6)
        y, _ = ops.conv1d(big, w[:, :cin0].contiguous().to(d), b.to(d), wfmt=wfmt, stats=False)
        assert not torch.isfinite(y).all()
        xn = cl(x0).clone()
        xn[0, 5, 3] = float("nan")
        y, _ = ops.conv1d(xn, w[:, :cin0].contiguous().to(d), b.to(d), wfmt=wfmt, stats=False)
        assert torch.isnan(y[0, 5]).any() and torch.isfinite(y[1]).all()


@pytest.mark.parametrize("cin0,cin1,cout,T,gn", [
    (256, 0, 768, 500, True), (128, 128, 512, 129, True), (128, 0, 512, 64, False), (64, 64, 1024, 300, True), (256, 0, 512, 31, False),
])
def test_conv_pointwise_input_stationary(cin0, cin1, cout, T, gn):
    """1x1 convs with several 256-channel output tiles and 128 / 256 input channels run the input-stationary variant (whole input
    tile staged once, the workgroup loops over the channel tiles): GN-only prologue (AttentionBlock.norm, blocks.py:138), two
    sources, embedding + residual epilogue, ragged T, statistics; and the bf16x3 generic path on the same data."""
    from tqdne_amd import _lib, ops
    g = torch.Generator().manual_seed(cin0 + 3 * cin1 + cout + T)
    B = 3
    x0 = torch.randn(B, cin0, T, generator=g) * 2 + 0.5
    x1 = torch.randn(B, cin1, T, generator=g) if cin1 else None
    cin = cin0 + cin1
    w = torch.randn(cout, cin, 1, generator=g) / math.sqrt(cin)
    b, emb, res = torch.randn(cout, generator=g), torch.randn(B, cout, generator=g), torch.randn(B, cout, T, generator=g)
    a, sh = (torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g)) if gn else (None, None)
    d = dev()
    xin = torch.cat([x0, x1], 1) if cin1 else x0
    if gn:
        xin = xin * a[:, :, None] + sh[:, :, None]
    ref = F.conv1d(xin, w, b) + emb[:, :, None] + res
    for wfmt in (_lib.TQ_WFMT_F16_MX8, _lib.TQ_WFMT_BF16X3):
        y, st = ops.conv1d(cl(x0), w.to(d), b.to(d), x1=cl(x1) if cin1 else None, gscale=a.to(d) if gn else None,
                           gshift=sh.to(d) if gn else None, silu=False, emb=emb.to(d), residual=cl(res), wfmt=wfmt)
        assert rel_err(ncw(y), ref) < TOL, wfmt
        assert rel_err(st.cpu(), ref_stats(ref)) < TOL, wfmt


@pytest.mark.parametrize("C0,C1,T,p,res,skip", [(64, 0, 4096, 0.0, True, None), (128, 64, 333, 0.0, False, None), (64, 0, 200, 0.3, True, None),
                                                 (64, 0, 700, 0.0, False, (128, 64)), (64, 0, 129, 0.3, False, (128, 0)), (128, 0, 64, 0.0, False, None)])
def test_conv_64_channel_mx6_tile(C0, C1, T, p, res, skip):
    """round 6: the 64-channel ResBlock convs (k = 5, GN + SiLU [+ dropout] prologue, emb, residual or fused 1x1 skip conv) in the
    fp16 + MX-fp6 scheme on the 64-channel x 128-position tile (2 x 2 waves of 32 x 64; the two position halves of a workgroup share one
    statistics slot through LDS) -- output and statistics vs fp32 PyTorch; with dropout vs the bf16x3 launch of the same seed."""
    from tqdne_amd import _lib, ops
    g = torch.Generator().manual_seed(C0 + C1 + T + int(100 * p))
    B, Co, Cin = 2, 64, C0 + C1
    x0 = torch.randn(B, C0, T, generator=g) * 1.5
    x1 = torch.randn(B, C1, T, generator=g) + 0.5 if C1 else None
    a, sh = torch.rand(B, Cin, generator=g) + 0.5, torch.randn(B, Cin, generator=g)
    w = torch.randn(Co, Cin, 5, generator=g) / math.sqrt(5 * Cin)
    b, emb = torch.randn(Co, generator=g), torch.randn(B, Co, generator=g)
    r = torch.randn(B, Co, T, generator=g) if res else None
    d = dev()
    srcs = [C0, C1] + (list(skip) if skip else [])
    # (the plans select this tile only with TQDNE_CONV_MX6_C64=1 -- measured neutral to slower, _lib.MX6_C64 -- the launch is asked for here)
    kw = dict(x1=cl(x1) if C1 else None, gscale=a.to(d), gshift=sh.to(d), silu=True, emb=emb.to(d), dropout_p=p, dropout_seed=13, dropout_site=5)
    sk = None
    if skip:
        s0 = torch.randn(B, skip[0], T, generator=g)
        s1 = torch.randn(B, skip[1], T, generator=g) if skip[1] else None
        wsk = torch.randn(Co, sum(skip), 1, generator=g) / math.sqrt(sum(skip))
        bsk = torch.randn(Co, generator=g)
        sk = (cl(s0), cl(s1) if skip[1] else None, wsk.to(d), bsk.to(d))
        kw["skip"] = sk
    else:
        kw["residual"] = cl(r) if res else None
    y, st = ops.conv1d(cl(x0), w.to(d), b.to(d), wfmt=_lib.TQ_WFMT_F16_MX6, **kw)
    if p == 0.0:
        xin = F.silu((torch.cat([x0, x1], 1) if C1 else x0) * a[:, :, None] + sh[:, :, None])
        ref = F.conv1d(xin, w, b, padding=2) + emb[:, :, None]
        if res:
            ref = ref + r
        if skip:
            ref = ref + F.conv1d(torch.cat([s0, s1], 1) if skip[1] else s0, wsk, bsk)
    else:   # the mask is the kernel's own counter hash: same seed / site in the three-product scheme
        ref = ncw(ops.conv1d(cl(x0), w.to(d), b.to(d), wfmt=_lib.TQ_WFMT_BF16X3, **kw)[0])
    e = rel_err(ncw(y), ref)
    print(f"64-channel f16+mx6 tile {C0}+{C1} -> 64, T={T}, p={p}, skip={skip}: {e:.2e}")
    assert e < TOL
    assert rel_err(st.cpu(), ref_stats(ref)) < TOL


def test_conv_fused_everything():
    """GN scale/shift + SiLU + two concat sources + emb + residual, ragged T."""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(5)
    B, C0, C1, Co, T = 3, 128, 64, 128, 333
    x0, x1 = torch.randn(B, C0, T, generator=g), torch.randn(B, C1, T, generator=g) * 2 + 1
    a, s = torch.randn(B, C0 + C1, generator=g), torch.randn(B, C0 + C1, generator=g)
    w = torch.randn(Co, C0 + C1, 5, generator=g) / 30
    b, emb = torch.randn(Co, generator=g), torch.randn(B, Co, generator=g)
    res = torch.randn(B, Co, T, generator=g)
    d = dev()
    y, st = ops.conv1d(cl(x0), w.to(d), b.to(d), x1=cl(x1), gscale=a.to(d), gshift=s.to(d), silu=True, emb=emb.to(d),
                       residual=cl(res))
    xin = F.silu(torch.cat([x0, x1], 1) * a[:, :, None] + s[:, :, None])
    ref = F.conv1d(xin, w, b, padding=2) + emb[:, :, None] + res
    assert rel_err(ncw(y), ref) < TOL
    assert rel_err(st.cpu(), ref_stats(ref)) < TOL


@pytest.mark.parametrize("C,Cs0,Cs1,Co,T,p", [
    (128, 64, 0, 128, 333, 0.0), (256, 256, 256, 256, 200, 0.0), (256, 128, 0, 256, 129, 0.0), (128, 128, 64, 128, 700, 0.0),
    (256, 32, 0, 256, 64, 0.0), (128, 96, 32, 128, 257, 0.3),
])
def test_conv_fused_skip(C, Cs0, Cs1, Co, T, p):
    """ResBlock tail in one launch: conv5(SiLU(GN(h))) + emb + 1x1 skip conv of the (concatenated, raw) block input."""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(C + Cs0 + Cs1 + T)
    B = 2
    h = torch.randn(B, C, T, generator=g)
    s0 = torch.randn(B, Cs0, T, generator=g)
    s1 = torch.randn(B, Cs1, T, generator=g) if Cs1 else None
    a, sh = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    w = torch.randn(Co, C, 5, generator=g) / math.sqrt(5 * C)
    wsk = torch.randn(Co, Cs0 + Cs1, 1, generator=g) / math.sqrt(Cs0 + Cs1)
    b, bsk, emb = torch.randn(Co, generator=g), torch.randn(Co, generator=g), torch.randn(B, Co, generator=g)
    d = dev()
    kw = dict(gscale=a.to(d), gshift=sh.to(d), silu=True, emb=emb.to(d), dropout_p=p, dropout_seed=11, dropout_site=3)
    y, st = ops.conv1d(cl(h), w.to(d), b.to(d), skip=(cl(s0), cl(s1) if Cs1 else None, wsk.to(d), bsk.to(d)), **kw)
    sx = torch.cat([s0, s1], 1) if Cs1 else s0
    skip_ref = F.conv1d(sx, wsk, bsk)
    if p == 0.0:
        ref = F.conv1d(F.silu(h * a[:, :, None] + sh[:, :, None]), w, b, padding=2) + emb[:, :, None] + skip_ref
    else:  # the dropout mask is the kernel's own (counter hash): compare with the two-launch form of the same seed / site
        res = ops.conv1d(cl(sx), wsk.to(d), bsk.to(d), stats=False)[0]
        ref = ncw(ops.conv1d(cl(h), w.to(d), b.to(d), residual=res, **kw)[0])
    assert rel_err(ncw(y), ref) < TOL
    assert rel_err(st.cpu(), ref_stats(ref)) < TOL


@pytest.mark.parametrize("C,T", [(64, 256), (128, 250), (32, 131), (256, 508)])
def test_conv_downsample(C, T):
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(C + T)
    x = torch.randn(2, C, T, generator=g)
    w = torch.randn(C, C, 3, generator=g) / math.sqrt(3 * C)
    b = torch.randn(C, generator=g)
    y, st = ops.conv1d(cl(x), w.to(dev()), b.to(dev()), stride=2)
    ref = F.conv1d(x, w, b, stride=2, padding=1)
    assert y.shape[1] == ref.shape[2]
    assert rel_err(ncw(y), ref) < TOL
    assert rel_err(st.cpu(), ref_stats(ref)) < TOL


@pytest.mark.parametrize("C0,C1,Co,T", [(256, 0, 256, 256), (128, 0, 128, 384), (64, 64, 64, 128), (32, 0, 32, 128), (256, 0, 128, 512),
                                        (256, 0, 256, 508), (128, 0, 128, 1016), (64, 0, 64, 252)])   # (ragged: the 4064-sample signals)
def test_conv_upsample_polyphase(C0, C1, Co, T):
    """TQ_CONV_POLY2: nearest x2 upsampling + conv k = 5 (Upsample.forward, blocks.py:56-66) as one two-phase k = 3 conv over the
    un-upsampled rows, through the C ABI: output, and the GroupNorm partial statistics summed over their slots."""
    import ctypes as C_
    from tqdne_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(C0 + C1 + Co + T)
    B, Cin = 2, C0 + C1
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Co, Cin, 5, generator=g) / math.sqrt(5 * Cin)
    b = torch.randn(Co, generator=g)
    ref = F.conv1d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=2)
    w2 = torch.empty(2 * Co, Cin, 3)
    w2[:Co, :, 0], w2[:Co, :, 1], w2[:Co, :, 2] = w[:, :, 0] + w[:, :, 1], w[:, :, 2] + w[:, :, 3], w[:, :, 4]
    w2[Co:, :, 0], w2[Co:, :, 1], w2[Co:, :, 2] = w[:, :, 0], w[:, :, 1] + w[:, :, 2], w[:, :, 3] + w[:, :, 4]
    d = dev()
    x0, x1 = cl(x[:, :C0]), (cl(x[:, C0:]) if C1 else None)
    for wfmt in {_lib.forward_wfmt(2 * Co, [C0, C1]), _lib.TQ_WFMT_BF16X3}:
        wp = ops.pack_conv_weight(w2.to(d), _lib.PACK_MODE[wfmt])
        y = torch.full((B, 2 * T, Co), float("nan"), device=d)
        st = torch.full((B, (2 * T + 127) // 128, Co, 2), float("nan"), device=d)
        desc = _lib.TqConvDesc()
        desc.B, desc.T_in, desc.T_out, desc.C_in0, desc.C_in1, desc.C_out = B, T, T, C0, C1, 2 * Co
        desc.ktaps, desc.stride, desc.pad, desc.upsample = 3, 1, 1, 0
        desc.flags, desc.wfmt = _lib.TQ_CONV_STATS | _lib.TQ_CONV_POLY2, wfmt
        bd = b.to(d)
        p = lambda t: None if t is None else t.data_ptr()
        rc = lib.tq_conv1d_fwd(C_.byref(desc), p(x0), p(x1), None, None, p(wp), p(bd), None, None, p(y), p(st),
                               torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        assert rel_err(ncw(y), ref) < TOL, wfmt
        tot = st.cpu().double().sum(1)
        assert rel_err(tot[..., 0].float(), ref.double().sum(-1).float()) < TOL
        assert rel_err(tot[..., 1].float(), (ref.double() ** 2).sum(-1).float()) < TOL
    desc.T_in = desc.T_out = T // 128 * 128 + 64  # a last tile of <= 64 rows: one statistics slot more than the tensor has
    assert lib.tq_conv1d_fwd(C_.byref(desc), p(x0), p(x1), None, None, p(wp), p(bd), None, None, p(y), p(st),
                             torch.cuda.current_stream().cuda_stream) == -2  # TQ_ERR_SHAPE


@pytest.mark.parametrize("C,T,k", [(128, 64, 5), (256, 127, 5), (64, 100, 3), (32, 62, 5)])
def test_conv_upsample(C, T, k):
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(C + T)
    x = torch.randn(2, C, T, generator=g)
    w = torch.randn(C, C, k, generator=g) / math.sqrt(k * C)
    b = torch.randn(C, generator=g)
    y, st = ops.conv1d(cl(x), w.to(dev()), b.to(dev()), upsample=True)
    ref = F.conv1d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=k // 2)
    assert rel_err(ncw(y), ref) < TOL
    assert rel_err(st.cpu(), ref_stats(ref)) < TOL


@pytest.mark.parametrize("C0,C1,T", [(64, 0, 256), (128, 64, 200), (256, 128, 100), (64, 32, 4064)])
def test_group_norm_via_stats(C0, C1, T):
    """producer statistics -> gn_finalize == GroupNorm32 over the (virtual) channel concat, incl. straddling groups."""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(C0 + C1 + T)
    B = 2
    x0 = torch.randn(B, C0, T, generator=g) * 3 + 0.7
    x1 = torch.randn(B, C1, T, generator=g) - 2 if C1 else None
    gamma, beta = torch.randn(C0 + C1, generator=g), torch.randn(C0 + C1, generator=g)
    d = dev()
    s0 = ref_stats(x0).to(d)
    s1 = ref_stats(x1).to(d) if C1 else None
    gs, gh, mr = ops.gn_finalize(s0, C0, T, gamma.to(d), beta.to(d), s1, C1)
    x = torch.cat([x0, x1], 1) if C1 else x0
    ref = F.group_norm(x, 32, gamma, beta, 1e-5)
    got = x * gs.cpu()[:, :, None] + gh.cpu()[:, :, None]
    assert rel_err(got, ref) < 2e-5


@pytest.mark.parametrize("H,D,T", [(4, 64, 512), (2, 32, 62), (1, 64, 127), (4, 64, 508), (1, 128, 512), (2, 128, 100)])
def test_attention(H, D, T):
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(H * D + T)
    B = 2
    qkv = torch.randn(B, 3 * H * D, T, generator=g) * 1.5
    out = ops.attention(cl(qkv), H)
    out1 = ops.attention(cl(qkv), H, workspace=False)
    q, k, v = qkv.chunk(3, dim=1)
    sc = 1 / math.sqrt(math.sqrt(D))
    w = torch.einsum("bct,bcs->bts", (q * sc).reshape(B * H, D, T), (k * sc).reshape(B * H, D, T))
    w = torch.softmax(w.float(), dim=-1)
    ref = torch.einsum("bts,bcs->bct", w, v.reshape(B * H, D, T)).reshape(B, -1, T)
    assert rel_err(ncw(out), ref) < TOL
    assert rel_err(ncw(out1), ref) < TOL


@pytest.mark.parametrize("B,H,T", [(4, 1, 512), (5, 1, 512), (2, 2, 333), (1, 1, 65)])
def test_attention_key_split_for_grids_far_below_the_chip(B, H, T):
    """Round 6: with one head of 128 channels and a handful of samples (the tiny config's middle block at B = 4) the first-generation
    kernel's grid is 32 workgroups walking 8 key tiles each; given the workspace it deals the key tiles over up to 8 workgroups per
    query tile (even and uneven splits, a ragged last tile) and a combine launch merges the partial rows.  Output and log-sum-exp
    against the unsplit launch and the reference, on scores with a peaked row distribution (the splits' maxima differ by tens)."""
    from tqdne_amd import ops
    D = 128
    g = torch.Generator().manual_seed(B * 1000 + T)
    qkv = torch.randn(B, 3 * H * D, T, generator=g)
    qkv[:, :2 * H * D] *= 2.5                      # q, k: score standard deviation ~ 6
    qkv[:, H * D:2 * H * D, T // 3] *= 3.0         # one key far outside the others' range
    out, lse = ops.attention(cl(qkv), H, return_lse=True)
    out1, lse1 = ops.attention(cl(qkv), H, return_lse=True, workspace=False)
    q, k, v = qkv.chunk(3, dim=1)
    sc = 1 / math.sqrt(math.sqrt(D))
    w = torch.einsum("bct,bcs->bts", (q * sc).reshape(B * H, D, T).double(), (k * sc).reshape(B * H, D, T).double())
    ref = torch.einsum("bts,bcs->bct", torch.softmax(w, dim=-1), v.reshape(B * H, D, T).double()).reshape(B, -1, T).float()
    assert rel_err(ncw(out), ref) < TOL and rel_err(ncw(out1), ref) < TOL
    assert rel_err(ncw(out), ncw(out1)) < 2e-5
    ref_lse = torch.logsumexp(w, dim=-1).reshape(B, H, T).float()
    assert rel_err(lse.cpu(), ref_lse) < 1e-5 and rel_err(lse.cpu(), lse1.cpu()) < 1e-5


@pytest.mark.parametrize("H,D,T,peaked", [(4, 64, 512, False), (2, 32, 190, False), (4, 64, 256, True), (1, 64, 64, False)])
def test_qkv_conv_feeding_the_presplit_attention(H, D, T, peaked):
    """The inference pair of an AttentionBlock (blocks.py:127-190): tq_conv1d_fwd_qkv writes q as fp32 and K / V as the attention
    kernel's planes, tq_attention_fwd_presplit consumes them.  Default: V as fp16 hi / lo planes and ONE fp16 softmax weight (two
    products: ~1e-4 of the output scale); TQDNE_ATTN_VF16=0: bf16 hi / lo V and P (three products: fp32-grade)."""
    import ctypes as C
    import os
    from tqdne_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(H * D + T)
    B, Cc = 2, H * D
    d = dev()
    x = torch.randn(B, T, Cc, generator=g)
    gs, gh = torch.rand(B, Cc, generator=g) + 0.5, torch.randn(B, Cc, generator=g)
    w = torch.randn(3 * Cc, Cc, 1, generator=g) / math.sqrt(Cc) * 1.5
    bias = torch.randn(3 * Cc, generator=g) * 0.1
    if peaked:   # one key row far outside the others' range: a softmax weight of ~1 next to many tiny ones
        x[:, 77] *= 6.0
    wfmt = _lib.forward_wfmt(3 * Cc, [Cc, 0])
    wp = ops.pack_conv_weight(w.to(d), _lib.PACK_MODE[wfmt])
    desc = _lib.TqConvDesc()
    desc.B, desc.T_in, desc.T_out, desc.C_in0, desc.C_in1, desc.C_out = B, T, T, Cc, 0, 3 * Cc
    desc.ktaps, desc.stride, desc.pad, desc.upsample = 1, 1, 0, 0
    desc.flags, desc.wfmt = 1, wfmt   # TQ_CONV_GN
    xd, gsd, ghd, bd = x.to(d), gs.to(d), gh.to(d), bias.to(d)
    xin = x * gs[:, None, :] + gh[:, None, :]
    qkv_ref = xin @ w[:, :, 0].T + bias
    q, k, v = [t.reshape(B, T, H, D).permute(0, 2, 1, 3) for t in qkv_ref.split(Cc, dim=2)]
    sc = 1 / math.sqrt(math.sqrt(D))
    att = torch.softmax((q * sc) @ (k * sc).transpose(-1, -2), dim=-1)
    ref = (att @ v).permute(0, 2, 1, 3).reshape(B, T, Cc)
    p = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    errs = {}
    flag = torch.zeros(1, dtype=torch.int32, device=d)
    desc.range_flag = flag.data_ptr()
    for vf16 in ("1", "0"):
        vfmt = _lib.TQ_KV_V_F16 if vf16 == "1" else _lib.TQ_KV_V_BF16
        qkv = torch.zeros(B, T, 3 * Cc, device=d)
        ws = torch.zeros(lib.tq_attention_workspace_bytes(B, T, H, D), dtype=torch.uint8, device=d)
        out = torch.empty(B, T, Cc, device=d)
        assert lib.tq_conv1d_fwd_qkv(C.byref(desc), p(xd), p(gsd), p(ghd), p(wp), p(bd), p(qkv), p(ws), H, D, vfmt, stream) == 0
        assert lib.tq_attention_fwd_presplit(p(qkv), p(ws), p(out), B, T, H, D, vfmt, stream) == 0
        torch.cuda.synchronize()
        assert int(flag.item()) == 0   # (V well inside the fp16 range: the guard stays down)
        assert rel_err(qkv[:, :, :Cc].cpu(), qkv_ref[:, :, :Cc]) < 2e-4   # (q: the conv's own fp16 + fp6 scheme)
        errs[vf16] = rel_err(out.cpu(), ref)
    print(f"attention pair H={H} D={D} T={T} peaked={peaked}: fp16 P / V {errs['1']:.2e}, bf16 hi / lo {errs['0']:.2e}")
    assert errs["1"] < 5e-4 and errs["0"] < 2e-4
    # round 6: TQ_CONV_CH_TILES (the hint of launch-bound plans: channel-tiled instead of input-stationary form) -- the same q and planes
    if 3 * Cc >= 512 and Cc in (128, 256) and wfmt == _lib.TQ_WFMT_F16_MX6:
        qkv2, ws2 = torch.zeros_like(qkv), torch.zeros_like(ws)
        desc.flags = 1 | _lib.TQ_CONV_CH_TILES
        assert lib.tq_conv1d_fwd_qkv(C.byref(desc), p(xd), p(gsd), p(ghd), p(wp), p(bd), p(qkv2), p(ws2), H, D, vfmt, stream) == 0
        desc.flags = 1
        torch.cuda.synchronize()
        assert torch.equal(qkv2[:, :, :Cc], qkv[:, :, :Cc]) and torch.equal(ws2, ws)
    # the V planes' range guard (ABI 6): a bias that lifts one V channel to 4e4 raises the flag in the fp16 format only
    if not peaked:
        big = bias.clone()
        big[2 * Cc + 3] = 4.0e4
        bigd = big.to(d)
        for vfmt, want in ((_lib.TQ_KV_V_BF16, 0), (_lib.TQ_KV_V_F16, 1)):
            flag.zero_()
            assert lib.tq_conv1d_fwd_qkv(C.byref(desc), p(xd), p(gsd), p(ghd), p(wp), p(bigd), p(qkv), p(ws), H, D, vfmt, stream) == 0
            torch.cuda.synchronize()
            assert int(flag.item()) == want, (vfmt, int(flag.item()))
        assert lib.tq_conv1d_fwd_qkv(C.byref(desc), p(xd), p(gsd), p(ghd), p(wp), p(bd), p(qkv), p(ws), H, D, 7, stream) == -1  # TQ_ERR_ARG


def test_attention_peaked_softmax():
    """one key dominates one query: exercises the online-softmax rescale path across key tiles"""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(3)
    B, H, D, T = 1, 1, 64, 256
    qkv = torch.randn(B, 3 * D, T, generator=g)
    qkv[0, D:2 * D, 200] = qkv[0, :D, 5] * 6.0  # key 200 aligned with query 5 (in a later tile)
    q, k, v = qkv.chunk(3, dim=1)
    sc = 1 / math.sqrt(math.sqrt(D))
    w = torch.softmax(torch.einsum("bct,bcs->bts", q * sc, k * sc), dim=-1)
    ref = torch.einsum("bts,bcs->bct", w, v)
    for ws in (True, False):
        assert rel_err(ncw(ops.attention(cl(qkv), H, workspace=ws)), ref) < TOL


@pytest.mark.parametrize("trend", ["rising", "falling", "offset"])
def test_attention_reference_level_moves(trend):
    """The forward kernel keeps a lazy softmax reference level per query (it only moves when a key tile's maximum exceeds it by
    2^6): scores that climb by tens of nats from key tile to key tile move it in every tile, falling ones never after the first,
    and a large common offset (all scores ~ -80 or +80 nats) must not under- or overflow the first tile."""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(11)
    B, H, D, T = 2, 2, 64, 500
    qkv = torch.randn(B, 3 * H * D, T, generator=g)
    q, k, v = [t.clone() for t in qkv.chunk(3, dim=1)]
    u = torch.randn(H * D, generator=g)
    u = u / u.reshape(H, D).norm(dim=1).repeat_interleave(D)  # unit vector per head
    ramp = torch.linspace(-1, 1, T)
    if trend == "offset":
        q = q * 0.3 + 8.0 * u[None, :, None]
        k = k * 0.3 + 80.0 * u[None, :, None] * torch.tensor([1.0, -1.0]).repeat_interleave(D)[None, :, None]  # head 0: +80 nats, head 1: -80
    else:
        q = q * 0.3 + 8.0 * u[None, :, None]
        k = k * 0.3 + 60.0 * u[None, :, None] * (ramp if trend == "rising" else -ramp)[None, None, :]
    qkv = torch.cat([q, k, v], 1)
    sc = 1 / math.sqrt(math.sqrt(D))
    w = torch.einsum("bct,bcs->bts", (q.double() * sc).reshape(B * H, D, T), (k.double() * sc).reshape(B * H, D, T))
    assert w.abs().max() > 50  # the case is what it claims to be
    ref = torch.einsum("bts,bcs->bct", torch.softmax(w, dim=-1), v.double().reshape(B * H, D, T)).reshape(B, -1, T).float()
    out, lse = ops.attention(cl(qkv), H, return_lse=True)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    assert rel_err(ncw(out), ref) < TOL
    assert rel_err(lse.cpu().reshape(B * H, T), torch.logsumexp(w, dim=-1).float(), elem=False) < 1e-5


@pytest.mark.parametrize("cin,cout,T", [(3, 64, 4096), (3, 32, 250), (6, 64, 4064), (16, 64, 512)])
def test_stem(cin, cout, T):
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(cin + cout + T)
    x = torch.randn(2, cin, T, generator=g)
    w, b = torch.randn(cout, cin, 5, generator=g) / 4, torch.randn(cout, generator=g)
    sc = torch.rand(2, generator=g) + 0.5
    d = dev()
    y, st = ops.stem_conv(x.to(d), w.to(d), b.to(d), in_scale=sc.to(d))
    ref = F.conv1d(x * sc[:, None, None], w, b, padding=2)
    assert rel_err(ncw(y), ref) < 1e-5
    assert rel_err(st.cpu(), ref_stats(ref)) < 1e-5


@pytest.mark.parametrize("cin,cout,T", [(64, 3, 4096), (32, 3, 250), (64, 4, 333)])
def test_head(cin, cout, T):
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(cin + cout + T)
    B = 2
    x = torch.randn(B, cin, T, generator=g)
    a, s = torch.randn(B, cin, generator=g), torch.randn(B, cin, generator=g)
    w, b = torch.randn(cout, cin, 5, generator=g) / 10, torch.randn(cout, generator=g)
    co, cs = torch.rand(B, generator=g), torch.rand(B, generator=g)
    skip = torch.randn(B, cout, T, generator=g)
    d = dev()
    y = ops.head_conv(cl(x), w.to(d), b.to(d), a.to(d), s.to(d), co.to(d), cs.to(d), skip.to(d))
    ref = F.conv1d(F.silu(x * a[:, :, None] + s[:, :, None]), w, b, padding=2) * co[:, None, None] + cs[:, None, None] * skip
    assert rel_err(y.cpu(), ref) < 1e-5
    y2 = ops.head_conv(cl(x), w.to(d), b.to(d))
    assert rel_err(y2.cpu(), F.conv1d(x, w, b, padding=2)) < 1e-5


@pytest.mark.parametrize("cin,cout,T,K", [(16, 1, 77, 5), (32, 2, 129, 3), (48, 2, 129, 3), (128, 3, 61, 1), (128, 4, 200, 5), (64, 3, 60, 5), (64, 3, 1, 5), (64, 6, 190, 5),
                                          (64, 6, 4064, 5), (64, 8, 130, 3), (64, 16, 257, 5), (32, 16, 64, 1), (64, 6, 59, 1), (64, 5, 100, 5), (64, 12, 100, 5)])
def test_head_other_shapes(cin, cout, T, K):
    """the row-per-thread form (C_out <= 4; round 5: 6 and 8 in one launch -- a wave emits two channels --, 16 in two launches: the heads
    of the 6-channel envelope representation and of the 16-channel latent) on ragged lengths (a wave emits 64 - (K - 1) outputs), every
    tap count and channel count it is dispatched for, and the round-3 kernel for the other channel counts (5, 12) and C_in = 48"""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(cin + cout + T + K)
    B = 3
    x = torch.randn(B, cin, T, generator=g)
    a, s = torch.randn(B, cin, generator=g), torch.randn(B, cin, generator=g)
    w, b = torch.randn(cout, cin, K, generator=g) / 10, torch.randn(cout, generator=g)
    co, cs = torch.rand(B, generator=g), torch.rand(B, generator=g)
    skip = torch.randn(B, cout, T, generator=g)
    d = dev()
    y = ops.head_conv(cl(x), w.to(d), b.to(d), a.to(d), s.to(d), co.to(d), cs.to(d), skip.to(d))
    ref = F.conv1d(F.silu(x * a[:, :, None] + s[:, :, None]), w, b, padding=K // 2) * co[:, None, None] + cs[:, None, None] * skip
    assert rel_err(y.cpu(), ref) < 1e-5


def test_linear():
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(1)
    x, w, b = torch.randn(5, 256, generator=g), torch.randn(200, 256, generator=g) / 16, torch.randn(200, generator=g)
    d = dev()
    assert rel_err(ops.linear(x.to(d), w.to(d), b.to(d)).cpu(), F.linear(x, w, b)) < 1e-5


def test_dropout_mask_statistics_and_determinism():
    from tqdne_amd import ops
    d = dev()
    B, C, T = 2, 64, 1024
    x = torch.ones(B, T, C, device=d)
    ones, zeros = torch.ones(B, C, device=d), torch.zeros(B, C, device=d)
    w = torch.zeros(C, C, 1)
    w[torch.arange(C), torch.arange(C), 0] = 1.0  # identity 1x1 conv exposes silu(1) * mask / (1-p)
    kw = dict(gscale=ones, gshift=zeros, silu=True, dropout_p=0.1, dropout_site=3)
    y1, _ = ops.conv1d(x, w.to(d), None, dropout_seed=42, **kw)
    y2, _ = ops.conv1d(x, w.to(d), None, dropout_seed=42, **kw)
    y3, _ = ops.conv1d(x, w.to(d), None, dropout_seed=43, **kw)
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)
    keep = (y1 != 0).float().mean().item()
    assert abs(keep - 0.9) < 0.01
    vals = torch.unique(y1)
    silu1 = float(torch.nn.functional.silu(torch.tensor(1.0)))
    assert len(vals) == 2 and abs(vals.max().item() - silu1 / 0.9) < 1e-4


def test_pack_jobs_equals_one_pack_per_tensor():
    """tq_pack_jobs (every re-pack of a plan in one launch) against tq_pack_conv_weight per tensor: same bytes, for every mode, odd
    shapes (padding rows / channels), and the plain-copy jobs that gather the embedding projections"""
    import torch
    from tqdne_amd import _lib, engine, ops
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    shapes = [((64, 64, 5), 0), ((256, 192, 5), 3), ((128, 128, 5), 2), ((96, 64, 3), 0), ((64, 3, 5), 0), ((256, 256, 1), 1),
              ((768, 256, 1), 3), ((64, 128, 5), 1), ((32, 64, 3), 1), ((512, 256, 5), 3)]
    ws, refs, outs, jobs = [], [], [], []
    for (co, ci, k), mode in shapes:
        w = torch.randn(co, ci, k, generator=g).to(dev)
        ws.append(w)
        refs.append(ops.pack_conv_weight(w, mode))
        out = torch.zeros_like(refs[-1])
        outs.append(out)
        jobs.append((w.data_ptr(), out.data_ptr(), co, ci, k, mode))
    src = torch.randn(1000, generator=g).to(dev)
    dst = torch.zeros(1003, device=dev)
    jobs.insert(4, (src.data_ptr(), dst.data_ptr() + 4 * 3, 1000, 0, 0, 4))     # a copy job in the middle of the table
    engine.pack_batch(lib, dev, jobs, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    for (shape, mode), r, o in zip(shapes, refs, outs):
        assert torch.equal(r, o), (shape, mode)
    assert torch.equal(dst[3:], src) and float(dst[:3].abs().sum()) == 0.0


@pytest.mark.parametrize("cin0,cin1,cout,T,wf,p,skipc", [
    (32, 0, 32, 300, 0, 0.0, 0), (64, 32, 64, 257, 0, 0.0, 0), (128, 64, 128, 130, 0, 0.0, 0), (128, 128, 128, 96, 2, 0.0, 0),
    (128, 0, 256, 65, 2, 0.0, 0), (64, 0, 96, 31, 0, 0.0, 0), (128, 128, 128, 200, 2, 0.0, 256), (64, 32, 64, 100, 0, 0.0, 96),
    (128, 0, 128, 160, 2, 0.1, 0), (32, 0, 64, 129, 0, 0.1, 32),
])
def test_conv_small_tile_equals_the_default_tile(cin0, cin1, cout, T, wf, p, skipc):
    """TqConvDesc.t_tile = 32 (launch-bound batches): the convolution is BIT-identical to the default tiles' (same accumulation order
    per output element), its 32-position statistics add up to the default 128-position ones, and tq_gn_finalize fed with them gives
    the same coefficients to rounding.  ResBlock forms: GN + SiLU (+ dropout) prologue, emb, residual or fused skip conv, concat."""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(cin0 + cin1 + cout + T)
    B, K = 2, 5
    d = dev()
    cin = cin0 + cin1
    x0 = torch.randn(B, T, cin0, generator=g).to(d)
    x1 = torch.randn(B, T, cin1, generator=g).to(d) if cin1 else None
    w = (torch.randn(cout, cin, K, generator=g) / math.sqrt(cin * K)).to(d)
    b = torch.randn(cout, generator=g).to(d)
    emb = torch.randn(B, cout, generator=g).to(d)
    gs, gh = (torch.rand(B, cin, generator=g) + 0.5).to(d), torch.randn(B, cin, generator=g).to(d)
    kw = dict(x1=x1, gscale=gs, gshift=gh, silu=True, emb=emb, wfmt=wf, dropout_p=p, dropout_seed=77, dropout_site=3)
    if skipc:
        sx = torch.randn(B, T, skipc, generator=g).to(d)
        kw["skip"] = (sx, None, (torch.randn(cout, skipc, 1, generator=g) / math.sqrt(skipc)).to(d), torch.randn(cout, generator=g).to(d))
    else:
        kw["residual"] = torch.randn(B, T, cout, generator=g).to(d)
    y0, st0 = ops.conv1d(x0, w, b, **kw)
    y1, st1 = ops.conv1d(x0, w, b, t_tile=32, **kw)
    assert torch.equal(y0, y1)
    assert st1.shape[1] == (T + 31) // 32
    # 32-position slots summed four at a time = the 128-position slots
    pad = (-st1.shape[1]) % 4
    s1 = torch.cat([st1, torch.zeros(B, pad, cout, 2, device=d)], 1).double().view(B, -1, 4, cout, 2).sum(2)
    assert rel_err(s1.cpu(), st0.double().cpu()) < 1e-5
    gam, bet = (torch.rand(cout, generator=g) + 0.5).to(d), torch.randn(cout, generator=g).to(d)
    a0, h0, m0 = ops.gn_finalize(st0, cout, T, gam, bet)
    a1, h1, m1 = ops.gn_finalize(st1, cout, T, gam, bet, slot0=32)
    assert rel_err(a1.cpu(), a0.cpu()) < 1e-5 and rel_err(h1.cpu(), h0.cpu()) < 1e-5 and rel_err(m1.cpu(), m0.cpu()) < 1e-5
    # a concat of a 32-slot and a 128-slot source (an output block reading the stem's output through the skip stack)
    if cout % 32 == 0:
        a2, h2, _ = ops.gn_finalize(st1, cout, T, torch.cat([gam, gam]), torch.cat([bet, bet]), stats1=st0, C1=cout, slot0=32, slot1=128)
        a3, h3, _ = ops.gn_finalize(st0, cout, T, torch.cat([gam, gam]), torch.cat([bet, bet]), stats1=st0, C1=cout)
        assert rel_err(a2.cpu(), a3.cpu()) < 1e-5 and rel_err(h2.cpu(), h3.cpu()) < 1e-5


@pytest.mark.parametrize("cin0,cin1,cout,T,wf,slots,skipc", [
    (32, 0, 32, 300, 0, (128, 0), 0), (64, 32, 64, 257, 0, (32, 128), 0), (128, 128, 128, 96, 2, (32, 32), 0), (128, 0, 256, 65, 2, (128, 0), 0),
    (256, 256, 256, 130, 2, (128, 32), 256), (64, 32, 64, 100, 0, (128, 128), 96), (128, 128, 128, 4096, 2, (128, 128), 0),
])
def test_conv_small_tile_folds_its_own_group_norm(cin0, cin1, cout, T, wf, slots, skipc):
    """round 6, TqConvDesc.gn_fold (consumer side): the small-tile launch forms its GroupNorm coefficients from the sources' partial
    statistics itself -- every workgroup folds its sample in its prologue -- instead of a tq_gn_finalize launch in front of it: the
    coefficients it WRITES (gscale, gshift, mean / rstd: the backward reads them) and its output are BIT-identical to the two-launch form,
    for one or two sources, either slot size per source, both schemes, with the fused skip conv."""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(cin0 + cin1 + cout + T)
    B, K = 3, 5
    d = dev()
    cin = cin0 + cin1
    x0 = torch.randn(B, T, cin0, generator=g).to(d) * 1.3 + 0.2
    x1 = (torch.randn(B, T, cin1, generator=g) - 0.4).to(d) if cin1 else None

    def slot_stats(x, slot):   # (B, ceil(T / slot), C, 2) partial sums, as a producing conv's epilogue leaves them
        n = (T + slot - 1) // slot
        xp = torch.cat([x, torch.zeros(B, n * slot - T, x.shape[2], device=d)], 1).view(B, n, slot, x.shape[2])
        return torch.stack([xp.sum(2), (xp * xp).sum(2)], -1).contiguous()
    st0 = slot_stats(x0, slots[0])
    st1 = slot_stats(x1, slots[1]) if cin1 else None
    gam, bet = (torch.rand(cin, generator=g) + 0.5).to(d), torch.randn(cin, generator=g).to(d)
    w = (torch.randn(cout, cin, K, generator=g) / math.sqrt(cin * K)).to(d)
    b, emb = torch.randn(cout, generator=g).to(d), torch.randn(B, cout, generator=g).to(d)
    kw = dict(x1=x1, silu=True, emb=emb, wfmt=wf, t_tile=32)
    if skipc:
        sx = torch.randn(B, T, skipc, generator=g).to(d)
        kw["skip"] = (sx, None, (torch.randn(cout, skipc, 1, generator=g) / math.sqrt(skipc)).to(d), torch.randn(cout, generator=g).to(d))
    else:
        kw["residual"] = torch.randn(B, T, cout, generator=g).to(d)
    a_ref, h_ref, m_ref = ops.gn_finalize(st0, cin0, T, gam, bet, stats1=st1, C1=cin1, slot0=slots[0], slot1=slots[1])
    y_ref, s_ref = ops.conv1d(x0, w, b, gscale=a_ref, gshift=h_ref, **kw)
    nan = float("nan")
    a, h, m = torch.full_like(a_ref, nan), torch.full_like(h_ref, nan), torch.full_like(m_ref, nan)
    y, s_ = ops.conv1d(x0, w, b, gscale=a, gshift=h, gn_fold=(st0, st1, slots[0], slots[1], gam, bet, m), **kw)
    assert torch.equal(a, a_ref) and torch.equal(h, h_ref) and torch.equal(m, m_ref)
    assert torch.equal(y, y_ref) and torch.equal(s_, s_ref)
    from tqdne_amd import _lib
    if wf == _lib.TQ_WFMT_F16_MX6:
        # the default tiles of the fp16 + MX-fp6 scheme fold too (behind the first chunk's loads, coefficients straight into the LDS table)
        a2, h2, m2 = torch.full_like(a_ref, nan), torch.full_like(h_ref, nan), torch.full_like(m_ref, nan)
        y_ref0, s_ref0 = ops.conv1d(x0, w, b, gscale=a_ref, gshift=h_ref, **dict(kw, t_tile=0))
        y2, s2 = ops.conv1d(x0, w, b, gscale=a2, gshift=h2, gn_fold=(st0, st1, slots[0], slots[1], gam, bet, m2), **dict(kw, t_tile=0))
        assert torch.equal(a2, a_ref) and torch.equal(h2, h_ref) and torch.equal(m2, m_ref)
        assert torch.equal(y2, y_ref0) and torch.equal(s2, s_ref0)
    else:   # the three-product scheme's default tiles are not built for it: refused, nothing launched
        with pytest.raises(_lib.TqError, match="TQ_ERR_SHAPE"):
            ops.conv1d(x0, w, b, gscale=a, gshift=h, gn_fold=(st0, st1, slots[0], slots[1], gam, bet, m), **dict(kw, t_tile=0))


def test_conv_small_tile_refuses_what_it_is_not_built_for():
    import ctypes as C
    from tqdne_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1 << 16, device=dev())
    d = _lib.TqConvDesc()
    d.B, d.T_in, d.T_out, d.C_in0, d.C_in1, d.C_out = 1, 64, 64, 64, 0, 64
    d.ktaps, d.stride, d.pad, d.upsample, d.flags, d.t_tile = 3, 1, 1, 0, 3, 32          # k = 3
    p = x.data_ptr()
    assert lib.tq_conv1d_fwd(C.byref(d), p, None, p, p, p, None, None, None, p, None, None) == -2
    d.ktaps, d.pad, d.flags = 5, 2, 0                                                      # no GN + SiLU prologue
    assert lib.tq_conv1d_fwd(C.byref(d), p, None, None, None, p, None, None, None, p, None, None) == -2
    d.flags, d.t_tile = 3, 64                                                              # not a tile that exists
    assert lib.tq_conv1d_fwd(C.byref(d), p, None, p, p, p, None, None, None, p, None, None) == -1
