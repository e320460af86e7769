"""The conv contraction schemes held to their bit-model (oracle/contraction.py): the weight packers bit for bit, the forward and
data-gradient kernels against the model built from the float32 activation the kernel stages, and a sweep of both operands' ranges.

Metric: e_m = max|y - y_model| / max|y_model| per output channel, the worst channel.  The model rounds every operand as the kernel does
and sums in float64, so e_m holds only the fp32 accumulation order of the matrix cores and, for GN + SiLU launches, the kernel's own exp /
rcp.  The bars below are 4 x the worst e_m measured per scheme and launch family (DESIGN_LOG.md, "Contraction schemes against their
bit-model"); every check also requires its bar to be at most one fifth of the scheme's own model-versus-exact error on the same data, so
that an error of the size of one dropped correction term cannot pass -- the families that cannot meet that are named at FIFTH below,
with what they meet instead.  The comparison against exact fp64 at 1e-4 stays alongside wherever the operands are inside the envelope
include/tqdne_hip.h states for the scheme.  `pytest -s` prints every figure."""

import ctypes as C_
import math

import numpy as np
import pytest
import torch

from oracle import contraction as M

pytestmark = pytest.mark.gpu

TOL = 1e-4
S0, S1, S2 = M.BF16X3, M.F16_MX8, M.F16_MX6
# 4 x the worst e_m measured per (launch family, scheme) on one MI355X -- room for another association order, nothing else.  Families:
# tile128 / tile256: plain launches of the 128- and 256-channel tiles; pw: the input-stationary 1x1 conv; poly2: the two-phase upsampling
# conv; gn_silu: launches that stage silu(a x + s) (64-channel tile, small tile, wide table, fused skip); dgrad: data gradients;
# sweep / dsweep: the range sweeps (forward / data gradient); *_sub: their cells with weights in fp16's SUBNORMAL range (weight scale 1e-5,
# 1e-6: |w| ~ 6e-7 ... 6e-8).  There the fp16 matrix instruction itself is ~2e-5 of the output off the exactly rounded sum -- we suppose
# it aligns the products of one instruction by the operands' exponent FIELDS, so that an unnormalised operand loses its leading zeros
# (the packed fragments are bit-equal to the model there, bf16x3 shows nothing, and with all-zero fp16 weights at 1e-7 the effect is
# gone) -- still 1e-3 of the scheme's own error in those cells.
BAR = {("tile128", S0): 4 * 5.66e-7, ("tile128", S1): 4 * 5.53e-7, ("tile128", S2): 4 * 4.64e-7,
       ("tile256", S0): 4 * 1.11e-6, ("tile256", S1): 4 * 9.55e-7, ("tile256", S2): 4 * 6.30e-7,
       ("pw", S0): 4 * 5.79e-7, ("pw", S1): 4 * 4.69e-7, ("pw", S2): 4 * 4.72e-7,
       ("poly2", S0): 4 * 3.39e-7, ("poly2", S1): 4 * 4.26e-7, ("poly2", S2): 4 * 3.12e-7,
       ("gn_silu", S0): 4 * 5.57e-6, ("gn_silu", S2): 4 * 7.42e-6,
       ("dgrad", S0): 4 * 8.85e-7, ("dgrad", S2): 4 * 6.76e-7,
       ("sweep", S0): 4 * 8.70e-7, ("sweep", S1): 4 * 1.18e-6, ("sweep", S2): 4 * 1.18e-6,
       ("sweep_sub", S1): 4 * 1.84e-5, ("sweep_sub", S2): 4 * 1.90e-5,
       ("dsweep", S0): 4 * 1.21e-6, ("dsweep", S2): 4 * 7.55e-7, ("dsweep_sub", S2): 4 * 2.44e-5}
# Every bar must be at most 1 / 5 of the scheme's own model-versus-exact error on the same data.  These families cannot meet that: their
# fp32 accumulation error times the margin of 4 is 1 / 2.3 ... 1 / 4.3 of the scheme's error (the longest sums: 960 terms x 3 products
# in tile256; the heavy-tailed and hot-channel rows of the sweeps) -- they are held to 1 / 2 instead, the bars stay where measured.
# gn_silu cannot meet any such condition: the kernel's exp2 / rcp differ from the CPU's exp in the last bit of some staged values, which
# flips the rounding of their low part (~70 of 8320 staged values, each by one step of 2^-16 |x|: measured with identity weights), so its
# e_m is of the size of the schemes' own error; one dropped correction block in four still fails every one of its fp16 + MX-fp6 tests
# (DESIGN_LOG.md, mutation 1).
FIFTH = {("tile256", S0): 2, ("tile256", S1): 2, ("dgrad", S0): 2, ("sweep", S0): 2, ("sweep", S1): 2, ("sweep", S2): 2, ("dsweep", S0): 2,
         ("gn_silu", S0): None, ("gn_silu", S2): None}


def dev():
    return torch.device("cuda:0")


def _g(t):
    return None if t is None else torch.as_tensor(np.ascontiguousarray(t)).to(dev())


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _weights(rng, co, ci, k, scale=1.0):
    return (rng.standard_normal((co, ci, k)) * (scale / math.sqrt(ci * k))).astype(np.float32)


def _hold(tag, family, scheme, y, model, exact, envelope=True):
    """print the three figures of one comparison, then assert them"""
    y = y.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(y) else np.asarray(y, np.float64)
    em = M.channel_err(y, model)
    mx = M.channel_err(model, exact)
    kx = float(np.abs(y - exact).max() / max(np.abs(exact).max(), 1e-300))
    bar = BAR[family, scheme]
    print(f"EM {family:8s} {M.SCHEME_NAME[scheme]:8s} {tag:44s} e_m {em:.2e}  model-vs-exact {mx:.2e}  kernel-vs-exact {kx:.2e}")
    assert np.isfinite(y).all(), tag
    assert em <= bar, f"{tag}: e_m {em:.3e} above the bar {bar:.1e} ({M.SCHEME_NAME[scheme]})"
    ratio = FIFTH.get((family, scheme), 5)
    if ratio and (envelope or family.endswith("_sub")):
        assert bar <= mx / ratio, f"{tag}: bar {bar:.1e} is not 1 / {ratio} of the scheme's own error {mx:.2e}"
    if envelope:
        assert kx < TOL, f"{tag}: {kx:.3e} against exact fp64"
    return em, mx, kx


# ------------------------------------------------------------------------------------------------ packers
PACK_SHAPES = [(32, 32, 1), (96, 64, 3), (64, 96, 5), (128, 64, 5), (160, 192, 1)]


def _placed(w, rng, scale):
    """values exact in float32 and away from rounding ties, at fixed places: 0, +-447 / +-449 (either side of the e4m3 clamp), 65504 (1 +-
    2^-8) (either side of the fp16 maximum), an fp32 denormal, and one large weight among 15 small ones of a 16-block"""
    co, ci, k = w.shape
    flat = w.reshape(co, -1)
    vals = [0.0, 447.0, -447.0, 449.0, -449.0, 65504.0 * (1 - 2.0 ** -8), 65504.0 * (1 + 2.0 ** -8), 2.0 ** -140]
    for i, v in enumerate(vals):
        assert float(np.float32(v)) == v
        flat[(5 * i + 1) % co, (7 * i + 3) % flat.shape[1]] = v
    w[co - 1, :16, 0] = _rand(rng, 16, scale=1e-4 * scale)      # forward blocks run along C_in ...
    w[co - 1, 5, 0] = 300.0 * scale
    w[:16, ci - 1, k - 1] = _rand(rng, 16, scale=1e-4 * scale)  # ... transposed ones along C_out
    w[9, ci - 1, k - 1] = -300.0 * scale
    return w


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_packers_bit_for_bit(shape, mode):
    """tq_pack_conv_weight against the documented layout and rounding, by equality: bf16 / fp16 fragments, e4m3 / e2m3 codes, E8M0 bytes,
    padding.  (A hardware rounding that differs from round-to-nearest-even would show here: it is a finding, the comparison stays.)"""
    from tqdne_amd import ops
    co, ci, k = shape
    rng = np.random.default_rng(1000 * mode + co + ci + k)
    for scale in (1.0, 1e-3, 1e-6, 1e3):
        w = _placed(_rand(rng, co, ci, k, scale=scale), rng, scale)
        packed = ops.pack_conv_weight(_g(w), mode).cpu().numpy()
        g = M.pack_geometry(co, ci, k, mode)
        assert packed.size == g["nbytes"]
        got, want = M.decode_packed(packed, co, ci, k, mode), M.pack_model(w, mode)
        for key in want:
            if key == "tail":
                assert not got["tail"].any(), "bytes after the E8M0 byte"
                continue
            bad = np.argwhere(got[key] != want[key])
            if len(bad):
                r, c, t = bad[0]
                a = M.operand_matrix(w, mode)
                cc = c * 16 if key == "e8m0" else c
                raise AssertionError(f"mode {mode} scale {scale:g} {key}: {len(bad)} differ; first at row {r} k {c} tap {t}: packed "
                                     f"{int(got[key][r, c, t]):#x}, model {int(want[key][r, c, t]):#x}, operand {a[r, cc:cc + (16 if key == 'e8m0' else 1), t]}")
        if mode in (3, 5):   # pad columns (and any pad rows) are all-zero blocks: lowest scale byte, zero codes
            padk = g["kdim"] // 16
            assert np.all(got["e8m0"][:, padk:] == 13) and np.all(got["e8m0"][g["rows"]:] == 13)
            assert not got["c0"][:, g["kdim"]:].any() and not got["c1"][:, g["kdim"]:].any() and not got["h"][:, g["kdim"]:].any()


# ------------------------------------------------------------------------------------------------ forward
def _forward(x0, w, scheme, *, x1=None, gn=None, t_tile=0, wide_table=False, skip=None):
    from tqdne_amd import ops
    a, s = gn if gn is not None else (None, None)
    sk = None
    if skip is not None:
        sk = (_g(skip[0]), _g(skip[1]), _g(skip[2]), None)
    y, _ = ops.conv1d(_g(x0), _g(w), None, x1=_g(x1), gscale=_g(a), gshift=_g(s), silu=gn is not None, stats=False, wfmt=scheme,
                      t_tile=t_tile, wide_table=wide_table, skip=sk)
    torch.cuda.synchronize()
    return y


def _staged(x0, x1, gn):
    x = x0 if x1 is None else np.concatenate([x0, x1], -1)
    return M.staged_gn_silu(x, *gn) if gn is not None else x


def _gn(rng, B, C):
    return (rng.random((B, C)) + 0.5).astype(np.float32), _rand(rng, B, C)


@pytest.mark.parametrize("scheme", M.SCHEMES, ids=lambda s: M.SCHEME_NAME[s])
@pytest.mark.parametrize("k,T", [(1, 127), (3, 127), (5, 127), (1, 129), (3, 129), (5, 129)])
def test_forward_128_channel_tile(k, T, scheme):
    rng = np.random.default_rng(10 * T + k)
    x, w = _rand(rng, 2, T, 64), _weights(rng, 128, 64, k)
    _hold(f"64->128 k{k} T{T}", "tile128", scheme, _forward(x, w, scheme), M.conv1d_model(x, w, scheme), M.conv1d_exact(x, w))


@pytest.mark.parametrize("scheme", M.SCHEMES, ids=lambda s: M.SCHEME_NAME[s])
def test_forward_256_channel_tile_concatenated_sources(scheme):
    rng = np.random.default_rng(256)
    x0, x1, w = _rand(rng, 2, 130, 128), _rand(rng, 2, 130, 64), _weights(rng, 256, 192, 5)
    x = _staged(x0, x1, None)
    _hold("128+64->256 k5 T130", "tile256", scheme, _forward(x0, w, scheme, x1=x1), M.conv1d_model(x, w, scheme), M.conv1d_exact(x, w))


@pytest.mark.parametrize("scheme", [S0, S2], ids=lambda s: M.SCHEME_NAME[s])
def test_forward_64_channel_tile_gn_silu(scheme):
    rng = np.random.default_rng(64)
    x0, w = _rand(rng, 2, 65, 64, scale=1.5), _weights(rng, 64, 64, 5)
    gn = _gn(rng, 2, 64)
    x = _staged(x0, None, gn)
    _hold("64->64 k5 T65 GN+SiLU", "gn_silu", scheme, _forward(x0, w, scheme, gn=gn), M.conv1d_model(x, w, scheme), M.conv1d_exact(x, w))


@pytest.mark.parametrize("scheme", [S0, S2], ids=lambda s: M.SCHEME_NAME[s])
def test_forward_small_tile_gn_silu(scheme):
    rng = np.random.default_rng(33)
    x0, w = _rand(rng, 2, 33, 64, scale=1.5), _weights(rng, 128, 64, 5)
    gn = _gn(rng, 2, 64)
    x = _staged(x0, None, gn)
    _hold("64->128 k5 T33 GN+SiLU t_tile 32", "gn_silu", scheme, _forward(x0, w, scheme, gn=gn, t_tile=32), M.conv1d_model(x, w, scheme),
          M.conv1d_exact(x, w))


@pytest.mark.parametrize("k,T,t_tile", [(5, 129, 0), (3, 127, 0), (1, 129, 0), (5, 33, 32)])
def test_forward_wide_table_tile_is_bit_equal(k, T, t_tile):
    rng = np.random.default_rng(2048 + k)
    x0, w = _rand(rng, 2, T, 64, scale=1.5), _weights(rng, 128, 64, k)
    gn = _gn(rng, 2, 64)
    narrow = _forward(x0, w, S2, gn=gn, t_tile=t_tile)
    wide = _forward(x0, w, S2, gn=gn, t_tile=t_tile, wide_table=True)
    assert torch.equal(narrow, wide)
    x = _staged(x0, None, gn)
    _hold(f"64->128 k{k} T{T} GN+SiLU wide table", "gn_silu", S2, wide, M.conv1d_model(x, w, S2), M.conv1d_exact(x, w))


@pytest.mark.parametrize("scheme", M.SCHEMES, ids=lambda s: M.SCHEME_NAME[s])
def test_forward_pointwise_input_stationary(scheme):
    rng = np.random.default_rng(512)
    x, w = _rand(rng, 2, 31, 256), _weights(rng, 512, 256, 1)
    _hold("256->512 k1 T31", "pw", scheme, _forward(x, w, scheme), M.conv1d_model(x, w, scheme), M.conv1d_exact(x, w))


@pytest.mark.parametrize("scheme", [S0, S2], ids=lambda s: M.SCHEME_NAME[s])
def test_forward_fused_skip(scheme):
    """tq_conv1d_fwd_skip: k = 5 conv of silu(GN(h)) plus the 1x1 conv of the un-activated block input (two sources), one accumulator"""
    rng = np.random.default_rng(77)
    T = 130
    h, w = _rand(rng, 2, T, 128, scale=1.5), _weights(rng, 128, 128, 5)
    sx0, sx1, wsk = _rand(rng, 2, T, 64), _rand(rng, 2, T, 64), _weights(rng, 128, 128, 1)
    gn = _gn(rng, 2, 128)
    x, sx = _staged(h, None, gn), np.concatenate([sx0, sx1], -1)
    y = _forward(h, w, scheme, gn=gn, skip=(sx0, sx1, wsk))
    _hold("128->128 k5 + skip 64+64->128 T130", "gn_silu", scheme, y, M.conv1d_model(x, w, scheme) + M.conv1d_model(sx, wsk, scheme),
          M.conv1d_exact(x, w) + M.conv1d_exact(sx, wsk))


@pytest.mark.parametrize("scheme", M.SCHEMES, ids=lambda s: M.SCHEME_NAME[s])
def test_forward_two_phase_upsampling_conv(scheme):
    """TQ_CONV_POLY2, 64 -> 2 x 64 channels, T = 128: output channel block p of the k = 3 conv is row 2 t + p of the result"""
    from tqdne_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(128)
    B, T, Ci, Co = 2, 128, 64, 64
    x, w2 = _rand(rng, B, T, Ci), _weights(rng, 2 * Co, Ci, 3)
    wp = ops.pack_conv_weight(_g(w2), _lib.PACK_MODE[scheme])
    xd = _g(x)
    y = torch.full((B, 2 * T, Co), float("nan"), device=dev())
    d = _lib.TqConvDesc()
    d.B, d.T_in, d.T_out, d.C_in0, d.C_in1, d.C_out = B, T, T, Ci, 0, 2 * Co
    d.ktaps, d.stride, d.pad, d.upsample = 3, 1, 1, 0
    d.flags, d.wfmt = _lib.TQ_CONV_POLY2, scheme
    rc = lib.tq_conv1d_fwd(C_.byref(d), xd.data_ptr(), None, None, None, wp.data_ptr(), None, None, None, y.data_ptr(), None,
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    fold = lambda a: a.reshape(B, T, 2, Co).reshape(B, 2 * T, Co)
    _hold("64->2x64 k3 T128 two-phase", "poly2", scheme, y, fold(M.conv1d_model(x, w2, scheme)), fold(M.conv1d_exact(x, w2)))


# ------------------------------------------------------------------------------------------------ data gradient
def _dgrad(dy, w, scheme, split=None, amax=None):
    from tqdne_amd import ops
    g0, g1, _ = ops.conv1d_bwd_data(_g(dy), _g(w), split=split, wfmt=scheme, dy_amax=amax)
    torch.cuda.synchronize()
    return g0 if g1 is None else torch.cat([g0, g1], -1)


def _amax(dy, times8=False):
    """the amax block of tq_colsum for dy and the word the kernel will take from it; times8: every word's exponent raised by three (an
    upper bound 8 times too large -- the header promises any bound within that factor)"""
    from tqdne_amd import ops
    blk = ops.amax_bits(_g(dy))
    word = int(blk.max().item())
    assert word == int(np.abs(dy).max().view(np.uint32)), "tq_colsum amax"
    if times8:
        blk = torch.where(blk > 0, blk + (3 << 23), blk)
        word += 3 << 23
    return blk, word


DGRAD_CASES = [(128, 64, None, 5, 130), (128, 128, 64, 3, 65), (64, 64, None, 1, 31)]   # C_dy, C_dx, split, k, T


@pytest.mark.parametrize("scheme", [S0, S2], ids=lambda s: M.SCHEME_NAME[s])
@pytest.mark.parametrize("cdy,cdx,split,k,T", DGRAD_CASES)
def test_data_gradient(cdy, cdx, split, k, T, scheme):
    rng = np.random.default_rng(cdy + cdx + k + T)
    w = _weights(rng, cdy, cdx, k)
    base = _rand(rng, 2, T, cdy)
    for scale in (1e-9, 1e-5, 1.0, 2e3):
        dy = (base * np.float32(scale)).astype(np.float32)
        exact = M.dgrad_exact(dy, w)
        for times8 in ((False, True) if scheme == S2 else (False,)):
            blk, word = _amax(dy, times8) if scheme == S2 else (None, None)
            y = _dgrad(dy, w, scheme, split=split, amax=blk)
            _hold(f"{cdy}->{cdx} k{k} T{T} dy {scale:g}{' amax x8' if times8 else ''}", "dgrad", scheme, y,
                  M.dgrad_model(dy, w, scheme, word), exact)


def test_data_gradient_samples_of_different_scale_under_one_amax():
    """one batch whose samples differ by 1, 1e-3 and 1e-6 in scale: the shared amax puts the largest sample at 2^13 and the others as far
    below as they are -- each sample is held to the model; its error against exact fp64 is what the scheme gives it (printed)"""
    rng = np.random.default_rng(9)
    cdy, cdx, k, T = 128, 64, 5, 130
    w = _weights(rng, cdy, cdx, k)
    dy = _rand(rng, 3, T, cdy) * np.array([1.0, 1e-3, 1e-6], np.float32)[:, None, None]
    exact = M.dgrad_exact(dy, w)
    for scheme in (S0, S2):
        blk, word = _amax(dy) if scheme == S2 else (None, None)
        y = _dgrad(dy, w, scheme, amax=blk).cpu().numpy().astype(np.float64)
        model = M.dgrad_model(dy, w, scheme, word)
        for b, s in enumerate((1.0, 1e-3, 1e-6)):
            em = M.channel_err(y[b], model[b])
            mx = float(np.abs(model[b] - exact[b]).max() / np.abs(exact[b]).max())
            kx = float(np.abs(y[b] - exact[b]).max() / np.abs(exact[b]).max())
            print(f"DYSAMPLE {M.SCHEME_NAME[scheme]:8s} sample scale {s:g}: e_m {em:.2e}  model-vs-exact {mx:.2e}  kernel-vs-exact {kx:.2e}")
            assert em <= BAR["dgrad", scheme], (scheme, s, em)
            if s == 1.0 or scheme == S0:
                assert kx < TOL


# ------------------------------------------------------------------------------------------------ range sweep
W_SCALES = (1.0, 1e-3, 1e-5, 1e-6, 1e-7, 1e-9)      # times 1 / sqrt(fan_in)
X_SCALES = (1e3, 1.0, 1e-3, 1e-5, 1e-6)
# cells inside the envelope include/tqdne_hip.h states (weights: typical magnitude; activations: scale): held to 1e-4 against fp64 too
ENVELOPE = {S0: lambda ws, xs: True,
            S1: lambda ws, xs: ws == 1.0 and xs == 1.0,
            S2: lambda ws, xs: ws >= 1e-3 and 1e-3 <= xs <= 1e3}


def _sweep_family(base, scheme, ws):
    """cells whose weights lie in fp16's subnormal range have a bar of their own in the fp16 schemes (see BAR)"""
    return base + "_sub" if scheme != S0 and ws in (1e-5, 1e-6) else base


def _sweep_cells(rng):
    """(tag, weight scale, activation scale, weights, activations) on 64 -> 128, k = 5, T = 128, B = 1; the activation tensor has the
    conv's input width for the forward (64) -- the data gradient draws its own"""
    w0 = _weights(rng, 128, 64, 5)
    cells = [(f"w {ws:g} x {xs:g}", ws, xs, (w0 * np.float32(ws)).astype(np.float32)) for ws in W_SCALES for xs in X_SCALES]
    return w0, cells


def _variants(rng, x, w, axis_blocks_w):
    """one hot channel x 1e3 inside a 16-block on either operand; 2 % heavy tails x 30 on either operand"""
    out = []
    xh = x.copy(); xh[..., 21] *= 1e3
    out.append(("hot activation channel", xh, w))
    wh = w.copy()
    if axis_blocks_w == 1:
        wh[:, 21, :] *= 1e3
    else:
        wh[21, :, :] *= 1e3
    out.append(("hot weight channel", x, wh))
    xt = x.copy(); xt[rng.random(x.shape) < 0.02] *= 30
    out.append(("heavy-tailed activations", xt, w))
    wt = w.copy(); wt[rng.random(w.shape) < 0.02] *= 30
    out.append(("heavy-tailed weights", x, wt))
    return out


@pytest.mark.parametrize("scheme", M.SCHEMES, ids=lambda s: M.SCHEME_NAME[s])
def test_range_sweep_forward(scheme):
    rng = np.random.default_rng(5)
    x0 = _rand(rng, 1, 128, 64)
    w0, cells = _sweep_cells(rng)
    for tag, ws, xs, w in cells:
        x = (x0 * np.float32(xs)).astype(np.float32)
        inside = ENVELOPE[scheme](ws, xs)
        em, mx, kx = _hold("sweep " + tag, _sweep_family("sweep", scheme, ws), scheme, _forward(x, w, scheme), M.conv1d_model(x, w, scheme),
                           M.conv1d_exact(x, w), envelope=inside)
        print(f"RANGE fwd {M.SCHEME_NAME[scheme]} | {ws:g} | {xs:g} | {kx:.1e} | {mx:.1e} | {'in' if inside else 'out'}")
    for tag, x, w in _variants(rng, x0, w0, 1):
        em, mx, kx = _hold("sweep " + tag, "sweep", scheme, _forward(x, w, scheme), M.conv1d_model(x, w, scheme), M.conv1d_exact(x, w),
                           envelope=False)
        print(f"RANGE fwd {M.SCHEME_NAME[scheme]} | {tag} | | {kx:.1e} | {mx:.1e} |")


@pytest.mark.parametrize("scheme", [S0, S2], ids=lambda s: M.SCHEME_NAME[s])
def test_range_sweep_data_gradient(scheme):
    rng = np.random.default_rng(6)
    dy0 = _rand(rng, 1, 128, 128)
    w0, cells = _sweep_cells(rng)
    env = (lambda ws, xs: True) if scheme == S0 else (lambda ws, xs: ws >= 1e-3)    # dy is scaled into range whatever its size
    def run(tag, dy, w, inside, ws=1.0):
        blk, word = _amax(dy) if scheme == S2 else (None, None)
        return _hold("sweep " + tag, _sweep_family("dsweep", scheme, ws), scheme, _dgrad(dy, w, scheme, amax=blk), M.dgrad_model(dy, w, scheme, word),
                     M.dgrad_exact(dy, w), envelope=inside)
    for tag, ws, xs, w in cells:
        inside = env(ws, xs)
        em, mx, kx = run(tag, (dy0 * np.float32(xs)).astype(np.float32), w, inside, ws)
        print(f"RANGE dgrad {M.SCHEME_NAME[scheme]} | {ws:g} | {xs:g} | {kx:.1e} | {mx:.1e} | {'in' if inside else 'out'}")
    for tag, dy, w in _variants(rng, dy0, w0, 0):
        em, mx, kx = run(tag, dy, w, False)
        print(f"RANGE dgrad {M.SCHEME_NAME[scheme]} | {tag} | | {kx:.1e} | {mx:.1e} |")
