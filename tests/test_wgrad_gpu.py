"""The conv weight gradient (wgrad_kernel + wgrad_reduce_kernel, csrc/backward.hip) in every kernel form and split regime, against
float64 and against the bit-model of its bf16x3 contraction (oracle/contraction.py: wgrad_exact, wgrad_model).

Every case runs the same steps (_run): the slab workspace and a guard tail behind it are filled with NaN, dw sits between NaN guard
bands; the launch runs twice and dw must be bit-identical (no atomics on that path); no NaN may reach dw -- so every slab element the
reduction reads was written by a workgroup -- and the guards (behind the queried byte count, and behind the launch's own n_splits slabs)
must be bit-unchanged.  The plan is read through tq_conv1d_bwd_weight_plan and each case ASSERTS the regime it is named for (form, units
per split, a split that crosses a sample, a shorter last split, the n_splits regime of the reduction, the block order): a case that is
not in its regime fails.  Samples differ visibly: sample b carries dy times 1 + b % 3, x times 1 + (b + 1) % 3 and its own gscale /
gshift rows, so a mix-up between neighbouring samples is orders above the bars.

Metric: e = max|dw - ref| / max|ref| per OUTPUT channel, the worst channel (wgrad_channel_err).
  * against float64 exact: 1e-4 (TOL), every case;
  * launches that stage no SiLU, against the model (operands split RNE / RNE, three exact products, float64 sums): BAR[form] = 4 x the
    worst e_m measured per form on one MI355X (DESIGN_LOG.md, "Weight gradient against its bit-model") -- room for another accumulation
    order, nothing else.  Inside every such comparison the bar must be at most one fifth of the error of the model with ONE cross product
    left out on the same data, so a dropped product cannot pass;
  * launches that stage SiLU: exp2 / rcp of the kernel flip the low part of some staged values (as found for the forward,
    tests/test_contraction_gpu.py), so they are held to BAR_SILU[form] = 4 x the worst e_m measured against the STAGED model
    (staged_gn_silu, then the dropout mask) WITHOUT the one-fifth condition, besides the 1e-4 against float64.
`pytest -s` prints every figure.

Shapes (confirmed with the query on one MI355X: 512 workgroup slots for C32 at k = 3 / 5, C128 and H64, 768 for C32 / C64 at k = 1, 256 for
W8); each is the smallest batch at its length that reaches the regime (the C32 256 -> 256 k5 row: the first with three units per split):

  multi-unit splits (GN + SiLU prologue; units per split / splits / units of the last split)
    H64   64 -> 64        k5  B 103 T 300   2 / 258 / 1   dropout        H64   128+64 -> 64    k5  B 35 T 300   2 / 88 / 1   concat, XCD order
    H64   64+64 -> 64     k3  B 53  T 300   2 / 133 / 1   concat         W8    128+128 -> 256  k5  B 7  T 300   2 / 18 / 1   concat, dropout
    W8    128+128 -> 256  k3  B 17  T 200   3 / 23 / 2    concat         C32   256 -> 256      k5  B 13 T 300   3 / 22 / 2   fused sums, dropout
    C32   96+32 -> 160    k5  B 13  T 300   2 / 33 / 1    concat         C32   256 -> 256      k3  B 17 T 200   3 / 23 / 2   fused sums
    C32   96 -> 96        k1  B 53  T 300   2 / 133 / 1   dropout        C32   96+32 -> 96     k1  B 39 T 300   2 / 98 / 1   concat
    C64   192+64 -> 320   k1  B 13  T 300   2 / 33 / 1    fused sums, concat, dropout (and once without the sums)
    C128  128+128 -> 768  k1  B 9   T 300   2 / 23 / 1    concat, dropout C128  256 -> 768      k1  B 9  T 300   2 / 23 / 1   fused sums
    stride 2 (k3):  W8  256 -> 256  B 7  T_in 599  2 / 18 / 1      C32  160 -> 160  B 11  T_in 600  2 / 28 / 1
    upsample:       W8  256 -> 256  B 7  T_in 150  k3 and k5  2 / 18 / 1      C32  160 -> 160  B 11  T_in 150  k3 and k5  2 / 28 / 1
    the paper UNet's T = 4096 level at B = 64 has 8 units per split in H64; its smallest relative, 64 -> 64 k5 B 9 T 4059 (2 units per
    split, 288 full splits, none crossing a sample: 64 units per sample), runs as a case of its own
  reduce regimes: 32 -> 32, T 40, k in {1, 3, 5}, B = n_splits in {16, 17, 32, 33, 48, 49, 97}
  block order: per form B = 2 (4 pairs, plain) and B = 4 (8 pairs, XCD) at T = 100
  partial output tiles: 96+32 -> 160 k5, 64 -> 96 k3, 128 -> 192 k3, plain and with the fused sums into all three destinations
  tile edges: per form B = 2, T in {1, 2, 63, 64, 65, 128, 129}; stride 2 with T_in in {1, 2, 127, 128, 129, 130}"""

import ctypes as C_

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import contraction as M

pytestmark = pytest.mark.gpu

TOL = 1e-4        # against float64, per output channel
CS_TOL = 1e-5     # fused column sums against float64
GUARD = 4096      # floats of NaN behind the workspace and on both sides of dw
NAN_BITS = 0x7FC00000

# 4 x the worst e_m measured per form on one MI355X (DESIGN_LOG.md)
BAR = {"C32": 4 * 2.93e-7, "C64": 4 * 2.42e-7, "C128": 4 * 3.20e-7, "W8": 4 * 2.82e-7, "H64": 4 * 2.78e-7}
BAR_SILU = {"C32": 4 * 1.71e-6, "C64": 4 * 1.97e-6, "C128": 4 * 1.95e-6, "W8": 4 * 2.43e-6, "H64": 4 * 1.54e-6}


def dev():
    return torch.device("cuda:0")


def _g(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev())


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev())


def _all_nan_bits(t):
    return bool((t.view(torch.int32) == NAN_BITS).all())


def _t_out(T_in, stride, up):
    return (T_in + 2 - 3) // 2 + 1 if stride == 2 else (2 * T_in if up else T_in)


def _run(tag, B, T_in, C0, C1, Co, K, stride=1, up=False, gn=True, silu=False, drop=0.0, cs=None):
    """one case, all steps of the file's header; returns the plan of the launch.  cs: None | "bc" | "bc+c" | "all" (bc, c and c2)"""
    from tqdne_amd import _lib, ops
    lib = _lib.load()
    seed = (B * 7919 + T_in * 104729 + C0 * 31 + C1 * 29 + Co * 17 + K) % (1 << 31)
    rng = np.random.default_rng([B, T_in, C0, C1, Co, K, stride, int(up)])
    Cin, T_out = C0 + C1, _t_out(T_in, stride, up)
    sb = (1.0 + (np.arange(B) % 3)).astype(np.float32)[:, None, None]
    dy = rng.standard_normal((B, T_out, Co)).astype(np.float32) * sb
    x = rng.standard_normal((B, T_in, Cin)).astype(np.float32) * np.roll(sb, 1, axis=0)
    a = s = None
    if gn:
        a = (1.0 + 0.5 * rng.standard_normal((B, Cin))).astype(np.float32)
        s = rng.standard_normal((B, Cin)).astype(np.float32)
    xhat = x if not gn else (M.staged_gn_silu(x, a, s) if silu else M.staged_gn(x, a, s))
    assert gn or not silu
    site, dseed = 3, 0x1234567 + seed
    if drop:
        xhat = M.staged_dropout(xhat, dseed, site, drop)
    exact = M.wgrad_exact(dy, xhat, K, stride, up)
    prods = M.wgrad_products(dy, xhat, K, stride, up)
    model = M.wgrad_model(dy, xhat, K, stride, up, products=prods)

    with_cs = cs is not None
    d = ops.wgrad_desc(B, T_in, T_out, C0, C1, Co, K, stride, up)
    plan = ops.conv1d_bwd_weight_plan(d, with_cs)
    need = lib.tq_conv1d_bwd_weight_workspace(C_.byref(d))
    assert need % 4 == 0 and plan["workspace_bytes"] <= need
    n = Co * Cin * K
    dy_d, x0_d, x1_d = _g(dy), _g(x[:, :, :C0]), (_g(x[:, :, C0:]) if C1 else None)
    kw = dict(x1=x1_d, gscale=_g(a), gshift=_g(s), silu=silu, stride=stride, upsample=up, dropout_p=drop, dropout_seed=dseed, dropout_site=site)
    starts = None
    if with_cs:
        starts = (rng.standard_normal((B, Co)).astype(np.float32), rng.standard_normal(Co).astype(np.float32) if cs != "bc" else None,
                  rng.standard_normal(Co).astype(np.float32) if cs == "all" else None)
    results = []
    for _ in range(2):
        wsbuf, dwbuf = _nan(need // 4 + GUARD), _nan(n + 2 * GUARD)
        dw = dwbuf[GUARD:GUARD + n].view(Co, Cin, K)
        sums = tuple(_g(t) for t in starts) if with_cs else None
        ops.conv1d_bwd_weight(dy_d, x0_d, (Co, Cin, K), out=dw, workspace=wsbuf.view(torch.uint8)[:need], colsum=sums, **kw)
        torch.cuda.synchronize()
        assert _all_nan_bits(wsbuf[need // 4:]), f"{tag}: the guard behind the queried workspace was written"
        assert _all_nan_bits(wsbuf[plan['workspace_bytes'] // 4:]), f"{tag}: written behind the launch's own n_splits slabs"
        assert _all_nan_bits(dwbuf[:GUARD]) and _all_nan_bits(dwbuf[GUARD + n:]), f"{tag}: a guard band of dw was written"
        assert not bool(torch.isnan(dw).any()), f"{tag}: NaN in dw -- a slab element the reduction reads was never written"
        results.append((dw.clone(), sums))
    assert torch.equal(results[0][0], results[1][0]), f"{tag}: two launches differ in dw"
    got = results[0][0].cpu().numpy().astype(np.float64)

    form = plan["form_name"]
    kx = M.wgrad_channel_err(got, exact)
    em = M.wgrad_channel_err(got, model)
    mx = M.wgrad_channel_err(model, exact)
    lo = min(M.wgrad_channel_err(model - prods[name], exact) for name in ("lo_hi", "hi_lo"))
    print(f"WGRAD {form:4s} {'silu ' if silu else 'model'} {tag:40s} e_m {em:.2e}  model-vs-exact {mx:.2e}  one-product-left-out {lo:.2e}  "
          f"kernel-vs-exact {kx:.2e}  ups {plan['units_per_split']} splits {plan['n_splits']} last {plan['last_split']} xcd {plan['xcd_order']}")
    assert kx < TOL, f"{tag}: {kx:.3e} against float64"
    if silu:
        assert em <= BAR_SILU[form], f"{tag}: e_m {em:.3e} against the staged model above the bar {BAR_SILU[form]:.1e}"
    else:
        assert em <= BAR[form], f"{tag}: e_m {em:.3e} above the bar {BAR[form]:.1e}"
        assert BAR[form] <= lo / 5, f"{tag}: bar {BAR[form]:.1e} is not one fifth of a left-out cross product's error {lo:.2e}"
    if with_cs:
        dyt = torch.from_numpy(dy).double()
        for r, (_, sums) in enumerate(results):
            bc, c1, c2 = sums
            assert rel_err(bc.cpu(), torch.from_numpy(starts[0]).double() + dyt.sum(1)) < CS_TOL, f"{tag}: colsum_bc, launch {r}"
            if c1 is not None:
                assert rel_err(c1.cpu(), torch.from_numpy(starts[1]).double() + dyt.sum((0, 1))) < CS_TOL, f"{tag}: colsum_c, launch {r}"
            if c2 is not None:
                assert rel_err(c2.cpu(), torch.from_numpy(starts[2]).double() + dyt.sum((0, 1))) < CS_TOL, f"{tag}: colsum_c2, launch {r}"
    return plan


# ------------------------------------------------------------------------------------------------ multi-unit splits
# (form, B, T_in, C_in0, C_in1, C_out, k, stride, upsample, dropout p, fused sums, (units per split, splits, units of the last split))
MULTI = [
    ("H64", 103, 300, 64, 0, 64, 5, 1, False, 0.25, None, (2, 258, 1)),
    ("H64", 35, 300, 128, 64, 64, 5, 1, False, 0.0, None, (2, 88, 1)),
    ("H64", 53, 300, 64, 64, 64, 3, 1, False, 0.0, None, (2, 133, 1)),
    ("W8", 7, 300, 128, 128, 256, 5, 1, False, 0.25, None, (2, 18, 1)),
    ("W8", 17, 200, 128, 128, 256, 3, 1, False, 0.0, None, (3, 23, 2)),
    ("C32", 13, 300, 256, 0, 256, 5, 1, False, 0.25, "all", (3, 22, 2)),
    ("C32", 13, 300, 96, 32, 160, 5, 1, False, 0.0, None, (2, 33, 1)),
    ("C32", 17, 200, 256, 0, 256, 3, 1, False, 0.0, "bc+c", (3, 23, 2)),
    ("C32", 53, 300, 96, 0, 96, 1, 1, False, 0.25, None, (2, 133, 1)),
    ("C32", 39, 300, 96, 32, 96, 1, 1, False, 0.0, None, (2, 98, 1)),
    ("C64", 13, 300, 192, 64, 320, 1, 1, False, 0.25, "all", (2, 33, 1)),
    ("C64", 13, 300, 192, 64, 320, 1, 1, False, 0.0, None, (2, 33, 1)),
    ("C128", 9, 300, 128, 128, 768, 1, 1, False, 0.25, None, (2, 23, 1)),
    ("C128", 9, 300, 256, 0, 768, 1, 1, False, 0.0, "bc", (2, 23, 1)),
    ("W8", 7, 599, 256, 0, 256, 3, 2, False, 0.0, None, (2, 18, 1)),
    ("C32", 11, 600, 160, 0, 160, 3, 2, False, 0.0, None, (2, 28, 1)),
    ("W8", 7, 150, 256, 0, 256, 3, 1, True, 0.0, None, (2, 18, 1)),
    ("W8", 7, 150, 256, 0, 256, 5, 1, True, 0.0, None, (2, 18, 1)),
    ("C32", 11, 150, 160, 0, 160, 3, 1, True, 0.0, None, (2, 28, 1)),
    ("C32", 11, 150, 160, 0, 160, 5, 1, True, 0.0, None, (2, 28, 1)),
]


def _id(c):
    form, B, T, C0, C1, Co, K, s, up, p, cs = c[:11]
    return f"{form}-{C0}+{C1}to{Co}-k{K}" + ("-s2" if s == 2 else "") + ("-up" if up else "") + f"-B{B}-T{T}" + ("-drop" if p else "") + (f"-cs_{cs}" if cs else "")


@pytest.mark.parametrize("case", MULTI, ids=_id)
def test_multi_unit_splits(case):
    """several units per split, a split that crosses a sample (gscale / gshift reload, dropout key, column-sum flush), a shorter last
    split -- with the GN + SiLU prologue on"""
    form, B, T_in, C0, C1, Co, K, stride, up, p, cs, regime = case
    plan = _run(_id(case), B, T_in, C0, C1, Co, K, stride, up, gn=True, silu=True, drop=p, cs=cs)
    ups = plan["units_per_split"]
    assert plan["form_name"] == form, plan
    assert ups >= 2 and plan["n_ttiles"] % ups != 0 and plan["crosses_sample"] and plan["last_split"] < ups, plan
    assert (ups, plan["n_splits"], plan["last_split"]) == regime, plan


def test_h64_long_samples_two_units_per_split():
    """the H64 plan of the paper UNet's longest level in small: 64 units per sample, 2 per split, 288 full splits inside their samples"""
    plan = _run("H64-64to64-k5-B9-T4059", 9, 4059, 64, 0, 64, 5, gn=True, silu=True, drop=0.1)
    assert plan["form_name"] == "H64" and (plan["units_per_split"], plan["n_splits"], plan["last_split"]) == (2, 288, 2), plan
    assert plan["n_ttiles"] == 64 and not plan["crosses_sample"]


def test_multi_unit_table_covers_what_it_must():
    """per form: dropout once, a concat source once; stride 2 and upsampling (k = 3 and 5) in the W8 and the C32 form; fused sums with a
    sample change in the C32 and the C64 form"""
    forms = ("C32", "C64", "C128", "W8", "H64")
    for f in forms:
        assert any(c[0] == f and c[9] > 0 for c in MULTI), f
        assert any(c[0] == f and c[4] > 0 for c in MULTI), f
    for f in ("W8", "C32"):
        assert any(c[0] == f and c[7] == 2 and c[6] == 3 for c in MULTI), f
        assert {c[6] for c in MULTI if c[0] == f and c[8]} == {3, 5}, f
    for f in ("C32", "C64"):
        assert any(c[0] == f and c[10] for c in MULTI), f


# ------------------------------------------------------------------------------------------------ reduce regimes
@pytest.mark.parametrize("B", [16, 17, 32, 33, 48, 49, 97])
@pytest.mark.parametrize("K", [1, 3, 5])
def test_reduce_regimes(K, B):
    """wgrad_reduce_kernel by n_splits: <= 16 the tail only, 17 - 32 one loop pass, 33 - 48 a pass and the tail, > 48 two passes and more
    -- with one unit per sample, so every split holds real data of its own sample"""
    plan = _run(f"reduce-k{K}-B{B}", B, 40, 32, 0, 32, K, gn=True)
    assert plan["n_units"] == B and plan["n_splits"] == B and plan["units_per_split"] == 1, plan
    assert plan["form_name"] == "C32"


# ------------------------------------------------------------------------------------------------ block order
ORDER = {"C32": (96, 0, 96, 5, None), "C32-sums": (64, 0, 64, 5, "bc+c"), "C64": (64, 0, 128, 1, None), "C128": (128, 0, 128, 1, None),
         "W8": (64, 0, 128, 3, None), "H64": (64, 0, 64, 3, None)}


@pytest.mark.parametrize("xcd", [0, 1], ids=["plain", "xcd"])
@pytest.mark.parametrize("name", list(ORDER))
def test_block_order(name, xcd):
    """both workgroup numberings of every form (8 | n_splits * n_cotiles or not), without a prologue"""
    C0, C1, Co, K, cs = ORDER[name]
    B = 4 if xcd else 2
    plan = _run(f"order-{name}-{'xcd' if xcd else 'plain'}", B, 100, C0, C1, Co, K, gn=False, cs=cs)
    assert plan["form_name"] == name.split("-")[0] and plan["xcd_order"] == xcd, plan
    assert plan["n_cichunks"] * plan["n_cotiles"] >= 1 and plan["n_splits"] == 2 * B


def test_block_order_with_several_input_chunks_and_output_tiles():
    """the XCD numbering with n_cichunks > 1 and n_cotiles > 1 (where sp / ct and the chunk index really differ), and its plain twin"""
    for B, xcd in ((4, 1), (3, 0)):
        for form, (C0, C1, Co, K) in {"C32": (96, 32, 256, 3), "W8": (128, 64, 256, 5), "C64": (64, 64, 256, 1), "C128": (128, 128, 256, 1),
                                      "H64": (128, 64, 64, 5)}.items():
            plan = _run(f"order2-{form}-B{B}", B, 100, C0, C1, Co, K, gn=True)
            assert plan["form_name"] == form and plan["xcd_order"] == xcd and plan["n_cichunks"] > 1, plan
            assert form == "H64" or plan["n_cotiles"] == 2


# ------------------------------------------------------------------------------------------------ partial output tiles
@pytest.mark.parametrize("cs", [None, "all"], ids=["plain", "sums"])
@pytest.mark.parametrize("shape", [(96, 32, 160, 5), (64, 0, 96, 3), (128, 0, 192, 3)], ids=lambda s: f"{s[0]}+{s[1]}to{s[2]}-k{s[3]}")
def test_partial_output_tiles(shape, cs):
    """C_out that is not a multiple of the 128-channel tile, plain and with the fused sums accumulated onto non-zero values in all
    three destinations"""
    C0, C1, Co, K = shape
    plan = _run(f"partial-{C0}+{C1}to{Co}-k{K}-{cs}", 3, 130, C0, C1, Co, K, gn=True, cs=cs)
    assert plan["form_name"] == "C32" and plan["n_cotiles"] == (Co + 127) // 128 and Co % 128 != 0, plan


# ------------------------------------------------------------------------------------------------ tile edges
EDGE = {"C32": (96, 0, 96, 5), "C64": (64, 0, 128, 1), "C128": (128, 0, 128, 1), "W8": (64, 0, 128, 3), "H64": (64, 0, 64, 5)}


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 128, 129])
@pytest.mark.parametrize("form", list(EDGE))
def test_tile_edges(form, T):
    C0, C1, Co, K = EDGE[form]
    plan = _run(f"edge-{form}-T{T}", 2, T, C0, C1, Co, K, gn=True)
    assert plan["form_name"] == form and plan["n_ttiles"] == (T + 63) // 64, plan


@pytest.mark.parametrize("T_in", [1, 2, 127, 128, 129, 130])
@pytest.mark.parametrize("form", ["C32", "W8"])
def test_tile_edges_stride_2(form, T_in):
    C0, C1, Co, K = EDGE[form]
    plan = _run(f"edge-s2-{form}-T{T_in}", 2, T_in, C0, C1, Co, 3, stride=2, gn=True)
    assert plan["form_name"] == form and plan["n_ttiles"] == ((T_in - 1) // 2 + 1 + 63) // 64, plan


# ------------------------------------------------------------------------------------------------ workspace contract
def test_workspace_one_byte_short_is_refused():
    from tqdne_amd import _lib, ops
    lib = _lib.load()
    B, T, Cn, K = 3, 100, 64, 5
    d = ops.wgrad_desc(B, T, T, Cn, 0, Cn, K)
    need = lib.tq_conv1d_bwd_weight_workspace(C_.byref(d))
    dy, x = torch.randn(B, T, Cn, device=dev()), torch.randn(B, T, Cn, device=dev())
    ws = torch.zeros(need, dtype=torch.uint8, device=dev())
    dw = torch.full((Cn, Cn, K), 7.0, device=dev())
    for cs in (None, (torch.zeros(B, Cn, device=dev()), None)):
        with pytest.raises(_lib.TqError, match="TQ_ERR_ARG"):
            ops.conv1d_bwd_weight(dy, x, (Cn, Cn, K), out=dw, workspace=ws[:need - 1], colsum=cs)
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all())     # nothing was launched
    ops.conv1d_bwd_weight(dy, x, (Cn, Cn, K), out=dw, workspace=ws)
    assert not bool((dw == 7.0).any())
