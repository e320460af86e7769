"""Weight gradient, host side (no GPU): the float64 / bit-model references of oracle/contraction.py against torch autograd, and the plan
query tq_conv1d_bwd_weight_plan -- its argument checks and, on a table of descriptors, the invariants every plan must satisfy.  The
slots behind a plan come from the device where there is one, so the table asserts invariants and form rules, never slot counts."""

import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import contraction as M

ERR_ARG, ERR_SHAPE = -1, -2


# ------------------------------------------------------------------------------------------------ references against autograd
def _autograd_dw(dy, xhat, K, stride, upsample):
    """float64 autograd of the conv on the staged activation (channels-last in, torch layout inside)"""
    x = torch.from_numpy(np.asarray(xhat, np.float64)).permute(0, 2, 1)
    if upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    Co, Ci = dy.shape[2], xhat.shape[2]
    w = torch.zeros(Co, Ci, K, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(x, w, None, stride=stride, padding=K // 2 if stride == 1 else 1)
    y.backward(torch.from_numpy(np.asarray(dy, np.float64)).permute(0, 2, 1))
    return w.grad.numpy()


@pytest.mark.parametrize("K,stride,upsample,T_in", [(1, 1, False, 70), (3, 1, False, 70), (5, 1, False, 1), (5, 1, False, 70),
                                                    (3, 2, False, 70), (3, 2, False, 71), (3, 2, False, 1), (3, 1, True, 35),
                                                    (5, 1, True, 35), (5, 1, True, 1)])
def test_wgrad_references_against_float64_autograd(K, stride, upsample, T_in):
    rng = np.random.default_rng(K * 100 + stride * 10 + T_in)
    B, Ci, Co = 3, 32, 48
    T_out = (T_in + 2 - 3) // 2 + 1 if stride == 2 else (2 * T_in if upsample else T_in)
    xhat = rng.standard_normal((B, T_in, Ci)).astype(np.float32)
    dy = rng.standard_normal((B, T_out, Co)).astype(np.float32)
    ref = _autograd_dw(dy, xhat, K, stride, upsample)
    ex = M.wgrad_exact(dy, xhat, K, stride, upsample)
    assert ex.shape == (Co, Ci, K) and ex.dtype == np.float64
    assert M.wgrad_channel_err(ex, ref) < 1e-13
    # the bit-model: three products of bf16 halves -- the lo lo term (2^-16 of each operand, squared) is all that is missing
    prods = M.wgrad_products(dy, xhat, K, stride, upsample)
    model = M.wgrad_model(dy, xhat, K, stride, upsample)
    assert np.array_equal(model, M.wgrad_model(dy, xhat, K, stride, upsample, products=prods))
    e_model = M.wgrad_channel_err(model, ref)
    assert e_model < 2e-5, e_model
    # one cross product left out is two orders above the model's own error: what the GPU tests size their bars against
    for name in ("lo_hi", "hi_lo"):
        out = M.wgrad_model(dy, xhat, K, stride, upsample, leave_out=name, products=prods)
        assert np.allclose(out + prods[name], model, rtol=0, atol=1e-12 * np.abs(model).max())
        assert M.wgrad_channel_err(out, ref) > 50 * e_model, name
    # operands that are exactly bf16 leave nothing to the low parts: model == exact
    xb, db = M.bf16_rne(xhat), M.bf16_rne(dy)
    assert M.wgrad_channel_err(M.wgrad_model(db, xb, K, stride, upsample), M.wgrad_exact(db, xb, K, stride, upsample)) < 1e-13


def test_staged_prologue_of_the_weight_gradient():
    """staged_gn / staged_gn_silu / staged_dropout against torch in float64, and the dropout mask's contract: per-sample keys, the
    element index t * C + c, kept values times 1 / (1 - p)"""
    from oracle.dropout import dropout_scale_mask
    rng = np.random.default_rng(5)
    B, T, Cn = 3, 37, 64
    x = rng.standard_normal((B, T, Cn)).astype(np.float32)
    a, s = rng.standard_normal((B, Cn)).astype(np.float32), rng.standard_normal((B, Cn)).astype(np.float32)
    u = torch.from_numpy(x).double() * torch.from_numpy(a).double()[:, None] + torch.from_numpy(s).double()[:, None]
    assert np.abs(M.staged_gn(x, a, s) - u.numpy()).max() < 1e-6
    assert np.abs(M.staged_gn_silu(x, a, s) - F.silu(u).numpy()).max() < 1e-6
    p = 0.25
    m = dropout_scale_mask(77, 3, B, T, Cn, p)
    assert set(np.unique(m)) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(p))}
    assert abs(float((m == 0).mean()) - p) < 0.03
    assert not np.array_equal(m[0], m[1]) and not np.array_equal(m, dropout_scale_mask(77, 4, B, T, Cn, p))
    assert np.array_equal(dropout_scale_mask(77, 3, B, 5, Cn, p), m[:, :5])      # element index t * C + c: a prefix in t
    assert np.array_equal(M.staged_dropout(x, 77, 3, p), x * m)


# ------------------------------------------------------------------------------------------------ the plan query
def _lib():
    from tqdne_amd import _build, _lib
    _build.build(verbose=False)
    return _lib, _lib.load()


def _desc(B, T_in, C0, C1, Co, K, stride=1, upsample=False):
    from tqdne_amd import ops
    T_out = (T_in + 2 - 3) // 2 + 1 if stride == 2 else (2 * T_in if upsample else T_in)
    return ops.wgrad_desc(B, T_in, T_out, C0, C1, Co, K, stride, upsample)


def test_plan_query_is_declared_exported_and_bound():
    import os
    import re
    from conftest import ROOT
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "tqdne_hip.h")).read()
    assert re.search(r"\bint\s+tq_conv1d_bwd_weight_plan\s*\(\s*const TqConvDesc\*\s*desc,\s*int with_colsum,\s*TqWgradPlan\*\s*out\)", header)
    assert "tq_conv1d_bwd_weight_plan" in L.exported_symbols() and hasattr(lib, "tq_conv1d_bwd_weight_plan")
    assert lib.tq_abi_version() == L.ABI_VERSION
    for name in ("C32", "C64", "C128", "W8", "H64"):     # the enum of the header is the binding's
        v = int(re.search(r"#define\s+TQ_WGRAD_%s\s+(\d+)" % name, header).group(1))
        assert getattr(L, "TQ_WGRAD_" + name) == v and L.WGRAD_FORM_NAME[v] == name
    assert "tq_conv1d_bwd_weight_plan" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_plan_query_argument_checks():
    L, lib = _lib()
    out = L.TqWgradPlan()
    good = _desc(2, 100, 64, 0, 64, 5)
    assert lib.tq_conv1d_bwd_weight_plan(None, 0, C.byref(out)) == ERR_ARG
    assert lib.tq_conv1d_bwd_weight_plan(C.byref(good), 0, None) == ERR_ARG
    assert lib.tq_conv1d_bwd_weight_plan(C.byref(good), 0, C.byref(out)) == 0
    sentinel = L.TqWgradPlan(*([-7] * 8))
    bad = []
    for field, value in (("C_in0", 0), ("C_in0", 48), ("C_in1", -32), ("C_in1", 16), ("C_out", 0), ("C_out", 72), ("ktaps", 7), ("ktaps", 2),
                         ("ktaps", 0), ("B", 0), ("B", -1), ("T_in", 0), ("T_out", 0)):
        d = _desc(2, 100, 64, 0, 64, 5)
        setattr(d, field, value)
        bad.append((field, value, d))
    bad.append(("stride 2, k 5", None, _desc(2, 100, 64, 0, 64, 5, stride=2)))
    bad.append(("stride 2, k 1", None, _desc(2, 100, 64, 0, 64, 1, stride=2)))
    bad.append(("upsample, k 1", None, _desc(2, 100, 64, 0, 64, 1, upsample=True)))
    for field, value, d in bad:
        for cs in (0, 1):
            assert lib.tq_conv1d_bwd_weight_plan(C.byref(d), cs, C.byref(sentinel)) == ERR_SHAPE, (field, value)
    assert all(getattr(sentinel, n) == -7 for n, _ in sentinel._fields_)     # a refused query leaves *out alone
    # the launch refuses the same shapes (before the device is touched: this may run without one)
    f = 0x1000   # never dereferenced
    for field, value, d in bad:
        if field in ("B", "T_in", "T_out"):
            continue
        assert lib.tq_conv1d_bwd_weight(C.byref(d), f, f, f, None, None, f, f, 1 << 40, None) == ERR_SHAPE, (field, value)
    assert lib.tq_conv1d_bwd_weight(C.byref(good), f, f, None, None, None, f, f, lib.tq_conv1d_bwd_weight_workspace(C.byref(good)) - 1,
                                    None) == ERR_ARG


# (B, T_in, C_in0, C_in1, C_out, k, stride, upsample): the shapes of the paper UNet's levels, the 1x1 skip / attention convs, partial
# output tiles, concat sources of every chunk width, strided and upsampling convs, batches that force several units per split
PLAN_TABLE = [
    (2, 100, 32, 0, 32, 1, 1, False), (2, 100, 32, 0, 32, 3, 1, False), (2, 100, 32, 0, 32, 5, 1, False), (64, 4096, 64, 0, 64, 5, 1, False),
    (64, 4096, 64, 64, 64, 5, 1, False), (3, 333, 128, 64, 64, 3, 1, False), (5, 65, 192, 0, 64, 5, 1, False), (64, 1024, 128, 0, 128, 5, 1, False),
    (64, 256, 256, 0, 256, 5, 1, False), (7, 300, 128, 128, 256, 5, 1, False), (13, 300, 256, 0, 256, 5, 1, False), (50, 300, 96, 0, 96, 1, 1, False),
    (9, 300, 192, 64, 320, 1, 1, False), (11, 200, 256, 0, 768, 1, 1, False), (64, 256, 256, 0, 768, 1, 1, False), (9, 300, 128, 128, 768, 1, 1, False),
    (20, 300, 96, 32, 160, 5, 1, False), (20, 300, 64, 0, 96, 3, 1, False), (20, 300, 128, 0, 192, 3, 1, False), (20, 300, 160, 0, 160, 1, 1, False),
    (64, 2048, 64, 0, 64, 3, 2, False), (7, 599, 256, 0, 256, 3, 2, False), (11, 600, 160, 0, 160, 3, 2, False), (2, 1, 64, 0, 128, 3, 2, False),
    (64, 512, 128, 0, 128, 3, 1, True), (7, 150, 256, 0, 256, 5, 1, True), (11, 150, 160, 0, 160, 3, 1, True), (64, 128, 256, 0, 256, 5, 1, True),
    (1, 1, 32, 0, 32, 5, 1, False), (97, 40, 32, 0, 32, 5, 1, False), (300, 64, 64, 0, 64, 5, 1, False), (700, 64, 32, 0, 32, 1, 1, False),
    (4, 100, 1024, 0, 1024, 5, 1, False), (4, 100, 1024, 1024, 1024, 1, 1, False), (64, 4096, 64, 0, 3072, 1, 1, False),
    # four and eight (split, output tile) pairs per form: one unit per split and both block orders on any device
    (4, 100, 32, 0, 32, 5, 1, False), (2, 100, 64, 0, 128, 1, 1, False), (4, 100, 64, 0, 128, 1, 1, False), (2, 100, 128, 0, 128, 1, 1, False),
    (4, 100, 128, 0, 128, 1, 1, False), (2, 100, 64, 0, 128, 3, 1, False), (4, 100, 64, 0, 128, 3, 1, False), (2, 100, 64, 0, 64, 5, 1, False),
    (4, 100, 64, 0, 64, 5, 1, False)]


def _expected_form(L, C0, C1, Co, K, stride, upsample, with_colsum):
    """the form rules as the comments of csrc/backward.hip state them (wgrad_nci, wgrad_w8, wgrad_h64, wgrad_form)"""
    whole64 = C0 % 64 == 0 and C1 % 64 == 0
    if not with_colsum and K != 1 and whole64:
        if stride == 1 and not upsample and Co == 64:
            return L.TQ_WGRAD_H64, 64, 64
        if Co % 128 == 0:
            return L.TQ_WGRAD_W8, 128, 64
    if K != 1:
        return L.TQ_WGRAD_C32, 128, 32
    if stride == 1 and not upsample and C0 % 128 == 0 and C1 % 128 == 0:
        return L.TQ_WGRAD_C128, 128, 128
    return (L.TQ_WGRAD_C64, 128, 64) if whole64 else (L.TQ_WGRAD_C32, 128, 32)


@pytest.mark.parametrize("shape", PLAN_TABLE, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_plan_invariants(shape):
    L, lib = _lib()
    from tqdne_amd import ops
    B, T_in, C0, C1, Co, K, stride, upsample = shape
    d = _desc(*shape)
    plans = []
    for cs in (False, True):
        p = ops.conv1d_bwd_weight_plan(d, cs)
        form, cot, chunk = _expected_form(L, C0, C1, Co, K, stride, upsample, cs)
        assert p["form"] == form, (cs, p)
        assert p["n_cotiles"] == (Co + cot - 1) // cot and p["n_cichunks"] * chunk == C0 + C1
        assert p["n_ttiles"] == (d.T_out + 63) // 64 and p["n_units"] == B * p["n_ttiles"]
        ups, ns, U = p["units_per_split"], p["n_splits"], p["n_units"]
        assert ups >= 1 and 1 <= ns <= U
        assert (ns - 1) * ups < U <= ns * ups                  # every unit in exactly one split, no empty split
        assert 1 <= p["last_split"] <= ups
        assert p["xcd_order"] == int((ns * p["n_cotiles"]) % 8 == 0)
        assert p["workspace_bytes"] == ns * K * Co * (C0 + C1) * 4
        plans.append(p)
    assert plans[1]["form"] in (L.TQ_WGRAD_C32, L.TQ_WGRAD_C64, L.TQ_WGRAD_C128)     # fused column sums: never W8 / H64
    assert lib.tq_conv1d_bwd_weight_workspace(C.byref(d)) == max(p["workspace_bytes"] for p in plans)
    # the query is a pure function of the descriptor
    assert ops.conv1d_bwd_weight_plan(_desc(*shape), False) == plans[0]


def test_plan_table_reaches_every_form_and_multi_unit_splits():
    """the table above is not vacuous: every form occurs, with and without several units per split, and with both block orders"""
    L, _ = _lib()
    from tqdne_amd import ops
    seen = set()
    for shape in PLAN_TABLE:
        for cs in (False, True):
            p = ops.conv1d_bwd_weight_plan(_desc(*shape), cs)
            seen.add((p["form_name"], p["units_per_split"] > 1))
            seen.add((p["form_name"], "xcd" if p["xcd_order"] else "plain"))
    for form in ("C32", "C64", "C128", "W8", "H64"):
        for what in (False, True, "xcd", "plain"):
            assert (form, what) in seen, (form, what)
