"""GroupNorm chain without a GPU: the float64 restatement of tests/_groupnorm_ref.py against torch.autograd of F.group_norm, the
fp32-slot yardstick against that restatement, and the argument checks of tq_gn_finalize and of the TQ_BWD_ACCUM | TQ_BWD_STATS
refusal of tq_conv1d_bwd_data.  The pointers below are never dereferenced: every library call in this file is rejected in
validation, none reaches a launch.  Companion of tests/test_groupnorm_gpu.py."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _groupnorm_ref as R

ARG, SHAPE = -1, -2
FAKE = 0x1000
BAR_F64 = 1e-12


def lib():
    from tqdne_amd import _lib
    return _lib.load()


def torch_group_norm(x_list, g_list, gamma, beta):
    """float64 autograd of F.group_norm on the channel concat: output, dx per source, dgamma, dbeta"""
    x = torch.from_numpy(np.concatenate(x_list, axis=2)).double().permute(0, 2, 1).contiguous().requires_grad_(True)
    g = torch.from_numpy(np.concatenate(g_list, axis=2)).double().permute(0, 2, 1).contiguous()
    gm = torch.from_numpy(gamma).double().requires_grad_(True)
    bt = torch.from_numpy(beta).double().requires_grad_(True)
    y = F.group_norm(x, R.GROUPS, gm, bt, R.EPS)
    y.backward(g)
    cl = lambda t: t.detach().permute(0, 2, 1).numpy()
    return cl(y), cl(x.grad), gm.grad.numpy(), bt.grad.numpy()


def chain_input(c_list, T, ratio, seed):
    if T == 1 and sum(c_list) == R.GROUPS:   # a group of one element has no spread to place a ratio on
        rng = np.random.default_rng(seed)
        sh = (2, 1, R.GROUPS)
        return ([rng.standard_normal(sh).astype(np.float32)], [rng.standard_normal(sh).astype(np.float32)],
                rng.standard_normal(R.GROUPS).astype(np.float32), rng.standard_normal(R.GROUPS).astype(np.float32))
    return R.regime_input(2, T, c_list, ratio, seed)


@pytest.mark.parametrize("T", [1, 130])
@pytest.mark.parametrize("c_list", [(32,), (64, 32), (256,)], ids=["G1", "G3_straddling", "G8"])
def test_restatement_against_torch_autograd(c_list, T):
    xs, gs, gamma, beta = chain_input(c_list, T, 3.0, 11 + T + sum(c_list))
    f = R.fold(xs, gamma, beta)
    b = R.backward(xs, gs, gamma, f["mean"], f["rstd"])
    y_ref, dx_ref, dg_ref, db_ref = torch_group_norm(xs, gs, gamma, beta)
    x = np.concatenate(xs, axis=2).astype(np.float64)
    y = f["scale"][:, None] * x + f["shift"][:, None]
    ag = np.abs(b["A"][:, None] * np.concatenate(gs, axis=2)).max()   # the scale of dx's terms (dx itself is 0 for a group of one)
    errs = dict(y=R.rel_max(y, y_ref), dx=float(np.abs(np.concatenate(b["dx"], axis=2) - dx_ref).max() / ag),
                dgamma=R.rel_max(b["dgamma"], dg_ref, floor=ag), dbeta=R.rel_max(b["dbeta"], db_ref))
    print(f"C {c_list} T {T}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAR_F64, errs
    assert np.allclose(b["dgamma_b"].sum(0), b["dgamma"]) and np.allclose(b["dbeta_b"].sum(0), b["dbeta"])


def emulation_errors(c_list, T, ratio, dtype, seed=5):
    xs, gs, gamma, beta = R.regime_input(2, T, c_list, ratio, seed)
    f = R.fold(xs, gamma, beta)
    b = R.backward(xs, gs, gamma, f["mean"], f["rstd"])
    e = R.emulate(xs, gs, gamma, beta, dtype=dtype)
    x = np.concatenate(xs, axis=2).astype(np.float64)
    fwd = R.rel_max(e["scale"][:, None] * x + e["shift"][:, None], f["scale"][:, None] * x + f["shift"][:, None])
    dx = R.rel_max(np.concatenate(e["dx"], axis=2), np.concatenate(b["dx"], axis=2))
    return dict(fwd=fwd, dx=dx, dgamma=R.rel_max(e["dgamma"], b["dgamma"]), dbeta=R.rel_max(e["dbeta"], b["dbeta"]))


@pytest.mark.parametrize("c_list,T", [((32,), 130), ((64, 32), 130), ((128, 64), 1153)])
def test_yardstick_is_exact_where_it_should_be_and_loses_where_it_must(c_list, T):
    """at ratio 0 the fp32-slot emulation agrees with float64 to 1e-5; at ratio 100 it is strictly worse than the same algorithm
    with float64 partials (which stays at float64 accuracy): the yardstick measures the fp32 slots and nothing else"""
    e0 = emulation_errors(c_list, T, 0.0, np.float32)
    e100 = emulation_errors(c_list, T, 100.0, np.float32)
    c100 = emulation_errors(c_list, T, 100.0, np.float64)
    print(f"C {c_list} T {T}: ratio 0 {e0}\n  ratio 100 {e100}\n  ratio 100, float64 partials {c100}")
    assert max(e0.values()) <= 1e-5, e0
    assert max(c100.values()) <= 1e-9, c100
    for k in ("fwd", "dx", "dgamma"):
        assert e100[k] > 100 * c100[k] and e100[k] > e0[k], (k, e100[k], c100[k], e0[k])


def test_slot_sums_and_seq32_sum():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((2, 300, 8)), rng.standard_normal((2, 300, 8))
    s = R.slot_sums(a, b, slot=128)
    assert s.shape == (2, 3, 8, 2)
    assert np.allclose(s[:, 2, :, 0], a[:, 256:].sum(1)) and np.allclose(s[:, 1, :, 1], (a * b)[:, 128:256].sum(1))
    assert np.allclose(R.slot_sums(a, slot=32).sum(1)[..., 1], (a * a).sum(1))
    v = np.full((4097, 2), 1.0, dtype=np.float32)
    v[0] = 2.0 ** 24   # every later 1.0 is absorbed by a sequential fp32 sum; a pairwise tree would keep most of them
    assert np.array_equal(R.seq32_sum(v, 0), np.full(2, 2.0 ** 24))


# ---------------------------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------------------------
def bwd_desc(flags, C0=64, C1=0):
    from tqdne_amd import _lib
    d = _lib.TqConvBwdDesc()
    d.B, d.T, d.C_dy, d.C_dx0, d.C_dx1, d.ktaps, d.flags = 2, 128, 64, C0, C1, 3, flags
    return d


def test_bwd_data_refuses_accumulate_with_stats():
    """TQ_BWD_ACCUM | TQ_BWD_STATS would sum the tensor after accumulation: TQ_ERR_ARG before the device is touched"""
    from tqdne_amd import _lib
    L = lib()
    call = lambda d: L.tq_conv1d_bwd_data(ctypes.byref(d), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None)
    chain = _lib.TQ_BWD_GN | _lib.TQ_BWD_SILU
    for extra in (0, chain, chain | _lib.TQ_BWD_DROPOUT):
        assert call(bwd_desc(_lib.TQ_BWD_ACCUM | _lib.TQ_BWD_STATS | extra)) == ARG, extra
    assert call(bwd_desc(_lib.TQ_BWD_ACCUM | _lib.TQ_BWD_STATS | chain, 32, 32)) == ARG
    # each flag alone passes this check: the call goes on to the next refusal (a channel count that is no multiple of 32)
    for flags in (_lib.TQ_BWD_ACCUM | chain, _lib.TQ_BWD_STATS | chain):
        d = bwd_desc(flags)
        d.C_dy = 48
        assert call(d) == SHAPE, flags


def test_gn_finalize_argument_checks():
    L = lib()
    #       stats0 C0 stats1 C1 B  T    gamma beta  gscale gshift mean_rstd slot0 slot1
    good = [FAKE, 64, FAKE, 32, 2, 130, FAKE, FAKE, FAKE, FAKE, FAKE, 0, 32]
    for i in (0, 6, 7, 8, 9):   # (mean_rstd, argument 10, is nullable)
        a = list(good)
        a[i] = None
        assert L.tq_gn_finalize(*a, None) == ARG, f"argument {i} NULL"
    a = list(good)
    a[2] = None
    assert L.tq_gn_finalize(*a, None) == ARG, "C1 > 0 with a NULL stats1"
    for C0, C1 in [(48, 0), (64, 16), (0, 0), (-32, 0), (3872, 0), (3840, 32), (2048, 2048)]:   # C % 32, C <= 0, C > 3840
        a = list(good)
        a[1], a[3] = C0, C1
        assert L.tq_gn_finalize(*a, None) == SHAPE, (C0, C1)
    for B, T in [(0, 130), (-1, 130), (2, 0), (2, -5)]:
        a = list(good)
        a[4], a[5] = B, T
        assert L.tq_gn_finalize(*a, None) == SHAPE, (B, T)
    for s0, s1 in [(64, 0), (0, 64), (1, 128), (128, 256), (-32, 32), (32, 31)]:
        a = list(good)
        a[11], a[12] = s0, s1
        assert L.tq_gn_finalize(*a, None) == ARG, (s0, s1)
