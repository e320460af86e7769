"""conv_resample=False and cond_emb_scale on the GPU: the three streaming kernels of csrc/resample_plain.hip against torch on the CPU
(values bit for bit, statistics against fp64 sums), and whole models -- UNet forward, EDM loss and gradients (also with use_checkpoint),
coders, the autoencoder's training step, the cond_emb_scale model -- against the reference's own recorded results
(tests/golden/plain_resample.npz, tools/make_plain_resample_goldens.py).  Bars: statistics 1e-5 (tests/test_hip_ops.py::test_stem),
GroupNorm coefficients 2e-5 (test_group_norm_via_stats), whole path 1e-3 (tests/test_hip_unet.py).

The fixture holds no weights (file-size limit): both sides build them with the tool's ``recipe_state`` and the fixture's sha256 per tensor
says they are the ones the reference ran with; of a large gradient tensor it holds the evenly spaced entries ``sample_index`` names."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, cfg_of, grad_err, load_golden, rel_err

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_plain_resample_goldens import recipe_state, sample_index, tensor_fingerprint  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_STATS, TOL_GN, TOL_PATH, TOL_TILES = 1e-5, 2e-5, 1e-3, 2e-5
SENTINEL = 12345.0
OPT = {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}
KERNEL_CASES = [(32, 2), (32, 255), (64, 256), (96, 258), (1024, 130), (36, 70)]   # (C, T_in), B = 2
NEW_ENTRY_POINTS = ("tq_avg_pool2_fwd", "tq_nearest_up2_fwd", "tq_avg_pool2_bwd")


def dev():
    return torch.device("cuda:0")


def cl(x):  # (B,C,T) -> channels-last (B,T,C) on device
    return x.permute(0, 2, 1).contiguous().to(dev())


def ncw(y):  # device (B,T,C) -> cpu (B,C,T)
    return y.permute(0, 2, 1).cpu()


def _name(fn):
    return getattr(fn, "__name__", "")


def guarded(*shape):
    """a NaN-filled device tensor of ``shape`` with 4096 sentinel floats in front of and behind it: (tensor, check)"""
    n, G = math.prod(shape), 4096
    flat = torch.full((n + 2 * G,), SENTINEL, device=dev())
    body = flat[G:G + n].view(*shape)
    body.fill_(float("nan"))

    def check():
        assert not torch.isnan(body).any(), "a value that should have been written was not"
        assert bool((flat[:G] == SENTINEL).all()) and bool((flat[G + n:] == SENTINEL).all()), "write outside the buffer"
    return body, check


def ref_stats(y_nct, slot=128):
    B, C, T = y_nct.shape
    ns = (T + slot - 1) // slot
    out = torch.zeros(B, ns, C, 2, dtype=torch.float64)
    for s in range(ns):
        seg = y_nct[:, :, s * slot:(s + 1) * slot].double()
        out[:, s, :, 0] = seg.sum(-1)
        out[:, s, :, 1] = (seg * seg).sum(-1)
    return out


def _x(C, T, seed=0):
    g = torch.Generator().manual_seed(1000 * C + T + seed)
    return torch.randn(2, C, T, generator=g) * 1.5 + 0.3


# ----------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("C,T", KERNEL_CASES)
def test_avg_pool2_values_and_statistics(C, T):
    from tqdne_amd import ops
    x = _x(C, T)
    ref = F.avg_pool1d(x, 2, 2)
    To = T // 2
    y, chk_y = guarded(2, To, C)
    st, chk_s = guarded(2, (To + 127) // 128, C, 2)
    ops.avg_pool2(cl(x), out=(y, st))
    y0, chk_0 = guarded(2, To, C)
    ops.avg_pool2(cl(x), out=(y0, None))   # stats = NULL: the flat kernel
    st2, chk_s2 = guarded(2, (To + 127) // 128, C, 2)
    y2, chk_y2 = guarded(2, To, C)
    ops.avg_pool2(cl(x), out=(y2, st2))
    torch.cuda.synchronize()
    chk_y(), chk_s(), chk_0(), chk_s2(), chk_y2()
    assert torch.equal(ncw(y), ref) and torch.equal(ncw(y0), ref)
    e = rel_err(st.cpu(), ref_stats(ref))
    print(f"avg_pool2 C={C} T_in={T}: statistics {e:.2e}")
    assert e < TOL_STATS
    assert torch.equal(st, st2)   # no atomics: the same bits from launch to launch


@pytest.mark.parametrize("C,T", KERNEL_CASES)
def test_nearest_up2_values_and_statistics(C, T):
    from tqdne_amd import ops
    x = _x(C, T, 1)
    ref = F.interpolate(x, scale_factor=2, mode="nearest")
    To = 2 * T
    y, chk_y = guarded(2, To, C)
    st, chk_s = guarded(2, (To + 127) // 128, C, 2)
    ops.nearest_up2(cl(x), out=(y, st))
    y0, chk_0 = guarded(2, To, C)
    ops.nearest_up2(cl(x), out=(y0, None))
    st2, chk_s2 = guarded(2, (To + 127) // 128, C, 2)
    y2, chk_y2 = guarded(2, To, C)
    ops.nearest_up2(cl(x), out=(y2, st2))
    torch.cuda.synchronize()
    chk_y(), chk_s(), chk_0(), chk_s2(), chk_y2()
    assert torch.equal(ncw(y), ref) and torch.equal(ncw(y0), ref)
    e = rel_err(st.cpu(), ref_stats(ref))
    print(f"nearest_up2 C={C} T_in={T}: statistics {e:.2e}")
    assert e < TOL_STATS
    assert torch.equal(st, st2)


@pytest.mark.parametrize("C,T", KERNEL_CASES)
def test_avg_pool2_bwd_is_the_autograd_of_avg_pool1d(C, T):
    from tqdne_amd import ops
    x = _x(C, T, 2).requires_grad_()
    dy = _x(C, T // 2, 3)
    F.avg_pool1d(x, 2, 2).backward(dy)
    dx, chk = guarded(2, T, C)
    from tqdne_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev()).cuda_stream
    dyd = cl(dy)
    _lib.check(lib.tq_avg_pool2_bwd(dyd.data_ptr(), dx.data_ptr(), 2, T, C, 0, stream), "avg_pool2_bwd")
    torch.cuda.synchronize()
    chk()   # (odd T_in: the dropped last row is written, as zero -- not left NaN)
    assert torch.equal(ncw(dx), x.grad)
    if T % 2:
        assert bool((dx[:, -1] == 0).all())
    prev = _x(C, T, 4)
    acc = ops.avg_pool2_bwd(dyd, T, accumulate_into=cl(prev))
    assert torch.equal(ncw(acc), prev + x.grad)
    assert torch.equal(ncw(ops.avg_pool2_bwd(dyd, T)), x.grad)


@pytest.mark.parametrize("kernel_first", [True, False])
@pytest.mark.parametrize("C,T", [(96, 258), (36 * 8, 70), (32, 255)])
def test_statistics_feed_gn_finalize_next_to_a_slot32_source(C, T, kernel_first):
    """the producer statistics of both kernels (slot 128) in a concatenated GroupNorm whose other source has one slot per 32 positions (the
    output of a small-tile conv): coefficients against GroupNorm32 of the concatenation"""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(C + T)
    for which in ("pool", "up"):
        x = _x(C, T, 5)
        y, st = (ops.avg_pool2 if which == "pool" else ops.nearest_up2)(cl(x))
        yr = F.avg_pool1d(x, 2, 2) if which == "pool" else F.interpolate(x, scale_factor=2, mode="nearest")
        To = yr.shape[2]
        other = torch.randn(2, 64, To, generator=g) * 2 - 1
        so = ref_stats(other, 32).float().to(dev())
        gamma, beta = torch.randn(C + 64, generator=g), torch.randn(C + 64, generator=g)
        if kernel_first:
            gs, gh, _ = ops.gn_finalize(st, C, To, gamma.to(dev()), beta.to(dev()), so, 64, slot0=0, slot1=32)
            cat = torch.cat([yr, other], 1)
        else:
            gs, gh, _ = ops.gn_finalize(so, 64, To, gamma.to(dev()), beta.to(dev()), st, C, slot0=32, slot1=0)
            cat = torch.cat([other, yr], 1)
        ref = F.group_norm(cat.double(), 32, gamma.double(), beta.double(), 1e-5)
        got = cat * gs.cpu()[:, :, None] + gh.cpu()[:, :, None]
        e = rel_err(got, ref)
        print(f"{which} C={C} T_in={T} kernel_first={kernel_first}: {e:.2e}")
        assert e < TOL_GN


# ----------------------------------------------------------------------------------------------------------- whole models
@pytest.fixture(scope="module")
def fx():
    return load_golden("plain_resample.npz")[1]


def seeds(d):
    return eval(str(d["seeds"]), {"__builtins__": {}}, {"dict": dict})


def load_recipe(module, d, tag, seed):
    sd = recipe_state(module, seed)
    assert [tensor_fingerprint(v) for v in sd.values()] == [str(s) for s in d[tag + ":sha256"]], "not the weights the reference ran with"
    module.load_state_dict(sd)
    return module


def t_(a):
    x = torch.from_numpy(a)
    return (x.float() if x.dtype == torch.float16 else x).to(dev())


def unet_of(d, tag, **kw):
    from tqdne_amd import UNetModel
    net = UNetModel(**dict(cfg_of(d, "cfg:" + tag), **kw))
    return load_recipe(net, d, tag, seeds(d)[tag]).to(dev()).eval()


def edm_of(d, tag, steps=25, **kw):
    from tqdne_amd import LightningEDM
    edm = LightningEDM(dict(cfg_of(d, "cfg:" + tag), **kw), OPT, num_sampling_steps=steps)
    load_recipe(edm.unet, d, tag, seeds(d)[tag])
    return edm.to(dev())


def check_sampled_grads(named_parameters, d, tag):
    gmax = float(d[tag + ":gmax"])
    worst, wname, n = 0.0, "", 0
    for name, p in named_parameters:
        if not p.requires_grad:
            assert f"{tag}:g:{name}" not in d, name
            continue
        assert p.grad is not None, name
        ref = d[f"{tag}:g:{name}"]
        got = p.grad.detach().reshape(-1).cpu()[sample_index(p.numel())]
        e = grad_err(got, ref, gmax, name)
        n += 1
        if e > worst:
            worst, wname = e, name
    print(f"{tag}: {n} gradient tensors, worst {worst:.2e} ({wname})")
    assert n > 0 and worst < TOL_PATH, (worst, wname)


@pytest.fixture(scope="module")
def plain_unet(fx):
    return unet_of(fx, "unet")


@pytest.mark.parametrize("T", [200, 136])
def test_unet_forward_vs_reference(fx, plain_unet, T):
    with torch.no_grad():
        y = plain_unet(t_(fx[f"unet:x{T}"]), t_(fx["unet:t"]), t_(fx["unet:cond"]))
    e = rel_err(y.cpu(), fx[f"unet:y{T}"])
    print(f"conv_resample=False UNet forward T={T}: {e:.2e}")
    assert e < TOL_PATH


def test_unet_plan_holds_the_new_launches_and_no_resampling_conv(fx, plain_unet):
    with torch.no_grad():
        plain_unet(t_(fx["unet:x200"]), t_(fx["unet:t"]), t_(fx["unet:cond"]))
    eng = plain_unet._engine(2, 200, dev())
    names = [_name(op[0]) for op in eng.ops]
    assert names.count("tq_avg_pool2_fwd") == 2 and names.count("tq_nearest_up2_fwd") == 2
    assert [_name(op[0]) for op in eng.ops_infer].count("tq_avg_pool2_fwd") == 2 and len(eng.ops_infer) == len(eng.ops)
    assert not [s.name for s in eng.conv_sites if s.name.endswith(".op") or s.name.endswith(".conv")]
    assert [k for k, _ in eng.tape].count("down_plain") == 2 and [k for k, _ in eng.tape].count("up_plain") == 2
    assert any(getattr(o, "t_tile", 0) == 32 for o in eng._keep)   # (B = 2: a small-tile plan -- the pooled tensor sits next to slot-32 sources)


@pytest.mark.parametrize("ckpt", [False, True])
def test_edm_loss_and_gradients_vs_reference(fx, ckpt):
    edm = edm_of(fx, "unet", use_checkpoint=ckpt).train()   # (dropout 0: train mode is deterministic)
    loss = edm.step_with_noise(t_(fx["unet:edm:signal"]), t_(fx["unet:edm:eps"]), t_(fx["unet:edm:noise"]), cond=t_(fx["unet:cond"]))
    e = rel_err(loss.detach().cpu(), fx["unet:edm:loss"])
    print(f"use_checkpoint={ckpt}: loss {float(loss):.6f}, error {e:.2e}")
    assert e < TOL_PATH
    loss.backward()
    check_sampled_grads(edm.unet.named_parameters(), fx, "unet:edm")
    eng = edm.unet._engine(2, 200, dev())
    assert eng.ckpt == ckpt
    bwd = [_name(op[0]) for op in eng._bwd.ops]
    assert bwd.count("tq_avg_pool2_bwd") == 2 and "tq_zero_stuff" not in bwd
    if ckpt:   # the resampling launches sit outside the recomputed blocks
        assert not [op[2] for op in eng._bwd.ops if op[2].startswith("recompute:") and ("avg_pool2" in op[2] or "nearest_up2" in op[2])]
        assert any(op[2].startswith("recompute:") for op in eng._bwd.ops)


def test_differentiable_call_gives_the_input_gradient(fx, plain_unet):
    x = t_(fx["unet:x200"]).requires_grad_()
    y = plain_unet(x, t_(fx["unet:t"]), t_(fx["unet:cond"]))
    y.sum().backward()
    e = rel_err(x.grad.cpu(), fx["unet:dx200"])
    print(f"d sum(y) / d x: {e:.2e}")
    assert e < TOL_PATH
    plain_unet.zero_grad()


def test_default_tiles_agree_with_the_small_tile_plan(fx, plain_unet):
    import tqdne_amd.engine as E
    x, t, c = t_(fx["unet:x200"]), t_(fx["unet:t"]), t_(fx["unet:cond"])
    with torch.no_grad():
        y2 = plain_unet(x, t, c)
        net8 = unet_of(fx, "unet")
        old_w = E.SMALL_TILE_WGS
        try:
            E.SMALL_TILE_WGS = 0   # (a plan of 8 samples that is alone on the device would still take the small tile per layer)
            y8 = net8(x.repeat(4, 1, 1), t.repeat(4), c.repeat(4, 1))
        finally:
            E.SMALL_TILE_WGS = old_w
    eng8 = net8._engine(8, 200, dev())
    assert not any(getattr(o, "t_tile", 0) == 32 for o in eng8._keep)
    for i in range(4):
        e = rel_err(y8[2 * i:2 * i + 2].cpu(), y2.cpu())
        print(f"copy {i}: {e:.2e}")
        assert e < TOL_TILES


def test_two_lane_sampler_is_bit_identical(fx):
    import tqdne_amd.engine as E
    from oracle import edm as OE
    edm = edm_of(fx, "unet", steps=4).eval()
    sig = OE.sampling_sigmas(OE.EDMParams(), 4).to(dev())
    g = torch.Generator().manual_seed(31)
    B = 16
    start = torch.randn(B, 3, 256, generator=g, dtype=torch.float64).to(dev()) * sig[0]
    cond = torch.randn(B, 5, generator=g).to(dev())
    old_w = E.SMALL_TILE_WGS
    try:
        E.SMALL_TILE_WGS = 0   # (same tiles in the one-lane plan and in the lanes' plans)
        one = edm.sample_deterministically(start, sig, None, cond, lanes=1)
        two = edm.sample_deterministically(start, sig, None, cond, lanes=2)
    finally:
        E.SMALL_TILE_WGS = old_w
    assert torch.isfinite(one).all() and torch.equal(one, two)
    engines = list(edm.unet._engine_cache.values())
    assert len(engines) >= 3 and all(any(_name(op[0]) == "tq_nearest_up2_fwd" for op in e.ops_infer) for e in engines)


def test_length_that_the_skip_stack_cannot_take_raises(fx, plain_unet):
    x = torch.zeros(2, 3, 250, device=dev())
    with pytest.raises(RuntimeError, match="must match"):
        with torch.no_grad():
            plain_unet(x, t_(fx["unet:t"]), t_(fx["unet:cond"]))


# ----------------------------------------------------------------------------------------------------------- coders
@pytest.fixture(scope="module")
def plain_ae(fx):
    from tqdne_amd import LightningAutoencoder
    ae = LightningAutoencoder(cfg_of(fx, "cfg:enc"), cfg_of(fx, "cfg:dec"), OPT, kl_weight=float(fx["ae:kl_weight"]))
    return load_recipe(ae, fx, "ae", seeds(fx)["ae"]).to(dev()).eval()   # (the reference ran in eval mode; dropout is 0)


def test_coder_forwards_vs_reference(fx, plain_ae):
    with torch.no_grad():
        for T in (202, 200):   # 202 -> 101 -> 50: the coders have no skip stack and floor at each level
            e_ = plain_ae.encoder(t_(fx[f"ae:x{T}"]))
            assert tuple(e_.shape) == (2, 8, 50)
            e = rel_err(e_.cpu(), fx[f"ae:enc{T}"])
            print(f"encoder T={T}: {e:.2e}")
            assert e < TOL_PATH
        r = plain_ae.decoder(t_(fx["ae:z"]))
    e = rel_err(r.cpu(), fx["ae:dec"])
    print(f"decoder: {e:.2e}")
    assert e < TOL_PATH
    for mod, T, fwd in ((plain_ae.encoder, 200, "tq_avg_pool2_fwd"), (plain_ae.decoder, 50, "tq_nearest_up2_fwd")):
        eng = mod._engine_cache.get((2, T, str(dev())))
        assert [_name(op[0]) for op in eng.ops].count(fwd) == 2
        assert not [s.name for s in eng.conv_sites if s.name.endswith(".op") or s.name.endswith(".conv")]


def test_autoencoder_training_step_vs_reference(fx, plain_ae):
    eps = t_(fx["ae:step:eps"])
    orig = torch.randn_like
    torch.randn_like = lambda t, **k: eps
    try:
        loss = plain_ae.training_step({"signal": t_(fx["ae:x200"])}, 0)
    finally:
        torch.randn_like = orig
    e = rel_err(loss.detach().cpu(), fx["ae:step:loss"])
    print(f"autoencoder step: loss {float(loss):.6f}, error {e:.2e}")
    assert e < TOL_PATH
    loss.backward()
    check_sampled_grads(plain_ae.named_parameters(), fx, "ae:step")
    plain_ae.zero_grad()


# ----------------------------------------------------------------------------------------------------------- cond_emb_scale
def test_cond_emb_scale_forward_and_gradients_vs_reference(fx):
    edm = edm_of(fx, "cf").train()
    with torch.no_grad():
        y = edm.unet(t_(fx["cf:x200"]), t_(fx["unet:t"]), t_(fx["cf:cond"]))
    e = rel_err(y.cpu(), fx["cf:y200"])
    print(f"cond_emb_scale forward: {e:.2e}")
    assert e < TOL_PATH
    loss = edm.step_with_noise(t_(fx["cf:edm:signal"]), t_(fx["cf:edm:eps"]), t_(fx["cf:edm:noise"]), cond=t_(fx["cf:cond"]))
    assert rel_err(loss.detach().cpu(), fx["cf:edm:loss"]) < TOL_PATH
    loss.backward()
    assert edm.unet.cond_embed.W.grad is None
    check_sampled_grads(edm.unet.named_parameters(), fx, "cf:edm")
    with pytest.raises(ValueError):
        with torch.no_grad():
            edm.unet(t_(fx["cf:x200"]), t_(fx["unet:t"]), t_(fx["unet:cond"]))   # five conditioning features


# ----------------------------------------------------------------------------------------------------------- established plans
def test_established_plans_do_not_reach_the_new_entry_points():
    """the paper and the tiny plan: forward, inference and backward op lists"""
    from tqdne_amd import LightningEDM, paper_1d_unet_config, tiny_1d_unet_config
    for cfg in (paper_1d_unet_config(), tiny_1d_unet_config()):
        torch.manual_seed(0)
        edm = LightningEDM(dict(cfg, dropout=0.0), OPT).to(dev()).train()
        B, T = 1, 512
        g = torch.Generator().manual_seed(1)
        cond = torch.randn(B, 5, generator=g).to(dev()) if cfg["cond_features"] else None
        loss = edm.step_with_noise(torch.randn(B, 3, T, generator=g).to(dev()), torch.randn(B, generator=g).to(dev()),
                                   torch.randn(B, 3, T, generator=g).to(dev()), cond=cond)
        loss.backward()
        eng = edm.unet._engine(B, T, dev())
        names = [_name(op[0]) for ops in (eng.ops, eng.ops_infer, eng._bwd.ops) for op in ops]
        assert "tq_conv1d_fwd" in names and "tq_conv1d_bwd_data" in names
        assert not [n for n in names if n in NEW_ENTRY_POINTS]
        assert not [k for k, _ in eng.tape if k.endswith("_plain")]
