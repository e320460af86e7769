"""Stem and head convs at every first-level width 32, 64, ... 1024 on the GPU (csrc/ends_wide.hip behind tq_stem_conv_fwd,
tq_head_conv_fwd, tq_head_conv_bwd_ws).

Kernel level: the three entry points against fp64 convolutions / fp64 autograd into sentinel-guarded buffers, at widths that are no
power of two (96, 160, 192, 224, 288, 992), at 512 and 1024 (too wide for one workgroup's LDS), for every tap count and 1 ... 16 signal
channels, on lengths below the tap count and ragged against the 60- / 62- / 64-position head tiles and the 128-position statistics slot.
Bar: 1e-5, the suite's for these exact-fp32 kernels (tests/test_hip_ops.py::test_head, tests/test_hip_bwd.py).
Whole models: mc96 / mc160 / mc256 / mc1024 (tests/test_first_level_widths_host.py) against the CPU oracle and its autograd with the
metric and bars of tests/test_wide_models_gpu.py; an Encoder with a 256-channel last level and a Decoder with a 96-channel first level
against oracle/autoencoder.py with the bars of tests/test_autoencoder_step.py.
Shapes are the smallest that still take every path of the chunking: B = 3 (2 for models), T <= 257."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import grad_err, rel_err
from test_first_level_widths_host import MODELS, width_cfg
from test_head_sizes_gpu import cl, dev, guarded, ncw, perturbed_state
from test_hip_bwd import ref_slot_sums
from test_wide_models_gpu import TOL_PATH, _batch, ref_stats

pytestmark = pytest.mark.gpu

TOL_OP = 1e-5   # tests/test_hip_ops.py::test_head


# ---- stem forward --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,cout,T,k", [(3, 96, 130, 5), (3, 160, 64, 3), (6, 224, 257, 5), (16, 992, 1, 1), (16, 1024, 130, 5), (3, 1024, 200, 5)])
def test_stem_forward_vs_fp64(cin, cout, T, k):
    """output and partial statistics; tiles of 96 / 128 + 32 / 128 + 96 / 7 x 128 + 96 / 8 x 128 channels, and the first kernel at
    3 -> 1024 (its weights fit the LDS: unchanged path, same checks)"""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(cin + cout + T + k)
    B = 3
    x = torch.randn(B, cin, T, generator=g)
    w, b = torch.randn(cout, cin, k, generator=g) / 4, torch.randn(cout, generator=g)
    sc = torch.rand(B, generator=g) + 0.5
    d = dev()
    y, cy = guarded(B, T, cout)
    st, cs = guarded(B, (T + 127) // 128, cout, 2)
    ops.stem_conv(x.to(d), w.to(d), b.to(d), in_scale=sc.to(d), out=(y, st))
    torch.cuda.synchronize()
    cy(), cs()
    ref = F.conv1d(x.double() * sc.double()[:, None, None], w.double(), b.double(), padding=k // 2)
    e, es = rel_err(ncw(y), ref), rel_err(st.cpu(), ref_stats(ref))
    print(f"stem {cin} -> {cout} k{k} T={T}: {e:.2e} (statistics {es:.2e})")
    assert e < TOL_OP and es < TOL_OP
    y2, st2 = ops.stem_conv(x.to(d), w.to(d), None, stats=False)   # no bias, no scale, no statistics
    assert st2 is None and rel_err(ncw(y2), F.conv1d(x.double(), w.double(), None, padding=k // 2)) < TOL_OP


# ---- head forward --------------------------------------------------------------------------------------------------------------------------

HEAD_CASES = [(160, 3, 5, 130), (192, 6, 3, 61), (256, 1, 1, 257), (256, 3, 5, 61), (288, 16, 5, 130), (512, 3, 3, 1), (512, 6, 5, 257),
              (992, 16, 1, 61), (992, 3, 5, 1), (1024, 3, 5, 257), (1024, 16, 3, 130), (1024, 1, 5, 61), (224, 5, 5, 64), (320, 11, 3, 63),
              (96, 6, 5, 130), (128, 16, 5, 61)]   # (C_in, C_out, k, T); the last two: shapes of old widths the first kernels refused


def _head_case(cin, cout, k, T, B=3):
    g = torch.Generator().manual_seed(cin + cout + T + k)
    x = torch.randn(B, cin, T, generator=g)
    a, s = torch.randn(B, cin, generator=g), torch.randn(B, cin, generator=g)
    w, b = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k), torch.randn(cout, generator=g)
    co, cs = torch.rand(B, generator=g) + 0.5, torch.rand(B, generator=g)
    skip = torch.randn(B, cout, T, generator=g)
    return x, a, s, w, b, co, cs, skip


@pytest.mark.parametrize("cin,cout,k,T", HEAD_CASES)
def test_head_forward_vs_fp64(cin, cout, k, T):
    """with the folded GroupNorm + SiLU prologue and the c_out / c_skip epilogue, with the prologue alone, and plain"""
    from tqdne_amd import ops
    x, a, s, w, b, co, cs, skip = _head_case(cin, cout, k, T)
    d = dev()
    z = F.silu(x.double() * a.double()[:, :, None] + s.double()[:, :, None])
    conv = lambda inp, bias: F.conv1d(inp, w.double(), bias, padding=k // 2)
    refs = [conv(z, b.double()) * co.double()[:, None, None] + cs.double()[:, None, None] * skip.double(), conv(z, None), conv(x.double(), b.double())]
    args = [(b.to(d), a.to(d), s.to(d), co.to(d), cs.to(d), skip.to(d)), (None, a.to(d), s.to(d)), (b.to(d),)]
    errs = []
    for ref, ar in zip(refs, args):
        y, cy = guarded(3, cout, T)
        ops.head_conv(cl(x), w.to(d), *ar, out=y)
        torch.cuda.synchronize()
        cy()
        errs.append(rel_err(y.cpu(), ref))
    print(f"head {cin} -> {cout} k{k} T={T}: full {errs[0]:.2e} prologue only {errs[1]:.2e} plain {errs[2]:.2e}")
    assert max(errs) < TOL_OP


# ---- head backward -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ws", [True, False])
@pytest.mark.parametrize("cin,cout,k,T", [(160, 3, 5, 130), (192, 6, 3, 61), (256, 3, 5, 257), (288, 16, 5, 130), (512, 3, 5, 257), (512, 1, 1, 1),
                                          (992, 6, 5, 61), (1024, 3, 5, 130), (1024, 16, 3, 61), (96, 3, 5, 200)])
def test_head_backward_vs_fp64_autograd(cin, cout, k, T, ws):
    """G = (W^T dF) silu', the GroupNorm partial sums, dw and db (zeroed first: they are added to), through per-workgroup partial rows
    in a workspace and with atomics; then the form without the prologue"""
    from tqdne_amd import ops
    x, a, s, w, b, co, _, _ = _head_case(cin, cout, k, T)
    g = torch.Generator().manual_seed(cin + T)
    dpred = torch.randn(3, cout, T, generator=g)
    d = dev()
    ns = (T + 127) // 128
    for prologue in (True, False):
        wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
        u = (x.double() * a.double()[:, :, None] + s.double()[:, :, None] if prologue else x.double()).requires_grad_(True)
        (F.conv1d(F.silu(u) if prologue else u, wd, bd, padding=k // 2) * co.double()[:, None, None]).backward(dpred.double())
        G, cG = guarded(3, T, cin)
        st, cst = guarded(3, ns, cin, 2)
        dw, cdw = guarded(cout, cin, k)
        db, cdb = guarded(cout)
        dw.zero_(), db.zero_()
        ops.head_conv_bwd(dpred.to(d), cl(x), w.to(d), a.to(d) if prologue else None, s.to(d) if prologue else None, co.to(d), workspace=ws,
                          out=(G, st, dw, db))
        torch.cuda.synchronize()
        cG(), cst(), cdw(), cdb()
        e = (rel_err(ncw(G), u.grad), rel_err(st.cpu(), ref_slot_sums(u.grad, x)), rel_err(dw.cpu(), wd.grad), rel_err(db.cpu(), bd.grad))
        print(f"head bwd {cout} -> {cin} k{k} T={T} ws={ws} prologue={prologue}: G {e[0]:.2e} GN sums {e[1]:.2e} dw {e[2]:.2e} db {e[3]:.2e}")
        assert max(e) < TOL_OP


# ---- whole models --------------------------------------------------------------------------------------------------------------------------

T_MODEL = 200
_STATE, _ORACLE = {}, {}


def width_model(which):
    """(cfg, perturbed state dict) -- built once per session"""
    if which not in _STATE:
        from tqdne_amd import UNetModel
        cfg = width_cfg(which)
        torch.manual_seed(0)
        _STATE[which] = (cfg, perturbed_state(UNetModel(**cfg), 61))
    return _STATE[which]


def oracle_module_grads(which):
    """oracle forward and autograd of y.square().mean() w.r.t. every parameter and the input -- computed once, shared, left unchanged"""
    if which not in _ORACLE:
        from oracle import unet as OU
        cfg, sd = width_model(which)
        x, t = _batch(2, T_MODEL)
        params = {k: v.clone().requires_grad_(k != "time_embed.W") for k, v in sd.items()}
        xr = x.clone().requires_grad_(True)
        y = OU.unet_forward(params, cfg, xr, t, None)
        y.square().mean().backward()
        _ORACLE[which] = (y.detach(), {k: v.grad for k, v in params.items()}, xr.grad)
    return _ORACLE[which]


def _module_backward(which, ckpt=False):
    from tqdne_amd import UNetModel
    cfg, sd = width_model(which)
    m = UNetModel(**dict(cfg, use_checkpoint=ckpt))
    m.load_state_dict(sd)
    m = m.to(dev()).train()
    x, t = _batch(2, T_MODEL)
    xg = x.to(dev()).requires_grad_(True)
    y = m(xg, t.to(dev()), None)
    y.square().mean().backward()
    return m, y.detach().cpu(), xg.grad.cpu()


@pytest.mark.parametrize("which", list(MODELS))
def test_forward_and_every_gradient_vs_oracle(which):
    """training-mode forward (dropout 0), then ALL parameter gradients and x.grad of y.square().mean() vs oracle autograd; the stem weight
    gradient is the dedicated kernel's at 96 and 160 channels and the generic weight gradient's at 256 and 1024"""
    yo, gref, xref = oracle_module_grads(which)
    m, y, xgrad = _module_backward(which)
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
    print(f"{which}: forward {e:.2e}; worst of {n} parameter gradients {worst:.2e} at {wname}; x.grad {ex:.2e}")
    assert e < TOL_PATH and worst < TOL_PATH and ex < TOL_PATH
    # (stems of more than 2048 weights -- mc256, mc1024 -- take the generic weight gradient, the others the dedicated kernel)
    sw = m.input_blocks[0][0].weight
    assert m._engine(2, T_MODEL, dev())._bwd.stem_generic == (sw.numel() > 2048) == (which in ("mc256", "mc1024"))


@pytest.mark.parametrize("which", ["mc256", "mc96"])
def test_checkpointed_plan_gives_the_gradients_of_the_plain_plan(which):
    """as tests/test_wide_models_gpu.py: same kernels on the same data, 1e-5 of each tensor's largest entry, and the oracle's bar"""
    _, gref, xref = oracle_module_grads(which)
    m0, y0, x0 = _module_backward(which)
    m1, y1, x1 = _module_backward(which, ckpt=True)
    assert m1._engine(2, T_MODEL, dev()).ckpt and not m0._engine(2, T_MODEL, dev()).ckpt
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
    cfg, sd = width_model(which)
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}, num_sampling_steps=steps)
    edm.unet.load_state_dict(sd)
    return edm, cfg, sd


@pytest.mark.parametrize("which", ["mc256", "mc96"])
def test_edm_training_step_loss_vs_oracle(which):
    from oracle import edm as OE
    edm, cfg, sd = _edm(which)
    edm = edm.to(dev()).train()
    B, T = 2, T_MODEL
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


@pytest.mark.parametrize("which", ["mc256", "mc96"])
def test_heun_sampler_3_steps_vs_oracle(which):
    from oracle import edm as OE
    edm, cfg, sd = _edm(which, 3)
    edm = edm.to(dev()).eval()
    g = torch.Generator().manual_seed(3)
    B, T = 2, T_MODEL
    start = torch.randn(B, 3, T, generator=g, dtype=torch.float64)
    sig = OE.sampling_sigmas(OE.EDMParams(), 3)
    out = edm.sample_deterministically((start * sig[0]).to(dev()), sig.to(dev()), None, None)
    with torch.no_grad():
        ref = OE.sample_deterministic(OE.EDMParams(), OE.make_net({("unet." + k): v for k, v in sd.items()}, cfg), start, 3, cond=None)
    e = rel_err(out.cpu(), ref)
    print(f"{which}: 3-step Heun sample (5 NFE): {e:.2e}")
    assert e < TOL_PATH


# ---- VAE -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("part", ["encoder", "decoder"])
def test_vae_coder_forward_and_backward_vs_oracle(part):
    """Encoder 64 x (1, 2, 4) with 8 output channels: a head of 256 input channels.  Decoder 96 x (1, 2) from 4 latent channels: a stem
    to 192 channels and a head of 96 input channels.  Forward, every parameter gradient and the input gradient of sum(y dout) against
    oracle/autoencoder.py; bars of tests/test_autoencoder_step.py (1e-3; gradients against max(|ref|, 1e-3 x the largest gradient))"""
    from oracle import autoencoder as OA
    from tqdne_amd.autoencoder import Decoder, Encoder, _seq_engine
    B, T = 2, 200
    if part == "encoder":
        cfg = dict(in_channels=3, model_channels=64, out_channels=8, num_res_blocks=1, attention_resolutions=(), dropout=0, channel_mult=(1, 2, 4),
                   conv_kernel_size=5, dims=1, num_heads=4)
        mod, fwd, cin, Tin = Encoder(**cfg), OA.encoder_forward, 3, T
    else:
        cfg = dict(in_channels=4, model_channels=96, out_channels=3, num_res_blocks=1, attention_resolutions=(), dropout=0, channel_mult=(1, 2),
                   conv_kernel_size=5, dims=1, num_heads=4)
        mod, fwd, cin, Tin = Decoder(**cfg), OA.decoder_forward, 4, T // 2
    torch.manual_seed(0)
    mod.load_state_dict(perturbed_state(mod, 5))
    sd = {k: v.clone() for k, v in mod.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, cin, Tin, generator=g)
    params = {part + "." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    yo = fwd(params, cfg, xr, part + ".")
    dout = torch.randn(yo.shape, generator=g)
    (yo * dout).sum().backward()
    mod = mod.to(dev()).train()
    eng = _seq_engine(mod, x.to(dev()))
    assert eng.out_mode == "head"
    with torch.no_grad():
        y = eng.forward(x.to(dev()), train=True).clone()
        grads, dx = eng.backward(dout.to(dev()), want_dx=True, clone=True)
    e = rel_err(y.cpu(), yo)
    gmax = max(float(v.grad.abs().max()) for v in params.values())
    worst, wname = 0.0, ""
    for (name, _), gr in zip(mod.named_parameters(), grads):
        ref = params[part + "." + name].grad
        ge = float((gr.cpu() - ref).abs().max() / max(float(ref.abs().max()), 1e-3 * gmax))
        if ge > worst:
            worst, wname = ge, name
    ex = rel_err(dx.cpu()[:, :cin], xr.grad)
    print(f"{part}: forward {e:.2e}; worst parameter gradient {worst:.2e} at {wname}; input gradient {ex:.2e}")
    assert e < 1e-3 and worst < 1e-3 and ex < 1e-3


# ---- concurrency ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin", [256, 1024])
def test_chunked_head_conv_next_to_attention_kernels(cin):
    """as tests/test_concurrency.py::test_head_conv_next_to_attention_kernels: the chunked head forward while attention launches run on
    another stream; every result bit-identical to the run alone.  One pass per aggressor."""
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(cin)
    B, T, H, D = 16, 512, 4, 64
    d = dev()
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(d)
    dout = torch.randn(B, T, H * D, generator=g).to(d)
    hx = torch.randn(8, 2048, cin, generator=g).to(d)
    hb = torch.randn(3, generator=g).to(d)
    gs, gh = (1 + 0.1 * torch.randn(8, cin, generator=g)).to(d), (0.1 * torch.randn(8, cin, generator=g)).to(d)
    hw = (torch.randn(3, cin, 5, generator=g) / math.sqrt(5 * cin)).to(d)
    o_ref, lse = ops.attention(qkv, H, return_lse=True)
    aggressors = [lambda: ops.attention(qkv, H), lambda: ops.attention(qkv, H, workspace=False), lambda: ops.attention_bwd(qkv, o_ref, dout, lse, H)]
    ref = ops.head_conv(hx, hw, hb, gs, gh).clone()
    cpu = F.conv1d(F.silu(hx.cpu().double() * gs.cpu().double()[:, None, :] + gh.cpu().double()[:, None, :]).permute(0, 2, 1), hw.cpu().double(),
                   hb.cpu().double(), padding=2)
    assert rel_err(ref.cpu(), cpu) < TOL_OP
    s_a, s_b = torch.cuda.Stream(d), torch.cuda.Stream(d)
    torch.cuda.synchronize()
    for afn in aggressors:
        outs = []
        for _ in range(8):
            with torch.cuda.stream(s_b):
                afn()
            with torch.cuda.stream(s_a):
                outs.append(ops.head_conv(hx, hw, hb, gs, gh))
        torch.cuda.synchronize()
        assert all(torch.equal(o, ref) for o in outs), f"head conv C_in={cin} changed its result next to a concurrent attention kernel"


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def test_a_1056_channel_first_level_fails_when_the_plan_is_built():
    """NotImplementedError naming the layer at plan construction: the stem of a UNet and of an Encoder, and the output layer of an Encoder
    whose last level alone is 1056 channels wide; the op-level entry points answer TQ_ERR_SHAPE"""
    from tqdne_amd import UNetModel, _lib, ops, tiny_1d_unet_config
    from tqdne_amd.autoencoder import Encoder
    d = dev()
    cfg = dict(tiny_1d_unet_config(), model_channels=1056, channel_mult=(1,), num_res_blocks=1, attention_resolutions=(), dropout=0.0, conv_kernel_size=3)
    torch.manual_seed(0)
    m = UNetModel(**cfg).to(d).eval()
    x, t = _batch(1, 64)
    with pytest.raises(NotImplementedError, match=r"input conv input_blocks\.0\.0: 3 -> 1056 channels"):
        with torch.no_grad():
            m(x.to(d), t.to(d), None)
    enc = dict(in_channels=3, out_channels=8, num_res_blocks=1, attention_resolutions=(), dropout=0, conv_kernel_size=3, dims=1, num_heads=4)
    with pytest.raises(NotImplementedError, match=r"input conv input_layer: 3 -> 1056 channels"):
        with torch.no_grad():
            Encoder(model_channels=1056, channel_mult=(1,), **enc).to(d).eval()(x.to(d))
    with pytest.raises(NotImplementedError, match=r"output conv output_layer: 1056 -> 8 channels"):
        with torch.no_grad():
            Encoder(model_channels=32, channel_mult=(1, 33), **enc).to(d).eval()(x.to(d))
    import tqdne_amd.engine as E
    with pytest.raises(NotImplementedError, match=r"backward of output conv out\.2: 1056 -> 3 channels"):
        E._check_head_bwd_limits(1056, 3, 5)
    w = torch.zeros(3, 1056, 5, device=d)
    with pytest.raises(_lib.TqError, match="TQ_ERR_SHAPE"):
        ops.head_conv(torch.zeros(1, 64, 1056, device=d), w, None)
    with pytest.raises(_lib.TqError, match="TQ_ERR_SHAPE"):
        ops.head_conv_bwd(torch.zeros(1, 3, 64, device=d), torch.zeros(1, 64, 1056, device=d), w)
    with pytest.raises(_lib.TqError, match="TQ_ERR_SHAPE"):
        ops.stem_conv(torch.zeros(1, 3, 64, device=d), torch.zeros(1056, 3, 5, device=d), None)
