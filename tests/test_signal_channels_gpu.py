"""Stems and heads of 17 ... 64 signal channels on the GPU: the two boundary kernels (csrc/boundary.hip), the stem and head as the plans
build them (boundary kernel + generic MFMA conv, weights packed from their real shape into the padded geometry), and whole models --
UNets with 17 ... 64 channels at either end, the signal-conditioned EDM (16 + 16 -> 16) with its samplers, the latent EDM with an
autoencoder, wide Encoder / Decoder ends, the consistency model with a conditioning signal -- against fp64 / the CPU oracle.

Bars (all the suite's own): exact-fp32 ops 1e-5 (tests/test_hip_ops.py::test_head); conv forward 1e-4 and conv gradients 2e-4
(TOL_FWD / TOL_BWD of tests/test_wide_models_gpu.py); whole models 1e-3 norm-wise and element-wise (TOL_PATH), gradients through
conftest.grad_err / GRAD_OWN_TOL."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import grad_err, rel_err
from test_head_sizes_gpu import cl, dev, guarded, ncw, perturbed_state
from test_signal_channels_host import UNETS, ae_cfgs, unet_cfg

pytestmark = pytest.mark.gpu

TOL_EXACT, TOL_FWD, TOL_BWD, TOL_PATH = 1e-5, 1e-4, 2e-4, 1e-3
LENGTHS = (1, 63, 130, 257)
B_K = 3   # batch of the kernel-level tests


# ---- the two boundary kernels --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("C0,C1,Cp", [(17, 0, 32), (16, 16, 32), (24, 9, 64), (32, 32, 64), (64, 0, 64), (3, 0, 32)])
def test_nct_to_btc_equals_torch_bit_for_bit(C0, C1, Cp, T, scaled):
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(C0 + 7 * C1 + T)
    x = torch.randn(B_K, C0, T, generator=g).to(dev())
    cond = torch.randn(B_K, C1, T, generator=g).to(dev()) if C1 else None
    scale = (torch.rand(B_K, generator=g) + 0.5).to(dev()) if scaled else None
    out, chk = guarded(B_K, T, Cp)
    ops.nct_to_btc(x, scale, cond, out=out)
    torch.cuda.synchronize()
    chk()
    ref = torch.zeros(B_K, T, Cp, device=dev())
    ref[:, :, :C0] = (x * scale[:, None, None] if scaled else x).permute(0, 2, 1)
    if C1:
        ref[:, :, C0:C0 + C1] = cond.permute(0, 2, 1)
    assert torch.equal(out, ref)
    assert bool((out[:, :, C0 + C1:] == 0).all())   # every padding channel exactly zero, written by this call (the buffer held NaN)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("C,c_off,Cp", [(17, 0, 32), (16, 0, 32), (16, 16, 32), (40, 0, 64), (64, 0, 64)])
def test_btc_to_nct_plain_scaled_and_with_the_skip_epilogue(C, c_off, Cp, T):
    from tqdne_amd import ops
    g = torch.Generator().manual_seed(C + 3 * c_off + T)
    v = torch.randn(B_K, T, Cp, generator=g)
    a, s = torch.rand(B_K, generator=g) + 0.5, torch.randn(B_K, generator=g)
    skip = torch.randn(B_K, C, T, generator=g)
    vd = v.to(dev())
    sl = v[:, :, c_off:c_off + C].permute(0, 2, 1).double()
    out, chk = guarded(B_K, C, T)
    ops.btc_to_nct(vd, C, c_off, out=out)
    torch.cuda.synchronize()
    chk()
    assert torch.equal(out.cpu(), v[:, :, c_off:c_off + C].permute(0, 2, 1))
    out, chk = guarded(B_K, C, T)
    ops.btc_to_nct(vd, C, c_off, a=a.to(dev()), out=out)
    torch.cuda.synchronize()
    chk()
    e_a = rel_err(out.cpu(), sl * a.double()[:, None, None])
    out, chk = guarded(B_K, C, T)
    ops.btc_to_nct(vd, C, c_off, a=a.to(dev()), s=s.to(dev()), skip_src=skip.to(dev()), out=out)
    torch.cuda.synchronize()
    chk()
    e_f = rel_err(out.cpu(), sl * a.double()[:, None, None] + s.double()[:, None, None] * skip.double())
    out, chk = guarded(B_K, C, T)
    ops.btc_to_nct(vd, C, c_off, s=s.to(dev()), skip_src=skip.to(dev()), out=out)   # (the skip term without the output scale)
    torch.cuda.synchronize()
    chk()
    e_s = rel_err(out.cpu(), sl + s.double()[:, None, None] * skip.double())
    print(f"btc_to_nct C={C} c_off={c_off} Cp={Cp} T={T}: a-only {e_a:.2e} full {e_f:.2e} skip-only {e_s:.2e}")
    assert e_a < TOL_EXACT and e_f < TOL_EXACT and e_s < TOL_EXACT


# ---- stem and head as the plans build them -------------------------------------------------------------------------------------------

ENDS = [(32, 64, 5), (17, 32, 3), (64, 128, 5), (33, 96, 1)]   # (signal channels, first-level width, k)


@pytest.mark.parametrize("T", [130, 61])
@pytest.mark.parametrize("S,W,k", ENDS)
def test_wide_stem_forward_and_gradients_vs_fp64(S, W, k, T):
    """tq_nct_to_btc (input scale folded in) + generic conv with statistics; weight gradient over the padded channels-last input;
    d loss / d x as the generic data gradient + tq_btc_to_nct (input scale folded in)"""
    from tqdne_amd import ops
    from test_wide_models_gpu import ref_stats
    g = torch.Generator().manual_seed(S + W + k + T)
    x = torch.randn(B_K, S, T, generator=g)
    sc = torch.rand(B_K, generator=g) + 0.5
    w = torch.randn(W, S, k, generator=g) / math.sqrt(S * k)
    b = torch.randn(W, generator=g)
    dy = torch.randn(B_K, W, T, generator=g)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = F.conv1d(x64 * sc.double()[:, None, None], w64, b.double(), padding=k // 2)
    ref.backward(dy.double())
    d = dev()
    Cp = (S + 31) // 32 * 32
    xb = ops.nct_to_btc(x.to(d), sc.to(d))
    assert xb.shape == (B_K, T, Cp)
    y, cy = guarded(B_K, T, W)
    st, cs = guarded(B_K, (T + 127) // 128, W, 2)
    ops.conv1d(xb, w.to(d), b.to(d), out=(y, st))
    torch.cuda.synchronize()
    cy(), cs()
    e, es = rel_err(ncw(y), ref.detach()), rel_err(st.cpu(), ref_stats(ref.detach()))
    dw, cw = guarded(W, Cp, k)
    ops.conv1d_bwd_weight(cl(dy), xb, (W, Cp, k), out=dw)
    gx, _, _ = ops.conv1d_bwd_data(cl(dy), w.to(d), pad_cin=Cp)
    dx, cx = guarded(B_K, S, T)
    ops.btc_to_nct(gx, S, a=sc.to(d), out=dx)
    torch.cuda.synchronize()
    cw(), cx()
    e_w, e_x = rel_err(dw[:, :S].cpu(), w64.grad), rel_err(dx.cpu(), x64.grad)
    print(f"wide stem {S} -> {W} k{k} T={T}: forward {e:.2e} statistics {es:.2e}; dw {e_w:.2e} dx {e_x:.2e}")
    assert e < TOL_FWD and es < TOL_FWD and e_w < TOL_BWD and e_x < TOL_BWD
    assert bool((dw[:, S:] == 0).all()) and bool((gx[:, :, S:] == 0).all())   # the padding carries exact zeros


@pytest.mark.parametrize("T", [130, 61])
@pytest.mark.parametrize("S,W,k", ENDS)
def test_wide_head_forward_and_gradients_vs_fp64(S, W, k, T):
    """GroupNorm + SiLU prologue -> generic conv to the padded channel count -> tq_btc_to_nct with the preconditioning epilogue; backward:
    dF = c_out * dpred by tq_nct_to_btc, bias gradient by column sums, generic weight and (chained) data gradients"""
    from tqdne_amd import ops
    from test_hip_bwd import ref_slot_sums
    g = torch.Generator().manual_seed(3 * S + W + k + T)
    h = torch.randn(B_K, W, T, generator=g) + 0.3
    a, sh = torch.rand(B_K, W, generator=g) + 0.5, torch.randn(B_K, W, generator=g)
    w = torch.randn(S, W, k, generator=g) / math.sqrt(W * k)
    b = torch.randn(S, generator=g)
    c_out, c_skip = torch.rand(B_K, generator=g) + 0.5, torch.randn(B_K, generator=g)
    skip = torch.randn(B_K, S, T, generator=g)
    dpred = torch.randn(B_K, S, T, generator=g) * 1e-2
    u = (h.double() * a.double()[:, :, None] + sh.double()[:, :, None]).requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = c_out.double()[:, None, None] * F.conv1d(F.silu(u), w64, b64, padding=k // 2) + c_skip.double()[:, None, None] * skip.double()
    ref.backward(dpred.double())
    d = dev()
    Cp = (S + 31) // 32 * 32
    bp = torch.zeros(Cp, device=d)
    bp[:S] = b.to(d)
    hb = cl(h)
    v, _ = ops.conv1d(hb, w.to(d), bp, gscale=a.to(d), gshift=sh.to(d), silu=True, stats=False, pad_cout=Cp)
    assert v.shape == (B_K, T, Cp) and bool((v[:, :, S:] == 0).all())
    y, cy = guarded(B_K, S, T)
    ops.btc_to_nct(v, S, a=c_out.to(d), s=c_skip.to(d), skip_src=skip.to(d), out=y)
    torch.cuda.synchronize()
    cy()
    e = rel_err(y.cpu(), ref.detach())
    dF = ops.nct_to_btc(dpred.to(d), c_out.to(d))
    db = ops.colsum(dF, per_sample=False)[1]
    dw = ops.conv1d_bwd_weight(dF, hb, (Cp, W, k), gscale=a.to(d), gshift=sh.to(d), silu=True)
    G, _, gst = ops.conv1d_bwd_data(dF, w.to(d), x0=hb, gscale=a.to(d), gshift=sh.to(d), silu=True, stats=True)
    torch.cuda.synchronize()
    e_b, e_w = rel_err(db[:S].cpu(), b64.grad), rel_err(dw[:S].cpu(), w64.grad)
    e_g, e_st = rel_err(ncw(G), u.grad), rel_err(gst.cpu(), ref_slot_sums(u.grad.float(), h))
    print(f"wide head {W} -> {S} k{k} T={T}: forward {e:.2e}; db {e_b:.2e} dw {e_w:.2e} G {e_g:.2e} GN sums {e_st:.2e}")
    assert e < TOL_FWD and e_b < TOL_BWD and e_w < TOL_BWD and e_g < TOL_BWD and e_st < TOL_BWD
    assert bool((dw[S:] == 0).all()) and bool((db[S:] == 0).all())


# ---- whole models --------------------------------------------------------------------------------------------------------------------

_MODELS, _ORACLE = {}, {}


def model(which):
    """(config, perturbed state dict) of one of the micro UNets -- built once per session"""
    if which not in _MODELS:
        from tqdne_amd import UNetModel
        cfg = unet_cfg(which)
        torch.manual_seed(0)
        _MODELS[which] = (cfg, perturbed_state(UNetModel(**cfg), 23))
    return _MODELS[which]


def batch(which, seed=7):
    cin, _, _, T = UNETS[which]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, cin, T, generator=g), 0.5 * torch.randn(2, generator=g), torch.randn(2, 5, generator=g)


def oracle_unet(which):
    """oracle forward and autograd of y.square().mean() with respect to every parameter and the input -- computed once"""
    if which not in _ORACLE:
        from oracle import unet as OU
        cfg, sd = model(which)
        x, t, c = batch(which)
        params = {k: v.clone().requires_grad_(k != "time_embed.W") for k, v in sd.items()}
        xr = x.clone().requires_grad_(True)
        y = OU.unet_forward(params, cfg, xr, t, c)
        y.square().mean().backward()
        _ORACLE[which] = (y.detach(), {k: v.grad for k, v in params.items()}, xr.grad)
    return _ORACLE[which]


def hip_unet(which, train=False):
    from tqdne_amd import UNetModel
    cfg, sd = model(which)
    m = UNetModel(**cfg)
    m.load_state_dict(sd)
    m = m.to(dev())
    return m.train() if train else m.eval()


def worst_grad(named_params, gref, prefix=""):
    gmax = max(float(v.abs().max()) for v in gref.values() if v is not None)
    worst, wname = 0.0, ""
    for name, p in named_params:
        if not p.requires_grad:
            continue
        assert p.grad is not None, name
        ge = grad_err(p.grad, gref[prefix + name], gmax, name)
        if ge > worst:
            worst, wname = ge, name
    return worst, wname


@pytest.mark.parametrize("which", sorted(UNETS))
def test_unet_inference_forward_vs_oracle(which):
    yo, _, _ = oracle_unet(which)
    m = hip_unet(which)
    x, t, c = (v.to(dev()) for v in batch(which))
    with torch.no_grad():
        y = m(x, t, c)
    e = rel_err(y.cpu(), yo)
    print(f"UNet ({which}) {UNETS[which]}: inference forward {e:.2e}")
    assert e < TOL_PATH
    eng = m._engine(2, UNETS[which][3], dev())
    assert eng.wide_stem == (UNETS[which][0] > 16) and eng.wide_head == (UNETS[which][1] > 16)


@pytest.mark.parametrize("which", sorted(UNETS))
def test_unet_training_forward_and_every_gradient_vs_oracle(which):
    """the ordinary-module path: loss = f(unet(x, t, c)); loss.backward() -- all parameter gradients and x.grad"""
    yo, gref, xref = oracle_unet(which)
    m = hip_unet(which, train=True)
    x, t, c = (v.to(dev()) for v in batch(which))
    xg = x.requires_grad_(True)
    y = m(xg, t, c)
    y.square().mean().backward()
    e, ex = rel_err(y.detach().cpu(), yo), rel_err(xg.grad.cpu(), xref)
    worst, wname = worst_grad(m.named_parameters(), gref)
    print(f"UNet ({which}): train forward {e:.2e}; worst parameter gradient {worst:.2e} at {wname}; x.grad {ex:.2e}")
    assert e < TOL_PATH and worst < TOL_PATH and ex < TOL_PATH


def _edm(steps=4, train=False):
    from tqdne_amd import LightningEDM
    cfg, sd = model("a")
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}, num_sampling_steps=steps)
    edm.unet.load_state_dict(sd)
    edm = edm.to(dev())
    return (edm.train() if train else edm.eval()), cfg, sd


def test_signal_conditioned_edm_forward_and_gradients_vs_oracle():
    """EDM.forward(sample, sigma, cond_sample, cond) with a 16-channel conditioning signal behind a 16-channel sample (the UNet's input
    conv sees 32 channels): value, parameter gradients, sample.grad"""
    from oracle import edm as OE
    edm, cfg, sd = _edm(train=True)
    B, T = 2, 200
    g = torch.Generator().manual_seed(11)
    sample, cs = 0.5 * torch.randn(B, 16, T, generator=g), torch.randn(B, 16, T, generator=g)
    cond, sigma = torch.randn(B, 5, generator=g), torch.tensor([0.4, 11.0])
    params = {("unet." + k): v.clone().requires_grad_(k != "time_embed.W") for k, v in sd.items()}
    sr = sample.clone().requires_grad_(True)
    yo = OE.denoise(OE.EDMParams(), OE.make_net(params, cfg), sr, sigma, cond_sample=cs, cond=cond)
    yo.square().mean().backward()
    sg = sample.to(dev()).requires_grad_(True)
    y = edm(sg, sigma.to(dev()), cond_sample=cs.to(dev()), cond=cond.to(dev()))
    y.square().mean().backward()
    e, ex = rel_err(y.detach().cpu(), yo.detach()), rel_err(sg.grad.cpu(), sr.grad)
    worst, wname = worst_grad(edm.unet.named_parameters(), {k: v.grad for k, v in params.items()}, "unet.")
    print(f"signal-conditioned EDM: forward {e:.2e}; worst parameter gradient {worst:.2e} at {wname}; sample.grad {ex:.2e}")
    assert e < TOL_PATH and worst < TOL_PATH and ex < TOL_PATH


LANES_B = 16   # smallest batch at which lanes = 2 takes the lanes branch (sub-batches of at least 8 samples)


def _sampler_case(B=4):
    g = torch.Generator().manual_seed(13 + B)
    T = 200
    start = torch.randn(B, 16, T, generator=g, dtype=torch.float64)
    cs, cond = torch.randn(B, 16, T, generator=g), torch.randn(B, 5, generator=g)
    churn = [torch.randn(B, 16, T, generator=g, dtype=torch.float64) for _ in range(4)]
    return start, cs, cond, churn


_SAMPLES = {}


def oracle_samples(B=4):
    if B not in _SAMPLES:
        from oracle import edm as OE
        _, cfg, sd = _edm()
        net = OE.make_net({("unet." + k): v for k, v in sd.items()}, cfg)
        start, cs, cond, churn = _sampler_case(B)
        with torch.no_grad():
            _SAMPLES[B] = dict(det=OE.sample_deterministic(OE.EDMParams(), net, start, 4, cond=cond, cond_sample=cs),
                               stoch=OE.sample_stochastic(OE.EDMParams(), net, start, churn, 4, cond=cond, cond_sample=cs))
    return _SAMPLES[B]


@pytest.mark.parametrize("B,lanes", [(LANES_B, 2), (4, 1)])
def test_samplers_with_a_conditioning_signal_vs_oracle(B, lanes):
    """deterministic and churned samplers with a 16-channel conditioning signal over 4 sigmas: on one stream (B = 4), and as two
    concurrent lanes of 8 samples (B = 16) -- each lane a plan of its own with its own padded stem input"""
    from oracle import edm as OE
    from tqdne_amd.engine import CONCURRENT_LANE0
    edm, _, _ = _edm()
    start, cs, cond, churn = _sampler_case(B)
    sig = OE.sampling_sigmas(OE.EDMParams(), 4)
    d = dev()
    ref = oracle_samples(B)
    out = edm.sample_deterministically((start * sig[0]).to(d), sig.to(d), cs.to(d), cond.to(d), lanes=lanes)
    e_d = rel_err(out.cpu(), ref["det"])
    out = edm.sample_stochastically((start * sig[0]).to(d), sig.to(d), cs.to(d), cond.to(d), churn_noises=[c.to(d) for c in churn],
                                    lanes=lanes)
    e_s = rel_err(out.cpu(), ref["stoch"])
    plans = list(edm.unet._engine_cache.keys())
    lane_plans = [k for k in plans if k[0] == B // lanes and k[3] >= CONCURRENT_LANE0]
    print(f"samplers with cond_sample, B={B} lanes={lanes}: deterministic {e_d:.2e} stochastic {e_s:.2e}; plans {plans}")
    assert e_d < TOL_PATH and e_s < TOL_PATH
    if lanes > 1:   # the lanes branch was taken: one sub-batch plan per lane, each with a wide stem
        assert len(lane_plans) == lanes, plans
        assert all(edm.unet._engine_cache.get(k).wide_stem for k in lane_plans)
    else:
        assert not lane_plans


def test_graphed_sampler_equals_the_eager_one(monkeypatch):
    from oracle import edm as OE
    edm, _, _ = _edm()
    start, cs, cond, _ = _sampler_case()
    sig = OE.sampling_sigmas(OE.EDMParams(), 4)
    d = dev()
    args = ((start * sig[0]).to(d), sig.to(d), cs.to(d), cond.to(d))
    eager = edm.sample_deterministically(*args, use_graph=False).clone()
    monkeypatch.setenv("TQDNE_SAMPLER_GRAPH", "1")
    graphed = edm.sample_deterministically(*args)
    assert torch.equal(eager, graphed)
    assert rel_err(graphed.cpu(), oracle_samples()["det"]) < TOL_PATH


def test_latent_edm_step_with_a_conditioning_signal_vs_oracle():
    """the signal-conditioned latent EDM in small: a frozen autoencoder (6 signal channels -> 16 latent channels) encodes the signal and
    the conditioning signal, the UNet sees 16 + 16 channels; loss and gradients of ``step`` with every draw injected"""
    from oracle import autoencoder as OA
    from oracle import edm as OE
    from tqdne_amd import LightningAutoencoder, LightningEDM
    enc_cfg, dec_cfg = ae_cfgs(signal=6, latent=16)
    torch.manual_seed(0)
    ae = LightningAutoencoder(enc_cfg, dec_cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0})
    ae_sd = perturbed_state(ae, 31)
    ae.load_state_dict(ae_sd)
    cfg, sd = model("a")
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}, autoencoder=ae)
    edm.unet.load_state_dict(sd)
    edm = edm.to(dev()).train()
    B, T = 2, 256
    g = torch.Generator().manual_seed(17)
    x, cx, cond = torch.randn(B, 6, T, generator=g), torch.randn(B, 6, T, generator=g), torch.randn(B, 5, generator=g)
    e0, e1 = torch.randn(B, 16, T // 2, generator=g), torch.randn(B, 16, T // 2, generator=g)
    eps, noise = torch.randn(B, generator=g), torch.randn(B, 16, T // 2, generator=g)
    params = {("unet." + k): v.clone().requires_grad_(k != "time_embed.W") for k, v in sd.items()}
    with torch.no_grad():
        z, _, _ = OA.encode(ae_sd, enc_cfg, x, e0)
        zc, _, _ = OA.encode(ae_sd, enc_cfg, cx, e1)
    lo = OE.loss_step(OE.EDMParams(), OE.make_net(params, cfg), z, eps, noise, cond=cond, cond_sample=zc)
    lo.backward()
    d = dev()
    draws = iter([e0.to(d), e1.to(d), noise.to(d)])
    o_rl, o_r = torch.randn_like, torch.randn
    torch.randn_like, torch.randn = (lambda t, **k: next(draws)), (lambda *a, **k: eps.to(d))
    try:
        loss = edm.step({"signal": x.to(d), "cond_signal": cx.to(d), "cond": cond.to(d)}, 0)
    finally:
        torch.randn_like, torch.randn = o_rl, o_r
    loss.backward()
    e = rel_err(loss.detach().cpu(), lo.detach())
    worst, wname = worst_grad(edm.unet.named_parameters(), {k: v.grad for k, v in params.items()}, "unet.")
    print(f"latent EDM with cond_signal: loss {float(loss):.6f} vs {float(lo):.6f} ({e:.2e}); worst gradient {worst:.2e} at {wname}")
    assert e < TOL_PATH and worst < TOL_PATH


def _coder_vs_oracle(kind, cfg, x, seed):
    """forward, parameter gradients and input gradient of an Encoder / Decoder plan against autograd through oracle/autoencoder.py"""
    from oracle import autoencoder as OA
    from tqdne_amd import Decoder, Encoder
    from tqdne_amd.autoencoder import _seq_engine
    torch.manual_seed(0)
    mod = (Encoder if kind == "encoder" else Decoder)(**cfg)
    sd = perturbed_state(mod, seed)
    mod.load_state_dict(sd)
    params = {(kind + "." + k): v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    yo = (OA.encoder_forward if kind == "encoder" else OA.decoder_forward)(params, cfg, xr)
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(yo.shape, generator=g) / yo.numel()
    yo.backward(dout)
    mod = mod.to(dev()).eval()
    xd = x.to(dev())
    with torch.no_grad():
        y = mod(xd)
    eng = _seq_engine(mod, xd)
    assert eng.wide_stem
    eng.forward(xd, train=False)
    grads, dx = eng.backward(dout.to(dev()), want_dx=True)
    e, ex = rel_err(y.cpu(), yo.detach()), rel_err(dx.cpu(), xr.grad)
    gref = {k: v.grad for k, v in params.items()}
    gmax = max(float(v.abs().max()) for v in gref.values())
    worst, wname = 0.0, ""
    for (name, _), gg in zip(mod.named_parameters(), grads):
        ge = grad_err(gg, gref[kind + "." + name], gmax, name)
        if ge > worst:
            worst, wname = ge, name
    print(f"{kind} with {cfg['in_channels']} input channels: forward {e:.2e}; worst gradient {worst:.2e} at {wname}; d input {ex:.2e}")
    assert e < TOL_PATH and worst < TOL_PATH and ex < TOL_PATH


def test_decoder_on_32_latent_channels_vs_oracle():
    _, dec_cfg = ae_cfgs(signal=6, latent=32)
    _coder_vs_oracle("decoder", dec_cfg, torch.randn(2, 32, 100, generator=torch.Generator().manual_seed(19)), 37)


def test_encoder_on_24_signal_channels_vs_oracle():
    enc_cfg, _ = ae_cfgs(signal=24, latent=16)
    _coder_vs_oracle("encoder", enc_cfg, torch.randn(2, 24, 200, generator=torch.Generator().manual_seed(21)), 41)


def _consistency(cin, cout, k=5):
    from tqdne_amd import UNetModel
    from tqdne_amd.consistency_model import LithningConsistencyModel
    cfg = dict(unet_cfg("a"), in_channels=cin, out_channels=cout, conv_kernel_size=k)
    torch.manual_seed(0)
    net = UNetModel(**cfg)
    sd = perturbed_state(net, 43)
    net.load_state_dict(sd)
    return LithningConsistencyModel(net).to(dev()).eval(), cfg, sd


@pytest.mark.parametrize("C", [3, 16])
def test_consistency_model_with_a_conditioning_signal_vs_oracle(C):
    """forward with C + C channels (3 + 3: the dedicated stem; 16 + 16: the boundary route) and, for the narrow one, a two-step
    sample_from: the network sees the concatenation, the skip term the sample alone"""
    from oracle import consistency as OC
    from oracle import edm as OE
    cm, cfg, sd = _consistency(2 * C, C)
    net = OE.make_net({("unet." + k): v for k, v in sd.items()}, cfg)
    B, T = 2, 200
    g = torch.Generator().manual_seed(23 + C)
    x, cs, cond = torch.randn(B, C, T, generator=g), torch.randn(B, C, T, generator=g), torch.randn(B, 5, generator=g)
    sigma = torch.tensor([0.7, 20.0])
    d = dev()
    with torch.no_grad():
        y = cm(x.to(d), sigma.to(d), cs.to(d), cond.to(d))
        ref = OC.forward(net, x, sigma, cs, cond, cm.sigma_min, cm.sigma_data)
    e = rel_err(y.cpu(), ref)
    print(f"consistency forward with {C} + {C} channels: {e:.2e}")
    assert e < TOL_PATH
    assert cm.net._engine(B, T, d).wide_stem == (2 * C > 16)
    if C == 3:
        us = [torch.rand(B, C, T, generator=g) for _ in range(2)]
        out = cm.sample_from(x.to(d), [5.0, 0.5], [u.to(d) for u in us], cs.to(d), cond.to(d))
        with torch.no_grad():
            ref = OC.sample(net, x, [5.0, 0.5], us, cs, cond, cm.sigma_min, cm.sigma_max, cm.sigma_data)
        e = rel_err(out.cpu(), ref)
        print(f"consistency two-step sample with a conditioning signal: {e:.2e}")
        assert e < TOL_PATH


def test_consistency_training_step_with_a_conditioning_signal_vs_oracle():
    """iCT step with ``cond_signal`` in the batch, draws injected: teacher and student both see the concatenation, the conditioning
    signal gets no gradient"""
    import numpy as np
    from oracle import consistency as OC
    from oracle import edm as OE
    cm, cfg, sd = _consistency(32, 16)
    cm.max_steps, cm.global_step = 100, 10
    B, T = 2, 200
    g = torch.Generator().manual_seed(29)
    x, cs, cond = 0.5 * torch.randn(B, 16, T, generator=g), torch.randn(B, 16, T, generator=g), torch.randn(B, 5, generator=g)
    epsilon = torch.randn(B, 16, T, generator=g)
    sigmas = cm._schedule().cpu()
    ts = torch.tensor([2, 7])
    params = {("unet." + k): v.clone().requires_grad_(k != "time_embed.W") for k, v in sd.items()}
    net = OE.make_net(params, cfg)
    t_sig, s_sig = sigmas[ts], sigmas[ts + 1]
    with torch.no_grad():
        target = OC.forward(net, x + epsilon * t_sig[:, None, None], t_sig, cs, cond, cm.sigma_min, cm.sigma_data)
    pred = OC.forward(net, x + epsilon * s_sig[:, None, None], s_sig, cs, cond, cm.sigma_min, cm.sigma_data)
    c = 0.00054 * np.sqrt(T)
    lo = ((torch.sqrt((pred - target) ** 2 + c**2) - c) * (1 / (sigmas[1:] - sigmas[:-1]))[ts][:, None, None]).mean()
    lo.backward()
    d = dev()
    o_m, o_r = torch.multinomial, torch.randn_like
    torch.multinomial, torch.randn_like = (lambda pdf, n, replacement=True: ts.to(d)), (lambda t, **k: epsilon.to(d))
    try:
        csd = cs.to(d).requires_grad_(True)
        loss = cm.step({"signal": x.to(d), "cond_signal": csd, "cond": cond.to(d)})
    finally:
        torch.multinomial, torch.randn_like = o_m, o_r
    loss.backward()
    assert csd.grad is None
    e = rel_err(loss.detach().cpu(), lo.detach())
    worst, wname = worst_grad(cm.net.named_parameters(), {k: v.grad for k, v in params.items()}, "unet.")
    print(f"iCT step with cond_signal: loss {float(loss):.6f} vs {float(lo):.6f} ({e:.2e}); worst gradient {worst:.2e} at {wname}")
    assert e < TOL_PATH and worst < TOL_PATH


@pytest.mark.parametrize("which", ["a", "d"])
def test_forward_follows_the_parameters_after_optimizer_steps(which):
    """two FusedAdamEMA steps, then a forward: equal to the oracle on the updated parameters.  Model (a) (32 -> 16): stale packed weights
    of the wide stem site would show.  Model (d) (24 -> 40): both ends are padded (24 -> 32 input rows, 40 -> 64 output rows and bias
    entries), so stale zero-filled fragments or a stale padded copy of ``out.2.bias`` behind the optimizer's raw-pointer update would."""
    from oracle import unet as OU
    from tqdne_amd.optim import FusedAdamEMA
    cfg, _ = model(which)
    m = hip_unet(which, train=True)
    x, t, c = (v.to(dev()) for v in batch(which))
    opt = FusedAdamEMA([(n, p) for n, p in m.named_parameters() if p.requires_grad], lr=1e-2)
    for _ in range(2):
        opt.zero_grad()
        m(x, t, c).square().mean().backward()
        opt.step()
    m.eval()
    with torch.no_grad():
        y = m(x, t, c)
        ref = OU.unet_forward({k: v.detach().cpu() for k, v in m.state_dict().items()}, cfg, x.cpu(), t.cpu(), c.cpu())
    _, sd0 = model(which)
    moved = float((m.out[2].bias.detach().cpu() - sd0["out.2.bias"]).abs().max())
    e = rel_err(y.cpu(), ref)
    print(f"({which}) after two optimizer steps: forward {e:.2e} (out.2.bias moved by {moved:.2e})")
    assert moved > 1e-3 and e < TOL_PATH
    if which == "d":   # the padded bias the head conv reads is the parameter's current value, zero beyond it
        eng = m._engine(2, UNETS[which][3], dev())
        bp = eng.head_rec.site.bias_pad
        assert bp is not None and torch.equal(bp[:40], m.out[2].bias.detach()) and bool((bp[40:] == 0).all())


# ---- narrow models are untouched, limits are refused -----------------------------------------------------------------------------------

def test_narrow_model_reaches_neither_boundary_kernel():
    """the 3-channel tiny model: the traced launch list of a forward names the dedicated stem / head and neither boundary kernel
    (the bit-for-bit comparison with another library build is the next test)"""
    from tqdne_amd import UNetModel, tiny_1d_unet_config
    cfg = dict(tiny_1d_unet_config(), dropout=0.0)
    torch.manual_seed(0)
    m = UNetModel(**cfg)
    m.load_state_dict(perturbed_state(m, 3))
    m = m.to(dev()).eval()
    g = torch.Generator().manual_seed(5)
    B, T = 2, 256
    x, t = torch.randn(B, cfg["in_channels"], T, generator=g).to(dev()), (0.5 * torch.randn(B, generator=g)).to(dev())
    c = torch.randn(B, cfg["cond_features"], generator=g).to(dev()) if cfg.get("cond_features") else None
    eng = m._engine(B, T, dev())
    assert not eng.wide_stem and not eng.wide_head
    eng._trace = []
    with torch.no_grad():
        m(x, t, c)
    names = [e[0] for e in eng._trace]
    eng._trace = None
    assert "stem" in names and "head" in names
    assert not any("nct_to_btc" in n or "btc_to_nct" in n for n in names + [op[2] for op in eng.ops])


_AB_CHILD = r"""
import ctypes, os, sys
import torch
sys.path.insert(0, sys.argv[1])
from tqdne_amd import UNetModel, _lib, tiny_1d_unet_config
raw = ctypes.CDLL(_lib.lib_path())
for name in ("tq_boundary_max_channels", "tq_nct_to_btc", "tq_btc_to_nct"):   # (a library from before these existed: a narrow model
    if not hasattr(raw, name):                                                  #  never calls them)
        _lib._PROTOS.pop(name)
cfg = dict(tiny_1d_unet_config(), dropout=0.0)
torch.manual_seed(0)
m = UNetModel(**cfg)
m.load_state_dict(torch.load(sys.argv[2]))
m = m.to("cuda:0").eval()
g = torch.Generator().manual_seed(5)
B, T = 2, 256
x, t = torch.randn(B, cfg["in_channels"], T, generator=g).cuda(), (0.5 * torch.randn(B, generator=g)).cuda()
c = torch.randn(B, cfg["cond_features"], generator=g).cuda() if cfg.get("cond_features") else None
with torch.no_grad():
    y = m(x, t, c)
xg = x.clone().requires_grad_(True)
m.train()
m(xg, t, c).square().mean().backward()
torch.save(dict(y=y.cpu(), dx=xg.grad.cpu(), dstem=m.input_blocks[0][0].weight.grad.cpu(), dhead=m.out[2].weight.grad.cpu()), sys.argv[3])
"""


def test_narrow_model_is_bit_identical_to_an_ab_library_build(tmp_path):
    """With a second library build at hand -- TQDNE_HIP_LIB_AB, or TQDNE_HIP_LIB where it names another file than the in-tree build, e.g.
    the parent commit's -- the tiny model's inference output, input gradient and end-conv weight gradients are ``torch.equal`` between
    the two builds, each loaded by a fresh child process.  Without one there is nothing to compare and the launch-list test stands alone."""
    import os
    import subprocess
    import sys
    from tqdne_amd import UNetModel, _build, tiny_1d_unet_config
    other = os.environ.get("TQDNE_HIP_LIB_AB") or os.environ.get("TQDNE_HIP_LIB")
    if not other or os.path.realpath(other) == os.path.realpath(_build.LIBPATH):
        return
    assert os.path.exists(other), other
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(0)
    m = UNetModel(**dict(tiny_1d_unet_config(), dropout=0.0))
    torch.save(perturbed_state(m, 3), tmp_path / "sd.pt")
    (tmp_path / "child.py").write_text(_AB_CHILD)
    outs = {}
    for tag, lib in (("tree", _build.LIBPATH), ("ab", other)):
        env = dict(os.environ, TQDNE_HIP_LIB=lib)
        env.pop("TQDNE_HIP_LIB_AB", None)
        r = subprocess.run([sys.executable, str(tmp_path / "child.py"), root, str(tmp_path / "sd.pt"), str(tmp_path / f"{tag}.pt")],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = torch.load(tmp_path / f"{tag}.pt")
    for k in outs["tree"]:
        assert torch.equal(outs["tree"][k], outs["ab"][k]), k


@pytest.mark.parametrize("cin,cout,layer", [(65, 3, r"input conv input_blocks\.0\.0: 65 signal channels"),
                                            (3, 65, r"output conv out\.2: 65 signal channels")])
def test_more_than_64_signal_channels_are_refused_when_the_plan_is_built(cin, cout, layer):
    from tqdne_amd import UNetModel
    torch.manual_seed(0)
    m = UNetModel(**dict(unet_cfg("a"), in_channels=cin, out_channels=cout)).to(dev()).eval()
    with pytest.raises(NotImplementedError, match=layer):
        m._engine(2, 64, dev())


def test_a_decoder_output_of_24_channels_is_refused_when_the_plan_is_built():
    """an Encoder / Decoder output layer is not padded like the UNet's wide head: beyond the head kernel's 16 channels only multiples of 32"""
    from tqdne_amd import Decoder
    torch.manual_seed(0)
    _, dec_cfg = ae_cfgs(signal=24, latent=16)
    dec = Decoder(**dec_cfg).to(dev()).eval()
    with pytest.raises(NotImplementedError, match=r"output_layer: 24 channels"):
        dec(torch.randn(2, 16, 64, device=dev()))


def test_the_dedicated_kernels_still_refuse_17_signal_channels():
    from tqdne_amd import ops
    from tqdne_amd._lib import TqError
    d = dev()
    with pytest.raises(TqError, match="TQ_ERR_SHAPE"):
        ops.stem_conv(torch.randn(2, 17, 64, device=d), torch.randn(32, 17, 5, device=d), torch.randn(32, device=d))
    with pytest.raises(TqError, match="TQ_ERR_SHAPE"):
        ops.head_conv(torch.randn(2, 64, 32, device=d), torch.randn(17, 32, 5, device=d), torch.randn(17, device=d))
