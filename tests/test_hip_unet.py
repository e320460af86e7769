"""Whole-path parity (GPU): tqdne_amd modules on MI355X vs the CPU oracle and the committed golden vectors.
Tolerance 1e-3 relative (north star), measured as max|a-b| / max|b|; observed values are printed."""

import numpy as np
import pytest
import torch

import os

from conftest import GOLDEN, cfg_of, grad_err, load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3


def dev():
    return torch.device("cuda:0")


def perturbed_state(model, seed):
    """zero-init convs re-drawn and GroupNorm affines jittered (same recipe as tools/make_goldens.py)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        v = v.clone()
        is_gn = v.ndim == 1 and (".in_layers.0." in k or ".out_layers.0." in k or ".norm." in k or k.startswith("out.0."))
        if is_gn and k.endswith("weight"):
            v = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif is_gn and k.endswith("bias"):
            v = 0.1 * torch.randn(v.shape, generator=g)
        elif torch.count_nonzero(v) == 0:
            v = 0.02 * torch.randn(v.shape, generator=g)
        sd[k] = v
    return sd


@pytest.mark.parametrize("T", [256, 248])
def test_unet_vs_golden_and_oracle(T):
    from oracle import unet as OU
    from tqdne_amd import UNetModel
    sd, d = load_golden("micro_unet.npz")
    cfg = cfg_of(d)
    m = UNetModel(**cfg)
    m.load_state_dict(sd)
    m = m.to(dev()).eval()
    x, t, c = (torch.from_numpy(d[f"T{T}:{k}"]) for k in ("x", "t", "cond"))
    with torch.no_grad():
        y = m(x.to(dev()), t.to(dev()), c.to(dev())).cpu()
        yo = OU.unet_forward(sd, cfg, x, t, c)
    e_gold, e_orc = rel_err(y, d[f"T{T}:y"]), rel_err(y, yo)
    print(f"micro unet T={T}: rel err vs golden {e_gold:.2e}, vs oracle {e_orc:.2e}")
    assert e_gold < TOL and e_orc < TOL


@pytest.mark.parametrize("which,B,T", [("tiny", 2, 4096), ("paper", 2, 4096), ("paper", 1, 4064)])
def test_full_size_unet_vs_oracle(which, B, T):
    from oracle import unet as OU
    from tqdne_amd import UNetModel, paper_1d_unet_config, tiny_1d_unet_config
    cfg = paper_1d_unet_config() if which == "paper" else tiny_1d_unet_config()
    torch.manual_seed(0)
    m = UNetModel(**cfg)
    sd = perturbed_state(m, 17)
    m.load_state_dict(sd)
    m = m.to(dev()).eval()
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(B, 3, T, generator=g)
    t = torch.randn(B, generator=g) * 0.5
    c = torch.randn(B, 5, generator=g) if cfg["cond_features"] else None
    taps = {}
    with torch.no_grad():
        y = m(x.to(dev()), t.to(dev()), c.to(dev()) if c is not None else None).cpu()
        yo = OU.unet_forward(sd, cfg, x, t, c, taps=taps)
    e = rel_err(y, yo)
    print(f"{which} unet B={B} T={T}: rel err vs oracle {e:.2e}")
    assert e < TOL


def test_wide_unet_model_channels_128_vs_oracle():
    """a 1-D UNet wider than the paper's (model_channels = 128: concatenated tensors of 768 channels feed a GroupNorm, the head
    reads 128 channels) -- the shapes the kernels' former fixed limits rejected at the first forward"""
    from oracle import unet as OU
    from tqdne_amd import UNetModel, tiny_1d_unet_config
    cfg = dict(tiny_1d_unet_config(), model_channels=128, channel_mult=(1, 2, 3), num_res_blocks=1, num_heads=6)  # (middle attention: D = 64)
    torch.manual_seed(0)
    m = UNetModel(**cfg)
    sd = perturbed_state(m, 31)
    m.load_state_dict(sd)
    m = m.to(dev()).eval()
    g = torch.Generator().manual_seed(5)
    B, T = 2, 512
    x, t = torch.randn(B, 3, T, generator=g), torch.randn(B, generator=g) * 0.5
    with torch.no_grad():
        y = m(x.to(dev()), t.to(dev())).cpu()
        yo = OU.unet_forward(sd, cfg, x, t, None)
    e = rel_err(y, yo)
    print(f"model_channels=128 unet: rel err vs oracle {e:.2e}")
    assert e < TOL


def _edm_pair(num_steps=18):
    from tqdne_amd import LightningEDM
    sd, _ = load_golden("micro_unet.npz")
    _, d = load_golden("micro_edm.npz")
    cfg = cfg_of(d)
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}, num_sampling_steps=num_steps)
    edm.unet.load_state_dict(sd)
    return edm.to(dev()).eval(), d


@pytest.mark.parametrize("sigma", [0.002, 0.5, 80.0])
def test_edm_denoise_vs_golden(sigma):
    edm, d = _edm_pair()
    x = torch.from_numpy(d[f"denoise:{sigma}:x"]).to(dev())
    with torch.no_grad():
        y = edm(x, torch.full((x.shape[0],), sigma, device=dev()), None, torch.from_numpy(d["cond"]).to(dev()))
    e = rel_err(y.cpu(), d[f"denoise:{sigma}:y"])
    print(f"denoise sigma={sigma}: {e:.2e}")
    assert e < TOL


def test_edm_sampler_vs_golden():
    edm, d = _edm_pair(18)
    from oracle import edm as OE
    sig = OE.sampling_sigmas(OE.EDMParams(), 18)
    assert np.array_equal(sig.numpy(), d["sigmas18"])
    start = torch.from_numpy(d["sample:start"])
    eps = (start * sig[0]).to(dev())
    cond = torch.from_numpy(d["cond"]).to(dev())
    for nsteps, key in ((1, "sample:state1"), (9, "sample:state9")):
        st = edm.sample_deterministically(eps, sig[: nsteps + 1].to(dev()), None, cond)
        e = rel_err(st.cpu(), d[key])
        print(f"sampler state after {nsteps} steps: {e:.2e}")
        assert e < TOL
    out = edm.sample_deterministically(eps, sig.to(dev()), None, cond).to(torch.float32)
    e = rel_err(out.cpu(), d["sample:out"])
    print(f"18-step sample (35 NFE): {e:.2e}")
    assert e < TOL


def test_edm_loss_value_vs_golden():
    edm, d = _edm_pair()
    with torch.no_grad():
        loss = edm.step_with_noise(torch.from_numpy(d["signal"]).to(dev()), torch.from_numpy(d["step:eps"]).to(dev()),
                                   torch.from_numpy(d["step:noise"]).to(dev()), cond=torch.from_numpy(d["cond"]).to(dev()))
    e = rel_err(loss.cpu(), d["step:loss"])
    print(f"loss: {e:.2e}")
    assert e < TOL


def test_consistency_vs_golden():
    from tqdne_amd import LithningConsistencyModel, UNetModel
    sd, _ = load_golden("micro_unet.npz")
    _, d = load_golden("micro_cm.npz")
    net = UNetModel(**cfg_of(d))
    net.load_state_dict(sd)
    cm = LithningConsistencyModel(net).to(dev()).eval()
    cond = torch.from_numpy(d["cond"]).to(dev())
    y1 = cm.sample_from(torch.from_numpy(d["start"]).to(dev()), [], [], cond=cond)
    y2 = cm.sample_from(torch.from_numpy(d["start"]).to(dev()), [1.0], [torch.from_numpy(d["uniform"]).to(dev())], cond=cond)
    e1, e2 = rel_err(y1.cpu(), d["one_step"]), rel_err(y2.cpu(), d["refined"])
    print(f"consistency 1-step {e1:.2e}, refined {e2:.2e}")
    assert e1 < TOL and e2 < TOL


def test_edm_step_gradients_vs_golden():
    """loss.backward() through the hand-written HIP backward vs the reference's autograd gradients (golden)."""
    edm, d = _edm_pair()
    edm.train()  # dropout is 0.0 in the micro config, so train mode is deterministic
    loss = edm.step_with_noise(torch.from_numpy(d["signal"]).to(dev()), torch.from_numpy(d["step:eps"]).to(dev()),
                               torch.from_numpy(d["step:noise"]).to(dev()), cond=torch.from_numpy(d["cond"]).to(dev()))
    assert rel_err(loss.detach().cpu(), d["step:loss"]) < TOL
    loss.backward()
    worst = 0.0
    n = 0
    for k in d:
        if k.startswith("step:grad:"):
            name = k[len("step:grad:"):]
            g = edm.get_parameter(name).grad
            assert g is not None, name
            e = rel_err(g.cpu(), d[k])
            print(f"grad {name}: {e:.2e}")
            worst = max(worst, e)
            n += 1
    assert n >= 15 and worst < TOL


@pytest.mark.parametrize("which", ["tiny", "paper"])
def test_full_size_gradients_vs_oracle(which):
    """every parameter gradient of the EDM loss at 3 x 4096 (B=2) vs torch autograd through the CPU oracle"""
    from oracle import edm as OE
    from tqdne_amd import LightningEDM, paper_1d_unet_config, tiny_1d_unet_config
    cfg = dict(paper_1d_unet_config() if which == "paper" else tiny_1d_unet_config(), dropout=0.0)
    torch.manual_seed(0)
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0})
    sd = perturbed_state(edm.unet, 23)
    edm.unet.load_state_dict(sd)
    edm = edm.to(dev()).train()
    g = torch.Generator().manual_seed(77)
    B, T = 2, 4096
    sig = 0.5 * torch.randn(B, 3, T, generator=g)
    cond = torch.randn(B, 5, generator=g) if cfg["cond_features"] else None
    eps, noise = torch.randn(B, generator=g), torch.randn(B, 3, T, generator=g)
    loss = edm.step_with_noise(sig.to(dev()), eps.to(dev()), noise.to(dev()), cond=cond.to(dev()) if cond is not None else None)
    loss.backward()
    params = {("unet." + k): v.clone().requires_grad_(k != "time_embed.W") for k, v in sd.items()}
    lo = OE.loss_step(OE.EDMParams(), OE.make_net(params, cfg), sig, eps, noise, cond=cond)
    lo.backward()
    assert rel_err(loss.detach().cpu(), lo.detach()) < TOL
    worst, wname = 0.0, ""
    # gradients that are exactly zero in exact arithmetic (a bias feeding a GroupNorm whose groups have one channel,
    # C=32) are pure rounding noise on both sides: errors are measured against max(|ref|, 1e-3 * largest gradient)
    gmax = max(float(v.grad.abs().max()) for v in params.values() if v.grad is not None)
    for name, p in edm.unet.named_parameters():
        ref = params["unet." + name].grad
        if not p.requires_grad:
            continue
        e = grad_err(p.grad, ref, gmax, name)
        if e > worst:
            worst, wname = e, name
    print(f"{which}: loss {float(loss):.6f}; worst gradient rel err {worst:.2e} at {wname}")
    assert worst < TOL


def test_cond_signal_step_and_denoise_vs_oracle():
    """edm.py:108-109,117-124: a conditioning signal concatenated on the channel axis (the up-sampling dataset's
    "cond_signal", dataset.py:171-177) -- denoiser output, loss and every gradient vs autograd through the CPU oracle"""
    from oracle import edm as OE
    from tqdne_amd import LightningEDM, tiny_1d_unet_config
    cfg = dict(tiny_1d_unet_config(in_channels=6, out_channels=3), dropout=0.0)
    torch.manual_seed(0)
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0})
    sd = perturbed_state(edm.unet, 5)
    edm.unet.load_state_dict(sd)
    edm = edm.to(dev())
    g = torch.Generator().manual_seed(9)
    B, T = 2, 1000
    sig, cs = 0.5 * torch.randn(B, 3, T, generator=g), torch.randn(B, 3, T, generator=g)
    eps, noise = torch.randn(B, generator=g), torch.randn(B, 3, T, generator=g)
    sigma = torch.tensor([0.4, 11.0])
    net = OE.make_net({("unet." + k): v for k, v in sd.items()}, cfg)
    edm.eval()
    with torch.no_grad():
        y = edm(sig.to(dev()), sigma.to(dev()), cond_sample=cs.to(dev()))
        ref = OE.denoise(OE.EDMParams(), net, sig, sigma, cond_sample=cs)
    assert rel_err(y.cpu(), ref) < TOL
    edm.train()
    loss = edm.step_with_noise(sig.to(dev()), eps.to(dev()), noise.to(dev()), cond_sample=cs.to(dev()))
    loss.backward()
    params = {("unet." + k): v.clone().requires_grad_(k != "time_embed.W") for k, v in sd.items()}
    lo = OE.loss_step(OE.EDMParams(), OE.make_net(params, cfg), sig, eps, noise, cond_sample=cs)
    lo.backward()
    assert rel_err(loss.detach().cpu(), lo.detach()) < TOL
    gmax = max(float(v.grad.abs().max()) for v in params.values() if v.grad is not None)
    worst = 0.0
    for name, p in edm.unet.named_parameters():
        if p.requires_grad:
            r = params["unet." + name].grad
            worst = max(worst, grad_err(p.grad, r, gmax, name))
    print(f"cond_signal: loss {float(loss):.6f}; worst gradient rel err {worst:.2e}")
    assert worst < TOL
    # the trainer's fused step takes the same batch key
    loss2, flat = edm.step_and_backward({"signal": sig.to(dev()), "cond_signal": cs.to(dev())})
    assert torch.isfinite(loss2) and float(flat.abs().max()) > 0
    # 4-step deterministic sampler with the conditioning signal (edm.py:169-196)
    edm.eval()
    edm.num_sampling_steps = 4
    sigmas = OE.sampling_sigmas(OE.EDMParams(), 4)
    start = torch.randn(B, 3, T, generator=g, dtype=torch.float64)
    out = edm.sample_deterministically((start * sigmas[0]).to(dev()), sigmas.to(dev()), cs.to(dev()), None)
    with torch.no_grad():
        ref = OE.sample_deterministic(OE.EDMParams(), net, start, 4, cond_sample=cs)
    assert rel_err(out.cpu(), ref) < TOL


def test_two_lane_sampler_is_bit_identical():
    """half batches on two streams (lanes=2, the default for B >= 16) integrate exactly the same per-sample arithmetic"""
    edm, d = _edm_pair(4)
    from oracle import edm as OE
    sig = OE.sampling_sigmas(OE.EDMParams(), 4).to(dev())
    g = torch.Generator().manual_seed(31)
    B = 16
    start = torch.randn(B, 3, 256, generator=g, dtype=torch.float64).to(dev()) * sig[0]
    cond = torch.randn(B, 5, generator=g).to(dev())
    import tqdne_amd.engine as E
    old_w = E.SMALL_TILE_WGS
    try:
        E.SMALL_TILE_WGS = 0   # (same tiles in the one-lane plan and in the lanes' plans)
        one = edm.sample_deterministically(start, sig, None, cond, lanes=1)
        two = edm.sample_deterministically(start, sig, None, cond, lanes=2)
        four = edm.sample_deterministically(start, sig, None, cond, lanes=4)  # 4 per lane < 8: falls back to one lane
    finally:
        E.SMALL_TILE_WGS = old_w
    assert torch.equal(one, two) and torch.equal(one, four)
    assert torch.isfinite(one).all()
    # default rule: a plan that has the device to itself takes the small position tile where the default grid is <= SMALL_TILE_WGS
    # workgroups (here: 16 samples x 2 tiles), the lanes' plans never do -> same convolution arithmetic, GroupNorm sums associated
    # differently, results equal at rounding level
    edm2, _ = _edm_pair(4)
    one_s = edm2.sample_deterministically(start, sig, None, cond, lanes=1)
    two_s = edm2.sample_deterministically(start, sig, None, cond, lanes=2)
    assert torch.equal(two_s, two)
    assert any(getattr(op_desc, "t_tile", 0) == 32 for e in edm2.unet._engine_cache.values() if e.solo for op_desc in e._keep
               if hasattr(op_desc, "t_tile")) or old_w == 0
    assert rel_err(one_s.cpu(), one.cpu()) < 1e-5


def test_autoencoder_vs_golden():
    from tqdne_amd import LightningAutoencoder
    sd, d = load_golden("micro_ae.npz")
    ae = LightningAutoencoder(cfg_of(d, "enc_cfg"), cfg_of(d, "dec_cfg"), {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0})
    ae.load_state_dict(sd)
    ae = ae.to(dev()).eval()
    with torch.no_grad():
        z, mean, log_std = ae._encode(torch.from_numpy(d["x"]).to(dev()), unit_noise=torch.from_numpy(d["eps"]).to(dev()))
        xr = ae.decode(z)
    errs = [rel_err(mean.cpu(), d["mean"]), rel_err(log_std.cpu(), d["log_std"]), rel_err(z.cpu(), d["z"]), rel_err(xr.cpu(), d["recon"])]
    print("autoencoder mean/log_std/z/recon:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < TOL


def test_latent_edm_pipeline_vs_oracle():
    """BASELINE config 3 at reduced batch: 3 x 16384 -> VAE encoder -> 16 x 4096 latent, latent UNet Heun sample, decoder."""
    from oracle import autoencoder as OA
    from oracle import edm as OE
    from tqdne_amd import LightningAutoencoder, LightningEDM, get_1d_autoencoder_configs, paper_1d_unet_config

    class C:
        channels, latent_channels = 3, 16

    enc_cfg, dec_cfg = get_1d_autoencoder_configs(C)
    torch.manual_seed(0)
    ae = LightningAutoencoder(enc_cfg, dec_cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0})
    ae_sd = perturbed_state(ae, 5)
    ae.load_state_dict(ae_sd)
    ucfg = paper_1d_unet_config(in_channels=16, out_channels=16)
    edm = LightningEDM(ucfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}, num_sampling_steps=3, autoencoder=ae)
    u_sd = perturbed_state(edm.unet, 6)
    edm.unet.load_state_dict(u_sd)
    edm = edm.to(dev()).eval()
    g = torch.Generator().manual_seed(9)
    B, T = 1, 16384
    x = 0.5 * torch.randn(B, 3, T, generator=g)
    eps_enc = torch.randn(B, 16, T // 4, generator=g)
    cond = torch.randn(B, 5, generator=g)
    start = torch.randn(B, 16, T // 4, generator=g, dtype=torch.float64)
    with torch.no_grad():
        z = ae._encode(x.to(dev()), unit_noise=eps_enc.to(dev()))[0].cpu()
        zo = OA.encode(ae_sd, enc_cfg, x, eps_enc)[0]
        sig = OE.sampling_sigmas(OE.EDMParams(), 3)
        lat = edm.sample_deterministically((start * sig[0]).to(dev()), sig.to(dev()), None, cond.to(dev())).float()
        rec = ae.decode(lat).cpu()
        net = OE.make_net({"unet." + k: v for k, v in u_sd.items()}, ucfg)
        lat_o = OE.sample_deterministic(OE.EDMParams(), net, start, 3, cond=cond).float()
        rec_o = OA.decode(ae_sd, dec_cfg, lat_o)
    e = [rel_err(z, zo), rel_err(lat.cpu(), lat_o), rel_err(rec, rec_o)]
    print("latent pipeline encode / latent sample / decode:", " ".join(f"{v:.2e}" for v in e))
    assert max(e) < TOL
    assert edm.sample((B, 3, T), cond=cond.to(dev())).shape == (B, 3, T)


def test_trainer_step_matches_autograd_path():
    """DataParallelTrainer's fused step (no autograd) produces the same loss / gradients as loss.backward()."""
    from tqdne_amd import LightningEDM
    from tqdne_amd.trainer import DataParallelTrainer
    sd, _ = load_golden("micro_unet.npz")
    _, d = load_golden("micro_edm.npz")
    edm = LightningEDM(cfg_of(d), {"learning_rate": 1e-3, "max_steps": 10, "eta_min": 0.0})
    edm.unet.load_state_dict(sd)
    edm = edm.to(dev()).train()
    sig, cond = torch.from_numpy(d["signal"]).to(dev()), torch.from_numpy(d["cond"]).to(dev())
    eps, noise = torch.from_numpy(d["step:eps"]).to(dev()), torch.from_numpy(d["step:noise"]).to(dev())
    loss = edm.step_with_noise(sig, eps, noise, cond=cond)
    loss.backward()
    ref = {n: p.grad.clone() for n, p in edm.unet.named_parameters() if p.grad is not None}
    for p in edm.parameters():
        p.grad = None
    from tqdne_amd.autograd import edm_loss_and_grads
    loss2, flat = edm_loss_and_grads(edm, sig, eps, noise, cond)
    assert rel_err(loss2.cpu(), loss.detach().cpu()) < 1e-6
    gmax = max(float(v.abs().max()) for v in ref.values())
    for n, p in edm.unet.named_parameters():
        if n in ref:  # (biases in front of a one-channel-per-group GroupNorm have an exactly-zero gradient: rounding noise)
            err = float((p.grad - ref[n]).abs().max()) / max(float(ref[n].abs().max()), 1e-3 * gmax)
            assert err < 1e-4, (n, err)
    before = {n: p.detach().clone() for n, p in edm.unet.named_parameters()}
    tr = DataParallelTrainer(edm, world_size=1, ema_decay=0.5)
    assert tr.fused  # on a GPU the update is the one-launch Adam + EMA
    tr.train_step({"signal": sig, "cond": cond})
    changed = sum(int(not torch.equal(before[n], p.detach())) for n, p in edm.unet.named_parameters() if p.requires_grad)
    assert changed > 100
    # first Adam step moves every weight with a gradient by lr (to rounding); the EMA is halfway between old and new
    ema = tr.ema_state()
    for n, p in edm.named_parameters():
        if p.requires_grad and n.startswith("unet.") and n[5:] in ref and float(ref[n[5:]].abs().max()) > 0:
            new = p.detach()
            assert rel_err(ema[n], 0.5 * (before[n[5:]] + new)) < 1e-5, n


def test_edm_stochastic_sampler_vs_golden():
    edm, d = _edm_pair(6)
    edm.deterministic_sampling = False
    from oracle import edm as OE
    sig = OE.sampling_sigmas(OE.EDMParams(), 6)
    start = torch.from_numpy(d["stoch:start"])
    churn = [torch.from_numpy(c).to(dev()) for c in d["stoch:churn"]]
    out = edm.sample_stochastically((start * sig[0]).to(dev()), sig.to(dev()), None, torch.from_numpy(d["cond"]).to(dev()),
                                    churn_noises=churn).to(torch.float32)
    e = rel_err(out.cpu(), d["stoch:out"])
    print(f"6-step stochastic sampler: {e:.2e}")
    assert e < TOL


def test_batch_of_one_and_repeated_calls_are_consistent():
    """plans are cached per (B, T): a second call with new inputs and a B=1 plan must agree with the B=2 result"""
    from tqdne_amd import UNetModel
    sd, d = load_golden("micro_unet.npz")
    m = UNetModel(**cfg_of(d))
    m.load_state_dict(sd)
    m = m.to(dev()).eval()
    x, t, c = (torch.from_numpy(d[f"T256:{k}"]).to(dev()) for k in ("x", "t", "cond"))
    with torch.no_grad():
        y2 = m(x, t, c)
        y1 = m(x[:1].contiguous(), t[:1].contiguous(), c[:1].contiguous())
        y2b = m(x, t, c)
    assert torch.equal(y2, y2b)
    assert rel_err(y1.cpu(), y2[:1].cpu()) < 1e-6


def test_graph_replayed_sampler_matches_eager():
    edm, d = _edm_pair(18)
    from oracle import edm as OE
    sig = OE.sampling_sigmas(OE.EDMParams(), 18).to(dev())
    eps = (torch.from_numpy(d["sample:start"]) * sig[0].cpu()).to(dev())
    cond = torch.from_numpy(d["cond"]).to(dev())
    a = edm.sample_deterministically(eps, sig, None, cond, use_graph=False)
    b = edm.sample_deterministically(eps, sig, None, cond, use_graph=True)   # the whole 18-step integration as one HIP graph
    c = edm.sample_deterministically(eps, sig, None, cond, use_graph=True)   # cached graph
    assert torch.equal(a, b) and torch.equal(a, c)
    assert rel_err(a.float().cpu(), d["sample:out"]) < TOL
    # new inputs through the cached graph (start state and conditioning are copied into the graph's static buffers)
    g = torch.Generator().manual_seed(77)
    eps2 = (torch.randn(eps.shape, generator=g, dtype=torch.float64) * float(sig[0])).to(dev())
    cond2 = torch.randn(cond.shape, generator=g).to(dev())
    a2 = edm.sample_deterministically(eps2, sig, None, cond2, use_graph=False)
    b2 = edm.sample_deterministically(eps2, sig, None, cond2, use_graph=True)
    assert torch.equal(a2, b2) and not torch.equal(a2, a)
    e = edm.sample_deterministically(eps, sig, None, cond, use_graph="denoiser")   # round 1's form: one captured evaluation per NFE
    f = edm.sample_deterministically(eps, sig, None, cond)                          # default at this batch size: the whole-loop graph
    assert torch.equal(a, e) and torch.equal(a, f)


def test_consistency_training_step_vs_reference():
    """iCT step (consistency_model.py:115-176): loss and gradients vs the reference's own step (micro_cm_step.npz), with its
    multinomial / randn_like draws injected"""
    import numpy as np
    from tqdne_amd import UNetModel
    from tqdne_amd.consistency_model import LithningConsistencyModel
    sd, d = load_golden("micro_unet.npz")
    s = np.load(os.path.join(GOLDEN, "micro_cm_step.npz"))
    net = UNetModel(**cfg_of(d))
    net.load_state_dict(sd)
    cm = LithningConsistencyModel(net).to(dev()).eval()  # golden taken in eval mode
    cm.max_steps, cm.global_step = int(s["max_steps"]), int(s["global_step"])
    sched = cm._schedule()
    from oracle import consistency as OC
    assert rel_err(sched.cpu(), OC.ict_schedule(cm.global_step, cm.max_steps)) < 1e-6
    o_m, o_r = torch.multinomial, torch.randn_like
    seen = {}

    def mult(pdf, n, replacement=True):
        seen["pdf"] = pdf
        return torch.from_numpy(s["timesteps"]).to(dev())

    torch.multinomial, torch.randn_like = mult, (lambda t, **k: torch.from_numpy(s["eps"]).to(dev()))
    try:
        loss = cm.step({"signal": torch.from_numpy(s["sample"]).to(dev()), "cond": torch.from_numpy(s["cond"]).to(dev())})
    finally:
        torch.multinomial, torch.randn_like = o_m, o_r
    assert rel_err(seen["pdf"].cpu(), s["pdf"]) < 1e-5
    assert rel_err(loss.detach().cpu(), s["loss"]) < TOL
    loss.backward()
    grads = dict(net.named_parameters())
    gmax = float(s["gnorm"].max())
    for n, gn, gp in zip(s["gnames"], s["gnorm"], s["gproj"]):
        g = grads[str(n)].grad.reshape(-1).double().cpu()
        pat = torch.cos(torch.arange(g.numel(), dtype=torch.float64) * 0.37 + 0.1)
        assert abs(float(g.norm()) - gn) < 1e-3 * max(gn, 1e-3 * gmax), n
        assert abs(float((g * pat).sum()) - gp) < 1e-3 * max(gn, 1e-3 * gmax), n
    for k in s.files:
        if k.startswith("g:"):
            ref = torch.from_numpy(s[k])
            e = float((grads[k[2:]].grad.cpu() - ref).abs().max() / max(float(ref.abs().max()), 1e-3 * gmax))
            assert e < TOL, (k, e)


def test_two_lane_training_step_matches_one_lane():
    """fused training step on two streams (sub-batches of 16): same loss and gradients as one stream (summation order only)"""
    from tqdne_amd import LightningEDM
    from tqdne_amd.autograd import edm_loss_and_grads
    sd, _ = load_golden("micro_unet.npz")
    _, d = load_golden("micro_edm.npz")
    edm = LightningEDM(dict(cfg_of(d), dropout=0.0), {"learning_rate": 1e-3, "max_steps": 10, "eta_min": 0.0})
    edm.unet.load_state_dict(sd)
    edm = edm.to(dev()).train()
    g = torch.Generator().manual_seed(12)
    B, T = 32, 256
    sig = (0.5 * torch.randn(B, 3, T, generator=g)).to(dev())
    cond = torch.randn(B, 5, generator=g).to(dev())
    eps, noise = torch.randn(B, generator=g).to(dev()), torch.randn(B, 3, T, generator=g).to(dev())
    l1, f1 = edm_loss_and_grads(edm, sig, eps, noise, cond, lanes=1)
    g1 = {n: p.grad.clone() for n, p in edm.unet.named_parameters() if p.grad is not None}
    l2, f2 = edm_loss_and_grads(edm, sig, eps, noise, cond, lanes=2)
    assert rel_err(l2.cpu(), l1.cpu()) < 1e-6
    gmax = max(float(v.abs().max()) for v in g1.values())
    for n, p in edm.unet.named_parameters():
        if n in g1:
            e = float((p.grad - g1[n]).abs().max()) / max(float(g1[n].abs().max()), 1e-3 * gmax)
            assert e < 1e-4, (n, e)


@pytest.mark.parametrize("which", ["micro", "paper"])
def test_inference_forward_matches_backward_capable_forward(which):
    """infer=True plans (qkv projection writing the attention kernel's pre-split K / V planes itself, no fp32 K / V, no split
    pass) compute the same arithmetic as the default plan: bit-identical outputs; and they refuse a backward"""
    from tqdne_amd import UNetModel, paper_1d_unet_config
    if which == "micro":
        sd, d = load_golden("micro_unet.npz")
        cfg, T = cfg_of(d), 248  # heads of 32 channels, ragged T (padding rows of the planes)
        net = UNetModel(**cfg)
        net.load_state_dict(sd)
    else:
        cfg, T = paper_1d_unet_config(), 4096
        torch.manual_seed(0)
        net = UNetModel(**cfg)
        net.load_state_dict(perturbed_state(net, 3))
    net = net.to(dev()).eval()
    g = torch.Generator().manual_seed(4)
    B = 2
    x = torch.randn(B, cfg["in_channels"], T, generator=g).to(dev())
    t = torch.randn(B, generator=g).to(dev())
    cond = torch.randn(B, 5, generator=g).to(dev())
    import copy
    import os
    os.environ["TQDNE_POLYPHASE_UPSAMPLE"] = "0"
    try:
        eng = copy.deepcopy(net)._engine(B, T, dev())
    finally:
        del os.environ["TQDNE_POLYPHASE_UPSAMPLE"]
    a = eng.forward(x, t, cond).clone()
    # (TQ_KV_V_BF16: the inference pair keeps V as bf16 hi / lo planes and P as a bf16 hi / lo pair, as the training forward does)
    from tqdne_amd import _lib
    fmt0 = eng.kv_v_format   # (fp16 planes by default; bf16 under TQDNE_CONV_SCHEME=bf16x3 / TQDNE_ATTN_VF16=0)
    assert fmt0 == _lib.attn_v_format()
    eng.set_kv_v_format(_lib.TQ_KV_V_BF16)
    b = eng.forward(x, t, cond, infer=True).clone()
    eng.set_kv_v_format(fmt0)
    assert torch.equal(a, b)
    # default inference form of the attention core: V as fp16 hi / lo planes, P as ONE fp16 value -- two products instead of
    # three; 1.4e-4 of the attention output's scale on random data, less at the UNet's output
    b16 = eng.forward(x, t, cond, infer=True).clone()
    e16 = rel_err(b16.cpu(), a.cpu())
    print(f"inference forward with fp16 P / V vs the three-product form: {e16:.2e}")
    assert (0 < e16 < 2e-4) if fmt0 == _lib.TQ_KV_V_F16 else e16 == 0.0
    assert any(op[2].endswith("+split") for op in eng.ops_infer) and len(eng.ops) == len(eng.ops_infer)
    with pytest.raises(RuntimeError):
        eng.backward(torch.zeros_like(a), torch.ones((), device=dev()))
    # default plan: the upsampling convs additionally run as two-phase k = 3 convs at inference (TQ_CONV_POLY2, where the
    # un-upsampled length is a multiple of 128 or leaves more than half a slot): same sums in a different order -> fp32-rounding-level differences only
    eng2 = net._engine(B, T, dev())
    a2 = eng2.forward(x, t, cond).clone()
    eng2.set_kv_v_format(_lib.TQ_KV_V_BF16)
    b2 = eng2.forward(x, t, cond, infer=True).clone()
    eng2.set_kv_v_format(fmt0)
    # round 6: forwards a backward may follow run the two-phase form too (their gradients are that conv's)
    assert torch.equal(a2, b2) and 0 < rel_err(a2.cpu(), a.cpu()) < 4e-5
    npoly = sum(op[2].endswith("+polyphase") for op in eng2.ops_infer)
    # (micro at T = 248: the up-sampling conv over 124 rows qualifies since round 5 -- a last tile of more than 64 rows --, the one over 62 does not)
    assert npoly == (3 if which == "paper" else 1)
    assert rel_err(b2.cpu(), a.cpu()) < 4e-5


def test_latent_edm_training_step_gradients_vs_oracle():
    """BASELINE config 3 training (train_1d_latent_edm.py): the latent UNet has 16 input / output channels -- loss and every
    gradient, incl. the 16-channel stem's (differentiated as a generic conv over a padded channels-last copy), vs autograd
    through the CPU oracle.  (The frozen autoencoder only supplies the latent; a random latent stands in for it here.)"""
    from oracle import edm as OE
    from tqdne_amd import LightningEDM, tiny_1d_unet_config
    cfg = dict(tiny_1d_unet_config(in_channels=16, out_channels=16), dropout=0.0)
    torch.manual_seed(0)
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0})
    sd = perturbed_state(edm.unet, 8)
    edm.unet.load_state_dict(sd)
    edm = edm.to(dev()).train()
    g = torch.Generator().manual_seed(21)
    B, T = 2, 1024
    lat = 0.5 * torch.randn(B, 16, T, generator=g)
    eps, noise = torch.randn(B, generator=g), torch.randn(B, 16, T, generator=g)
    loss = edm.step_with_noise(lat.to(dev()), eps.to(dev()), noise.to(dev()))
    loss.backward()
    params = {("unet." + k): v.clone().requires_grad_(k != "time_embed.W") for k, v in sd.items()}
    lo = OE.loss_step(OE.EDMParams(), OE.make_net(params, cfg), lat, eps, noise)
    lo.backward()
    assert rel_err(loss.detach().cpu(), lo.detach()) < TOL
    gmax = max(float(v.grad.abs().max()) for v in params.values() if v.grad is not None)
    worst, wname = 0.0, ""
    for name, p in edm.unet.named_parameters():
        if p.requires_grad:
            r = params["unet." + name].grad
            e = grad_err(p.grad, r, gmax, name)
            if e > worst:
                worst, wname = e, name
    print(f"latent step: loss {float(loss.detach()):.6f}; worst gradient rel err {worst:.2e} at {wname}")
    assert worst < TOL
    stem_err = rel_err(edm.unet.input_blocks[0][0].weight.grad.cpu(), params["unet.input_blocks.0.0.weight"].grad)
    assert stem_err < TOL, stem_err


def test_length_not_divisible_by_downsampling_raises_like_the_reference():
    """T = 252 through two stride-2 levels: 252 -> 126 -> 63 -> up 126 ok; T = 250: 250 -> 125 -> 63 -> up 126 != 125"""
    from tqdne_amd import UNetModel
    sd, d = load_golden("micro_unet.npz")
    net = UNetModel(**cfg_of(d))
    net.load_state_dict(sd)
    net = net.to(dev()).eval()
    x = torch.randn(1, 3, 250, device=dev())
    with pytest.raises(RuntimeError, match="must match"):
        net(x, torch.zeros(1, device=dev()), torch.zeros(1, 5, device=dev()))


def test_sampler_does_not_retain_start_state():
    """repeated LightningEDM.sample calls (2 lanes at B = 32) with the cyclic collector switched off: the integration objects must
    not keep the start state / conditioning alive through reference cycles (device memory would grow by one state per call)"""
    import gc
    from tqdne_amd import LightningEDM, tiny_1d_unet_config
    torch.manual_seed(0)
    cfg = tiny_1d_unet_config()
    edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}, num_sampling_steps=3)
    edm = edm.to(dev()).eval()
    cond = torch.randn(32, cfg["cond_features"], device=dev()) if cfg["cond_features"] else None
    gc.collect()
    gc.disable()
    try:
        used = []
        for _ in range(4):
            x = edm.sample((32, 3, 1024), cond=cond)
            torch.cuda.synchronize()
            used.append(torch.cuda.memory_allocated())
        assert torch.isfinite(x).all()
        # (a 512-byte schedule tensor per call may wait for the collector; a start state is 786 KB)
        assert used[-1] - used[1] < 100_000, used
    finally:
        gc.enable()


def test_conv_scheme_bf16x3_moves_the_data_gradients_too(monkeypatch):
    """TQDNE_CONV_SCHEME=bf16x3 is the documented fp32-range switch: forward convs AND data gradients must then run the three-product
    scheme (round-4 advisor finding: the data gradients kept fp16-packed weights).  The default leaves f16+mx6 data gradients on."""
    from tqdne_amd import LightningEDM, _lib, paper_1d_unet_config
    cfg = dict(paper_1d_unet_config(), dropout=0.0)   # (has 128 | C_in layers: the mx6 data gradient is eligible)
    g = torch.Generator().manual_seed(5)
    B, T = 2, 512
    sig, cond = 0.5 * torch.randn(B, 3, T, generator=g), torch.randn(B, 5, generator=g)
    eps, noise = torch.randn(B, generator=g), torch.randn(B, 3, T, generator=g)
    grads = {}
    for scheme in ("f16mx6", "bf16x3"):
        monkeypatch.setenv("TQDNE_CONV_SCHEME", scheme)
        torch.manual_seed(0)
        edm = LightningEDM(cfg, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0})
        edm.unet.load_state_dict(perturbed_state(edm.unet, 3))
        edm = edm.to(dev()).train()
        loss = edm.step_with_noise(sig.to(dev()), eps.to(dev()), noise.to(dev()), cond=cond.to(dev()) if cfg["cond_features"] else None)
        loss.backward()
        eng = edm.unet._engine(B, T, dev())
        wf = [d.wfmt for d in eng._bwd.dgrad_descs]
        assert wf, "no data-gradient descriptors recorded"
        if scheme == "bf16x3":
            assert all(w == _lib.TQ_WFMT_BF16X3 for w in wf), wf
            assert all(d.wfmt == _lib.TQ_WFMT_BF16X3 for d, _s, _p in eng._wfmt_sites)
        else:
            assert any(w == _lib.TQ_WFMT_F16_MX6 for w in wf), wf
        grads[scheme] = {n: p.grad.detach().cpu().clone() for n, p in edm.unet.named_parameters() if p.grad is not None}
    # per tensor, the suite's gradient metric (against the tensor's own scale, floored at 1e-3 of the largest gradient): the two schemes
    # differ by their rounding (2^-15 vs 2^-16 per product) only
    gmax = max(float(v.abs().max()) for v in grads["bf16x3"].values())
    worst = max(grad_err(grads["f16mx6"][n], grads["bf16x3"][n], gmax, n) for n in grads["bf16x3"])
    flat = lambda d: torch.cat([v.reshape(-1) for v in d.values()])
    assert worst < TOL and rel_err(flat(grads["f16mx6"]), flat(grads["bf16x3"]), elem=False) < 1e-4


def test_attention_backward_reuses_the_training_forwards_kv_planes():
    """Round 5: once a backward plan exists, every attention block's training forward keeps its K / V planes in a workspace of its own
    and the backward's prep pass forms Q, dO and delta only (tq_attention_bwd_ws_kv).  The first sweep of a plan still re-derives the
    planes (its forward ran before the plan existed): same inputs, same gradients on both routes."""
    from tqdne_amd import LightningEDM
    sd, d = load_golden("micro_unet.npz")
    cfg = dict(cfg_of(d), dropout=0.0)
    edm = LightningEDM(cfg, {"learning_rate": 1e-3, "max_steps": 10, "eta_min": 0.0})
    edm.unet.load_state_dict(sd)
    edm = edm.to(dev()).train()
    g = torch.Generator().manual_seed(21)
    B, T = 3, 256
    sig, cond = (0.5 * torch.randn(B, 3, T, generator=g)).to(dev()), torch.randn(B, 5, generator=g).to(dev())
    eps, noise = torch.randn(B, generator=g).to(dev()), torch.randn(B, 3, T, generator=g).to(dev())
    runs = []
    for _ in range(3):
        for p in edm.unet.parameters():
            p.grad = None
        loss = edm.step_with_noise(sig, eps, noise, cond=cond)
        loss.backward()
        eng = edm.unet._engine(B, T, dev())
        runs.append((eng._last["block_kv"], float(loss), torch.cat([p.grad.reshape(-1) for p in edm.unet.parameters() if p.grad is not None]).clone()))
    assert [r[0] for r in runs] == [False, True, True]
    assert any(t[0] == "attn" and "kv_ws" in t[1] for t in eng.tape)
    # (column sums and GroupNorm-backward sums use atomics: two sweeps agree to rounding, not to the bit -- the two routes must agree as
    # closely as two sweeps of the same route do)
    same_route = rel_err(runs[2][2].cpu(), runs[1][2].cpu())
    two_routes = rel_err(runs[1][2].cpu(), runs[0][2].cpu())
    print(f"attention backward: planes re-derived vs re-used {two_routes:.2e}; re-used twice {same_route:.2e}")
    assert abs(runs[0][1] - runs[1][1]) < 1e-6 * abs(runs[0][1]) and two_routes < 2e-6 and same_route < 2e-6
    # an inference forward in between uses the shared workspace and leaves the kept planes alone
    edm.eval()
    with torch.no_grad():
        edm(sig, torch.full((B,), 0.7, device=dev()), None, cond)
    edm.train()
    for p in edm.unet.parameters():
        p.grad = None
    loss = edm.step_with_noise(sig, eps, noise, cond=cond)
    loss.backward()
    assert rel_err(torch.cat([p.grad.reshape(-1) for p in edm.unet.parameters() if p.grad is not None]).cpu(), runs[0][2].cpu()) < 2e-6


@pytest.mark.parametrize("which,B,T", [("micro", 3, 256), ("paper", 2, 1024)])
def test_use_checkpoint_recomputes_block_activations_same_gradients_less_memory(which, B, T):
    """``use_checkpoint=True`` (reference unet.py:202,129; blocks.py:137; nn.py:137-215: block-internal activations are recomputed in the
    backward instead of kept): here the activations inside a ResBlock (conv1's output and its statistics) and inside an AttentionBlock
    (qkv, the attention output, the log-sum-exp, the K / V planes) live in buffers shared by all blocks of a shape, and the backward plan
    re-issues the block's forward launches first.  Same loss, same gradients (to the rounding of the atomics-summed column sums), fewer
    bytes held by the plans; and the forward's result does not depend on the flag."""
    from tqdne_amd import LightningEDM, paper_1d_unet_config
    if which == "micro":
        sd, d = load_golden("micro_unet.npz")
        cfg = dict(cfg_of(d), dropout=0.1)
    else:
        cfg = dict(paper_1d_unet_config(), dropout=0.1)
        torch.manual_seed(0)
        sd = perturbed_state(LightningEDM(cfg, {"learning_rate": 1e-3, "max_steps": 10, "eta_min": 0.0}).unet, 9)
    g = torch.Generator().manual_seed(31)
    sig, cond = (0.5 * torch.randn(B, 3, T, generator=g)).to(dev()), torch.randn(B, 5, generator=g).to(dev())
    eps, noise = torch.randn(B, generator=g).to(dev()), torch.randn(B, 3, T, generator=g).to(dev())
    from tqdne_amd import rng
    res = {}
    import gc
    for ck in (False, True):
        gc.collect()   # (plans sit in reference cycles: the previous run's buffers must be gone before the baseline is read)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        edm = LightningEDM(dict(cfg, use_checkpoint=ck), {"learning_rate": 1e-3, "max_steps": 10, "eta_min": 0.0})
        edm.unet.load_state_dict(sd)
        edm = edm.to(dev()).train()
        steps = []
        for _ in range(2):   # (the second step runs on the kept / recomputed K / V planes)
            rng.seed_rank(77, 0)   # same dropout masks in every run
            for p in edm.unet.parameters():
                p.grad = None
            loss = edm.step_with_noise(sig, eps, noise, cond=cond)
            loss.backward()
            steps.append((float(loss), torch.cat([p.grad.reshape(-1) for p in edm.unet.parameters() if p.grad is not None]).clone()))
        torch.cuda.synchronize()
        eng = edm.unet._engine(B, T, dev())
        assert eng.ckpt == ck
        nrec = sum(op[2].startswith("recompute:") for op in eng._bwd.ops)
        n_res = sum(t[0] == "res" for t in eng.tape)
        n_att = sum(t[0] == "attn" for t in eng.tape)
        assert nrec == (2 * n_res + 2 * n_att if ck else 0)
        # block-internal activations of the plan: every block's own tensor (plain) / the shared ones (checkpointing)
        inner = [t[1][k].buf for t in eng.tape for k in (("h1",) if t[0] == "res" else ("qkv", "att") if t[0] == "attn" else ())]
        gc.collect()
        res[ck] = dict(steps=[(l, gr.cpu()) for l, gr in steps], mem=torch.cuda.memory_allocated() - base, inner=sum(b.numel() * 4 for b in inner),
                       inner_unique=sum(b.numel() * 4 for b in {b.data_ptr(): b for b in inner}.values()))
        del edm, eng, inner, loss, steps
    for s in (0, 1):
        assert abs(res[True]["steps"][s][0] - res[False]["steps"][s][0]) < 1e-6 * abs(res[False]["steps"][s][0])
        e = rel_err(res[True]["steps"][s][1], res[False]["steps"][s][1])
        assert e < 2e-6, (s, e)
    assert res[False]["inner_unique"] == res[False]["inner"] and res[True]["inner"] == res[False]["inner"]
    saved_expect = res[False]["inner"] - res[True]["inner_unique"]
    saved = res[False]["mem"] - res[True]["mem"]
    print(f"use_checkpoint ({which}, B={B}, T={T}): plan memory {res[False]['mem'] / 2**20:.1f} -> {res[True]['mem'] / 2**20:.1f} MiB; block-internal "
          f"activations {res[False]['inner'] / 2**20:.1f} -> {res[True]['inner_unique'] / 2**20:.1f} MiB (weights, packed fragments and gradients unchanged)")
    assert saved_expect > 0.5 * res[False]["inner"] and saved >= 0.8 * saved_expect
