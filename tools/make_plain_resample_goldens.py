#!/usr/bin/env python3
"""Generate tests/golden/plain_resample.npz by running the *reference itself* (imported, never copied; CPU only): models built with
``conv_resample=False`` (Downsample = mean of every pair of positions, Upsample = nearest x2, no resampling convs) and with
``cond_emb_scale`` (a Fourier projection of the single conditioning feature in front of cond_mlp).

Run:  python tools/make_plain_resample_goldens.py       (same requirements as tools/make_goldens.py)

  unet   1-D micro UNet, conv_resample=False, B = 2: key list and shapes; forward at T = 200 and T = 136; d sum(y) / d x at T = 200; the EDM
         loss and its parameter gradients at injected draws (T = 200)
  ae     Encoder / Decoder with channel_mult (1, 2, 2), conv_resample=False: encoder forward at T = 202 (floors twice: 202 -> 101 -> 50) and
         T = 200, decoder forward, the training-step loss and its parameter gradients at T = 200 (injected draw)
  cf     the unet config with cond_features 1, cond_emb_scale 0.5 and learned resampling: forward, EDM loss and gradients at T = 200, and
         the fingerprints of the reference's freshly initialised state under a fixed seed
  2d     dims=2 micro UNets with conv_resample=False (and one with cond_emb_scale as well): forward on (2, 1, 16, 16)

What the file does NOT hold, and why.  No committed file may exceed 1 MiB, and the three 1-D models have ~0.8 M parameters each:
  * weights are not stored.  Both sides build them with ``recipe_state`` below -- a function of the tensors' names and shapes and of a
    seed, every value rounded to an fp16-representable one -- and the file holds one sha256 per tensor, so a test that rebuilt other
    weights than the reference saw fails at the fingerprint, not at the comparison;
  * gradients are stored for EVERY parameter, but of a tensor with more than GRAD_SAMPLE entries only the entries ``sample_index``
    names (evenly spaced over the flattened tensor), next to the largest |gradient| of the whole model (``gmax``: grad_err's floor).
Signal-shaped inputs are rounded to fp16-representable values and stored as float16; everything else is float32.
"""

from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import OUT, REF, install_lightning_standin  # noqa: E402

UNET = dict(in_channels=3, out_channels=3, model_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, attention_resolutions=(2,),
            num_heads=4, conv_kernel_size=5, dims=1, cond_features=5, dropout=0.0, conv_resample=False, flash_attention=False)
UNET_CF = dict(UNET, cond_features=1, cond_emb_scale=0.5, conv_resample=True)
AE = dict(model_channels=32, channel_mult=(1, 2, 2), attention_resolutions=(), num_res_blocks=1, dims=1, conv_kernel_size=5, dropout=0.0,
          conv_resample=False)
ENC, DEC = dict(AE, in_channels=3, out_channels=8), dict(AE, in_channels=4, out_channels=3)
UNET_2D = dict(in_channels=1, out_channels=1, model_channels=32, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(2,),
               num_heads=2, conv_kernel_size=3, dims=2, cond_features=5, dropout=0.0, conv_resample=False, flash_attention=False)
UNET_2D_CF = dict(UNET_2D, cond_features=1, cond_emb_scale=0.5)
OPT = {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}
KL_WEIGHT = 1e-2
B = 2
SEEDS = dict(unet=401, ae=402, cf=403, d2=404, d2cf=405, inputs=4100, init=5)
GRAD_SAMPLE = 512


def fp16_exact(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(torch.float32)


def tensor_fingerprint(t: torch.Tensor) -> str:
    t = t.detach().cpu().contiguous()
    h = hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode())
    h.update(t.numpy().tobytes())
    return h.hexdigest()


def recipe_state(module: torch.nn.Module, seed: int) -> dict:
    """A state_dict for ``module`` drawn from a CPU generator: a function of the tensors' names, shapes and order and of ``seed`` alone (not
    of the module's own initialisation), every value fp16-representable.  Fourier frequencies keep their scale (0.02, or the model's
    cond_emb_scale), GroupNorm affines are 1 + 0.1 n / 0.1 n, biases 0.1 n, weights n / sqrt(fan_in) -- none of them zero, so the
    zero-initialised convs of a fresh model pin something."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in module.state_dict().items():
        n = torch.randn(v.shape, generator=g)
        if k.endswith("time_embed.W"):
            n = 0.02 * n
        elif k.endswith("cond_embed.W"):
            n = 0.5 * n
        elif v.ndim == 1 and k.endswith("weight"):
            n = 1.0 + 0.1 * n
        elif v.ndim == 1:
            n = 0.1 * n
        else:
            n = n / float(np.sqrt(np.prod(v.shape[1:])))
        sd[k] = fp16_exact(n)
    return sd


def sample_index(numel: int) -> torch.Tensor:
    """the entries of a flattened gradient that the fixture keeps: all of a small tensor, GRAD_SAMPLE evenly spaced ones of a large one"""
    if numel <= GRAD_SAMPLE:
        return torch.arange(numel)
    return torch.arange(GRAD_SAMPLE) * numel // GRAD_SAMPLE


def describe(fx: dict, tag: str, sd: dict):
    keys = list(sd)
    fx[tag + ":keys"] = np.array(keys)
    fx[tag + ":shapes"] = np.array([" ".join(str(int(s)) for s in sd[k].shape) for k in keys])
    fx[tag + ":sha256"] = np.array([tensor_fingerprint(sd[k]) for k in keys])


def record_grads(fx: dict, tag: str, module: torch.nn.Module):
    gmax = 0.0
    for n, p in module.named_parameters():
        if p.grad is None:
            continue
        flat = p.grad.detach().reshape(-1)
        gmax = max(gmax, float(flat.abs().max()))
        fx[f"{tag}:g:{n}"] = flat[sample_index(flat.numel())].numpy().copy()
    fx[tag + ":gmax"] = np.array(gmax, dtype=np.float64)


def edm_step(fx: dict, tag: str, LightningEDM, cfg: dict, sd: dict, sig, cond, seed: int):
    """LightningEDM.step (edm.py:115-134) with its two draws replicated by re-seeding the global generator, as tools/make_goldens.py does"""
    edm = LightningEDM(cfg, OPT).eval()
    edm.unet.load_state_dict(sd)
    torch.manual_seed(seed)
    eps = torch.randn(B)
    noise = torch.randn_like(sig)
    torch.manual_seed(seed)
    loss = edm.step({"signal": sig, "cond": cond}, 0)
    loss.backward()
    fx.update({tag + ":signal": sig.numpy().astype(np.float16), tag + ":eps": eps.numpy(), tag + ":noise": noise.numpy(),
               tag + ":loss": loss.detach().numpy()})
    record_grads(fx, tag, edm.unet)


def main():
    sys.path.insert(0, REF)
    install_lightning_standin()
    torch.set_num_threads(8)
    from tqdne.autoencoder import LightningAutoencoder
    from tqdne.edm import LightningEDM
    from tqdne.unet import UNetModel

    os.makedirs(OUT, exist_ok=True)
    fx = {}
    g = torch.Generator().manual_seed(SEEDS["inputs"])

    # ---------------------------------------------------------------- unet: conv_resample=False
    net = UNetModel(**UNET).eval()
    sd = recipe_state(net, SEEDS["unet"])
    net.load_state_dict(sd)
    describe(fx, "unet", sd)
    t = torch.randn(B, generator=g) * 0.5
    c = torch.randn(B, 5, generator=g)
    fx.update({"unet:t": t.numpy(), "unet:cond": c.numpy()})
    for T in (200, 136):
        x = fp16_exact(torch.randn(B, 3, T, generator=g))
        with torch.no_grad():
            y = net(x, t, c)
        fx.update({f"unet:x{T}": x.numpy().astype(np.float16), f"unet:y{T}": y.numpy()})
        if T == 200:
            xg = x.clone().requires_grad_()
            net(xg, t, c).sum().backward()
            fx["unet:dx200"] = xg.grad.numpy().copy()
            net.zero_grad()
    sig = fp16_exact(0.5 * torch.randn(B, 3, 200, generator=g))
    edm_step(fx, "unet:edm", LightningEDM, UNET, sd, sig, c, 4242)

    # ---------------------------------------------------------------- ae: conv_resample=False coders
    ae = LightningAutoencoder(ENC, DEC, OPT, kl_weight=KL_WEIGHT).eval()
    sd = recipe_state(ae, SEEDS["ae"])
    ae.load_state_dict(sd)
    describe(fx, "ae", sd)
    for T in (202, 200):
        x = fp16_exact(0.5 * torch.randn(B, 3, T, generator=g))
        with torch.no_grad():
            e = ae.encoder(x)
        fx.update({f"ae:x{T}": x.numpy().astype(np.float16), f"ae:enc{T}": e.numpy()})
    z = fp16_exact(torch.randn(B, 4, 50, generator=g))
    with torch.no_grad():
        r = ae.decoder(z)
    fx.update({"ae:z": z.numpy().astype(np.float16), "ae:dec": r.numpy()})
    draw = torch.randn(B, 4, 50, generator=g)
    orig = torch.randn_like
    torch.randn_like = lambda t_, **k: draw   # the draw of _encode (autoencoder.py:39)
    try:
        loss = ae.training_step({"signal": x}, 0)
    finally:
        torch.randn_like = orig
    loss.backward()
    fx.update({"ae:step:eps": draw.numpy(), "ae:step:loss": loss.detach().numpy(), "ae:kl_weight": np.array(KL_WEIGHT)})
    record_grads(fx, "ae:step", ae)

    # ---------------------------------------------------------------- cf: cond_emb_scale
    torch.manual_seed(SEEDS["init"])
    fresh = UNetModel(**UNET_CF).state_dict()
    fx["cf:init:keys"] = np.array(list(fresh))
    fx["cf:init:sha256"] = np.array([tensor_fingerprint(v) for v in fresh.values()])
    fx["cf:init:seed"] = np.array(SEEDS["init"])
    net = UNetModel(**UNET_CF).eval()
    sd = recipe_state(net, SEEDS["cf"])
    net.load_state_dict(sd)
    describe(fx, "cf", sd)
    c1 = torch.randn(B, 1, generator=g)
    x = fp16_exact(torch.randn(B, 3, 200, generator=g))
    with torch.no_grad():
        y = net(x, t, c1)
    fx.update({"cf:cond": c1.numpy(), "cf:x200": x.numpy().astype(np.float16), "cf:y200": y.numpy()})
    edm_step(fx, "cf:edm", LightningEDM, UNET_CF, sd, sig, c1, 4243)

    # ---------------------------------------------------------------- 2d
    x2 = fp16_exact(torch.randn(B, 1, 16, 16, generator=g))
    fx["2d:x"] = x2.numpy().astype(np.float16)
    for tag, cfg, cond, seed in (("2d", UNET_2D, c, SEEDS["d2"]), ("2dcf", UNET_2D_CF, c1, SEEDS["d2cf"])):
        net = UNetModel(**cfg).eval()
        sd = recipe_state(net, seed)
        net.load_state_dict(sd)
        describe(fx, tag, sd)
        with torch.no_grad():
            fx[tag + ":y"] = net(x2, t, cond).numpy()

    for name, cfg in (("unet", UNET), ("cf", UNET_CF), ("enc", ENC), ("dec", DEC), ("2d", UNET_2D), ("2dcf", UNET_2D_CF)):
        fx["cfg:" + name] = np.array(repr(cfg))
    fx["seeds"] = np.array(repr(SEEDS))
    path = os.path.join(OUT, "plain_resample.npz")
    np.savez_compressed(path, **fx)
    print("plain_resample.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
