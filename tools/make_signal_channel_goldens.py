#!/usr/bin/env python3
"""Generate tests/golden/signal_channels.npz by running the *reference itself* (imported, never copied; CPU only).

Run:  python tools/make_signal_channel_goldens.py       (same requirements as tools/make_goldens.py)

  signal_channels.npz   the 16 + 16 -> 16 micro model of the signal-conditioned latent EDM (edm.py:105-113 with
                        LatentMovingAverageEnvelopeConfig.latent_channels = 16: the UNet's input conv sees 32 channels):
                        UNetModel.forward on a 32-channel input, and LightningEDM.forward(sample, sigma, cond_sample, cond) with a
                        16-channel sample and a 16-channel conditioning signal, at B = 2, T = 200.

As in tools/make_head_size_goldens.py the weights are rounded to fp16-representable values BEFORE the reference runs and stored as
float16 (the stored value is exactly the value the reference saw); so are the three signal-shaped inputs, which keeps the file under
the size limit for a committed file.  The small inputs and the outputs are stored as float32.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import OUT, REF, install_lightning_standin, perturb_  # noqa: E402

SIGNAL_UNET = dict(
    in_channels=32, out_channels=16, model_channels=32, channel_mult=(1, 2), num_res_blocks=1,
    attention_resolutions=(2,), num_heads=4, conv_kernel_size=5, dims=1, cond_features=5,
    dropout=0.0, flash_attention=False,
)
B, T = 2, 200
SEED_WEIGHTS, SEED_INPUTS = 171, 1716
SIGMAS = (0.4, 11.0)


def fp16_exact(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(torch.float32)


def main():
    sys.path.insert(0, REF)
    install_lightning_standin()
    torch.set_num_threads(8)
    from tqdne.edm import LightningEDM
    from tqdne.unet import UNetModel

    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    net = UNetModel(**SIGNAL_UNET).eval()
    perturb_(net, SEED_WEIGHTS)
    with torch.no_grad():
        for v in net.state_dict().values():   # (parameters and buffers: the tensors share the module's storage)
            v.copy_(fp16_exact(v))
    fx = {"w:" + k: v.detach().numpy().astype(np.float16) for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(SEED_INPUTS)
    x = fp16_exact(torch.randn(B, 32, T, generator=g))
    t = torch.randn(B, generator=g) * 0.5
    c = torch.randn(B, 5, generator=g)
    sample = fp16_exact(0.5 * torch.randn(B, 16, T, generator=g))
    cond_sample = fp16_exact(torch.randn(B, 16, T, generator=g))
    sigma = torch.tensor(SIGMAS)
    edm = LightningEDM(SIGNAL_UNET, {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}).eval()
    edm.unet.load_state_dict(net.state_dict())
    with torch.no_grad():
        y = net(x, t, c)
        d = edm(sample, sigma, cond_sample, c)
    fx.update({"unet:x": x.numpy().astype(np.float16), "unet:t": t.numpy(), "cond": c.numpy(), "unet:y": y.numpy(),
               "edm:sample": sample.numpy().astype(np.float16), "edm:cond_sample": cond_sample.numpy().astype(np.float16), "edm:sigma": sigma.numpy(), "edm:y": d.numpy(),
               "seeds": np.array([SEED_WEIGHTS, SEED_INPUTS], dtype=np.int64), "cfg": np.array(repr(SIGNAL_UNET))})
    path = os.path.join(OUT, "signal_channels.npz")
    np.savez_compressed(path, **fx)
    print("signal_channels.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
