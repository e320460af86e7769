#!/usr/bin/env python3
"""Generate the head-size fixtures under tests/golden/ by running the *reference itself* (imported, never copied; CPU only).

Run:  python tools/make_head_size_goldens.py       (same requirements as tools/make_goldens.py)

  head_size_ops.npz    QKVAttention(H) (blocks.py:148-190) on four small cases with head sizes 16, 48, 96 and 256: its output, and the
                       qkv gradient its autograd gives for a stored ``dout``.
  head_size_unet.npz   UNetModel.forward of a micro UNet whose attention runs at head size 8 (32 channels over 4 heads) and head
                       size 16 (64 channels, middle block included), at T = 200 and the ragged T = 196.

No committed file may pass 1 MiB, so everything that is an INPUT of the reference here -- qkv, dout, and the UNet's weights after the
``perturb_`` recipe of tools/make_goldens.py -- is rounded to fp16-representable values BEFORE the reference runs and stored as
float16: the stored value is exactly the value the reference saw.  Outputs are stored as the float32 the reference produced.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import OUT, REF, install_lightning_standin, perturb_  # noqa: E402

OPS_CASES = [(4, 16, 70), (2, 48, 66), (1, 96, 70), (1, 256, 66)]   # (heads, head size, T), B = 1
HEAD_UNET = dict(
    in_channels=3, out_channels=3, model_channels=32, channel_mult=(1, 2), num_res_blocks=1,
    attention_resolutions=(1, 2), num_heads=4, conv_kernel_size=5, dims=1, cond_features=5,
    dropout=0.0, flash_attention=False,
)
UNET_LENGTHS = (200, 196)


def fp16_exact(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(torch.float32)


def main():
    sys.path.insert(0, REF)
    install_lightning_standin()
    torch.set_num_threads(8)
    from tqdne.blocks import QKVAttention
    from tqdne.unet import UNetModel

    os.makedirs(OUT, exist_ok=True)
    g = torch.Generator().manual_seed(4321)

    fx = {}
    for H, D, T in OPS_CASES:
        qkv = fp16_exact(torch.randn(1, 3 * H * D, T, generator=g) * 1.2).requires_grad_(True)
        dout = fp16_exact(torch.randn(1, H * D, T, generator=g))
        out = QKVAttention(H)(qkv)
        out.backward(dout)
        key = f"H{H}:D{D}:T{T}"
        fx.update({key + ":qkv": qkv.detach().numpy().astype(np.float16), key + ":dout": dout.numpy().astype(np.float16),
                   key + ":out": out.detach().numpy(), key + ":dqkv": qkv.grad.numpy()})
    fx["cases"] = np.array(OPS_CASES, dtype=np.int32)
    np.savez_compressed(os.path.join(OUT, "head_size_ops.npz"), **fx)

    torch.manual_seed(0)
    net = UNetModel(**HEAD_UNET).eval()
    perturb_(net, 99)
    with torch.no_grad():
        for v in net.state_dict().values():   # (parameters and buffers: the tensors share the module's storage)
            v.copy_(fp16_exact(v))
    fx = {"w:" + k: v.detach().numpy().astype(np.float16) for k, v in net.state_dict().items()}
    for T in UNET_LENGTHS:
        x = torch.randn(2, 3, T, generator=g)
        t = torch.randn(2, generator=g) * 0.5
        c = torch.randn(2, 5, generator=g)
        with torch.no_grad():
            y = net(x, t, c)
        fx.update({f"T{T}:x": x.numpy(), f"T{T}:t": t.numpy(), f"T{T}:cond": c.numpy(), f"T{T}:y": y.numpy()})
    fx["cfg"] = np.array(repr(HEAD_UNET))
    np.savez_compressed(os.path.join(OUT, "head_size_unet.npz"), **fx)
    for name in ("head_size_ops.npz", "head_size_unet.npz"):
        print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")


if __name__ == "__main__":
    main()
