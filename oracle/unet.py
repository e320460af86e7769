"""Functional CPU restatement of the reference UNet (test infrastructure only).

Everything here is a pure function of ``(state_dict, config, inputs)``; the
state-dict keys are the reference's own, so a checkpoint of the
reference, or ``tqdne_amd.UNetModel(...).state_dict()``, can be fed in directly.

Reference lines restated (all under /root/reference/tqdne/):
  * UNetModel.__init__ / forward ............ unet.py:188-398
  * ResBlock (time-conditioned) ............. unet.py:42-143
  * AttentionBlock / QKVAttention ........... blocks.py:111-190
  * Upsample / Downsample ................... blocks.py:29-108
  * GaussianFourierProjection ............... blocks.py:15-26
  * GroupNorm32 (32 groups, eps 1e-5) ....... nn.py:11-13, 90-105
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
SD = Dict[str, Tensor]

GN_GROUPS = 32
GN_EPS = 1e-5

UNET_DEFAULTS = dict(
    attention_resolutions=(8, 16, 32),
    dropout=0,
    channel_mult=(1, 2, 4, 8),
    conv_kernel_size=3,
    conv_resample=True,
    dims=2,
    cond_features=None,
    cond_emb_scale=None,
    use_checkpoint=False,
    num_heads=1,
    use_scale_shift_norm=False,
    flash_attention=True,
    use_causal_mask=False,
)


def full_config(cfg: dict) -> dict:
    """Fill in the reference's constructor defaults (unet.py:188-207)."""
    out = dict(UNET_DEFAULTS)
    out.update(cfg)
    if out["dims"] != 1:
        raise NotImplementedError("oracle covers the 1-D hot path only (dims=1)")
    if out["use_scale_shift_norm"]:
        raise NotImplementedError("use_scale_shift_norm is unused by every reference config")
    if out["cond_emb_scale"] is not None:
        raise NotImplementedError("cond_emb_scale is unused by every reference config")
    if not out["conv_resample"]:
        raise NotImplementedError("conv_resample=False is unused by every reference config")
    return out


# --------------------------------------------------------------------------
# structure: which blocks exist, in which order, with which channel counts
# --------------------------------------------------------------------------
def unet_layout(cfg: dict):
    """Enumerate the blocks of the UNet exactly as unet.py:229-358 builds them.

    Returns (input_blocks, middle, output_blocks, final_ch) where each block is
    a list of layer tuples:
      ("stem", prefix, cin, cout) | ("res", prefix, cin, cout) |
      ("attn", prefix, ch) | ("down", prefix, ch) | ("up", prefix, ch)
    """
    cfg = full_config(cfg)
    mc = cfg["model_channels"]
    mult = cfg["channel_mult"]
    nres = cfg["num_res_blocks"]
    att = tuple(cfg["attention_resolutions"])

    ch = int(mult[0] * mc)
    inputs = [[("stem", "input_blocks.0.0", cfg["in_channels"], ch)]]
    skip_chans = [ch]
    ds = 1
    for level, m in enumerate(mult):
        for _ in range(nres):
            i = len(inputs)
            cout = int(m * mc)
            layers = [("res", f"input_blocks.{i}.0", ch, cout)]
            ch = cout
            if ds in att:
                layers.append(("attn", f"input_blocks.{i}.1", ch))
            inputs.append(layers)
            skip_chans.append(ch)
        if level != len(mult) - 1:
            i = len(inputs)
            inputs.append([("down", f"input_blocks.{i}.0", ch)])
            skip_chans.append(ch)
            ds *= 2

    middle = [
        ("res", "middle_block.0", ch, ch),
        ("attn", "middle_block.1", ch),
        ("res", "middle_block.2", ch, ch),
    ]

    outputs = []
    for level, m in list(enumerate(mult))[::-1]:
        for j in range(nres + 1):
            i = len(outputs)
            ich = skip_chans.pop()
            cout = int(mc * m)
            layers = [("res", f"output_blocks.{i}.0", ch + ich, cout)]
            ch = cout
            if ds in att:
                layers.append(("attn", f"output_blocks.{i}.{len(layers)}", ch))
            if level and j == nres:
                layers.append(("up", f"output_blocks.{i}.{len(layers)}", ch))
                ds //= 2
            outputs.append(layers)
    return inputs, middle, outputs, ch


# --------------------------------------------------------------------------
# leaf ops
# --------------------------------------------------------------------------
def group_norm32(sd: SD, p: str, x: Tensor) -> Tensor:
    # nn.py:11-13 -- computed on x.float(), cast back (a float64 run of the oracle, the high-precision reference of some tests, stays in
    # float64: the up-cast is there for half-precision activations)
    xf = x if x.dtype == torch.float64 else x.float()
    return F.group_norm(xf, GN_GROUPS, sd[p + ".weight"], sd[p + ".bias"], GN_EPS).type(x.dtype)


def conv_same(sd: SD, p: str, x: Tensor) -> Tensor:
    w = sd[p + ".weight"]
    k = w.shape[-1]
    assert k % 2 == 1
    return F.conv1d(x, w, sd[p + ".bias"], padding=k // 2)


def linear(sd: SD, p: str, x: Tensor) -> Tensor:
    return F.linear(x, sd[p + ".weight"], sd[p + ".bias"])


def fourier_features(W: Tensor, t: Tensor) -> Tensor:
    # blocks.py:22-26
    h = t[:, None] * W[None, :] * 2 * torch.pi
    return torch.cat([torch.sin(h), torch.cos(h)], dim=-1)


def res_block(
    sd: SD,
    p: str,
    x: Tensor,
    emb: Optional[Tensor],
    dropout_mask: Optional[Tensor] = None,
) -> Tensor:
    """unet.py:131-143 (emb given) and blocks.py:233-260 (emb None).

    ``dropout_mask``: optional tensor already scaled by 1/(1-p) (keep -> 1/(1-p),
    drop -> 0) applied where the reference applies nn.Dropout; None = eval mode.
    """
    h = conv_same(sd, p + ".in_layers.2", F.silu(group_norm32(sd, p + ".in_layers.0", x)))
    if emb is not None:
        e = linear(sd, p + ".emb_layers.1", F.silu(emb)).type(h.dtype)
        h = h + e[:, :, None]
    h = F.silu(group_norm32(sd, p + ".out_layers.0", h))
    if dropout_mask is not None:
        h = h * dropout_mask
    h = conv_same(sd, p + ".out_layers.3", h)
    if (p + ".skip_connection.weight") in sd:
        w = sd[p + ".skip_connection.weight"]
        x = F.conv1d(x, w, sd[p + ".skip_connection.bias"], padding=w.shape[-1] // 2)
    return x + h


def qkv_attention(qkv: Tensor, n_heads: int) -> Tensor:
    # blocks.py:156-190, no causal mask (use_causal_mask=False in every 1-D config)
    bs, width, length = qkv.shape
    assert width % (3 * n_heads) == 0
    ch = width // (3 * n_heads)
    q, k, v = qkv.chunk(3, dim=1)
    scale = 1 / math.sqrt(math.sqrt(ch))
    w = torch.einsum(
        "bct,bcs->bts",
        (q * scale).reshape(bs * n_heads, ch, length),
        (k * scale).reshape(bs * n_heads, ch, length),
    )
    w = torch.softmax(w.float(), dim=-1).type(w.dtype)
    a = torch.einsum("bts,bcs->bct", w, v.reshape(bs * n_heads, ch, length))
    return a.reshape(bs, -1, length)


def attention_block(sd: SD, p: str, x: Tensor, n_heads: int) -> Tensor:
    # blocks.py:139-145
    qkv = F.conv1d(group_norm32(sd, p + ".norm", x), sd[p + ".qkv.weight"], sd[p + ".qkv.bias"])
    h = qkv_attention(qkv, n_heads)
    h = F.conv1d(h, sd[p + ".proj_out.weight"], sd[p + ".proj_out.bias"])
    return x + h


def downsample(sd: SD, p: str, x: Tensor) -> Tensor:
    # blocks.py:92-101: conv stride 2, padding k//2 (k=3 inside the UNet, unet.py:273)
    w = sd[p + ".op.weight"]
    return F.conv1d(x, w, sd[p + ".op.bias"], stride=2, padding=w.shape[-1] // 2)


def upsample(sd: SD, p: str, x: Tensor) -> Tensor:
    # blocks.py:58-66: nearest x2 then "same" conv
    x = F.interpolate(x, scale_factor=2, mode="nearest")
    return conv_same(sd, p + ".conv", x)


# --------------------------------------------------------------------------
# embedding + whole network
# --------------------------------------------------------------------------
def embedding(sd: SD, cfg: dict, timesteps: Tensor, cond: Optional[Tensor], prefix: str = "") -> Tensor:
    # unet.py:383-388
    cfg = full_config(cfg)
    assert (cond is not None) == (cfg["cond_features"] is not None), (
        "must specify cond if and only if the model is conditioned"
    )
    P = prefix
    e = fourier_features(sd[P + "time_embed.W"], timesteps)
    e = linear(sd, P + "time_mlp.2", F.silu(linear(sd, P + "time_mlp.0", e)))
    if cond is not None:
        e = e + linear(sd, P + "cond_mlp.2", F.silu(linear(sd, P + "cond_mlp.0", cond)))
    return e


def _run_layers(sd, cfg, layers, h, emb, P, masks):
    for layer in layers:
        kind, p = layer[0], P + layer[1]
        if kind == "stem":
            h = conv_same(sd, p, h)
        elif kind == "res":
            h = res_block(sd, p, h, emb, None if masks is None else masks.get(layer[1]))
        elif kind == "attn":
            h = attention_block(sd, p, h, cfg["num_heads"])
        elif kind == "down":
            h = downsample(sd, p, h)
        elif kind == "up":
            h = upsample(sd, p, h)
        else:  # pragma: no cover
            raise ValueError(kind)
    return h


def unet_forward(
    sd: SD,
    cfg: dict,
    x: Tensor,
    timesteps: Tensor,
    cond: Optional[Tensor] = None,
    prefix: str = "",
    dropout_masks: Optional[Dict[str, Tensor]] = None,
    taps: Optional[Dict[str, Tensor]] = None,
) -> Tensor:
    """unet.py:360-398.  ``taps`` (optional dict) receives intermediate tensors
    keyed by block name, for per-block parity tests."""
    cfg = full_config(cfg)
    inputs, middle, outputs, _ = unet_layout(cfg)
    emb = embedding(sd, cfg, timesteps, cond, prefix)
    if taps is not None:
        taps["emb"] = emb
    hs: List[Tensor] = []
    h = x
    for i, layers in enumerate(inputs):
        h = _run_layers(sd, cfg, layers, h, emb, prefix, dropout_masks)
        hs.append(h)
        if taps is not None:
            taps[f"input_blocks.{i}"] = h
    h = _run_layers(sd, cfg, middle, h, emb, prefix, dropout_masks)
    if taps is not None:
        taps["middle_block"] = h
    for i, layers in enumerate(outputs):
        h = torch.cat([h, hs.pop()], dim=1)
        h = _run_layers(sd, cfg, layers, h, emb, prefix, dropout_masks)
        if taps is not None:
            taps[f"output_blocks.{i}"] = h
    h = F.silu(group_norm32(sd, prefix + "out.0", h))
    return conv_same(sd, prefix + "out.2", h)


def res_block_names(cfg: dict) -> List[Tuple[str, int]]:
    """(prefix, out_channels) of every ResBlock -- the dropout-mask sites."""
    inputs, middle, outputs, _ = unet_layout(cfg)
    out = []
    for blk in inputs + [middle] + outputs:
        for layer in blk:
            if layer[0] == "res":
                out.append((layer[1], layer[3]))
    return out
