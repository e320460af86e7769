#!/usr/bin/env python3
"""Stem / head kernels at B = 64, T = 4096, 3 signal channels, k = 5: time per launch (median of 7 x 20 launches between HIP events,
after 5 warm-up launches) and the rate 4 B T (C_in + C_out) bytes / time.
usage: [TQDNE_HIP_LIB=...] python tools/bench_ends.py [B] [--widths 64,128,256,512,1024]   (developer tool, GPU box)
Without --widths: the paper UNet's 3 -> 64 stem and 64 -> 3 head.  With it: stem forward, head forward and head backward (with a
workspace) at every listed first-level width, in one run on one box -- the yardstick of the channel-tiled kernels (csrc/ends_wide.hip)
is the rate the first kernels reach in the same run at 64 channels (stem) and 128 channels (head)."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tqdne_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=64)
ap.add_argument("--widths", default="64", help="comma-separated first-level widths")
args = ap.parse_args()
B, T = args.B, 4096
dev = torch.device("cuda:0")
x = torch.randn(B, 3, T, device=dev)
sc = torch.rand(B, device=dev) + 0.5
co, cs = torch.rand(B, device=dev), torch.rand(B, device=dev)
dpred = torch.randn(B, 3, T, device=dev)


def timed(fn):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 20 * 1e3)
    return sorted(ts)[3]


for C in (int(v) for v in args.widths.split(",")):
    nbytes = 4 * B * T * (C + 3)
    rate = lambda us: nbytes / us * 1e-6   # TB/s
    w, b = torch.randn(C, 3, 5, device=dev) / 4, torch.randn(C, device=dev)
    h = torch.randn(B, T, C, device=dev)
    hw, hb = torch.randn(3, C, 5, device=dev) / (C * 5) ** 0.5, torch.randn(3, device=dev)
    gs, gh = torch.rand(B, C, device=dev) + 0.5, torch.randn(B, C, device=dev)
    y, st = torch.empty(B, T, C, device=dev), torch.empty(B, T // 128, C, 2, device=dev)
    yh = torch.empty(B, 3, T, device=dev)
    us = timed(lambda: ops.stem_conv(x, w, b, in_scale=sc, out=(y, st)))
    print(f"stem 3->{C} k5 B={B} T={T}: {us:.1f} us  {rate(us):.2f} TB/s")
    us = timed(lambda: ops.head_conv(h, hw, hb, gscale=gs, gshift=gh, c_out=co, c_skip=cs, skip_src=x, out=yh))
    print(f"head {C}->3 k5 B={B} T={T}: {us:.1f} us  {rate(us):.2f} TB/s")
    if args.widths != "64":
        G, gst = torch.empty_like(h), torch.empty(B, T // 128, C, 2, device=dev)
        dw, db = torch.zeros_like(hw), torch.zeros(3, device=dev)   # (added to on every launch: the timing does not care)
        us = timed(lambda: ops.head_conv_bwd(dpred, h, hw, gs, gh, co, out=(G, gst, dw, db)))
        print(f"head bwd 3->{C} k5 B={B} T={T}: {us:.1f} us  {rate(us):.2f} TB/s (same byte count; the kernel also writes G)")
        del G, gst
    del h, y, st
