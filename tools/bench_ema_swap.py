"""Cost of getting the EMA weights into the module and the training weights back, paper UNet (EDM).

    python tools/bench_ema_swap.py [--rounds R] [--batch B] [--length T] [--json OUT.json]

Two routes, timed alternately with a host clock around work that ends in a device synchronise (medians over the rounds, every round
printed):
  swap  ``with trainer.ema_weights(): pass`` -- tq_ema_swap twice, in place
  copy  the reference's EMA callback (tqdne/ema.py:30-36): ``deepcopy(module.state_dict())``, ``load_state_dict(ema_state,
        strict=False)``, then ``load_state_dict(original)``
and, with HIP events, the swap launch alone (20 back to back) and what any change of the weights costs afterwards: the first inference
forward behind a swap (it re-packs the weights) against a forward on unchanged weights.  Also the peak allocation of either route."""

import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def peak_over(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--length", type=int, default=4096)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    from tqdne_amd import LightningEDM, paper_1d_unet_config, rng
    from tqdne_amd.trainer import DataParallelTrainer

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    edm = LightningEDM(paper_1d_unet_config(), {"learning_rate": 1e-4, "max_steps": 100000, "eta_min": 0.0})
    with torch.no_grad():
        for p in edm.unet.parameters():
            if torch.count_nonzero(p) == 0:   # (the zero-initialised convs: a net at initialisation has zero gradients behind them)
                p.normal_(0, 0.02)
    edm = edm.to(dev).train()
    g = torch.Generator().manual_seed(1)
    x, cond = (0.5 * torch.randn(a.batch, 3, a.length, generator=g)).to(dev), torch.randn(a.batch, 5, generator=g).to(dev)
    sigma = torch.full((a.batch,), 0.7, device=dev)
    rng.seed_rank(0, 0)
    tr = DataParallelTrainer(edm, world_size=1, ema_decay=0.999)
    tr.train_step({"signal": x, "cond": cond})   # (the EMA leaves the weights)
    opt = tr.optimizer

    def swap():
        with tr.ema_weights():
            pass

    def copy_route():
        original = copy.deepcopy(edm.state_dict())
        edm.load_state_dict(tr.ema_state(), strict=False)
        edm.load_state_dict(original)

    def forward():
        with torch.no_grad():
            edm(x, sigma, None, cond)

    for fn in (swap, copy_route, forward, forward):
        fn()
    rounds = []
    for r in range(a.rounds):
        row = dict(swap=wall_ms(swap), copy=wall_ms(copy_route))
        row["forward_after_change"] = wall_ms(forward)   # (the copy route has just changed every version: this forward re-packs)
        row["forward"] = wall_ms(forward)
        rounds.append(row)
        print(f"round {r}: " + ", ".join(f"{k} {v:.3f}" for k, v in row.items()) + " ms", flush=True)
    launch = [event_ms(opt.swap_ema, 20) for _ in range(a.rounds)]
    assert not opt.ema_swapped
    med = statistics.median
    nbytes = 4 * sum(p.numel() for p in opt.param_groups[0]["params"])
    res = dict(device=torch.cuda.get_device_name(0), batch=a.batch, length=a.length, rounds=a.rounds, chunks=opt._swap_chunks,
               parameter_bytes=nbytes, tensors=len(opt.param_groups[0]["params"]),
               ms={k: med([row[k] for row in rounds]) for k in rounds[0]}, per_round=rounds, swap_launch_ms=med(launch),
               peak_bytes=dict(swap=peak_over(swap), copy=peak_over(copy_route)))
    m = res["ms"]
    print(f"EMA weights in and out, paper UNet ({res['tensors']} tensors, {nbytes / 1e6:.1f} MB) on {res['device']}, medians of {a.rounds}:\n"
          f"  swap (two launches) {m['swap']:.3f} ms   copy route {m['copy']:.3f} ms   peak allocation: swap {res['peak_bytes']['swap']} B, "
          f"copy {res['peak_bytes']['copy'] / 1e6:.1f} MB\n"
          f"  one tq_ema_swap launch (20 back to back, {res['chunks']} chunks): {1e3 * res['swap_launch_ms']:.1f} us = "
          f"{4 * nbytes / res['swap_launch_ms'] / 1e9:.2f} TB/s over 2 x {nbytes / 1e6:.1f} MB read and written\n"
          f"  inference forward at B = {a.batch}: {m['forward']:.3f} ms, the first one after a change of the weights {m['forward_after_change']:.3f} ms")
    print("RESULT " + json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
