"""iCT training step of the consistency model, paper UNet at B = 64 x 3 x 4096: the fused route against the autograd route.

    python tools/bench_consistency_train.py [--rounds R] [--steps N] [--batch B] [--length T] [--json OUT.json]

  fused     DataParallelTrainer.train_step: step_and_backward (gradients in the backward plan's flat buffer) + one-launch RAdam + EMA
  autograd  loss = cm.step(batch); loss.backward(); torch.optim.RAdam.step()   (torch's multi-tensor RAdam; no EMA)

Both routes live in one process on one device, each with its own model and plans, and are timed alternately (autograd, fused, autograd,
...) with HIP events around ``steps`` consecutive steps, after a warm-up of each; the medians over the rounds are reported, and every
round's figures are printed so that drift shows.  The optimizers alone are timed the same way on the gradients of the last step."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, n):
    """mean milliseconds of ``n`` consecutive calls, between two events on the current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--length", type=int, default=4096)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    from tqdne_amd import UNetModel, paper_1d_unet_config, rng
    from tqdne_amd.consistency_model import LithningConsistencyModel
    from tqdne_amd.trainer import DataParallelTrainer

    dev = torch.device("cuda:0")
    MAX_STEPS = 100000   # (the schedule stays at its first length, 11 points, for both routes)

    def make():
        torch.manual_seed(0)
        net = UNetModel(**paper_1d_unet_config())
        with torch.no_grad():
            for p in net.parameters():
                if torch.count_nonzero(p) == 0:   # (the zero-initialised convs: a net at initialisation has zero gradients behind them)
                    p.normal_(0, 0.02)
        return LithningConsistencyModel(net).to(dev).train()

    g = torch.Generator().manual_seed(1)
    batch = {"signal": (0.5 * torch.randn(a.batch, 3, a.length, generator=g)).to(dev), "cond": torch.randn(a.batch, 5, generator=g).to(dev)}
    rng.seed_rank(0, 0)

    cm_a = make()
    cm_a.max_steps, cm_a.global_step = MAX_STEPS, 0
    opt_a = cm_a.configure_optimizers()

    def autograd_step():
        opt_a.zero_grad()
        loss = cm_a.step(batch)
        loss.backward()
        opt_a.step()

    cm_f = make()
    tr = DataParallelTrainer(cm_f, world_size=1, fused_optimizer=True, ema_decay=0.999, max_steps=MAX_STEPS)

    def fused_step():
        tr.train_step(batch)

    for fn in (autograd_step, fused_step):
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    rounds = []
    for r in range(a.rounds):
        t_a = timed(autograd_step, a.steps)
        t_f = timed(fused_step, a.steps)
        rounds.append((t_a, t_f))
        print(f"round {r}: autograd route {t_a:.2f} ms / step, fused route {t_f:.2f} ms / step", flush=True)
    # the optimizers alone, on the gradients the last step left
    flag = tr._range_skip_flag()
    o_rounds = []
    for r in range(a.rounds):
        o_a = timed(opt_a.step, a.steps)
        o_f = timed(lambda: tr.optimizer.step(skip_flag=flag), a.steps)
        o_rounds.append((o_a, o_f))
    med = lambda xs: statistics.median(xs)
    res = dict(device=torch.cuda.get_device_name(0), batch=a.batch, length=a.length, rounds=a.rounds, steps=a.steps,
               autograd_step_ms=med([x for x, _ in rounds]), fused_step_ms=med([y for _, y in rounds]),
               torch_radam_ms=med([x for x, _ in o_rounds]), fused_radam_ema_ms=med([y for _, y in o_rounds]),
               per_round=rounds, per_round_optimizer=o_rounds,
               parameters=sum(p.numel() for p in cm_f.net.parameters()), tensors=len(list(cm_f.net.parameters())))
    print(f"iCT training step, paper UNet, B = {a.batch} x 3 x {a.length} on {res['device']} (medians of {a.rounds} rounds of {a.steps} steps):\n"
          f"  autograd route (step + backward + torch RAdam)        {res['autograd_step_ms']:.2f} ms\n"
          f"  fused route (DataParallelTrainer.train_step, RAdam+EMA) {res['fused_step_ms']:.2f} ms\n"
          f"  optimizer alone: torch RAdam {res['torch_radam_ms']:.3f} ms, one-launch RAdam + EMA {res['fused_radam_ema_ms']:.3f} ms")
    print("RESULT " + json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
