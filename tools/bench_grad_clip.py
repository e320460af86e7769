"""Cost of gradient clipping / gradient-norm tracking in the fused training step, paper UNet (EDM) at B = 64 x 3 x 4096.

    python tools/bench_grad_clip.py [--rounds R] [--steps N] [--batch B] [--length T] [--only MODE] [--json OUT.json]

One model, one DataParallelTrainer; the trainer's clipping options are switched between rounds, so the modes
  off    today's step (no norm, the _guarded optimizer launch)
  norm   gradient_clip_val (below the gradient norm: the coefficient is < 1), algorithm "norm": tq_grad_sumsq + tq_grad_clip_coef + the
         _clipped launch
  value  algorithm "value": the _clipped launch alone
  track  track_grad_norm alone: the two norm launches + the _guarded launch
are timed alternately (off, norm, value, track, off, ...) with HIP events around ``steps`` consecutive steps; medians over the rounds
are reported and every round is printed so that drift shows.  Then the launches alone, on the gradients the last step left: the two
norm kernels and the optimizer launch with and without the coefficient.  ``--only MODE`` runs ``steps`` steps of one mode and nothing
else (for a kernel trace of that mode)."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ("off", "norm", "value", "track")


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
    ap.add_argument("--only", default=None, choices=MODES)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    from tqdne_amd import LightningEDM, paper_1d_unet_config, rng
    from tqdne_amd._lib import check
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
    batch = {"signal": (0.5 * torch.randn(a.batch, 3, a.length, generator=g)).to(dev), "cond": torch.randn(a.batch, 5, generator=g).to(dev)}
    rng.seed_rank(0, 0)
    tr = DataParallelTrainer(edm, world_size=1, ema_decay=0.999)

    def set_mode(mode, clip=1e-3):
        tr.gradient_clip_val = None if mode in ("off", "track") else clip
        tr.gradient_clip_algorithm = "value" if mode == "value" else "norm"
        tr.track_grad_norm = mode == "track"

    def step():
        tr.train_step(batch)

    if a.only:
        set_mode(a.only)
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        print(f"{a.steps} steps of mode {a.only}; last_grad_norm {None if tr.last_grad_norm is None else float(tr.last_grad_norm)}")
        return

    for mode in MODES:
        set_mode(mode)
        for _ in range(a.warmup):
            step()
    torch.cuda.synchronize()
    norm = float(tr.last_grad_norm)
    rounds = []
    for r in range(a.rounds):
        row = {}
        for mode in MODES:
            set_mode(mode, clip=0.5 * norm if mode == "norm" else 1e-3)
            row[mode] = timed(step, a.steps)
        rounds.append(row)
        print(f"round {r}: " + ", ".join(f"{m} {row[m]:.3f}" for m in MODES) + " ms / step", flush=True)

    # the launches alone
    opt = tr.optimizer
    flag = tr._range_skip_flag()
    lib, stream = opt._lib, torch.cuda.current_stream(dev).cuda_stream
    opt.step(skip_flag=flag, max_grad_norm=0.5 * norm)   # (the buffers of this table exist from here on)
    partials, out = opt._norm_buf
    n = opt._n_chunks
    alone = {k: [] for k in ("grad_sumsq", "grad_clip_coef", "optimizer_guarded", "optimizer_clipped_norm", "optimizer_clipped_value")}
    for r in range(a.rounds):
        alone["grad_sumsq"].append(timed(lambda: check(lib.tq_grad_sumsq(opt._table.data_ptr(), n, partials.data_ptr(), stream)), 50))
        alone["grad_clip_coef"].append(timed(lambda: check(lib.tq_grad_clip_coef(partials.data_ptr(), n, 1.0, 0.5 * norm, out.data_ptr(),
                                                                                stream)), 50))
        alone["optimizer_guarded"].append(timed(lambda: opt.step(skip_flag=flag), 20))
        alone["optimizer_clipped_norm"].append(timed(lambda: opt._launch(opt._step, opt.param_groups[0], 1e-3, 1.0, flag.data_ptr(), stream,
                                                                         (out.data_ptr() + 4, 0.0)), 20))
        alone["optimizer_clipped_value"].append(timed(lambda: opt.step(skip_flag=flag, clip_value=1e-3), 20))
    med = statistics.median
    res = dict(device=torch.cuda.get_device_name(0), batch=a.batch, length=a.length, rounds=a.rounds, steps=a.steps, chunks=n,
               gradient_bytes=4 * sum(p.numel() for p in opt._updated), grad_norm=norm,
               step_ms={m: med([row[m] for row in rounds]) for m in MODES}, per_round=rounds,
               launch_ms={k: med(v) for k, v in alone.items()})
    s, l = res["step_ms"], res["launch_ms"]
    print(f"EDM training step, paper UNet, B = {a.batch} x 3 x {a.length} on {res['device']} (medians of {a.rounds} rounds of {a.steps} steps):\n"
          f"  off {s['off']:.3f} ms   norm {s['norm']:.3f} ms ({s['norm'] - s['off']:+.3f})   value {s['value']:.3f} ms ({s['value'] - s['off']:+.3f})"
          f"   track {s['track']:.3f} ms ({s['track'] - s['off']:+.3f})\n"
          f"  launches alone (back to back, {n} chunks, {res['gradient_bytes'] / 1e6:.1f} MB of gradients): tq_grad_sumsq {1e3 * l['grad_sumsq']:.1f} us, "
          f"tq_grad_clip_coef {1e3 * l['grad_clip_coef']:.1f} us,\n"
          f"  optimizer launch: guarded {1e3 * l['optimizer_guarded']:.1f} us, clipped by norm {1e3 * l['optimizer_clipped_norm']:.1f} us, "
          f"clipped by value {1e3 * l['optimizer_clipped_value']:.1f} us")
    print("RESULT " + json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
