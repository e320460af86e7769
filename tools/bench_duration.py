"""Cost of the duration measures at the reference's validation batch (192 waveforms of 3 x 4064 samples: 192 pairs of horizontal
components), next to (a) the host path of the same functions on the same box, both copies included, (b) the same measure composed from
stock torch operators on the device, and the 18-step sample of the same batch.

    python tools/bench_duration.py [--waveforms N] [--length T] [--rounds R] [--no-sample] [--json OUT.json]

HIP events around calls issued back to back after a warm-up, medians over the rounds:
  significant_duration   duration.significant_duration(w[:, 1], w[:, 0], normalize=True): one tqd_arias launch and the few small
                         operators that turn energy, peak and indices into Ia and times
  arias_launch           the tqd_arias launch alone, through the binding, into preallocated outputs
  husid                  duration.husid(w[:, 1], w[:, 0]): one launch that also writes the (N, T) curve
  gradient               duration.compute_time_derivative(w): one launch over 3 N rows
  *_torch                (b): squares in float64, cumsum, comparisons and argmax (torch.gradient for the derivative), on the device
  *_host                 (a): the same function's host path on the same GPU tensors: device-to-host copy, numpy / scipy, copy back
The *_host rows are a host clock around a call that ends on the host; everything else is device events.
Parity at the timed size: energy against the exactly rounded float64 total, crossings against the torch composition.
Prints one JSON line (RESULT {...})."""

import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def host_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def torch_cumulative(x, y, step):
    s = x.double() ** 2 + y.double() ** 2
    cum = torch.cumsum(0.5 * (s[:, :-1] + s[:, 1:]) * step, -1)
    return torch.nn.functional.pad(cum, (1, 0)), s


def torch_significant_duration(x, y, step, lo=0.05, hi=0.95, gravity=9.81):
    cum, s = torch_cumulative(x, y, step)
    total = cum[:, -1]
    Ia = (math.pi / (2 * gravity)) * total / s.amax(-1)
    n0 = (cum >= (lo * total)[:, None]).to(torch.int8).argmax(-1)
    n1 = (cum >= (hi * total)[:, None]).to(torch.int8).argmax(-1)
    return Ia, n0 * step, n1 * step, (n1 - n0) * step


def torch_husid(x, y, step):
    cum, _ = torch_cumulative(x, y, step)
    return (cum / cum[:, -1:]).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waveforms", type=int, default=192)
    ap.add_argument("--length", type=int, default=4064)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import _duration_ref as R
    from tqdne_amd import _lib_duration
    from tqdne_amd import duration as D

    if not torch.cuda.is_available():
        raise SystemExit("bench_duration.py measures on the GPU: no GPU is visible")
    dev = torch.device("cuda:0")
    N, T = a.waveforms, a.length
    step = 0.01
    x_h, y_h = R.make_pairs(N, T, seed=1)
    w_h = np.stack([x_h, y_h, 0.5 * x_h[::-1]], axis=1)
    w = torch.from_numpy(w_h).to(dev)
    ew, ns = w[:, 1], w[:, 0]

    lib = _lib_duration.load()
    energy, peak2 = torch.empty(N, device=dev, dtype=torch.float64), torch.empty(N, device=dev, dtype=torch.float64)
    index = torch.empty((N, 2), device=dev, dtype=torch.int32)
    fr = (ctypes.c_double * 2)(0.05, 0.95)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def arias_launch():
        rc = lib.tqd_arias(ew.data_ptr(), ns.data_ptr(), energy.data_ptr(), peak2.data_ptr(), index.data_ptr(), None, N, T, 3 * T, 3 * T,
                           step, fr, 2, stream)
        assert rc == 0, rc

    to_dev = lambda r: [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (r if isinstance(r, tuple) else (r,))]
    fns = dict(significant_duration=lambda: D.significant_duration(ew, ns, dt=step, normalize=True), arias_launch=arias_launch,
               husid=lambda: D.husid(ew, ns, dt=step), gradient=lambda: D.compute_time_derivative(w),
               significant_duration_torch=lambda: torch_significant_duration(ew, ns, step),
               husid_torch=lambda: torch_husid(ew, ns, step), gradient_torch=lambda: torch.gradient(w, spacing=step, dim=-1))
    host = dict(significant_duration_host=lambda: to_dev(D.significant_duration(ew.cpu().numpy(), ns.cpu().numpy(), dt=step, normalize=True)),
                husid_host=lambda: to_dev(D.husid(ew.cpu().numpy(), ns.cpu().numpy(), dt=step)),
                gradient_host=lambda: to_dev(D.compute_time_derivative(w.cpu().numpy())))
    for fn in fns.values():   # warm-up: code objects, allocator
        fn(), fn()
    for fn in host.values():
        fn()
    torch.cuda.synchronize()
    rows = {k: [] for k in list(fns) + list(host)}
    for i in range(a.rounds):
        for k, fn in fns.items():
            rows[k].append(event_ms(fn, 20))
        for k, fn in host.items():
            rows[k].append(host_ms(fn, 1))
        print(f"round {i}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in rows.items()) + " ms", flush=True)
    ms = {k: statistics.median(v) for k, v in rows.items()}
    names = ("significant_duration", "husid", "gradient")
    res = dict(device=torch.cuda.get_device_name(0), waveforms=N, length=T, rounds=a.rounds, ms=ms,
               ms_min_max={k: (min(v), max(v)) for k, v in rows.items()},
               torch_over_kernel={k: ms[k + "_torch"] / ms[k] for k in names},
               host_over_kernel={k: ms[k + "_host"] / ms[k] for k in names},
               ranges_apart={k: max(rows[k]) < min(rows[k + "_torch"]) for k in names})

    # parity at the timed size
    Ia, t0, t1, d = D.significant_duration(ew, ns, dt=step)
    exact = math.pi / (2 * 9.81) * R.exact_total(y_h, x_h, step)
    tq = torch_significant_duration(ew, ns, step)
    res["parity"] = dict(energy_to_exact=float((np.abs(Ia.cpu().numpy() - exact) / exact).max()),
                         crossings_differing_from_torch=int((torch.round(t0 / step) != torch.round(tq[1] / step)).sum()
                                                            + (torch.round(t1 / step) != torch.round(tq[2] / step)).sum()),
                         husid_to_torch=float((D.husid(ew, ns, dt=step) - torch_husid(ew, ns, step)).abs().max()))

    if not a.no_sample:
        from tqdne_amd import LightningEDM
        from tqdne_amd.architectures import paper_1d_unet_config
        torch.manual_seed(0)
        edm = LightningEDM(paper_1d_unet_config(in_channels=6, out_channels=6), {"learning_rate": 1e-4, "max_steps": 1000, "eta_min": 0.0},
                           num_sampling_steps=18)
        with torch.no_grad():
            for p in edm.parameters():
                if torch.count_nonzero(p) == 0:
                    p.normal_(0, 0.02)
        edm = edm.to(dev).eval()
        B = max(1, N // 3)
        cond = torch.randn(B, 5).to(dev)
        sample = lambda: edm.sample((B, 6, T), cond=cond)
        sample(), sample()
        torch.cuda.synchronize()
        ts = [event_ms(sample, 2) for _ in range(max(3, a.rounds // 2))]
        res["sample_18_steps_ms"] = statistics.median(ts)
        res["sample_batch"] = B
        res["duration_over_sample"] = ms["significant_duration"] / res["sample_18_steps_ms"]
    print("RESULT " + json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
