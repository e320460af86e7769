"""Cost of the ground-motion intensity measures at the reference's batch (3 x 4064 waveforms, B = 64: N = 192 two-component pairs),
for its own 4 periods (0.1 / 0.3 / 1 / 2 s) and for a 100-period spectrum (log-spaced 0.03 ... 10 s), next to the float64 numpy
restatement on one core of the same box and the 18-step sample of the same batch.

    python tools/bench_intensity.py [--waveforms N] [--length T] [--rounds R] [--host-waveforms H] [--no-sample] [--json OUT.json]

HIP events around calls issued back to back after a warm-up, medians over the rounds:
  rotd_peaks         tq_rotd_peaks: the directional peaks (N, 3 + P, 180), one launch
  gmrotdpp_with_pg   the same launch plus the percentile over the angles in torch (PGA, PGV, PGD, SA)
  host restatement   tests/_intensity_ref.py in float64 on one core, one waveform at a time as the reference's pool maps them
  sample             LightningEDM.sample of the paper UNet (6 -> 6 channels) at (B, 6, T), 18 Heun steps
Parity at the timed size: the per-series error of the peaks against float64 for the waveforms the host computed.
Prints one JSON line (RESULT {...})."""

import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waveforms", type=int, default=192)
    ap.add_argument("--length", type=int, default=4064)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-waveforms", type=int, default=2)
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import _intensity_ref as R
    from tqdne_amd import ground_motion as GM

    dev = torch.device("cuda:0")
    N, T, dt = a.waveforms, a.length, a.dt
    x, y = R.make_waveforms(N, T)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    cases = {"P4": (0.1, 0.3, 1.0, 2.0), "P100": tuple(float(p) for p in R.periods_log(100))}
    res = dict(device=torch.cuda.get_device_name(0), waveforms=N, length=T, dt=dt, rounds=a.rounds, cases={})
    nh = max(1, min(a.host_waveforms, N))
    for name, per in cases.items():
        fns = dict(rotd_peaks=lambda: GM.rotd_peaks(xd, yd, dt, per), gmrotdpp_with_pg=lambda: GM.gmrotdpp_with_pg(xd, yd, dt, per, 50))
        for fn in fns.values():   # warm-up: code objects, tables, allocator
            fn(), fn()
        torch.cuda.synchronize()
        rows = {k: [] for k in fns}
        for i in range(a.rounds):
            for k, fn in fns.items():
                rows[k].append(event_ms(fn, 10))
            print(f"{name} round {i}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in rows.items()) + " ms", flush=True)
        ms = {k: statistics.median(v) for k, v in rows.items()}
        t0 = time.perf_counter()
        refs = [R.rotd_peaks(x[i:i + 1], y[i:i + 1], dt, per) for i in range(nh)]   # one waveform at a time
        for r in refs:
            R.combine(r, 50)
        host = (time.perf_counter() - t0) / nh
        ref = np.concatenate(refs)
        got = GM.rotd_peaks(xd[:nh], yd[:nh], dt, per).cpu().numpy()
        err = float(R.series_error(got, ref).max())
        emu = float(R.series_error(R.emulate_peaks_f32(x[:nh], y[:nh], dt, per), ref).max())
        res["cases"][name] = dict(periods=len(per), ms=ms, ms_min_max={k: (min(v), max(v)) for k, v in rows.items()},
                                  us_per_waveform=1e3 * ms["gmrotdpp_with_pg"] / N, host_f64_restatement_s_per_waveform=host,
                                  host_core_seconds_for_batch=host * N, speedup_vs_one_host_core=host * N / (1e-3 * ms["gmrotdpp_with_pg"]),
                                  worst_series_error_vs_float64=err, fp32_emulation_error=emu)
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
        for c in res["cases"].values():
            c["over_sample"] = c["ms"]["gmrotdpp_with_pg"] / res["sample_18_steps_ms"]
    print("RESULT " + json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
