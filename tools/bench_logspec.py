"""Cost of the LogSpectrogram launches at the reference's configuration (stft_channels = 256, hop_size = 32, 3 x 4064 waveforms,
B = 64: N = 192 waveforms of 128 frames), next to the float32 numpy restatement on the host and the 18-step sample of the same box.

    python tools/bench_logspec.py [--waveforms N] [--length T] [--hop H] [--rounds R] [--no-sample] [--json OUT.json]

HIP events around launches issued back to back after a warm-up, medians over the rounds:
  get_representation     tq_stft_fwd writing the normalised log-magnitude (one launch)
  get_spectrogram        tq_stft_fwd writing the complex spectrogram
  invert_representation  tq_griffinlim, 128 iterations, log-magnitude input (one launch, one workgroup per waveform)
  host restatement       tests/_logspec_ref.py in float32 / complex64 on one core: stft + log map, and griffinlim, per waveform
  sample                 LightningEDM.sample of the paper UNet (6 -> 6 channels) at (B, 6, T), 18 Heun steps
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
    ap.add_argument("--hop", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-waveforms", type=int, default=2)
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import _logspec_ref as R
    from tqdne_amd.representation import LogSpectrogram

    dev = torch.device("cuda:0")
    N, T, hop = a.waveforms, a.length, a.hop
    rep = LogSpectrogram(256, hop)
    x = R.make_signal(T, N).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    r = rep.get_representation(xd)
    fns = dict(get_representation=lambda: rep.get_representation(xd), get_spectrogram=lambda: rep.get_spectrogram(xd),
               invert_representation=lambda: rep.invert_representation(r))
    reps = dict(get_representation=50, get_spectrogram=50, invert_representation=3)
    for fn in fns.values():   # warm-up: code objects, tables, allocator
        fn(), fn()
    torch.cuda.synchronize()
    rows = {k: [] for k in fns}
    for i in range(a.rounds):
        for k, fn in fns.items():
            rows[k].append(event_ms(fn, reps[k]))
        print(f"round {i}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in rows.items()) + " ms", flush=True)
    ms = {k: statistics.median(v) for k, v in rows.items()}
    spread = {k: (min(v), max(v)) for k, v in rows.items()}

    # parity at the timed size: the forward against float64, the inversion by its spectral convergence
    S64 = np.abs(R.get_spectrogram(x[:2].astype(np.float64), 256, hop))
    y = rep.invert_representation(r[:2]).cpu().numpy().astype(np.float64)
    conv = float(np.linalg.norm(np.abs(R.get_spectrogram(y, 256, hop)) - S64) / np.linalg.norm(S64))

    nh = max(1, min(a.host_waveforms, N))
    t0 = time.perf_counter()
    r_host = R.to_representation(R.get_spectrogram(x[:nh], 256, hop, dtype=np.float32))
    host_fwd = (time.perf_counter() - t0) / nh
    m_host = R.with_nyquist(R.from_representation(r_host).astype(np.float32))
    t0 = time.perf_counter()
    for i in range(nh):   # one waveform at a time, as the reference's pool maps them
        R.griffinlim(m_host[i:i + 1], 128, hop, 256, dtype=np.float32)
    host_inv = (time.perf_counter() - t0) / nh

    res = dict(device=torch.cuda.get_device_name(0), waveforms=N, length=T, hop=hop, frames=1 + T // hop, rounds=a.rounds, ms=ms,
               ms_min_max=spread, inversion_us_per_waveform=1e3 * ms["invert_representation"] / N,
               spectral_convergence_128=conv, host_fp32_restatement_s_per_waveform=dict(get_representation=host_fwd, invert=host_inv),
               host_core_seconds_for_batch=host_inv * N, speedup_vs_one_host_core=host_inv * N / (1e-3 * ms["invert_representation"]))
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
        res["inversion_over_sample"] = ms["invert_representation"] / res["sample_18_steps_ms"]
    print("RESULT " + json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
