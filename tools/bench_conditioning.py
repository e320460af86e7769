"""Cost of the time-domain conditioning at the reference's validation batch (B = 192 waveforms of 3 x 4064 samples: 576 rows), next to
the host path of the same functions on the same box (both copies included) and the 18-step sample of the same batch.

    python tools/bench_conditioning.py [--waveforms N] [--length T] [--rounds R] [--no-sample] [--json OUT.json]

HIP events around calls issued back to back after a warm-up, medians over the rounds:
  highpass           conditioning.highpass_filter: tqs_sosfilt, 2 sections, no detrend, all 576 rows: one launch
  highpass_channel   the same on the channel view w[:, 0] (192 rows with a row stride of 3 T)
  condition_stream   conditioning.condition_stream: linear detrend + 4 sections: one launch
  envelope           conditioning.moving_average_envelope_adaptive, window 128: one launch
  *_host             the same function's host path on the same GPU tensor: device-to-host copy, scipy / numpy, host-to-device copy
  sample             LightningEDM.sample of the paper UNet (6 -> 6 channels) at (B / 3, 6, T), 18 Heun steps
The *_host rows are a host clock around a call that ends on the host; everything else is device events.
Parity at the timed size: the kernel's distance from float64 sosfilt and from the reference's lfilter(b, a), of each row's peak.
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


def host_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waveforms", type=int, default=192)
    ap.add_argument("--length", type=int, default=4064)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import _conditioning_ref as R
    from tqdne_amd import conditioning as C

    if not torch.cuda.is_available():
        raise SystemExit("bench_conditioning.py measures on the GPU: no GPU is visible")
    dev = torch.device("cuda:0")
    N, T = a.waveforms, a.length
    w_h = R.make_series(3 * N, T, seed=1).reshape(N, 3, T)
    w = torch.from_numpy(w_h).to(dev)
    via_host = lambda f: (lambda: torch.from_numpy(np.ascontiguousarray(f(w.cpu().numpy()))).to(dev))
    fns = dict(highpass=lambda: C.highpass_filter(w), highpass_channel=lambda: C.highpass_filter(w[:, 0]),
               condition_stream=lambda: C.condition_stream(w), envelope=lambda: C.moving_average_envelope_adaptive(w))
    host = dict(highpass_host=via_host(C.highpass_filter), condition_stream_host=via_host(C.condition_stream),
                envelope_host=via_host(C.moving_average_envelope_adaptive))
    for fn in fns.values():   # warm-up: code objects, tables, allocator
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
    res = dict(device=torch.cuda.get_device_name(0), waveforms=N, rows=3 * N, length=T, rounds=a.rounds, ms=ms,
               ms_min_max={k: (min(v), max(v)) for k, v in rows.items()},
               host_over_device={k: ms[k + "_host"] / ms[k] for k in ("highpass", "condition_stream", "envelope")})

    # parity at the timed size
    x = w_h.reshape(3 * N, T)
    sos = R.butter_sos(4, R.HIGHPASS_WN, "high")
    y64, y_ba = R.sosfilt64(sos, x), R.highpass_ba64(x)
    peak = np.abs(y64).max(-1)
    y = C.highpass_filter(w).cpu().numpy().reshape(3 * N, T).astype(np.float64)
    c64 = R.sosfilt64(R.bandpass_sos(0.1, 30, 100), x, "linear")
    c = C.condition_stream(w).cpu().numpy().reshape(3 * N, T).astype(np.float64)
    env64, _ = R.hold_envelope(x[:24], 128, 1e-6)
    env = C.moving_average_envelope_adaptive(w).cpu().numpy().reshape(3 * N, T)[:24].astype(np.float64)
    res["parity"] = dict(highpass_to_sosfilt64=float((np.abs(y - y64).max(-1) / peak).max()),
                         highpass_to_lfilter_ba=float((np.abs(y - y_ba).max(-1) / peak).max()),
                         lfilter_ba_to_sosfilt64=float((np.abs(y_ba - y64).max(-1) / peak).max()),
                         condition_stream_to_float64=float((np.abs(c - c64).max(-1) / np.abs(c64).max(-1)).max()),
                         envelope_to_float64=float((np.abs(env - env64).max(-1) / env64.max(-1)).max()))

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
        res["conditioning_over_sample"] = (ms["highpass"] + ms["envelope"]) / res["sample_18_steps_ms"]
    print("RESULT " + json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
