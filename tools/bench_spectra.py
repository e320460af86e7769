"""Cost of the amplitude spectra at the reference's validation batch (B = 192 waveforms of 3 x 4064 samples: 576 rows), next to the
host path of the same metric class on the same box (its device-to-host copy included) and the 18-step sample of the same batch.

    python tools/bench_spectra.py [--waveforms N] [--length T] [--rounds R] [--no-sample] [--json OUT.json]

HIP events around calls issued back to back after a warm-up, medians over the rounds:
  rdft_complex       tqe_rdft, COMPLEX mode, all 576 rows: one launch
  rdft_log_channel   tqe_rdft, LOG mode, on the channel view pred[:, 0] (192 rows with a row stride of 3 T): one launch
  spectral_filter    tqe_spectral_filter with the integration multiplier, all 576 rows: one launch
  column_moments     tqe_column_moments of the (192, T/2+1) log spectra: one launch
  asd_device         metric.AmplitudeSpectralDensity(channel=0) on two GPU tensors, its result read back (.item())
  asd_host           the same object's host path on the same two GPU tensors: device-to-host copy, numpy rfft, numpy moments
  evaluate_ratio     ground_motion.evaluate_ratio of 192 two-component pairs (PGV, both sets)
  sample             LightningEDM.sample of the paper UNet (6 -> 6 channels) at (B / 3, 6, T), 18 Heun steps
asd_host is a host clock around a call that ends on the host; everything else is device events.
Parity at the timed size: the forward and integration errors next to scipy.fft's in float32 (tests/test_spectra_gpu.py's figures).
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
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import scipy.fft
    import _spectra_ref as R
    from tqdne_amd import ground_motion as GM, metric, spectra
    from tqdne_amd._lib_eval import TQE_RDFT_COMPLEX, TQE_RDFT_LOG

    if not torch.cuda.is_available():
        raise SystemExit("bench_spectra.py measures on the GPU: no GPU is visible")
    dev = torch.device("cuda:0")
    N, T, dt = a.waveforms, a.length, a.dt
    pred_h = R.make_rows(3 * N, T, seed=1).reshape(N, 3, T)
    target_h = R.make_rows(3 * N, T, seed=2).reshape(N, 3, T)
    pred, target = torch.from_numpy(pred_h).to(dev), torch.from_numpy(target_h).to(dev)
    logs = spectra.log_amplitude_spectrum(pred[:, 0])
    asd = metric.AmplitudeSpectralDensity(fs=1.0 / dt, channel=0)
    fns = dict(rdft_complex=lambda: spectra._rdft(pred, TQE_RDFT_COMPLEX),
               rdft_log_channel=lambda: spectra._rdft(pred[:, 0], TQE_RDFT_LOG, 1e-8),
               spectral_filter=lambda: spectra.integrate_frequency_domain(pred, dt),
               column_moments=lambda: spectra._moments(logs),
               asd_device=lambda: asd(pred, target),
               evaluate_ratio=lambda: GM.evaluate_ratio(target, pred, dt))
    asd_host = lambda: metric.Metric.__call__(asd, pred, target)
    for fn in list(fns.values()) + [asd_host]:   # warm-up: code objects, tables, allocator
        fn(), fn()
    torch.cuda.synchronize()
    rows = {k: [] for k in list(fns) + ["asd_host"]}
    for i in range(a.rounds):
        for k, fn in fns.items():
            rows[k].append(event_ms(fn, 20))
        rows["asd_host"].append(host_ms(asd_host, 3))
        print(f"round {i}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in rows.items()) + " ms", flush=True)
    ms = {k: statistics.median(v) for k, v in rows.items()}
    res = dict(device=torch.cuda.get_device_name(0), waveforms=N, rows=3 * N, length=T, dt=dt, rounds=a.rounds, ms=ms,
               ms_min_max={k: (min(v), max(v)) for k, v in rows.items()}, us_per_row_rdft=1e3 * ms["rdft_complex"] / (3 * N),
               asd_host_over_device=ms["asd_host"] / ms["asd_device"], asd_device_value=float(asd(pred, target)),
               asd_host_value=float(asd_host()))

    # parity at the timed size (every row but the all-zero one)
    x = pred_h.reshape(3 * N, T)[:-1]
    x64 = x.astype(np.float64)
    X64, norm = np.fft.rfft(x64, axis=-1), np.linalg.norm(x64, axis=-1)
    got = spectra.rdft(torch.from_numpy(x).to(dev)).cpu().numpy()
    err = lambda X: float((np.abs(X - X64).max(-1) / norm).max())
    y64 = R.integrate_frequency_domain(x64, dt)
    ferr = lambda y: float((np.abs(y - y64).max(-1) / np.abs(y64).max(-1)).max())
    res["parity"] = dict(rdft_error=err(got), rdft_scipy_float32=err(scipy.fft.rfft(x, axis=-1)),
                         integrate_error=ferr(spectra.integrate_frequency_domain(torch.from_numpy(x).to(dev), dt).cpu().numpy()),
                         integrate_scipy_complex64=ferr(R.integrate_frequency_domain(x, dt, scipy.fft)))

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
        res["asd_device_over_sample"] = ms["asd_device"] / res["sample_18_steps_ms"]
    print("RESULT " + json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
