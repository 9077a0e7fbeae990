#!/usr/bin/env python3
"""A/B of the per-segment measurements on one MI355X: the device path (whisperseg_amd.measure.measure: wseg_measure_segments_f32 on
PCM that is resident in HBM) against the host definition (measure_host: numpy float64, a Python loop with an STFT per segment) on
the same rows.  Not on the product path.

    python tools/measure_bench.py [--segments 10000] [--seconds 600] [--out profiles/measure_ab.txt]

For each of two rates, 16 kHz (n_fft 512) and 250 kHz (n_fft 4096), a recording of --seconds seconds (seeded noise under a
gated tone) and --segments random segments of 20 .. 200 ms.  Reported per rate:
  * the kernel pair alone: HIP-event time around the one call that enqueues the table's copy and both kernels, PCM resident;
  * wall time of measure() — bounds on the host, the launch pair, the rows' way back, scaling — with the PCM resident, as
    segment(measure=True) calls it;
  * wall time of measure_host on the same rows, the PCM already in host memory (what a user pays today AFTER loading the file
    again or copying the PCM back, neither of which is counted).
One warm-up of each, then five repetitions, device and host alternating; all five are printed, the median is the figure.  The
columns of both sides are compared once (largest difference per column)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATES = (16000, 250000)
REPS = 5


def recording(sr, seconds, seed=5):
    rng = np.random.default_rng(seed)
    n = int(sr * seconds)
    x = (0.01 * rng.standard_normal(n, dtype=np.float32))
    t = np.arange(n, dtype=np.float32)
    x += (0.3 * np.sin(2 * np.pi * 0.11 * t) * (np.sin(2 * np.pi * 3.0 / sr * t) > 0)).astype(np.float32)
    return x


def rows(sr, seconds, count, seed=6):
    rng = np.random.default_rng(seed)
    length = rng.uniform(0.02, 0.2, count)
    onset = np.sort(rng.uniform(0, seconds - 0.2, count))
    return {"onset": onset.tolist(), "offset": (onset + length).tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_ab.txt"))
    args = ap.parse_args()
    import torch
    from whisperseg_amd import _lib, measure as M
    from whisperseg_amd.audio_utils import get_n_fft_given_sr
    _lib.load(require_device=True)
    lines = [f"per-segment measurements, device against host: {args.segments} segments of 20 .. 200 ms in {args.seconds:g} s "
             f"({torch.cuda.get_device_name(0)}; warm-up, then {REPS} repetitions, alternating; times in ms)"]
    for sr in RATES:
        n_fft = get_n_fft_given_sr(sr)
        print(f"sr {sr} ...", flush=True)
        x = recording(sr, args.seconds)
        pred = rows(sr, args.seconds, args.segments)
        pcm = torch.from_numpy(x).cuda()
        bounds = M.bounds_of(pred, sr, len(x))
        band = M.band_bins(sr, n_fft)
        frames = sum(M.frame_count(int(b - a), n_fft) for a, b in bounds)

        def kernels():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            M.measure_rows(pcm, bounds, n_fft, *band)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)

        def device():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = M.measure(pcm, sr, pred)
            return (time.perf_counter() - t0) * 1e3, got

        def host():
            t0 = time.perf_counter()
            got = M.measure_host(x, sr, pred)
            return (time.perf_counter() - t0) * 1e3, got

        kernels(), device(), host()                      # warm-up: tables, allocator, page faults
        t_kernel, t_device, t_host = [], [], []
        for _ in range(REPS):
            t_kernel.append(kernels())
            ms, got = device()
            t_device.append(ms)
            ms, want = host()
            t_host.append(ms)
        fmt = lambda v: " ".join(f"{t:.2f}" for t in v)
        med = statistics.median
        lines.append(f"sr {sr} (n_fft {n_fft}): {len(bounds)} segments, {frames} frames")
        lines.append(f"  kernel pair (HIP events)   median {med(t_kernel):9.2f}   [{fmt(t_kernel)}]   {frames / med(t_kernel) / 1e3:.2f} M frames/s")
        lines.append(f"  measure(), PCM resident    median {med(t_device):9.2f}   [{fmt(t_device)}]")
        lines.append(f"  measure_host               median {med(t_host):9.2f}   [{fmt(t_host)}]")
        lines.append(f"  host / device wall: {med(t_host) / med(t_device):.0f}x (spread {min(t_host) / max(t_device):.0f}x .. {max(t_host) / min(t_device):.0f}x)")
        scale = {name: (sr / n_fft if name.startswith(("peak_f", "centroid", "freq_")) else 1.0) for name in M.COLUMNS}
        worst = {name: float(np.nanmax(np.abs(got[name].astype(np.float64) - want[name]) / scale[name])) for name in M.COLUMNS}
        lines.append("  largest |device - host| (frequencies in bins, everything else absolute): " +
                     ", ".join(f"{name} {v:.2g}" for name, v in worst.items()))
        del pcm
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
