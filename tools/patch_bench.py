#!/usr/bin/env python3
"""What the per-segment log-mel patches cost on one MI355X (whisperseg_amd.patches: wseg_patches_f32 on PCM that is resident in
HBM), against the front-end on the same number of frames of the same n_fft and against the host definition on the same rows.
Not on the product path.

    python tools/patch_bench.py [--seconds 600] [--out profiles/patch_ab.txt]

Two cases: 16 kHz (n_fft 512), 10 000 segments of 20 .. 200 ms at width 32; 250 kHz (n_fft 4096), 2 000 segments at width 64 — in
a recording of --seconds seconds (seeded noise under a gated tone).  Reported per case:
  * the kernel pair: HIP-event time around the one call that enqueues the bounds' copy and both kernels, PCM resident and the
    output allocated — ms per call and frames transformed per second;
  * wseg_logmel_f32 (extract_windows: its launch pair) on as many frames of that n_fft — windows of 1 000 columns at the default
    hop of 2.5 ms: the yardstick of what an FFT + mel frame costs in this tree — and the ratio of the two times per frame;
  * wall time of patches() — bounds on the host, the launch pair, the pictures' way back — with the PCM resident, as
    segment(patches=W) calls it;
  * wall time of patches_host on the same rows, the PCM already in host memory.
One warm-up of each, then five repetitions; all five are printed, the median is the figure.  The pictures of both sides are
compared once (largest difference)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((16000, 10000, 32), (250000, 2000, 64))          # rate, segments, width
REPS = 5
FRONT_END_COLUMNS, FRONT_END_STEP = 1000, 0.0025


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
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_ab.txt"))
    args = ap.parse_args()
    import torch
    from whisperseg_amd import _lib, measure as M, patches as P
    from whisperseg_amd.audio_utils import WhisperSegFeatureExtractor, get_n_fft_given_sr
    _lib.load(require_device=True)
    lines = [f"per-segment log-mel patches in {args.seconds:g} s of PCM ({torch.cuda.get_device_name(0)}; warm-up, then {REPS} repetitions; times in ms)"]
    for sr, count, width in CASES:
        n_fft = get_n_fft_given_sr(sr)
        print(f"sr {sr} ...", flush=True)
        x = recording(sr, args.seconds)
        pred = rows(sr, args.seconds, count)
        pcm = torch.from_numpy(x).cuda()
        bounds = M.bounds_of(pred, sr, len(x))
        tables = P.device_tables(sr, 0, None, pcm.device)
        frames = count * width
        out = torch.empty((count, 80, width), dtype=torch.float32, device=pcm.device)
        # the front-end on as many frames: windows of 1 000 columns, laid over the recording one after the other (wrapping round)
        extractor = WhisperSegFeatureExtractor(sr, FRONT_END_STEP, n_cols=FRONT_END_COLUMNS, device="cuda")
        win_len = FRONT_END_COLUMNS * extractor.hop_length
        n_windows = -(-frames // FRONT_END_COLUMNS)
        win_start = (torch.arange(n_windows, dtype=torch.int64) * win_len) % max(len(x) - win_len, 1)

        def timed(fn):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)

        kernels = lambda: timed(lambda: P.patch_rows(pcm, bounds, tables, width, out=out))
        front_end = lambda: timed(lambda: extractor.extract_windows(pcm, win_start, win_len))

        def device():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = P.patches(pcm, sr, pred, width=width)
            return (time.perf_counter() - t0) * 1e3, got

        def host():
            t0 = time.perf_counter()
            got = P.patches_host(x, sr, pred, width=width)
            return (time.perf_counter() - t0) * 1e3, got

        kernels(), front_end(), device(), host()         # warm-up: tables, allocator, page faults
        t_kernel, t_front, t_device, t_host = [], [], [], []
        for _ in range(REPS):
            t_kernel.append(kernels())
            t_front.append(front_end())
            ms, got = device()
            t_device.append(ms)
            ms, want = host()
            t_host.append(ms)
        fmt = lambda v: " ".join(f"{t:.2f}" for t in v)
        med = statistics.median
        front_frames = n_windows * FRONT_END_COLUMNS
        per_patch, per_front = med(t_kernel) / frames, med(t_front) / front_frames
        lines.append(f"sr {sr} (n_fft {n_fft}): {count} segments of 20 .. 200 ms, width {width}: {frames} frames")
        lines.append(f"  kernel pair (HIP events)        median {med(t_kernel):9.2f}   [{fmt(t_kernel)}]   {frames / med(t_kernel) / 1e3:.2f} M frames/s")
        lines.append(f"  wseg_logmel_f32, {front_frames} frames  median {med(t_front):9.2f}   [{fmt(t_front)}]   {front_frames / med(t_front) / 1e3:.2f} M frames/s")
        lines.append(f"  a patch frame costs {per_patch / per_front:.2f}x a front-end frame")
        lines.append(f"  patches(), PCM resident         median {med(t_device):9.2f}   [{fmt(t_device)}]")
        lines.append(f"  patches_host                    median {med(t_host):9.2f}   [{fmt(t_host)}]")
        lines.append(f"  host / device wall: {med(t_host) / med(t_device):.0f}x")
        lines.append(f"  largest |device - host| of a normalised value: {float(np.abs(got.astype(np.float64) - want).max()):.2g}")
        del pcm, out
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
