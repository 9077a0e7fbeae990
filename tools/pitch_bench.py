#!/usr/bin/env python3
"""A/B of the per-segment pitch contour on one MI355X: the device path (whisperseg_amd.pitch.pitch: wseg_pitch_frames_f64 on PCM
that is resident in HBM) against the host definition (pitch_host: numpy float64, a loop over the terms of YIN's difference
function, vectorised over lags and frames) on the same rows.  Not on the product path.

    python tools/pitch_bench.py [--segments 10000] [--seconds 600] [--out profiles/pitch_ab.txt]

tools/measure_bench.py's workload: for each of two rates, 16 kHz (the default range: lags 8 .. 256, hop 128) and 250 kHz (lags
8 .. 2048, hop 1024), a recording of --seconds seconds (seeded noise under a gated tone) and --segments random segments of
20 .. 200 ms.  Reported per rate:
  * the kernel alone: HIP-event time around the one call that enqueues the table's copy and the kernel, PCM resident — a warm-up,
    then five repetitions: the median, min .. max, and the achieved terms (x[i] - x[i + tau])^2 per second against the fp64 vector
    rate of the data sheet (78.6 TFLOP/s counts a fused multiply-add as two; a term is a subtraction, a multiplication and an
    addition that must round separately, three instructions: 13.1 T terms/s at most);
  * wall time of pitch() — bounds on the host, the launch, the frames' way back, the columns — with the PCM resident, as
    segment(pitch=True) calls it: a warm-up, then five repetitions;
  * wall time of pitch_host on the FIRST --host_segments rows only (the whole workload would take minutes at 16 kHz and an hour at
    250 kHz), once after a warm-up on a tenth of them, and that time scaled up by the ratio of the frame counts.  The file says so.
The frames of both sides on that subset are compared once: they must be equal bit for bit."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.measure_bench import recording, rows  # noqa: E402

RATES = ((16000, 1000), (250000, 20))                # (rate, rows of the host subset)
REPS = 5
FP64_VECTOR_TFLOPS = 78.6                            # MI355X data sheet, vector fp64, an FMA counted as two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_ab.txt"))
    args = ap.parse_args()
    import torch
    from whisperseg_amd import _lib, measure as M, pitch as P
    _lib.load(require_device=True)
    peak_terms = FP64_VECTOR_TFLOPS / 2 / 3
    lines = [f"per-segment pitch contour, device against host: {args.segments} segments of 20 .. 200 ms in {args.seconds:g} s "
             f"({torch.cuda.get_device_name(0)}; warm-up, then {REPS} repetitions; times in ms)"]
    for sr, host_rows in RATES:
        print(f"sr {sr} ...", flush=True)
        tau_min, tau_max = P.lag_range(sr)
        hop = P.default_hop(sr)
        x = recording(sr, args.seconds)
        pred = rows(sr, args.seconds, args.segments)
        pcm = torch.from_numpy(x).cuda()
        bounds = M.bounds_of(pred, sr, len(x))
        frames = int(P.frame_offsets_of(bounds, tau_max, hop)[-1])
        terms = frames * tau_max * tau_max

        def kernel():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            P.pitch_rows(pcm, bounds, tau_min, tau_max, hop)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)

        def device():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = P.pitch(pcm, sr, pred)
            return (time.perf_counter() - t0) * 1e3, got

        kernel(), device()                               # warm-up: allocator, staging buffer
        t_kernel = [kernel() for _ in range(REPS)]
        t_device = [device()[0] for _ in range(REPS)]
        host_rows = min(host_rows, len(bounds))
        subset = bounds[:host_rows]
        P.frames_host(x, subset[:max(1, host_rows // 10)], tau_min, tau_max, hop)      # warm-up
        t0 = time.perf_counter()
        want, offsets = P.frames_host(x, subset, tau_min, tau_max, hop)
        t_host = (time.perf_counter() - t0) * 1e3
        got = P.pitch_rows(pcm, subset, tau_min, tau_max, hop)[0].cpu().numpy()
        same = np.array_equal(got.view(np.uint32), want.view(np.uint32))
        fmt = lambda v: " ".join(f"{t:.2f}" for t in v)
        med = statistics.median
        scaled = t_host * frames / max(1, len(want))
        lines.append(f"sr {sr} (lags {tau_min} .. {tau_max}, hop {hop}): {len(bounds)} segments, {frames} frames, {terms:.3g} terms")
        lines.append(f"  kernel (HIP events)        median {med(t_kernel):9.2f}   min .. max {min(t_kernel):.2f} .. {max(t_kernel):.2f}   [{fmt(t_kernel)}]")
        lines.append(f"                             {frames / med(t_kernel) / 1e3:.3f} M frames/s, {terms / med(t_kernel) / 1e9:.2f} T terms/s = "
                     f"{100 * terms / med(t_kernel) / 1e9 / peak_terms:.0f} % of the {peak_terms:.1f} T terms/s the data sheet's {FP64_VECTOR_TFLOPS} TFLOP/s allow")
        lines.append(f"  pitch(), PCM resident      median {med(t_device):9.2f}   [{fmt(t_device)}]")
        lines.append(f"  pitch_host, the first {host_rows} rows ({len(want)} frames), once: {t_host:.0f} ms; scaled by the frame counts to all rows: {scaled / 1e3:.0f} s")
        lines.append(f"  host (scaled) / device wall: {scaled / med(t_device):.0f}x;  device frames == host frames on the subset, bit for bit: {same}")
        del pcm
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
