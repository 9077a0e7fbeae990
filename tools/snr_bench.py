#!/usr/bin/env python3
"""What the per-segment signal-to-noise ratio costs on one MI355X (whisperseg_amd.snr: wseg_frame_energy_f32 and wseg_snr_rows_f64
on PCM that is resident in HBM), stage by stage.  Not on the product path.

    python tools/snr_bench.py [--host_seconds 600] [--out profiles/snr_ab.txt]

Four cases: 16 kHz (n_fft 512) and 250 kHz (n_fft 4096), recordings of 10 minutes and of one hour (seeded noise under a gated tone,
made on the device), 2 000 rows of 20 .. 200 ms.  Reported per case:
  * the track kernel: HIP-event time around wseg_frame_energy_f32, PCM resident and the track allocated — ms, frames per second
    and the bytes of PCM it reads per second;
  * wseg_logmel_f32 (extract_windows: its launch pair) over the same samples — windows of 1 000 columns at the default hop of
    2.5 ms laid end to end: the yardstick of what an FFT pass over a recording costs in this tree;
  * frame_energy_host on the same samples (recordings up to --host_seconds seconds; "not measured" beyond), and the largest
    difference of the two tracks relative to the largest energy;
  * the select: wseg_snr_rows_f64 with one row and ONE window over the whole track (the context=None shape: a split window) against
    torch.sort of the same track on the same GPU, and the two floors compared bit for bit;
  * the rows call as snr() makes it with a context of 2 s (a window per row, short ones);
  * wall time of snr() — frame ranges on the host, the launches, the rows' way back — with the PCM resident, as segment(snr=True)
    calls it.
One warm-up of each, then five repetitions; all five are printed, the median is the figure."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((16000, 600), (16000, 3600), (250000, 600), (250000, 3600))          # rate, seconds
ROWS = 2000
REPS = 5
FRONT_END_COLUMNS, FRONT_END_STEP = 1000, 0.0025


def device_recording(torch, sr, seconds, seed=5):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed + sr)
    n = int(sr * seconds)
    x = torch.randn(n, dtype=torch.float32, device="cuda", generator=gen).mul_(0.01)
    step = 1 << 24                                       # the tone in pieces: no second array of the recording's size
    for lo in range(0, n, step):
        t = torch.arange(lo, min(n, lo + step), dtype=torch.float64, device="cuda")
        x[lo:lo + step] += (0.3 * torch.sin(2 * np.pi * 0.11 * t) * (torch.sin(2 * np.pi * 3.0 / sr * t) > 0)).float()
    return x


def rows(seconds, count, seed=6):
    rng = np.random.default_rng(seed)
    length = rng.uniform(0.02, 0.2, count)
    onset = np.sort(rng.uniform(0, seconds - 0.2, count))
    return {"onset": onset.tolist(), "offset": (onset + length).tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host_seconds", type=float, default=600.0, help="the longest recording frame_energy_host is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snr_ab.txt"))
    args = ap.parse_args()
    import torch
    from whisperseg_amd import _lib, snr as S
    from whisperseg_amd.audio_utils import WhisperSegFeatureExtractor, get_n_fft_given_sr
    from whisperseg_amd.segments import bounds_of
    _lib.load(require_device=True)
    lines = [f"per-segment signal-to-noise ratio ({torch.cuda.get_device_name(0)}; warm-up, then {REPS} repetitions; times in ms)"]

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    def five(fn):
        fn()
        return [fn() for _ in range(REPS)]

    fmt = lambda v: " ".join(f"{t:.3f}" for t in v)      # noqa: E731
    med = statistics.median
    for sr, seconds in CASES:
        n_fft = get_n_fft_given_sr(sr)
        print(f"sr {sr}, {seconds} s ...", flush=True)
        pcm = device_recording(torch, sr, seconds)
        n = int(pcm.numel())
        J = S.frame_count(n, n_fft)
        pred = rows(seconds, ROWS)
        bounds = bounds_of(pred, sr, n)
        track = torch.empty(J, dtype=torch.float32, device="cuda")
        t_track = five(lambda: timed(lambda: S.frame_energy(pcm, sr, out=track)))
        extractor = WhisperSegFeatureExtractor(sr, FRONT_END_STEP, n_cols=FRONT_END_COLUMNS, device="cuda")
        win_len = FRONT_END_COLUMNS * extractor.hop_length
        n_windows = max(1, n // win_len)
        win_start = torch.arange(n_windows, dtype=torch.int64) * win_len
        t_front = five(lambda: timed(lambda: extractor.extract_windows(pcm, win_start, win_len)))
        whole_t, whole_w = np.array([[0, 1, 0]], np.int64), np.array([[0, J, S.frame_ranges(bounds[:1], n, n_fft, sr)[1][0][2]]], np.int64)
        out1 = torch.empty((1, 3), dtype=torch.float64, device="cuda")
        t_select = five(lambda: timed(lambda: S.snr_rows(track, whole_t, whole_w, out=out1)))
        t_sort = five(lambda: timed(lambda: torch.sort(track)))
        floor_sort = torch.sort(track)[0][int(whole_w[0, 2])].item()
        same = np.float32(out1[0, 2].item()).tobytes() == np.float32(floor_sort).tobytes()
        ctx_t, ctx_w = S.frame_ranges(bounds, n, n_fft, sr, 0.1, 2.0)
        outn = torch.empty((ROWS, 3), dtype=torch.float64, device="cuda")
        t_rows = five(lambda: timed(lambda: S.snr_rows(track, ctx_t, ctx_w, out=outn)))

        def wall():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S.snr(pcm, sr, pred)
            return (time.perf_counter() - t0) * 1e3

        t_wall = five(wall)
        lines.append(f"sr {sr} (n_fft {n_fft}), {seconds} s: {n} samples, {J} frames, {ROWS} rows")
        lines.append(f"  wseg_frame_energy_f32 (HIP events)      median {med(t_track):9.3f}   [{fmt(t_track)}]   {J / med(t_track) / 1e3:.2f} M frames/s, "
                     f"{4 * n / med(t_track) / 1e6:.1f} GB/s of PCM")
        lines.append(f"  wseg_logmel_f32 over the same samples   median {med(t_front):9.3f}   [{fmt(t_front)}]   ({n_windows} windows of {FRONT_END_COLUMNS} columns)")
        if seconds <= args.host_seconds:
            x = pcm.cpu().numpy()
            t0 = time.perf_counter()
            want = S.frame_energy_host(x, sr)
            t_host = (time.perf_counter() - t0) * 1e3
            err = float(np.abs(track.cpu().numpy().astype(np.float64) - want).max() / want.max())
            lines.append(f"  frame_energy_host (one run)                    {t_host:9.1f}   host / device: {t_host / med(t_track):.0f}x; largest |device - host| / max E: {err:.2g}")
            del x
        else:
            lines.append("  frame_energy_host                       not measured")
        lines.append(f"  select, one window of {J} frames         median {med(t_select):9.3f}   [{fmt(t_select)}]")
        lines.append(f"  torch.sort of the same track            median {med(t_sort):9.3f}   [{fmt(t_sort)}]   sort / select: {med(t_sort) / med(t_select):.2f}x; "
                     f"the floors are {'bit-equal' if same else 'DIFFERENT'}")
        lines.append(f"  rows call, {ROWS} rows, context 2 s        median {med(t_rows):9.3f}   [{fmt(t_rows)}]   ({len(ctx_w)} windows of up to {int((ctx_w[:, 1] - ctx_w[:, 0]).max())} frames)")
        lines.append(f"  snr(), PCM resident (wall)              median {med(t_wall):9.3f}   [{fmt(t_wall)}]")
        del pcm, track
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
