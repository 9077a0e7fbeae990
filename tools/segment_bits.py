#!/usr/bin/env python3
"""SHA-256 of the raw device output of the three per-segment analyses that read a recording's resident PCM — measurements, log-mel
patches, pitch — over the case sets of their device tests, at the default grid and at a grid cap of 1 and of 3.  Two commits whose
listings are equal compute the same bits: the device tests of the measurements and the patches compare within a tolerance and
would not notice a changed rounding.  Not on the product path.

    python tools/segment_bits.py [--out FILE]

  measure   tests/measure_cases.py: recording(sr) x segments(sr) at every rate of RATES, the whole band
  patch     tests/patch_cases.py: recording(sr) x rows_for(sr, width) at every rate, every width of widths(sr)
  pitch     tests/pitch_cases.py: all_cases()"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def digest(tensor):
    return hashlib.sha256(tensor.cpu().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import measure_cases as MC
    import patch_cases as PC
    import pitch_cases as TC
    from whisperseg_amd import measure as M, patches as P, pitch as Y
    from whisperseg_amd.audio_utils import get_n_fft_given_sr
    lines = []
    for cap in ("", "1", "3"):
        for knob in ("WSEG_MEASURE_GRID", "WSEG_PATCH_GRID", "WSEG_PITCH_GRID"):
            os.environ.pop(knob, None)
            if cap:
                os.environ[knob] = cap
        grid = "grid " + (cap or "default")
        for sr in MC.RATES:
            n_fft = get_n_fft_given_sr(sr)
            pcm = torch.from_numpy(MC.recording(sr)).cuda()
            rows = M.measure_rows(pcm, MC.segments(sr), n_fft, *M.band_bins(sr, n_fft))
            lines.append(f"{grid}  measure sr {sr}: {digest(rows)}")
            for width in PC.widths(sr):
                pictures = P.patch_rows(pcm, PC.rows_for(sr, width), P.device_tables(sr, device=pcm.device), width)
                lines.append(f"{grid}  patch sr {sr} width {width}: {digest(pictures)}")
        for c in TC.all_cases():
            frames, _ = Y.pitch_rows(torch.from_numpy(np.array(c.x)).cuda(), c.bounds, c.tau_min, c.tau_max, c.hop, c.threshold)
            lines.append(f"{grid}  pitch {c.name}: {digest(frames)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
