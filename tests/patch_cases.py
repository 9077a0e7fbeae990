"""Recordings, segment lists and tolerances shared by tests/test_patch_cpu.py and tests/test_patch_gpu.py (whisperseg_amd/patches.py).

Signals and the general segment lists are tests/measure_cases.py's; added here are the segments at which the patch kernel can go
wrong — lengths around the width (several columns on one centre), segments whose frames reach outside the recording on either
side, overlapping ones, and a recording shorter than one frame."""
import numpy as np

import measure_cases as MC
from whisperseg_amd import patches as P
from whisperseg_amd.audio_utils import get_n_fft_given_sr

RATES = MC.RATES                                  # one per n_fft: 512, 1024, 2048, 4096, 8192
WIDTHS = (1, 2, 5, 32, 64)                        # at every rate
WIDE = 256                                        # only at WIDE_RATES
WIDE_RATES = (16000, 400000)
SHORT_N = 100                                     # a recording shorter than every n_fft
BAND_RATE, BAND_WIDTH, BAND_MIN_FREQUENCY = 16000, 32, 2000      # the second band of the device tests (the first is 0 .. sr / 2)
# A third band, 0 .. 1000 Hz at 16 kHz: its 80 Slaney filters lie 12.3 Hz apart, a bin is 31.25 Hz wide, so most filters hold one bin
# and many hold none (from 0 Hz to sr / 2 every filter of every rate of the ladder spans at least two bins: none is empty there).
NARROW_BAND = (0, 1000)


def widths(sr):
    return WIDTHS + ((WIDE,) if sr in WIDE_RATES else ())


def structural(sr, width, n=None):
    """int64 [*, 2]: L = 0, 1, W - 1, W, W + 1, an odd L and a long odd L at odd starts; a segment at sample 0 and one ending at n,
    and empty ones at 0 and at n (their frames reach n_fft / 2 samples outside the recording); two overlapping segments."""
    n = sr if n is None else n
    rows = []
    for i, length in enumerate((0, 1, max(width - 1, 0), width, width + 1, 2 * width + 1, 1001)):
        s0 = n // 4 + 37 * i + 1
        rows.append((s0, s0 + length))
    rows += [(0, width + 3), (n - width - 2, n), (0, 0), (n, n), (n // 2, n // 2 + 901), (n // 2 + 450, n // 2 + 1351)]
    return np.asarray(rows, dtype=np.int64)


def rows_for(sr, width):
    """The rows the device tests compare at (sr, width) in recording(sr): the structural ones, then measure_cases.segments(sr)."""
    return np.concatenate([structural(sr, width), MC.segments(sr)])


def short_recording(sr):
    return MC.recording(sr)[:SHORT_N].copy()


def short_rows():
    return np.asarray([(0, SHORT_N), (0, 0), (SHORT_N, SHORT_N), (30, 71), (99, 100), (0, 1)], dtype=np.int64)


def compared_cases(sr):
    """Every (recording, rows, width, min_frequency, max_frequency) the device tests hold against the definition at this rate."""
    x = MC.recording(sr)
    cases = [(x, rows_for(sr, w), w, 0, None) for w in widths(sr)]
    cases += [(short_recording(sr), short_rows(), w, 0, None) for w in (1, 5, 32)]
    if sr == BAND_RATE:
        cases.append((x, rows_for(sr, BAND_WIDTH), BAND_WIDTH, BAND_MIN_FREQUENCY, None))
    return cases


def narrow_cases():
    """The device test of empty filters: the band NARROW_BAND at BAND_RATE.  Kept apart from compared_cases, with a constant of its
    own (NARROW_SPREAD): the chirps lie above the band, so its values sit 60 .. 80 dB below their frame's strongest bins, where fp32
    butterflies cost ten times what they cost the full band — that must not widen the tolerance of every other case at n_fft 512."""
    return [(MC.recording(BAND_RATE), rows_for(BAND_RATE, BAND_WIDTH), BAND_WIDTH, *NARROW_BAND)]


# ---- tolerance of the device tests -------------------------------------------------------------------------------------------------
# The fp32 transform and the float32 bank are the device path's only inexact stages; log10, clamp and scale are 1-Lipschitz into
# the normalised value apart from the / 4.  Their cost is measured WITHOUT the code under test: the definition run with frames,
# window and scipy.fft.rfft in float32 and the bank rounded to float32 (everything behind the transform float64) against the
# float64 run, both normalised in float64 (no output rounding in the figure), over exactly compared_cases(sr).  Largest difference
# of a normalised value, measured here (`fp32_spread` re-measures a line; tests/test_patch_cpu.py holds the constants against it):
#       sr         n_fft     largest spread
#       16 000     512       2.2e-5
#       48 000     1024      1.5e-5
#       96 000     2048      1.3e-5
#       250 000    4096      2.2e-5
#       400 000    8192      1.5e-5
# SPREAD holds those figures times about 1.35: pocketfft's vector width differs between CPUs and the constant must stay at or above what a
# host re-measures (and below twice it).  A device value may differ from the definition's by FOUR times the spread (the kernel's
# butterfly order and twiddle rounding are not pocketfft's, its mel sum is an fp32 fmaf chain) plus 2 ulp of the expected float32:
# the device rounds v and the scaled value, the definition rounds once.
# narrow_cases(), measured the same way: 2.4e-4.
NARROW_SPREAD = 3.3e-4
SPREAD = {512: 3.0e-5, 1024: 2.0e-5, 2048: 1.8e-5, 4096: 3.0e-5, 8192: 2.1e-5}


def tolerance(expected, sr, spread=None):
    """Allowed |device - definition| for the float32 array `expected`: 4 x the fp32 spread (the rate's, unless one is given) + 2 ulp."""
    ulp = np.spacing(np.abs(np.asarray(expected, dtype=np.float32))).astype(np.float64)
    return 4 * (SPREAD[get_n_fft_given_sr(sr)] if spread is None else spread) + 2 * ulp


def normalise64(v):
    return (np.maximum(v, v.max() - 8.0) + 4.0) / 4.0


def fp32_spread(sr, cases=None):
    """Re-measures one line of the table above: the largest |float32 run - float64 run| of a normalised value over compared_cases(sr)
    (or over `cases` at that rate)."""
    n_fft = get_n_fft_given_sr(sr)
    worst = 0.0
    for x, rows, width, low, high in (compared_cases(sr) if cases is None else cases):
        fb = P.filterbank(sr, n_fft, low, high)
        fb32 = fb.astype(np.float32).astype(np.float64)
        for s0, s1 in rows:
            centres = P.column_centres(s0, s1, width)
            a = normalise64(P.log_mel_columns(x, centres, n_fft, fb))
            b = normalise64(P.log_mel_columns(x, centres, n_fft, fb32, np.float32))
            worst = max(worst, float(np.abs(a - b).max()))
    return worst
