"""Recordings, frame tables, select arrays and tolerances shared by tests/test_snr_cpu.py and tests/test_snr_gpu.py
(whisperseg_amd/snr.py).  Everything is made from fixed seeds, computed once and handed out read-only."""
import functools

import numpy as np

import measure_cases as MC
from whisperseg_amd import measure as M
from whisperseg_amd import snr as S
from whisperseg_amd.audio_utils import get_n_fft_given_sr

RATES = MC.RATES                                         # one per n_fft: 512, 1024, 2048, 4096, 8192
SEED = 20261021
FLOOR = 0.002                                            # amplitude of the white-noise floor under measure_cases.recording
SPLIT = S.SPLIT                                          # the plan's split constant: longer windows are shared by workgroups


@functools.lru_cache(maxsize=None)
def recording(sr):
    """measure_cases.recording(sr) — one second of chirps with a stretch of digital silence — over a white-noise floor, so that
    no frame is exactly zero."""
    x = MC.recording(sr).astype(np.float64) + FLOOR * np.random.default_rng(SEED + sr).standard_normal(sr)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def bands(sr):
    """(min_frequency, max_frequency) of the three bands of the track tests: full, from 500 Hz, one bin wide."""
    n_fft = get_n_fft_given_sr(sr)
    k = n_fft // 5
    return ((0, None), (500, None), (k * sr / n_fft, k * sr / n_fft))


def track_lengths(sr):
    """The sample counts of the track tests: no frame, one, still one, two, about 40."""
    n_fft = get_n_fft_given_sr(sr)
    hop = n_fft // 4
    return (n_fft - 1, n_fft, n_fft + hop - 1, n_fft + hop, n_fft + 39 * hop + 17)


@functools.lru_cache(maxsize=None)
def total_power(sr, n=None):
    """P_tot float64 [J]: the whole one-sided power of every frame of recording(sr)[:n]."""
    n_fft = get_n_fft_given_sr(sr)
    out = S.frame_band_energy(recording(sr)[:n], n_fft, 0, n_fft // 2)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def energy64(sr, band, n=None):
    """The track of recording(sr)[:n] in bands(sr)[band] BEFORE its rounding to float32: float64 [J]."""
    n_fft = get_n_fft_given_sr(sr)
    out = S.frame_band_energy(recording(sr)[:n], n_fft, *M.band_bins(sr, n_fft, *bands(sr)[band]))
    out.setflags(write=False)
    return out


# ---- the tolerance of a device track ------------------------------------------------------------------------------------------------
# The fp32 FFT is the device track's only inexact stage.  Its cost is measured WITHOUT the code under test: frame_energy_host run
# with the frames, the window and scipy.fft.rfft in float32 against the float64 run, over recording(sr) in the three bands, as the
# largest |E32[j] - E64[j]| / P_tot[j] — relative to the frame's WHOLE one-sided power, because the error of an fp32 transform
# scales with the frame and not with a narrow band's share of it.  `fp32_spread` re-measures a line; tests/test_snr_cpu.py checks
# the constants against it (within a factor: pocketfft's vector width differs between CPUs).  A device value may differ from the
# float64 definition by delta_j = 4 x spread x P_tot[j] + 1 ulp of the float32 it rounds to: the factor 4 is the project's margin
# for a butterfly order and twiddle rounding that are not pocketfft's (tests/measure_cases.py).
FP32_SPREAD = {16000: 1.4e-7, 48000: 1.4e-7, 96000: 1.3e-7, 250000: 1.5e-7, 400000: 1.3e-7}


def fp32_spread(sr):
    """Re-measures FP32_SPREAD[sr]."""
    worst = 0.0
    for band, (lo, hi) in enumerate(bands(sr)):
        e32 = S.frame_energy_host(recording(sr), sr, lo, hi, fft_dtype=np.float32).astype(np.float64)
        worst = max(worst, float((np.abs(e32 - energy64(sr, band)) / total_power(sr)).max()))
    return worst


def delta(sr, band, n=None):
    """delta_j float64 [J] of recording(sr)[:n] in bands(sr)[band]."""
    ulp = np.spacing(energy64(sr, band, n).astype(np.float32)).astype(np.float64)
    return 4 * FP32_SPREAD[sr] * total_power(sr, n) + ulp


# ---- the end-to-end intervals -------------------------------------------------------------------------------------------------------
def segments(sr):
    """The rows of the end-to-end test: measure_cases.segments — every structural length, rows at sample 0 and up to n, overlapping
    ones, an empty one, one inside the zeroed stretch — which hold rows shorter than a frame too."""
    return MC.segments(sr)


def column_intervals(sr, band, bounds, quantile, context):
    """(lo, hi): dicts of float64 [n_seg] per column, the interval every device column must lie in.  Order statistics, means and
    maxima are monotone in every element, so a track within +-delta of E64 gives N, S and M between those of E64 - delta and of
    E64 + delta; a ratio is smallest at (lowest numerator, highest denominator).  Each end is widened by 2 ulp of its float32."""
    n_fft = get_n_fft_given_sr(sr)
    x = recording(sr)
    e, d = energy64(sr, band), delta(sr, band)
    table, windows = S.frame_ranges(bounds, len(x), n_fft, sr, quantile, context)
    raw_lo, raw_hi = (rows64(v, table, windows) for v in (np.maximum(e - d, 0.0), e + d))
    ref = S.reference_energy(n_fft)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = lambda v: 10.0 * np.log10(v)                                                # noqa: E731
        lo = {"signal_level_db": db(raw_lo[:, 0] / ref), "noise_level_db": db(raw_lo[:, 2] / ref),
              "snr_db": db(raw_lo[:, 0] / raw_hi[:, 2]), "peak_snr_db": db(raw_lo[:, 1] / raw_hi[:, 2])}
        hi = {"signal_level_db": db(raw_hi[:, 0] / ref), "noise_level_db": db(raw_hi[:, 2] / ref),
              "snr_db": db(raw_hi[:, 0] / raw_lo[:, 2]), "peak_snr_db": db(raw_hi[:, 1] / raw_lo[:, 2])}
    for c in S.COLUMNS:
        lo[c] = lo[c] - 2 * ulp32(lo[c])
        hi[c] = hi[c] + 2 * ulp32(hi[c])
    return lo, hi


def ulp32(v):
    """The spacing of float32 at the float64 values v; 0 at an infinite or NaN end, which no widening moves."""
    v = np.asarray(v, dtype=np.float64)
    finite = np.isfinite(v)
    return np.where(finite, np.spacing(np.abs(np.where(finite, v, 0.0)).astype(np.float32)).astype(np.float64), 0.0)


def rows64(track, table, windows):
    """rows_host's (S, M, N) of a FLOAT64 track (the ends of the intervals are not float32 values)."""
    out = np.full((len(table), 3), np.nan)
    for row, (j0, j1, w) in zip(out, table):
        if j1 > j0:
            w0, w1, r = windows[w]
            row[:] = track[j0:j1].mean(), track[j0:j1].max(), np.sort(track[w0:w1])[r]
    return out


# ---- the arrays of the select tests -------------------------------------------------------------------------------------------------
SELECT_LENGTHS = (1, 2, 255, 256, 257, SPLIT - 1, SPLIT, SPLIT + 1, 3 * SPLIT)
QUANTILES = (0.0, 0.1, 0.5, 1.0)
VALUE_FAMILIES = ("random", "all equal", "half ties", "zeros", "denormals", "inf", "nan", "lowest byte")


def select_values(family, length, seed=SEED):
    """float32 [length] of one family: non-negative values, +inf and NaN of both signs — what a band-energy track may hold."""
    rng = np.random.default_rng(seed + length + 31 * VALUE_FAMILIES.index(family))
    v = (rng.standard_normal(length) ** 2 * 10.0 ** rng.uniform(-6, 6, length)).astype(np.float32)
    if family == "all equal":
        v[:] = np.float32(0.37)
    elif family == "half ties":
        v[rng.random(length) < 0.5] = np.float32(1.25)
    elif family == "zeros":
        v[rng.random(length) < 0.7] = 0.0
    elif family == "denormals":
        v = rng.integers(0, 1 << 23, length).astype(np.uint32).view(np.float32).copy()      # (0 and every denormal pattern)
        v[::3] = np.float32(1e-30)
    elif family == "inf":
        v[rng.random(length) < 0.3] = np.inf
    elif family == "nan":
        bad = rng.random(length) < 0.3
        v.view(np.uint32)[bad] = np.where(rng.random(int(bad.sum())) < 0.5, 0x7fc00000, 0xffc00001).astype(np.uint32)
    elif family == "lowest byte":
        v = (np.uint32(0x3f800000) + rng.integers(0, 256, length).astype(np.uint32)).view(np.float32).copy()
    return v


def rank(q, length):
    return int(np.floor(q * (length - 1)))


def same_value(got, want):
    """Whether float64 `got` (the device's N) is float32 `want` (np.sort(window)[r]) bit for bit; any NaN equals any NaN: numpy.sort
    orders every NaN last and says nothing about which of them comes first."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return both_nan | (got.astype(np.float32).view(np.uint32) == want.view(np.uint32)) & (got == want.astype(np.float64))
