"""Signals and segment lists shared by tests/test_measure_cpu.py and tests/test_measure_gpu.py (whisperseg_amd/measure.py).

Everything is made from fixed seeds.  Segments are laid out in SAMPLES (the lengths at which the kernels change path are sample
counts: one frame, a second frame, the seam between two chunks of 64 frames) and handed on as onset / offset seconds whose
sample_bounds give those samples back, which `prediction` asserts."""
import numpy as np

from whisperseg_amd.audio_utils import get_n_fft_given_sr
from whisperseg_amd.measure import sample_bounds

RATES = (16000, 48000, 96000, 250000, 400000)          # one per n_fft: 512, 1024, 2048, 4096, 8192
SILENT = (0.70, 0.75)                                   # seconds of `recording` that are exactly zero
SEED = 20251019


def chirps(sr, n, seed=SEED):
    """Gated linear chirps (20 .. 120 ms, random band below 0.45 sr, Hann-gated) on a floor of white noise 40 dB below them."""
    rng = np.random.default_rng(seed + sr)
    x = 0.003 * rng.standard_normal(n)
    pos = 0
    while True:
        pos += int(rng.uniform(0.005, 0.05) * sr)
        length = int(rng.uniform(0.02, 0.12) * sr)
        if pos + length >= n:
            break
        f0, f1 = rng.uniform(0.02, 0.45, 2) * sr
        t = np.arange(length) / sr
        phase = 2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / t[-1])
        x[pos:pos + length] += rng.uniform(0.1, 0.6) * np.hanning(length) * np.sin(phase)
        pos += length
    return x.astype(np.float32)


def tone(sr, k, n, amplitude=0.5):
    """A sine at the centre of bin k of the rate's n_fft."""
    n_fft = get_n_fft_given_sr(sr)
    return (amplitude * np.sin(2 * np.pi * k * np.arange(n) / n_fft)).astype(np.float32)


def white_noise(n, seed=SEED, amplitude=0.25):
    return (amplitude * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def silence(n):
    return np.zeros(n, np.float32)


def recording(sr):
    """One second of chirps on noise with the stretch SILENT zeroed."""
    x = chirps(sr, sr)
    x[int(SILENT[0] * sr):int(SILENT[1] * sr)] = 0.0
    return x


def structural_lengths(sr, seams=True):
    """The sample counts at which the code takes another path: 1 and 7 samples; around one frame; around the second frame; 63, 64
    (one sample short of 65, and exactly) and 65 frames — the seam of two chunks (seams=False: only the 65-frame one)."""
    n_fft = get_n_fft_given_sr(sr)
    hop = n_fft // 4
    out = [1, 7, n_fft - 1, n_fft, n_fft + 1, n_fft + hop, n_fft + hop + 1]
    return out + ([n_fft + 62 * hop, n_fft + 63 * hop - 1, n_fft + 63 * hop, n_fft + 63 * hop + 1, n_fft + 64 * hop] if seams
                  else [n_fft + 64 * hop])


def segments(sr, n=None, seed=SEED):
    """int64 [n_seg, 2] sample ranges in a recording of n (default sr) samples: every structural length and a dozen random lengths
    of 5 .. 400 ms at odd starts, then one segment from sample 0, one up to sample n, two overlapping ones, an empty one and one
    inside SILENT."""
    n = sr if n is None else n
    rng = np.random.default_rng(seed + 7 * sr)
    lengths = structural_lengths(sr) + [int(v * sr) for v in rng.uniform(0.005, 0.4, 12)]
    rows = []
    for length in lengths:
        s0 = int(rng.integers(0, (n - length) // 2)) * 2 + 1
        s0 = min(s0, n - length)
        rows.append((s0, s0 + length))
    a = int(0.03 * sr)
    rows += [(0, a + 1), (n - a - 3, n), (n // 3, n // 3 + 2 * a), (n // 3 + a, n // 3 + 3 * a + 5), (n // 2 + 1, n // 2 + 1),
             (int(SILENT[0] * sr) + 3, int(SILENT[0] * sr) + 3 + int(0.02 * sr))]
    return np.asarray(rows, dtype=np.int64)


def spaced_segments(sr, n=None, seed=SEED):
    """Segments that neither touch nor overlap, each with a sample of its own in front and behind (s0 >= 1, s1 < n, a gap of at
    least two samples): what the leak test poisons.  The structural lengths (one seam) and three random ones, back to back."""
    n = sr if n is None else n
    rng = np.random.default_rng(seed + 11 * sr)
    lengths = structural_lengths(sr, seams=False) + [int(v * sr) for v in rng.uniform(0.005, 0.1, 3)]
    rows, pos = [], 1
    for length in lengths:
        rows.append((pos, pos + length))
        pos += length + int(rng.integers(2, 9))
    assert pos < n
    return np.asarray(rows, dtype=np.int64)


def random_segments(sr, n, count, seed=SEED, ms=(5, 50)):
    """`count` random segments of ms[0] .. ms[1] milliseconds anywhere in n samples (overlaps as they fall)."""
    rng = np.random.default_rng(seed + count)
    length = (rng.uniform(ms[0], ms[1], count) * sr / 1000).astype(np.int64)
    s0 = (rng.uniform(0, 1, count) * (n - length)).astype(np.int64)
    return np.stack([s0, s0 + length], axis=1)


def prediction(bounds, sr, n):
    """{"onset", "offset"} in seconds whose sample_bounds are exactly `bounds`."""
    pred = {"onset": [int(s0) / sr for s0, _ in bounds], "offset": [int(s1) / sr for _, s1 in bounds]}
    for (s0, s1), on, off in zip(bounds, pred["onset"], pred["offset"]):
        assert sample_bounds(on, off, sr, n) == (s0, s1)
    return pred


# ---- tolerances of the device tests ------------------------------------------------------------------------------------------------
# The fp32 FFT is the device path's only inexact stage.  Its cost is measured WITHOUT the code under test: the host definition run
# a second time with the frames, the window and scipy.fft.rfft in float32 (everything behind the transform still float64), against
# the float64 run, over every case the device tests compare: recording(sr) x segments(sr), 26 / 27 non-silent segments per rate,
# and at 16 kHz the 1 + 257 + 1 000 random_segments in the band from 500 Hz (`fp32_spread` below re-measures it;
# tests/test_measure_cpu.py checks the constants against it).  Largest differences, per n_fft:
#               centroid      freq_05       freq_95      (bins)     spectral_entropy     power, relative to the band's maximum
#   512         6.3e-7        9.4e-7        1.8e-6                  5.2e-9               2.6e-7      segments(16000)
#   512         2.6e-6        3.8e-5        1.6e-4                  2.1e-8               3.3e-7      the random segments: short ones, whose
#                                                                   5 % / 95 % points fall into bins 60 dB below the band's total
#   1024        3.6e-6        1.1e-6        1.6e-6                  3.5e-9               2.3e-7
#   2048        6.7e-6        1.4e-5        7.8e-6                  5.1e-9               2.9e-7
#   4096        3.4e-6        1.9e-5        2.4e-5                  5.1e-9               2.7e-7
#   8192        1.6e-5        5.3e-6        4.1e-5                  3.8e-9               3.1e-7
# and the float32 run picked the float64 run's peak bin in all 1 367 cases.  A device column may differ from the definition's by
# FOUR times that spread (the kernel's butterfly order and twiddle rounding are not pocketfft's) plus what the float32 OUTPUT
# costs, which no spread of float64 values contains: the definition rounds a column once, the device path twice (the kernel's
# rate-free row, then the scaled column; entropy once) — 2 ulp of the expected float32, 1 for the entropy.
# The peak bin k must be a near-maximiser of the definition's float64 spectrum: P64[k] >= (1 - PEAK_TAU) max P64[band].  With
# every bin of the kernel's spectrum within e max P64 of P64, the bin that maximises the kernel's spectrum has
# P64[k] >= max P64 - 2 e max P64; e = 4 x the largest relative power spread above, so PEAK_TAU = 8 x 3.3e-7.
SPREAD = {        # n_fft: spread of (centroid_frequency, freq_05, freq_95) in bins, of spectral_entropy
    512: (2.6e-6, 3.8e-5, 1.6e-4, 2.1e-8),
    1024: (3.6e-6, 1.1e-6, 1.6e-6, 3.5e-9),
    2048: (6.7e-6, 1.4e-5, 7.8e-6, 5.1e-9),
    4096: (3.4e-6, 1.9e-5, 2.4e-5, 5.1e-9),
    8192: (1.6e-5, 5.3e-6, 4.1e-5, 3.8e-9),
}
RANDOM_RATE, RANDOM_COUNTS, RANDOM_MIN_FREQUENCY = 16000, (0, 1, 257, 1000), 500      # the device test of the segment counts
POWER_SPREAD = 3.3e-7
PEAK_TAU = 8 * POWER_SPREAD
SPREAD_COLUMNS = ("centroid_frequency", "freq_05", "freq_95", "spectral_entropy")


def tolerance(column, expected, sr):
    """Allowed |device - definition| of the float32 array `expected` of a spectral column: 4 x the fp32 spread + the output's ulps."""
    n_fft = get_n_fft_given_sr(sr)
    spread = SPREAD[n_fft][SPREAD_COLUMNS.index(column)]
    ulp = np.spacing(np.abs(np.asarray(expected, dtype=np.float32))).astype(np.float64)
    if column == "spectral_entropy":
        return 4 * spread + ulp
    return 4 * spread * sr / n_fft + 2 * ulp


def fp32_spread(sr):
    """Re-measures one line of the table above -> (centroid, freq_05, freq_95 in bins, entropy, relative power, peak bins moved)."""
    from whisperseg_amd import measure as M
    n_fft = get_n_fft_given_sr(sr)
    x = recording(sr)
    cases = [(segments(sr), 0)] + ([(random_segments(sr, len(x), count), RANDOM_MIN_FREQUENCY) for count in RANDOM_COUNTS] if sr == RANDOM_RATE else [])
    worst, power, moved = np.zeros(4), 0.0, 0
    for s0, s1, k in ((s0, s1, M.band_bins(sr, n_fft, low)) for rows, low in cases for s0, s1 in rows):
        p64 = M.power_spectrum(x, int(s0), int(s1), n_fft)
        if not p64[k[0]:k[1] + 1].sum() > 0:
            continue
        p32 = M.power_spectrum(x, int(s0), int(s1), n_fft, np.float32)
        c64, c32 = np.array(M.spectral_columns(p64, *k)), np.array(M.spectral_columns(p32, *k))
        worst = np.maximum(worst, np.abs(c64 - c32)[1:])
        power = max(power, np.abs(p32 - p64)[k[0]:k[1] + 1].max() / p64[k[0]:k[1] + 1].max())
        moved += int(c64[0] != c32[0])
    return (*worst, power, moved)
