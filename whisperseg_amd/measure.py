"""Per-segment acoustic measurements: the table a segmenter's users compute next, one line per detected call.

`measure_host` is THE definition (numpy, float64) and the oracle of every device test, as wavio.load_audio is for the ingest;
`measure` computes the same eight columns on the GPU from PCM that is already resident there (wseg_measure_segments_f32:
whisperseg_amd/csrc/wseg_measure.hip), one launch pair per recording.  `SegmenterBase.segment*(..., measure=True)` adds the
columns to every prediction dict, measured on the device PCM the front-end used.

For a mono recording x (float32 [n]) at rate sr and a segment (onset, offset) in seconds:

  sample range   s0 = clamp(floor(onset sr + 0.5), 0, n),  s1 = max(s0, clamp(floor(offset sr + 0.5), 0, n))      (sample_bounds:
                 Python floats on the host; the device gets int64 and does no time arithmetic)
  time domain    over x[s0:s1]: peak_amplitude = max |x| (the float32's bits), rms = sqrt(mean x^2), zero_crossing_rate = the
                 number of i in (s0, s1) with (x[i] < 0) != (x[i - 1] < 0), divided by (s1 - s0) / sr; x[s0 - 1] is never looked at
  spectrum       n_fft = get_n_fft_given_sr(sr), hop = n_fft / 4, the front-end's periodic Hann window; frame j is
                 x[s0 + j hop : s0 + j hop + n_fft] with every sample at or behind s1 replaced by zero; J = 1 frame for
                 s1 - s0 <= n_fft, else 1 + ceil((s1 - s0 - n_fft) / hop);  P[k] = sum_j |rfft(w frame_j)[k]|^2, k = 0 .. n_fft / 2
  band           k_lo = max(1, ceil(min_frequency n_fft / sr)) (DC is never in it), k_hi = min(n_fft / 2, floor(max_frequency
                 n_fft / sr)), max_frequency None = sr / 2 (band_bins);  B = P[k_lo .. k_hi], T = sum B
  spectral       peak_frequency = k sr / n_fft for the lowest k that maximises B;  centroid_frequency = sum k B[k] / T sr / n_fft;
                 freq_05 / freq_95: with C the running sum of B and k the first bin with C[k] >= q T,
                 (k - 0.5 + (q T - C[k - 1]) / B[k]) sr / n_fft — interpolated inside the crossing bin (bin k spans k -+ 0.5), so
                 that it is a continuous function of P;  spectral_entropy = -sum p ln p / ln(len(B)), p = B / T, over p > 0
  conventions    s1 == s0: all eight NaN.  T == 0 (silence; one sample, because w[0] = 0): the five spectral columns NaN, the
                 three time-domain ones as computed.  k_lo > k_hi: ValueError before anything runs.
"""
import ctypes as C
import math

import numpy as np

from . import _lib, resident as RS
from .audio_utils import get_n_fft_given_sr
from .segments import bounds_of, device_pcm, sample_bounds  # noqa: F401 (bounds_of, sample_bounds: re-exported)

COLUMNS = ("peak_amplitude", "rms", "zero_crossing_rate", "peak_frequency", "centroid_frequency", "freq_05", "freq_95",
           "spectral_entropy")
CHUNK_FRAMES = 64             # frames of a segment per work item of the first kernel (csrc/wseg_measure_plan.h::kMeasureChunkFrames)
_FRAME_BLOCK = 256            # frames measure_host transforms at a time (bounds its memory, nothing else)


def hann_periodic(n):
    """The front-end's window (oracle.frontend.hann_periodic, HF window_function(n, 'hann')): np.hanning(n + 1)[:-1], float64."""
    return np.hanning(n + 1)[:-1]


def frame_count(length, n_fft):
    """Frames of a segment of `length` samples (0 for an empty one)."""
    if length <= 0:
        return 0
    if length <= n_fft:
        return 1
    hop = n_fft // 4
    return 1 + -((length - n_fft) // -hop)


def band_bins(sr, n_fft, min_frequency=0, max_frequency=None):
    """(k_lo, k_hi), both inside the band; ValueError for an empty band."""
    if max_frequency is None:
        max_frequency = sr / 2
    k_lo = max(1, int(math.ceil(min_frequency * n_fft / sr)))
    k_hi = min(n_fft // 2, int(math.floor(max_frequency * n_fft / sr)))
    if k_lo > k_hi:
        raise ValueError(f"the band {min_frequency} .. {max_frequency} Hz holds no FFT bin at sr={sr}, n_fft={n_fft} "
                         f"(k_lo={k_lo} > k_hi={k_hi})")
    return k_lo, k_hi


def power_spectrum(x, s0, s1, n_fft, fft_dtype=np.float64):
    """P[0 .. n_fft / 2] of x[s0:s1], float64 (zeros for an empty segment).  fft_dtype=np.float32 takes the frames, the window and
    the transform (scipy.fft keeps float32) in single precision and everything behind it in float64: the yardstick of what fp32
    butterflies cost, which the device tests take their tolerances from."""
    hop = n_fft // 4
    length = s1 - s0
    n_frames = frame_count(length, n_fft)
    power = np.zeros(n_fft // 2 + 1, dtype=np.float64)
    if n_frames == 0:
        return power
    window = hann_periodic(n_fft).astype(fft_dtype)
    padded = np.zeros((n_frames - 1) * hop + n_fft, dtype=fft_dtype)
    padded[:length] = x[s0:s1]
    if fft_dtype == np.float64:
        rfft = np.fft.rfft
    else:
        import scipy.fft
        rfft = scipy.fft.rfft
    for j0 in range(0, n_frames, _FRAME_BLOCK):
        j = np.arange(j0, min(n_frames, j0 + _FRAME_BLOCK))
        frames = padded[j[:, None] * hop + np.arange(n_fft)[None, :]] * window
        spec = rfft(frames, axis=1)
        assert spec.real.dtype == fft_dtype
        power += (spec.real.astype(np.float64) ** 2 + spec.imag.astype(np.float64) ** 2).sum(axis=0)
    return power


def spectral_columns(power, k_lo, k_hi):
    """The five spectral columns IN BINS (peak bin, centroid, 5 % and 95 % points, entropy) of a float64 spectrum, float64;
    NaN where the band holds no power."""
    band = power[k_lo:k_hi + 1]
    total = band.sum()
    if not total > 0:
        return (math.nan,) * 5
    k = np.arange(k_lo, k_hi + 1, dtype=np.float64)
    cum = np.cumsum(band)
    points = []
    for q in (0.05, 0.95):
        i = min(int(np.searchsorted(cum, q * total, side="left")), len(band) - 1)      # the first bin with cum >= q T
        before = cum[i - 1] if i else 0.0
        points.append(k_lo + i - 0.5 + (q * total - before) / band[i])
    p = band[band > 0] / total
    with np.errstate(divide="ignore", invalid="ignore"):
        entropy = -(p * np.log(p)).sum() / np.log(len(band))
    return float(k_lo + int(np.argmax(band))), float((k * band).sum() / total), float(points[0]), float(points[1]), float(entropy)


def columns_from_rows(raw, lengths, sr, n_fft):
    """Rate-free rows (float64 [n_seg, 8]: amplitude, rms, crossing COUNT, four bin positions, entropy) -> the dict of COLUMNS."""
    raw = np.asarray(raw, dtype=np.float64).reshape(-1, 8)
    lengths = np.asarray(lengths, dtype=np.float64)
    out = raw.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:, 2] = raw[:, 2] / (lengths / sr)
    out[:, 3:7] = raw[:, 3:7] * (sr / n_fft)
    out[lengths == 0] = np.nan
    return {name: out[:, i].astype(np.float32) for i, name in enumerate(COLUMNS)}


def measure_host(audio, sr, prediction, min_frequency=0, max_frequency=None, fft_dtype=np.float64):
    """The definition: {column: float32 [n_seg]} of the rows of `prediction` in the mono recording `audio` (float32 [n])."""
    x = np.ascontiguousarray(audio, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("audio must be one mono recording [n]")
    n_fft = get_n_fft_given_sr(sr)
    k_lo, k_hi = band_bins(sr, n_fft, min_frequency, max_frequency)
    bounds = bounds_of(prediction, sr, len(x))
    raw = np.full((len(bounds), 8), np.nan, dtype=np.float64)
    for row, (s0, s1) in zip(raw, bounds):
        if s1 == s0:
            continue
        seg = x[s0:s1]
        seg64 = seg.astype(np.float64)
        negative = seg < 0
        row[0] = np.abs(seg).max()
        row[1] = np.sqrt(np.mean(seg64 * seg64))
        row[2] = np.count_nonzero(negative[1:] != negative[:-1])
        row[3:] = spectral_columns(power_spectrum(x, int(s0), int(s1), n_fft, fft_dtype), k_lo, k_hi)
    return columns_from_rows(raw, bounds[:, 1] - bounds[:, 0], sr, n_fft)


# ---- the device path ---------------------------------------------------------------------------------------------------------------
_TABLES = {}


def _device_tables(n_fft, device):
    """(window [n_fft], twiddle [n_fft / 2, 2]) on `device`: computed in float64, rounded to float32 and kept per n_fft, as the
    log-mel descriptor's (audio_utils._DeviceTables)."""
    import torch
    key = (n_fft, str(device))
    if key not in _TABLES:
        angle = 2.0 * np.pi * np.arange(n_fft // 2, dtype=np.float64) / n_fft
        twiddle = np.stack([np.cos(angle), -np.sin(angle)], axis=1)
        _TABLES[key] = (torch.tensor(hann_periodic(n_fft), dtype=torch.float32, device=device),
                        torch.tensor(twiddle, dtype=torch.float32, device=device).contiguous())
    return _TABLES[key]


def scratch_bytes(bounds, n_fft):
    """wseg_measure_scratch_bytes (host arithmetic, no device) of int64 bounds [n_seg, 2]; WsegError for invalid input."""
    bounds = np.ascontiguousarray(bounds, dtype=np.int64).reshape(-1, 2)
    return _lib.size_or_raise(_lib.load().wseg_measure_scratch_bytes(bounds.ctypes.data_as(C.c_void_p), len(bounds), int(n_fft)))


def measure_rows(pcm, bounds, n_fft, k_lo, k_hi, out=None):
    """The launch pair: rate-free rows, a float32 DEVICE tensor [n_seg, 8] (`out`, where given), of the int64 sample ranges
    `bounds` [n_seg, 2] (host) in the device tensor `pcm` (float32 [n], contiguous).  Stream-ordered, no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    RS.check_tensor(pcm, "the recording of measure_rows", "[n]", ndim=1)
    bounds = np.ascontiguousarray(bounds, dtype=np.int64).reshape(-1, 2)
    n_seg = len(bounds)
    out = RS.out_tensor(out, "out", "[n_seg, 8]", torch.float32, (n_seg, 8), pcm.device)
    window, twiddle = _device_tables(n_fft, pcm.device)
    scratch = RS.new_scratch(scratch_bytes(bounds, n_fft), pcm.device)
    with torch.cuda.device(pcm.device):
        _lib.check(lib.wseg_measure_segments_f32(pcm.data_ptr() if pcm.numel() else None, int(pcm.numel()),
                                                 bounds.ctypes.data_as(C.c_void_p), n_seg, int(n_fft), int(k_lo), int(k_hi),
                                                 window.data_ptr(), twiddle.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                 out.data_ptr(), _lib.stream_ptr()))
    return out


def measure(audio, sr, prediction, min_frequency=0, max_frequency=None, device="cuda"):
    """measure_host's columns, computed on the GPU: {column: float32 numpy [n_seg]}.  `audio`: numpy [n] (uploaded to `device`) or
    a device tensor, which is measured where it lies — no PCM travels back to the host, only the rows do."""
    pcm = device_pcm(audio, device)
    n_fft = get_n_fft_given_sr(sr)
    k_lo, k_hi = band_bins(sr, n_fft, min_frequency, max_frequency)
    bounds = bounds_of(prediction, sr, int(pcm.numel()))
    if not len(bounds):
        return {name: np.zeros(0, dtype=np.float32) for name in COLUMNS}
    rows = measure_rows(pcm, bounds, n_fft, k_lo, k_hi).cpu().numpy()
    return columns_from_rows(rows, bounds[:, 1] - bounds[:, 0], sr, n_fft)


def with_columns(prediction, columns):
    """A copy of a prediction dict carrying the eight columns as lists, aligned with `onset`."""
    out = dict(prediction)
    for name in COLUMNS:
        out[name] = [float(v) for v in columns[name]]
    return out
