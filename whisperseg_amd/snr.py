"""Per-segment signal-to-noise ratio: how far above the recording's background every detected call lies.

`frame_energy_host` / `frame_ranges` / `snr_host` are THE definition (numpy, float64) and the oracle of every device test, as
measure.measure_host is for the measurements; `frame_energy` / `snr_rows` / `snr` compute the same on the GPU from PCM that is
already resident there (wseg_frame_energy_f32, wseg_snr_rows_f64: whisperseg_amd/csrc/wseg_snr.hip).
`SegmenterBase.segment*(..., snr=True)` adds the columns to every prediction dict, rated on the device PCM the front-end used.

For a mono recording x (float32 [n]) at rate sr and a segmenter's min_frequency:

  frames         n_fft = get_n_fft_given_sr(sr), hop = n_fft / 4, measure's periodic Hann window and band (band_bins).  WHOLE frames
                 only: frame j is x[j hop : j hop + n_fft]; J = 0 for n < n_fft, else 1 + (n - n_fft) // hop (frame_count).  No
                 sample at or behind n is ever read
  track          E[j] = sum_{k = k_lo .. k_hi} |rfft(w frame_j)[k]|^2 in float64, rounded to float32 (frame_energy_host);
                 fft_dtype=np.float32 is the single-precision yardstick, as measure.power_spectrum's
  frame ranges   integer arithmetic on the host (frame_ranges; the device gets int64 and does no time arithmetic).  (s0, s1) of a
                 row = segments.bounds_of.  Signal frames: the frames wholly inside the row, j0 = ceil(s0 / hop), j1 = min(J,
                 (s1 - n_fft) // hop + 1) (0 where s1 < n_fft); where that range is empty, the one frame centred nearest the row's
                 centre: jc = clamp(((s0 + s1) // 2 - n_fft // 2 + hop // 2) // hop, 0, J - 1), [j0, j1) = [jc, jc + 1).
                 Noise window [w0, w1): context None = [0, J); context seconds, c = ceil(floor(context sr + 0.5) / hop):
                 [max(0, j0 - c), min(J, j1 + c)).  Rank r = floor(q (w1 - w0 - 1)) in Python floats, quantile q in [0, 1]
  row            N = sort(E[w0:w1])[r] with NaN ordered last, as numpy.sort has it (a float file may hold NaN); without NaN it is
                 np.quantile(E[w0:w1], q, method="lower").  S = mean E[j0:j1] in float64, M = max E[j0:j1]
  columns        E_ref = 3 n_fft^2 / 32, the band energy of a full-scale sine under this window (0 dB: a full-scale sine inside
                 the band): signal_level_db = 10 log10(S / E_ref), noise_level_db = 10 log10(N / E_ref), snr_db = 10 log10(S / N),
                 peak_snr_db = 10 log10(M / N), float32 (columns_from_rows: host arithmetic, shared by both paths — the device
                 returns raw (S, M, N))
  conventions    an empty row (s1 == s0) or J == 0: all four NaN.  N == 0 (digital silence): what numpy's division and log10
                 give — +inf, -inf, or NaN for 0 / 0
"""
import ctypes as C
import math

import numpy as np

from . import _lib, resident as RS
from .audio_utils import get_n_fft_given_sr
from .measure import _device_tables, band_bins, hann_periodic
from .segments import bounds_of, device_pcm

COLUMNS = ("signal_level_db", "noise_level_db", "snr_db", "peak_snr_db")
TRACK_KEYS = ("frame_energy", "hop", "n_fft")
SPLIT = 8192                  # frames of a noise window one workgroup selects in LDS (csrc/wseg_snr_plan.h::kSnrSplit); more: split
_FRAME_BLOCK = 256            # frames frame_band_energy transforms at a time (bounds its memory, nothing else)
_OPTIONS = ("quantile", "context", "max_frequency", "track")


def frame_count(n, n_fft):
    """Whole frames of a recording of n samples."""
    return 0 if n < n_fft else 1 + (n - n_fft) // (n_fft // 4)


def reference_energy(n_fft):
    """E_ref: the band energy of a full-scale sine on a bin inside the band, under the periodic Hann window."""
    return 3.0 * n_fft * n_fft / 32.0


def check_args(quantile, context):
    """ValueError for a quantile outside [0, 1] or a context that is neither None nor a finite, non-negative number of seconds."""
    if isinstance(quantile, bool) or not isinstance(quantile, (int, float, np.integer, np.floating)) or not 0 <= quantile <= 1:
        raise ValueError(f"quantile must lie in [0, 1] (got {quantile!r})")
    if context is not None and (isinstance(context, bool) or not isinstance(context, (int, float, np.integer, np.floating))
                                or not 0 <= context < math.inf):
        raise ValueError(f"context must be None or a non-negative number of seconds (got {context!r})")


def frame_band_energy(audio, n_fft, k_lo, k_hi, fft_dtype=np.float64):
    """float64 [J]: the energy of the bins k_lo .. k_hi of every whole frame of the mono recording `audio` — the track before its
    rounding (k_lo = 0, k_hi = n_fft / 2: a frame's whole one-sided power, which the device tests scale their tolerance by)."""
    x = np.ascontiguousarray(audio, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("audio must be one mono recording [n]")
    hop = n_fft // 4
    n_frames = frame_count(len(x), n_fft)
    out = np.zeros(n_frames, dtype=np.float64)
    window = hann_periodic(n_fft).astype(fft_dtype)
    if fft_dtype == np.float64:
        rfft = np.fft.rfft
    else:
        import scipy.fft
        rfft = scipy.fft.rfft
    for f0 in range(0, n_frames, _FRAME_BLOCK):
        j = np.arange(f0, min(n_frames, f0 + _FRAME_BLOCK))
        frames = x[j[:, None] * hop + np.arange(n_fft)[None, :]].astype(fft_dtype) * window
        spec = rfft(frames, axis=1)[:, k_lo:k_hi + 1]
        assert spec.real.dtype == fft_dtype
        out[j] = (spec.real.astype(np.float64) ** 2 + spec.imag.astype(np.float64) ** 2).sum(axis=1)
    return out


def frame_energy_host(audio, sr, min_frequency=0, max_frequency=None, fft_dtype=np.float64):
    """The track's definition: E float32 [J] of the mono recording `audio` (float32 [n]) in the band min_frequency .. max_frequency."""
    n_fft = get_n_fft_given_sr(sr)
    k_lo, k_hi = band_bins(sr, n_fft, min_frequency, max_frequency)
    with np.errstate(over="ignore"):
        return frame_band_energy(audio, n_fft, k_lo, k_hi, fft_dtype).astype(np.float32)


def context_frames(context, sr, n_fft):
    """c of the definition: the frames a context of `context` seconds reaches to either side (None: the whole recording, -1)."""
    if context is None:
        return -1
    hop = n_fft // 4
    return -(-int(math.floor(context * sr + 0.5)) // hop)


def frame_ranges(bounds, n, n_fft, sr, quantile=0.1, context=None):
    """(table int64 [n_seg, 3], windows int64 [n_win, 3]) of int64 sample ranges `bounds` [n_seg, 2] in a recording of n samples:
    a row of the table is (j0, j1, window), a window (w0, w1, r) — what wseg_snr_rows_f64 takes.  context=None: one window for all
    rows; else a window per row (equal ones are selected once: the plan's dedup).  J == 0: every row (0, 0, 0) and no window."""
    check_args(quantile, context)
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    hop = n_fft // 4
    J = frame_count(n, n_fft)
    c = context_frames(context, sr, n_fft)
    table = np.zeros((len(bounds), 3), dtype=np.int64)
    if J == 0:
        return table, np.zeros((0, 3), dtype=np.int64)
    windows = []
    if c < 0:
        windows.append((0, J, int(math.floor(quantile * (J - 1)))))
    for row, (s0, s1) in zip(table, bounds):
        s0, s1 = int(s0), int(s1)
        j0 = -(-s0 // hop)
        j1 = min(J, (s1 - n_fft) // hop + 1) if s1 >= n_fft else 0
        if j1 <= j0:
            jc = min(max(((s0 + s1) // 2 - n_fft // 2 + hop // 2) // hop, 0), J - 1)
            j0, j1 = jc, jc + 1
        if c >= 0:
            w0, w1 = max(0, j0 - c), min(J, j1 + c)
            windows.append((w0, w1, int(math.floor(quantile * (w1 - w0 - 1)))))
        row[:] = j0, j1, len(windows) - 1
    return table, np.asarray(windows, dtype=np.int64).reshape(-1, 3)


def rows_host(track, table, windows):
    """The rows' definition: raw float64 [n_seg, 3] = (S, M, N) of a float32 track — what wseg_snr_rows_f64 writes."""
    track = np.asarray(track, dtype=np.float32)
    table = np.asarray(table, dtype=np.int64).reshape(-1, 3)
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 3)
    out = np.full((len(table), 3), np.nan, dtype=np.float64)
    floors = {}
    for row, (j0, j1, w) in zip(out, table):
        if j1 == j0:
            continue
        if w not in floors:
            w0, w1, r = windows[w]
            floors[w] = float(np.sort(track[w0:w1])[r])
        e = track[j0:j1]
        with np.errstate(invalid="ignore"):
            row[:] = e.astype(np.float64).sum() / len(e), e.max(), floors[w]
    return out


def columns_from_rows(raw, lengths, n_fft):
    """Raw rows (float64 [n_seg, 3]: S, M, N) and the rows' sample counts -> the dict of COLUMNS, float32 [n_seg]; the logs and
    E_ref, shared by the host and the device path.  An empty row: all NaN."""
    raw = np.asarray(raw, dtype=np.float64).reshape(-1, 3)
    lengths = np.asarray(lengths, dtype=np.int64)
    S, M, N = raw[:, 0], raw[:, 1], raw[:, 2]
    ref = reference_energy(n_fft)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        out = np.stack([10.0 * np.log10(S / ref), 10.0 * np.log10(N / ref), 10.0 * np.log10(S / N), 10.0 * np.log10(M / N)], axis=1)
    out[lengths == 0] = np.nan
    return {name: out[:, i].astype(np.float32) for i, name in enumerate(COLUMNS)}


def _result(raw, bounds, n_fft, track, keep_track):
    out = columns_from_rows(raw, bounds[:, 1] - bounds[:, 0], n_fft)
    if keep_track:
        out.update(frame_energy=np.asarray(track, dtype=np.float32), hop=n_fft // 4, n_fft=n_fft)
    return out


def snr_host(audio, sr, prediction, min_frequency=0, max_frequency=None, quantile=0.1, context=None, track=False,
             fft_dtype=np.float64):
    """The definition: {column: float32 [n_seg]} of the rows of `prediction` in the mono recording `audio` (float32 [n]); with
    track=True also TRACK_KEYS: the recording's track (float32 [J]), its hop and its n_fft."""
    x = np.ascontiguousarray(audio, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("audio must be one mono recording [n]")
    check_args(quantile, context)
    n_fft = get_n_fft_given_sr(sr)
    energy = frame_energy_host(x, sr, min_frequency, max_frequency, fft_dtype)
    bounds = bounds_of(prediction, sr, len(x))
    table, windows = frame_ranges(bounds, len(x), n_fft, sr, quantile, context)
    return _result(rows_host(energy, table, windows), bounds, n_fft, energy, track)


def options(snr, sr=None, min_frequency=0):
    """The keyword arguments of snr() a segmenter's `snr=` stands for: True -> {}, a dict of quantile / context / max_frequency /
    track -> itself; anything else, an unknown key, a quantile outside [0, 1], a negative context or — where `sr` is known — a
    band without a bin is a ValueError."""
    if snr is True:
        opts = {}
    elif isinstance(snr, dict):
        unknown = sorted(set(snr) - set(_OPTIONS))
        if unknown:
            raise ValueError(f"snr= takes the keys {', '.join(_OPTIONS)} (got {', '.join(map(str, unknown))})")
        opts = dict(snr)
    else:
        raise ValueError("snr must be None, True or a dict of quantile, context, max_frequency, track")
    check_args(opts.get("quantile", 0.1), opts.get("context"))
    v = opts.get("max_frequency")
    if v is not None and not (isinstance(v, (int, float)) and not isinstance(v, bool) and 0 < v < math.inf):
        raise ValueError(f"max_frequency must be a positive frequency in Hz (got {v!r})")
    if sr is not None:
        band_bins(sr, get_n_fft_given_sr(sr), min_frequency or 0, v)
    return opts


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def frame_energy(pcm, sr, min_frequency=0, max_frequency=None, out=None):
    """The track on the GPU: a float32 DEVICE tensor [J] (`out`, where given) of the device tensor `pcm` (float32 [n], contiguous).
    Stream-ordered, no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    RS.check_tensor(pcm, "the recording of frame_energy", "[n]", ndim=1)
    n_fft = get_n_fft_given_sr(sr)
    k_lo, k_hi = band_bins(sr, n_fft, min_frequency, max_frequency)
    n = int(pcm.numel())
    J = frame_count(n, n_fft)
    out = RS.out_tensor(out, "out", "[J]", torch.float32, (J,), pcm.device)
    window, twiddle = _device_tables(n_fft, pcm.device)
    with torch.cuda.device(pcm.device):
        _lib.check(lib.wseg_frame_energy_f32(pcm.data_ptr() if n else None, n, int(n_fft), int(k_lo), int(k_hi), window.data_ptr(),
                                             twiddle.data_ptr(), out.data_ptr() if J else None, _lib.stream_ptr()))
    return out


def scratch_bytes(J, table, windows):
    """wseg_snr_rows_scratch_bytes (host arithmetic, no device) of int64 table [n_seg, 3] and windows [n_win, 3]; WsegError for
    invalid input."""
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
    windows = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 3)
    return _lib.size_or_raise(_lib.load().wseg_snr_rows_scratch_bytes(int(J), table.ctypes.data_as(C.c_void_p), len(table),
                                                                      windows.ctypes.data_as(C.c_void_p), len(windows)))


def snr_rows(track, table, windows, out=None):
    """The launch: raw rows, a float64 DEVICE tensor [n_seg, 3] = (S, M, N) (`out`, where given), of the host int64 `table`
    [n_seg, 3] and `windows` [n_win, 3] (frame_ranges) over the device tensor `track` (float32 [J], contiguous).  Stream-ordered,
    no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    RS.check_tensor(track, "the track of snr_rows", "[J]", ndim=1)
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
    windows = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 3)
    J = int(track.numel())
    nbytes = scratch_bytes(J, table, windows)         # (validates the table, the windows and the ranks)
    out = RS.out_tensor(out, "out", "[n_seg, 3]", torch.float64, (len(table), 3), track.device)
    scratch = RS.new_scratch(nbytes, track.device)
    with torch.cuda.device(track.device):
        _lib.check(lib.wseg_snr_rows_f64(track.data_ptr() if J else None, J, table.ctypes.data_as(C.c_void_p), len(table),
                                         windows.ctypes.data_as(C.c_void_p), len(windows), scratch.data_ptr(), nbytes,
                                         out.data_ptr() if len(table) else None, _lib.stream_ptr()))
    return out


def snr(audio, sr, prediction, min_frequency=0, max_frequency=None, quantile=0.1, context=None, track=False, device="cuda"):
    """snr_host's columns (and, with track=True, TRACK_KEYS), computed on the GPU: `audio` is numpy [n] (uploaded to `device`) or a
    device tensor, which is rated where it lies — no PCM travels back to the host, only the rows (and the track asked for) do."""
    check_args(quantile, context)                     # (before any device work)
    n_fft = get_n_fft_given_sr(sr)
    band_bins(sr, n_fft, min_frequency, max_frequency)
    pcm = device_pcm(audio, device)
    n = int(pcm.numel())
    bounds = bounds_of(prediction, sr, n)
    table, windows = frame_ranges(bounds, n, n_fft, sr, quantile, context)
    energy = None
    raw = np.full((len(bounds), 3), np.nan, dtype=np.float64)
    if frame_count(n, n_fft) and (len(bounds) or track):
        energy = frame_energy(pcm, sr, min_frequency, max_frequency)
        if len(bounds):
            raw = snr_rows(energy, table, windows).cpu().numpy()
    host_track = (np.zeros(0, np.float32) if energy is None else energy.cpu().numpy()) if track else None
    return _result(raw, bounds, n_fft, host_track, track)


def with_columns(prediction, columns):
    """A copy of a prediction dict carrying COLUMNS as lists aligned with `onset`, and the recording's track where `columns` has it."""
    out = dict(prediction)
    for name in COLUMNS:
        out[name] = [float(v) for v in columns[name]]
    for key in TRACK_KEYS:
        if key in columns:
            out[key] = columns[key]
    return out
