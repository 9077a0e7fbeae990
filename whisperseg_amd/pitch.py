"""Per-segment fundamental frequency: a YIN pitch contour of every detected call.

`frames_host` / `pitch_host` are THE definition (numpy, float64, every sum in a stated order) and the oracle of every device test,
as measure.measure_host is for the measurements; `pitch_rows` / `pitch` compute the same contour on the GPU from PCM that is already
resident there (wseg_pitch_frames_f64: whisperseg_amd/csrc/wseg_pitch.hip) — the same BITS, because every step is a float64
+ - x / or a comparison, correctly rounded on both sides and taken in the same order.  `frames_plain` states the definition a second
time as a plain double loop over Python floats (its own frame count, its own prefix sum): the host test holds the two together.
`SegmenterBase.segment*(..., pitch=True)` adds the columns to every prediction dict, taken on the device PCM the front-end used.

For a mono recording x (float32 [n]) at rate sr and a row's sample range (s0, s1) = measure.sample_bounds(...):

  lags           tau_min = max(2, floor(sr / f_max)), tau_max = ceil(sr / f_min); f_max None = sr / 8 (below eight samples a period a
                 sampled tone's dip no longer falls under 0.1: tones between sr / 8 and sr / 4 come out an octave low), f_min None =
                 2 sr / n_fft with n_fft = get_n_fft_given_sr(sr), i.e. tau_max = n_fft / 2;  ValueError before anything runs unless
                 2 <= tau_min < tau_max <= 2048 (lag_range, check_args)
  frames         hop None = n_fft / 4 (measure's); frame j starts at t_j = s0 + j hop and reads exactly x[t_j : t_j + 2 tau_max];
                 L = s1 - s0: J = 0 for L < 2 tau_max, else 1 + (L - 2 tau_max) // hop (frame_count).  No zero padding: nothing at or
                 behind s1 and nothing in front of s0 is ever read
  difference     d(tau) = sum_{i = 0}^{tau_max - 1} (f64(x[t + i]) - f64(x[t + i + tau]))^2 for tau = 0 .. tau_max: ONE sequential chain
                 in i per lag, the square and the addition rounded separately
  normalisation  d'(0) = 1, d'(tau) = (d(tau) tau) / run(tau) where run(tau) > 0, else 1.  run is the prefix sum of d(1 .. tau) in
                 two levels: blocks of BLOCK = 64 lags (64 b + 1 .. 64 b + 64); inside a block the sum runs sequentially from the
                 block's first lag; the block bases are the sequential sum of the earlier blocks' totals; run = base + inner
  dip            the smallest c in [tau_min, tau_max - 1] with d'(c) < threshold, walked up while c + 1 <= tau_max - 1 and
                 d'(c + 1) < d'(c): voiced.  No such c: the lowest minimiser of d' over that range: unvoiced
  refinement     a, b, c = d'(tau - 1), d'(tau), d'(tau + 1); den = (a - 2 b) + c; shift = clamp((0.5 (a - c)) / den, -0.5, 0.5) if
                 den > 0, else 0; period = tau + shift
  output         per frame float32 (period, d'(tau), voiced 0 / 1) — rate-free; Python scales by sr
  conventions    silence: d' == 1, unvoiced, tau = tau_min, shift 0.  Non-finite input: unspecified values (and nothing outside the
                 outputs is written)
  columns        COLUMNS, of a row's frames in frame order (columns_from_contour): f0 = sr / period over the VOICED frames — their
                 mean (sequential float64), smallest, largest, first and last; the fraction of voiced frames; aperiodicity = the mean
                 d'(tau) over ALL frames.  A row without frames: all NaN; without a voiced frame: the five f0_* NaN
"""
import ctypes as C
import math

import numpy as np

from . import _lib, resident as RS
from .audio_utils import get_n_fft_given_sr
from .segments import bounds_of, device_pcm

COLUMNS = ("f0_mean", "f0_min", "f0_max", "f0_first", "f0_last", "voiced_fraction", "aperiodicity")
CONTOUR_KEYS = ("f0_contour", "aperiodicity_contour", "frame_time")
BLOCK = 64                    # lags per block of the two-level prefix sum (csrc/wseg_pitch_plan.h::kPitchBlock)
MAX_LAG = 2048                # the largest tau_max (csrc/wseg_pitch_plan.h::kPitchMaxLag): the frame then fills 16 KiB of LDS
_FRAME_BLOCK = 64             # frames frames_host takes at a time (bounds its memory, nothing else)
_OPTIONS = ("f_min", "f_max", "threshold", "contour")


def lag_range(sr, f_min=None, f_max=None):
    """(tau_min, tau_max) of the range f_min .. f_max Hz at rate sr; ValueError unless 2 <= tau_min < tau_max <= 2048."""
    n_fft = get_n_fft_given_sr(sr)
    if f_max is None:
        f_max = sr / 8
    if f_min is None:
        f_min = 2 * sr / n_fft
    if not (f_min > 0 and f_max > 0 and math.isfinite(f_min) and math.isfinite(f_max)):
        raise ValueError(f"the pitch range {f_min} .. {f_max} Hz must be positive and finite")
    tau_min = max(2, int(math.floor(sr / f_max)))
    tau_max = int(math.ceil(sr / f_min))
    if not 2 <= tau_min < tau_max <= MAX_LAG:
        raise ValueError(f"the pitch range {f_min} .. {f_max} Hz gives the lags {tau_min} .. {tau_max} at sr={sr}: "
                         f"2 <= tau_min < tau_max <= {MAX_LAG} is required")
    return tau_min, tau_max


def default_hop(sr):
    return get_n_fft_given_sr(sr) // 4


def check_args(tau_min, tau_max, hop, threshold):
    """ValueError for lags outside 2 <= tau_min < tau_max <= 2048, a hop that is no positive int32 or a threshold outside (0, 1)."""
    if not (isinstance(tau_min, (int, np.integer)) and isinstance(tau_max, (int, np.integer)) and 2 <= tau_min < tau_max <= MAX_LAG):
        raise ValueError(f"the lags must satisfy 2 <= tau_min < tau_max <= {MAX_LAG} (got {tau_min}, {tau_max})")
    if not (isinstance(hop, (int, np.integer)) and 1 <= hop <= 2 ** 31 - 1):
        raise ValueError(f"hop must be an integer 1 .. 2^31 - 1 (got {hop})")
    if not 0 < threshold < 1:
        raise ValueError(f"threshold must lie in (0, 1) (got {threshold})")


def frame_count(length, tau_max, hop):
    """Frames of a segment of `length` samples."""
    if length < 2 * tau_max:
        return 0
    return 1 + (length - 2 * tau_max) // hop


def frame_offsets_of(bounds, tau_max, hop):
    """int64 [n_seg + 1]: the exclusive prefix of the frame counts of int64 bounds [n_seg, 2] (the kernel's table)."""
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    counts = [frame_count(int(s1 - s0), tau_max, hop) for s0, s1 in bounds]
    return np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)


def difference(frames, tau_max):
    """d(0 .. tau_max) float64 [F, tau_max + 1] of float32 frames [F, 2 tau_max]."""
    x = np.asarray(frames, dtype=np.float32).astype(np.float64)
    d = np.zeros((len(x), tau_max + 1), dtype=np.float64)
    for i in range(tau_max):                          # one chain in i per lag: vectorised over lags and frames only
        t = x[:, i:i + 1] - x[:, i:i + tau_max + 1]
        d = d + t * t
    return d


def normalised_difference(frames, tau_max):
    """d'(0 .. tau_max) float64 [F, tau_max + 1] of float32 frames [F, 2 tau_max]."""
    return normalise(difference(frames, tau_max))


def normalise(d):
    """d'(0 .. tau_max) of d(0 .. tau_max), float64 [F, tau_max + 1]: the cumulative mean in the two-level order."""
    n_frames, tau_max = len(d), d.shape[1] - 1
    n_blocks = -(-tau_max // BLOCK)
    padded = np.zeros((n_frames, n_blocks * BLOCK), dtype=np.float64)
    padded[:, :tau_max] = d[:, 1:]
    inner = np.cumsum(padded.reshape(n_frames, n_blocks, BLOCK), axis=2)
    base = np.zeros((n_frames, n_blocks), dtype=np.float64)
    base[:, 1:] = np.cumsum(inner[:, :-1, BLOCK - 1], axis=1)
    run = (base[:, :, None] + inner).reshape(n_frames, -1)[:, :tau_max]
    out = np.ones((n_frames, tau_max + 1), dtype=np.float64)
    tau = np.arange(1, tau_max + 1, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:, 1:] = np.where(run > 0, (d[:, 1:] * tau) / run, 1.0)
    return out


def pick(dn, tau_min, tau_max, threshold):
    """(period, d'(tau), voiced) float32 [3] of one frame's d' (float64 [tau_max + 1]): dip, descent, parabola."""
    hi = tau_max - 1
    below = np.flatnonzero(dn[tau_min:hi + 1] < threshold)
    voiced = len(below) > 0
    if voiced:
        tau = tau_min + int(below[0])
        while tau + 1 <= hi and dn[tau + 1] < dn[tau]:
            tau += 1
    else:
        tau = tau_min + int(np.argmin(dn[tau_min:hi + 1]))
    a, b, c = dn[tau - 1], dn[tau], dn[tau + 1]
    den = (a - 2.0 * b) + c
    shift = min(max((0.5 * (a - c)) / den, -0.5), 0.5) if den > 0 else 0.0
    return np.array([tau + shift, b, 1.0 if voiced else 0.0], dtype=np.float32)


def frames_host(audio, bounds, tau_min, tau_max, hop, threshold=0.1):
    """The definition, rate-free: (contour float32 [total_frames, 3], frame_offsets int64 [n_seg + 1]) of the int64 sample ranges
    `bounds` [n_seg, 2] in the mono recording `audio` (float32 [n]) — what pitch_rows returns from the device."""
    x = np.ascontiguousarray(audio, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("audio must be one mono recording [n]")
    check_args(tau_min, tau_max, hop, threshold)
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    if len(bounds) and not ((0 <= bounds[:, 0]) & (bounds[:, 0] <= bounds[:, 1]) & (bounds[:, 1] <= len(x))).all():
        raise ValueError("bounds must satisfy 0 <= s0 <= s1 <= n")
    offsets = frame_offsets_of(bounds, tau_max, hop)
    out = np.zeros((int(offsets[-1]), 3), dtype=np.float32)
    width = 2 * tau_max
    for (s0, s1), first, last in zip(bounds, offsets[:-1], offsets[1:]):
        seg = x[int(s0):int(s1)]                      # all a row may read
        for j0 in range(0, int(last - first), _FRAME_BLOCK):
            j = np.arange(j0, min(int(last - first), j0 + _FRAME_BLOCK))
            dn = normalised_difference(seg[j[:, None] * hop + np.arange(width)[None, :]], tau_max)
            for k, row in zip(j, dn):
                out[first + k] = pick(row, tau_min, tau_max, threshold)
    return out, offsets


def frames_plain(audio, s0, s1, tau_min, tau_max, hop, threshold=0.1):
    """The definition once more, of ONE sample range, as a plain double loop over Python floats: float32 [J, 3].  Used by the host
    test only (slow: tau_max^2 interpreted steps a frame)."""
    x = [float(v) for v in np.asarray(audio, dtype=np.float32)]
    rows = []
    t = s0
    while t + 2 * tau_max <= s1:                      # a frame exists where all its samples lie inside the row
        d = [0.0] * (tau_max + 1)
        for tau in range(1, tau_max + 1):
            acc = 0.0
            for i in range(tau_max):
                diff = x[t + i] - x[t + i + tau]
                acc = acc + diff * diff
            d[tau] = acc
        dn = [1.0] * (tau_max + 1)
        base, inner = 0.0, 0.0
        for tau in range(1, tau_max + 1):
            if (tau - 1) % BLOCK == 0 and tau > 1:    # a new block: the finished one's total joins the base
                base = base + inner
                inner = 0.0
            inner = inner + d[tau]
            run = base + inner
            dn[tau] = (d[tau] * tau) / run if run > 0 else 1.0
        chosen, voiced = None, 0.0
        for tau in range(tau_min, tau_max):
            if dn[tau] < threshold:
                chosen, voiced = tau, 1.0
                break
        if chosen is None:
            chosen = tau_min
            for tau in range(tau_min + 1, tau_max):
                if dn[tau] < dn[chosen]:
                    chosen = tau
        else:
            while chosen + 1 < tau_max and dn[chosen + 1] < dn[chosen]:
                chosen += 1
        a, b, c = dn[chosen - 1], dn[chosen], dn[chosen + 1]
        den = (a - 2.0 * b) + c
        shift = 0.0
        if den > 0:
            shift = (0.5 * (a - c)) / den
            shift = -0.5 if shift < -0.5 else 0.5 if shift > 0.5 else shift
        rows.append((chosen + shift, b, voiced))
        t += hop
    return np.asarray(rows, dtype=np.float32).reshape(-1, 3)


def columns_from_contour(contour, frame_offsets, sr):
    """Rate-free frames (float32 [total_frames, 3]) + the rows' frame offsets -> the dict of COLUMNS, float32 [n_seg]; shared by the
    host and the device path.  Means are sequential float64 sums in frame order."""
    contour = np.asarray(contour, dtype=np.float32).reshape(-1, 3)
    offsets = np.asarray(frame_offsets, dtype=np.int64)
    out = np.full((len(offsets) - 1, len(COLUMNS)), np.nan, dtype=np.float64)
    for row, first, last in zip(out, offsets[:-1], offsets[1:]):
        if last == first:
            continue
        frames = contour[first:last].astype(np.float64)
        voiced = frames[:, 2] != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            f0 = float(sr) / frames[voiced, 0]
        if len(f0):
            row[0] = np.cumsum(f0)[-1] / len(f0)
            row[1:5] = f0.min(), f0.max(), f0[0], f0[-1]
        row[5] = len(f0) / len(frames)
        row[6] = np.cumsum(frames[:, 1])[-1] / len(frames)
    return {name: out[:, i].astype(np.float32) for i, name in enumerate(COLUMNS)}


def contours_of(contour, frame_offsets, bounds, tau_max, hop, sr):
    """The per-row arrays of contour=True: "f0_contour" (Hz, NaN where unvoiced) and "aperiodicity_contour", lists of float32 [J],
    and "frame_time", the frames' centres (t_j + tau_max) / sr in seconds, a list of float64 [J]."""
    contour = np.asarray(contour, dtype=np.float32).reshape(-1, 3)
    offsets = np.asarray(frame_offsets, dtype=np.int64)
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    out = {key: [] for key in CONTOUR_KEYS}
    for (s0, _), first, last in zip(bounds, offsets[:-1], offsets[1:]):
        frames = contour[first:last].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            f0 = np.where(frames[:, 2] != 0, float(sr) / frames[:, 0], np.nan)
        out["f0_contour"].append(f0.astype(np.float32))
        out["aperiodicity_contour"].append(frames[:, 1].astype(np.float32))
        out["frame_time"].append((int(s0) + np.arange(int(last - first), dtype=np.int64) * hop + tau_max) / float(sr))
    return out


def _resolved(sr, f_min, f_max, threshold, hop):
    tau_min, tau_max = lag_range(sr, f_min, f_max)
    hop = default_hop(sr) if hop is None else hop
    check_args(tau_min, tau_max, hop, threshold)
    return tau_min, tau_max, int(hop)


def _result(frames, offsets, bounds, tau_max, hop, sr, contour):
    out = columns_from_contour(frames, offsets, sr)
    if contour:
        out.update(contours_of(frames, offsets, bounds, tau_max, hop, sr))
    return out


def pitch_host(audio, sr, prediction, f_min=None, f_max=None, threshold=0.1, hop=None, contour=False):
    """The definition: {column: float32 [n_seg]} of the rows of `prediction` in the mono recording `audio` (float32 [n]); with
    contour=True also CONTOUR_KEYS."""
    x = np.ascontiguousarray(audio, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("audio must be one mono recording [n]")
    tau_min, tau_max, hop = _resolved(sr, f_min, f_max, threshold, hop)
    bounds = bounds_of(prediction, sr, len(x))
    frames, offsets = frames_host(x, bounds, tau_min, tau_max, hop, threshold)
    return _result(frames, offsets, bounds, tau_max, hop, sr, contour)


def options(pitch, sr=None):
    """The keyword arguments of pitch() a segmenter's `pitch=` stands for: True -> {}, a dict of f_min / f_max / threshold / contour
    -> itself; anything else, an unknown key, a threshold outside (0, 1) or — where `sr` is known — a range whose lags do not
    satisfy 2 <= tau_min < tau_max <= 2048 is a ValueError."""
    if pitch is True:
        opts = {}
    elif isinstance(pitch, dict):
        unknown = sorted(set(pitch) - set(_OPTIONS))
        if unknown:
            raise ValueError(f"pitch= takes the keys {', '.join(_OPTIONS)} (got {', '.join(map(str, unknown))})")
        opts = dict(pitch)
    else:
        raise ValueError("pitch must be None, True or a dict of f_min, f_max, threshold, contour")
    threshold = opts.get("threshold", 0.1)
    if not (isinstance(threshold, (int, float)) and 0 < threshold < 1):
        raise ValueError(f"threshold must lie in (0, 1) (got {threshold})")
    for name in ("f_min", "f_max"):
        v = opts.get(name)
        if v is not None and not (isinstance(v, (int, float)) and v > 0 and math.isfinite(v)):
            raise ValueError(f"{name} must be a positive frequency in Hz (got {v})")
    if opts.get("f_min") is not None and opts.get("f_max") is not None and opts["f_min"] > opts["f_max"]:
        raise ValueError(f"f_min must not lie above f_max (got {opts['f_min']}, {opts['f_max']})")
    if sr is not None:
        lag_range(sr, opts.get("f_min"), opts.get("f_max"))
    return opts


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(bounds, tau_max, hop):
    """wseg_pitch_scratch_bytes (host arithmetic, no device) of int64 bounds [n_seg, 2]; WsegError for invalid input."""
    bounds = np.ascontiguousarray(bounds, dtype=np.int64).reshape(-1, 2)
    return _lib.size_or_raise(_lib.load().wseg_pitch_scratch_bytes(bounds.ctypes.data_as(C.c_void_p), len(bounds), int(tau_max), int(hop)))


def pitch_rows(pcm, bounds, tau_min, tau_max, hop, threshold=0.1, out=None):
    """The launch: (contour, frame_offsets) — a float32 DEVICE tensor [total_frames, 3] (`out`, where given) of (period, d'(tau),
    voiced) per frame, rate-free, and the host int64 [n_seg + 1] offsets of every row's frames in it — of the int64 sample ranges
    `bounds` [n_seg, 2] (host) in the device tensor `pcm` (float32 [n], contiguous).  Stream-ordered, no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    RS.check_tensor(pcm, "the recording of pitch_rows", "[n]", ndim=1)
    bounds = np.ascontiguousarray(bounds, dtype=np.int64).reshape(-1, 2)
    n_seg = len(bounds)
    nbytes = scratch_bytes(bounds, tau_max, hop)      # (validates bounds, tau_max and hop: the frame counts below are then defined)
    offsets = frame_offsets_of(bounds, int(tau_max), int(hop))
    total = int(offsets[-1])
    out = RS.out_tensor(out, "out", "[total_frames, 3]", torch.float32, (total, 3), pcm.device)
    scratch = RS.new_scratch(nbytes, pcm.device)
    with torch.cuda.device(pcm.device):
        _lib.check(lib.wseg_pitch_frames_f64(pcm.data_ptr() if pcm.numel() else None, int(pcm.numel()),
                                             bounds.ctypes.data_as(C.c_void_p), n_seg, int(tau_min), int(tau_max), int(hop),
                                             float(threshold), scratch.data_ptr(), nbytes, out.data_ptr() if total else None,
                                             _lib.stream_ptr()))
    return out, offsets


def pitch(audio, sr, prediction, f_min=None, f_max=None, threshold=0.1, hop=None, contour=False, device="cuda"):
    """pitch_host's columns (and, with contour=True, its per-row contours), computed on the GPU: `audio` is numpy [n] (uploaded to
    `device`) or a device tensor, which is used where it lies — no PCM travels back to the host, only the frames do."""
    tau_min, tau_max, hop = _resolved(sr, f_min, f_max, threshold, hop)      # (before any device work)
    pcm = device_pcm(audio, device)
    bounds = bounds_of(prediction, sr, int(pcm.numel()))
    if not len(bounds):
        frames, offsets = np.zeros((0, 3), dtype=np.float32), np.zeros(1, dtype=np.int64)
    else:
        frames, offsets = pitch_rows(pcm, bounds, tau_min, tau_max, hop, threshold)
        frames = frames.cpu().numpy()
    return _result(frames, offsets, bounds, tau_max, hop, sr, contour)


def with_columns(prediction, columns):
    """A copy of a prediction dict carrying COLUMNS as lists aligned with `onset`, and the per-row contours where `columns` has them."""
    out = dict(prediction)
    for name in COLUMNS:
        out[name] = [float(v) for v in columns[name]]
    for key in CONTOUR_KEYS:
        if key in columns:
            out[key] = list(columns[key])
    return out
