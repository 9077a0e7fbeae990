"""Per-segment log-mel patches: one fixed-size spectrogram picture per detected call — what clustering, embedding (UMAP over
syllables), nearest-neighbour review and a labelling tool's thumbnails are computed from.

`patches_host` is THE definition (numpy, float64) and the oracle of every device test, as measure.measure_host is for the
measurements; `patches` computes the same pictures on the GPU from PCM that is already resident there (wseg_patches_f32:
whisperseg_amd/csrc/wseg_patch.hip), one launch pair per block of rows.  `SegmenterBase.segment*(..., patches=W)` adds the key
"patch" to every prediction dict, taken on the device PCM the front-end used.

For a mono recording x (float32 [n]) at rate sr, a segment (onset, offset) in seconds and a width W (1 .. 256 columns):

  sample range   (s0, s1) = measure.sample_bounds(onset, offset, sr, n),  L = s1 - s0
  column centres n_fft = get_n_fft_given_sr(sr);  column c (0 <= c < W) is centred on sample t_c = s0 + ((2c + 1) L) // (2W) —
                 integers only, and time-normalised: every patch has W columns whatever the call's duration (which the row carries)
  frames         frame c is x[t_c - n_fft / 2 + i], i = 0 .. n_fft - 1, every index outside [0, n) read as zero.  The frame does see
                 the recording outside [s0, s1): the picture is a slice of the spectrogram, as the front-end's centred frames are.  It
                 is not reflect-padded.  With L < W several columns share a centre, with L == 0 all do: no special case, no NaN
  spectrum, mel  S_c[k] = |rfft(w frame_c)[k]|^2 with the periodic Hann window (measure.hann_periodic);  mel_c[m] = sum_k fb[k, m] S_c[k]
                 with fb = audio_utils.slaney_mel_filters(sr, n_fft, min_frequency, max_frequency or sr // 2) — the front-end's own
                 bank, 80 filters, its filters that hold no bin included;  v[m, c] = log10(max(1e-10, mel_c[m]))
  normalisation  the front-end's rule per patch: V = max over (m, c), patch[m, c] = (max(v[m, c], V - 8) + 4) / 4, float32.  A silent
                 segment is -1.5 everywhere
  conventions    an empty band (measure.band_bins) or a width outside 1 .. 256: ValueError before anything runs
"""
import ctypes as C

import numpy as np

from . import _lib, measure as M, resident as RS
from .audio_utils import N_MELS, get_n_fft_given_sr, slaney_mel_filters
from .segments import bounds_of, device_pcm

MAX_WIDTH = 256                        # columns of a patch (csrc/wseg_patch_plan.h::kPatchMaxWidth)
PATCH_BLOCK_BYTES = 256 << 20          # device output `patches` holds at a time: the rows go through in blocks of at most this


def check_width(width):
    """`width` as an int, ValueError unless it is an integer in 1 .. 256."""
    return RS.check_int(width, "width", 1, MAX_WIDTH)


def filterbank(sr, n_fft, min_frequency=0, max_frequency=None):
    """The front-end's bank for the band, float64 [n_fft / 2 + 1, 80]; ValueError for a band that holds no FFT bin."""
    M.band_bins(sr, n_fft, min_frequency, max_frequency)
    return slaney_mel_filters(sr, n_fft, min_frequency, max_frequency if max_frequency else sr // 2)


def column_centres(s0, s1, width):
    """int64 [width]: the sample every column of the segment [s0, s1) is centred on."""
    c = np.arange(width, dtype=np.int64)
    return int(s0) + ((2 * c + 1) * (int(s1) - int(s0))) // (2 * width)


def log_mel_columns(x, centres, n_fft, fb, fft_dtype=np.float64):
    """v [n_mels, len(centres)], float64: log10 mel of the zero-padded frames of x centred on `centres`, before normalisation."""
    idx = np.asarray(centres, dtype=np.int64)[:, None] - n_fft // 2 + np.arange(n_fft, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < len(x))
    frames = np.where(inside, x[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0).astype(fft_dtype)
    frames = frames * M.hann_periodic(n_fft).astype(fft_dtype)
    if fft_dtype == np.float64:
        spec = np.fft.rfft(frames, axis=1)
    else:
        import scipy.fft
        spec = scipy.fft.rfft(frames, axis=1)
    assert spec.real.dtype == fft_dtype
    power = spec.real.astype(np.float64) ** 2 + spec.imag.astype(np.float64) ** 2
    return np.log10(np.maximum(1e-10, power @ fb)).T


def normalise(v):
    """The front-end's rule on one picture v [n_mels, W] (float64) -> float32."""
    return ((np.maximum(v, v.max() - 8.0) + 4.0) / 4.0).astype(np.float32)


def patches_host(audio, sr, prediction, width=32, min_frequency=0, max_frequency=None, fft_dtype=np.float64):
    """The definition: float32 [n_seg, 80, width] of the rows of `prediction` in the mono recording `audio` (float32 [n]).
    fft_dtype=np.float32 takes the frames, the window and the transform (scipy.fft keeps float32) in single precision, the bank
    rounded to float32 and everything behind the transform in float64: the yardstick of what the device path's fp32 stages cost,
    which the device tests take their tolerances from."""
    x = np.ascontiguousarray(audio, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("audio must be one mono recording [n]")
    width = check_width(width)
    n_fft = get_n_fft_given_sr(sr)
    fb = filterbank(sr, n_fft, min_frequency, max_frequency)
    if fft_dtype != np.float64:
        fb = fb.astype(np.float32).astype(np.float64)
    bounds = bounds_of(prediction, sr, len(x))
    out = np.empty((len(bounds), fb.shape[1], width), dtype=np.float32)
    for row, (s0, s1) in zip(out, bounds):
        row[...] = normalise(log_mel_columns(x, column_centres(s0, s1, width), n_fft, fb, fft_dtype))
    return out


# ---- the device path ---------------------------------------------------------------------------------------------------------------
_TABLES = {}


def device_tables(sr, min_frequency=0, max_frequency=None, device="cuda"):
    """audio_utils._DeviceTables (window, twiddles, the bank's sparse rows and the descriptor over them) of the rate's n_fft and the
    band, on `device`: built once per key and kept, as measure._TABLES is."""
    import torch
    from .audio_utils import _DeviceTables
    n_fft = get_n_fft_given_sr(sr)
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (sr, n_fft, min_frequency, max_frequency, str(device))
    if key not in _TABLES:
        _TABLES[key] = _DeviceTables(n_fft, n_fft // 4, filterbank(sr, n_fft, min_frequency, max_frequency), MAX_WIDTH, device)
    return _TABLES[key]


def scratch_bytes(n_seg, n_mels, width):
    """wseg_patches_scratch_bytes (host arithmetic, no device); WsegError for invalid input."""
    return _lib.size_or_raise(_lib.load().wseg_patches_scratch_bytes(int(n_seg), int(n_mels), int(width)))


def patch_rows(pcm, bounds, tables, width, out=None):
    """The launch pair: a float32 DEVICE tensor [n_seg, n_mels, width] (`out`, where given) of the int64 sample ranges `bounds`
    [n_seg, 2] (host) in the device tensor `pcm` (float32 [n], contiguous), with the `tables` of device_tables.  Stream-ordered, no
    host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    RS.check_tensor(pcm, "the recording of patch_rows", "[n]", ndim=1)
    if tables.window.device != pcm.device:
        raise _lib.WsegError(f"the tables are on {tables.window.device}, the recording on {pcm.device}")
    width = check_width(width)
    bounds = np.ascontiguousarray(bounds, dtype=np.int64).reshape(-1, 2)
    n_seg, n_mels = len(bounds), int(tables.desc.n_mels)
    out = RS.out_tensor(out, "out", "[n_seg, n_mels, width]", torch.float32, (n_seg, n_mels, width), pcm.device)
    scratch = RS.new_scratch(scratch_bytes(n_seg, n_mels, width), pcm.device)
    with torch.cuda.device(pcm.device):
        _lib.check(lib.wseg_patches_f32(C.byref(tables.desc), pcm.data_ptr() if pcm.numel() else None, int(pcm.numel()),
                                        bounds.ctypes.data_as(C.c_void_p), n_seg, width, scratch.data_ptr(), scratch.numel(),
                                        out.data_ptr() if out.numel() else None, _lib.stream_ptr()))
    return out


def patches(audio, sr, prediction, width=32, min_frequency=0, max_frequency=None, device="cuda"):
    """patches_host's pictures, computed on the GPU: float32 numpy [n_seg, 80, width].  `audio`: numpy [n] (uploaded to `device`) or
    a device tensor, which is measured where it lies — no PCM travels back to the host, only the pictures do.  The rows go through
    in blocks of at most PATCH_BLOCK_BYTES of device output (a recording with 100 000 rows needs no 2 GB tensor); a segment's bits
    do not depend on the block it falls into."""
    width = check_width(width)
    pcm = device_pcm(audio, device)
    n_fft = get_n_fft_given_sr(sr)
    M.band_bins(sr, n_fft, min_frequency, max_frequency)
    bounds = bounds_of(prediction, sr, int(pcm.numel()))
    out = np.empty((len(bounds), N_MELS, width), dtype=np.float32)
    if not len(bounds):
        return out
    tables = device_tables(sr, min_frequency, max_frequency, pcm.device)
    rows = max(1, PATCH_BLOCK_BYTES // (N_MELS * width * 4))
    for r0 in range(0, len(bounds), rows):
        out[r0:r0 + rows] = patch_rows(pcm, bounds[r0:r0 + rows], tables, width).cpu().numpy()
    return out


def with_patch(prediction, patch):
    """A copy of a prediction dict carrying the pictures under "patch" (float32 [n_seg, 80, W], aligned with `onset`)."""
    out = dict(prediction)
    out["patch"] = patch
    return out
