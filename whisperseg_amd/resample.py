"""Sample-rate conversion on the GPU (audio ingest).

The reference resamples implicitly through `librosa.load(path, sr=target)` (scripts/segment.py:48,61, evaluate.py:58):
a third-party resampler that is neither pinned nor installed here.  This module implements the standard rational
polyphase scheme — Kaiser(beta=5)-windowed sinc low-pass of half-length 10*max(up, down), unity DC gain times `up`,
centred output of ceil(n*up/down) samples — which is also what `scipy.signal.resample_poly` computes; the arithmetic runs
in libwseg: `wseg_resample_f32` for one signal, `wseg_resample_planar_f32` for the channels of a recording kept apart
([channels, n]: one launch, every row with the bits of the one-signal call), `wseg_resample_planar_range_f32` for a range of
those outputs from a segment of the planes.  The file path — FilePipeline(sr=), load_wav_device(sr=), segment_files(sr=) and the
CLI's --sr — resamples a file piece by piece with the range call (wavio.StreamResampler, planned by stream_plan below: the bits of
resample() on the whole file, which never exists at its native rate); wavio.DeviceIngest.resample is resample()."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib


def filter_half_len(up, down):
    """Half the filter's length for the reduced ratio up/down: 2 * half_len + 1 taps (design_taps makes them, _ratio counts them)."""
    return 10 * max(up, down)


def design_taps(up, down, beta=5.0):
    """float32 FIR taps (already scaled by `up`) + half length, for the reduced ratio up/down."""
    max_rate = max(up, down)
    half_len = filter_half_len(up, down)
    n = 2 * half_len + 1
    m = np.arange(n, dtype=np.float64) - half_len
    cutoff = 1.0 / max_rate
    h = cutoff * np.sinc(cutoff * m) * np.kaiser(n, beta)
    h /= h.sum()
    h = h.astype(np.float32)
    h *= np.float32(up)
    return h, half_len


def _ratio(sr_in, sr_out):
    """-> (up, down, n_taps, pre_pad, pre_remove): plan()'s integers without the taps."""
    g = math.gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    half_len = filter_half_len(up, down)
    pre_pad = down - half_len % down
    return up, down, 2 * half_len + 1, pre_pad, (half_len + pre_pad) // down


def plan(n_in, sr_in, sr_out):
    up, down, n_taps, pre_pad, pre_remove = _ratio(sr_in, sr_out)
    n_out = -(-n_in * up // down)
    taps, _ = design_taps(up, down)
    assert len(taps) == n_taps                       # stream_plan / stream_capacity count the taps without designing them
    return dict(up=up, down=down, n_out=n_out, taps=taps, pre_pad=pre_pad, pre_remove=pre_remove)


def stream_capacity(sr_in, sr_out, piece_frames):
    """The frames (per plane) a segment buffer must hold to resample a recording in pieces of at most `piece_frames` frames: the
    frames retained from the pieces before plus one piece.  It depends on the ratio and the piece size only.
    The retained frames are at most row - 1, row = ceil(n_taps / up): behind a piece that ends at frame E (exclusive) the first
    output m not yet emitted has k_c(m) = floor(c / up) >= E, i.e. c >= E * up, hence
    k_lo(m) >= ceil((E * up - n_taps + 1) / up) = E - floor((n_taps - 1) / up) = E - (row - 1), and frames k_lo(m) .. E - 1 are kept."""
    up, _, n_taps, _, _ = _ratio(sr_in, sr_out)
    return -(-n_taps // up) - 1 + int(piece_frames)


def stream_plan(n_in, sr_in, sr_out, piece_frames):
    """Resampling a recording of n_in frames piece by piece (wseg_resample_planar_range_f32), pure arithmetic: for every piece
    [frame0, frame0 + n) of at most `piece_frames` frames, in order, yields dict(frame0, n, x_first, m_first, m_count, keep_from):
      m_first .. m_first + m_count - 1  the outputs that become computable with this piece — those whose chain ends inside it or
                                        before it, k_c(m) <= frame0 + n - 1, and that no earlier piece emitted; on the last piece
                                        all that remain.  m_count == 0 is legal (a piece shorter than the step between two outputs);
      x_first                           the first frame the segment holds when they are computed: keep_from of the piece before
                                        (0 for the first), so the segment is [x_first, frame0 + n);
      keep_from                         the first frame still needed afterwards: min(k_lo(next output), frame0 + n); frame0 + n once
                                        every output has been emitted.
    frame0 + n - keep_from never exceeds stream_capacity(sr_in, sr_out, piece_frames) - piece_frames."""
    n_in, piece_frames = int(n_in), int(piece_frames)
    if piece_frames <= 0:
        raise ValueError("piece_frames must be positive")
    up, down, n_taps, pre_pad, pre_remove = _ratio(sr_in, sr_out)
    n_out = -(-n_in * up // down)
    emitted, x_first = 0, 0
    for frame0 in range(0, n_in, piece_frames):
        n = min(piece_frames, n_in - frame0)
        end = frame0 + n
        if end >= n_in:
            m_end = n_out
        else:        # floor(c / up) <= end - 1  <=>  (m + pre_remove) * down <= (end - 1) * up + up - 1 + pre_pad
            m_end = min(n_out, max(emitted, (end * up - 1 + pre_pad) // down - pre_remove + 1))
        keep_from = end
        if m_end < n_out:
            c = (m_end + pre_remove) * down - pre_pad
            keep_from = min(max(0, -(-(c - n_taps + 1) // up)), end)
        yield dict(frame0=frame0, n=n, x_first=x_first, m_first=emitted, m_count=m_end - emitted, keep_from=keep_from)
        emitted, x_first = m_end, keep_from


PLANAR_GRID_CAP = 2048           # kResampleGridCap of csrc/wseg_resample.hip: with more tiles x planes than this the workgroups take a grid stride
MAX_PLANES = 64

_TAPS = {}


def launch_plan(n_in, sr_in, sr_out):
    """What wseg_resample_planar_f32 launches for this ratio (wseg_debug_resample_plan: host arithmetic, no device)
    -> dict(tile, window, x_staged, taps_staged)."""
    lib = _lib.load()
    p = plan(int(n_in), sr_in, sr_out)
    out = [C.c_int32() for _ in range(4)]
    _lib.check(lib.wseg_debug_resample_plan(int(n_in), p["n_out"], len(p["taps"]), p["up"], p["down"], p["pre_pad"], p["pre_remove"],
                                            *[C.byref(v) for v in out]), lib)
    return dict(zip(("tile", "window", "x_staged", "taps_staged"), (v.value for v in out)))


def _device_taps(p, device):
    key = (p["up"], p["down"], str(device))
    if key not in _TAPS:
        _TAPS[key] = torch.from_numpy(p["taps"]).to(device)
    return _TAPS[key]


def resample(audio, sr_in, sr_out, device="cuda"):
    """audio: float32 numpy array or device tensor, [N] or [channels, N], at sr_in -> float32 device tensor at sr_out of the same
    rank.  [N] goes through wseg_resample_f32; [channels, N] through ONE wseg_resample_planar_f32 launch whose rows have the
    bits of the 1-D call.  Rows of a device tensor with unit sample stride and a row stride of at least N are read where they
    are (rows of a larger tensor); anything else — numpy arrays, reversed or transposed views — is copied first."""
    x = audio if torch.is_tensor(audio) else torch.as_tensor(np.ascontiguousarray(audio, dtype=np.float32))
    if x.ndim not in (1, 2):
        raise ValueError("audio must be [n] or [channels, n]")
    x = x.to(device=device, dtype=torch.float32)
    if x.ndim == 1 or x.stride(-1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    if int(sr_in) == int(sr_out):
        return x.clone()
    lib = _lib.load(require_device=True)
    n_in = int(x.shape[-1])
    p = plan(n_in, sr_in, sr_out)
    y = torch.empty(tuple(x.shape[:-1]) + (p["n_out"],), dtype=torch.float32, device=x.device)
    if not (p["n_out"] and n_in and y.numel()):
        return y.zero_()
    taps = _device_taps(p, x.device)
    with torch.cuda.device(x.device):
        if x.ndim == 1:
            _lib.check(lib.wseg_resample_f32(x.data_ptr(), n_in, taps.data_ptr(), int(taps.numel()), p["up"], p["down"],
                                             p["pre_pad"], p["pre_remove"], y.data_ptr(), p["n_out"], _lib.stream_ptr()))
        else:
            if x.shape[0] > MAX_PLANES:
                raise ValueError(f"{x.shape[0]} channels (one resample launch takes up to {MAX_PLANES})")
            _lib.check(lib.wseg_resample_planar_f32(x.data_ptr(), n_in, int(x.stride(0)), int(x.shape[0]), taps.data_ptr(),
                                                    int(taps.numel()), p["up"], p["down"], p["pre_pad"], p["pre_remove"], y.data_ptr(),
                                                    p["n_out"], int(y.stride(0)), _lib.stream_ptr()))
    return y
