"""Sample-rate conversion on the GPU (audio ingest).

The reference resamples implicitly through `librosa.load(path, sr=target)` (scripts/segment.py:48,61, evaluate.py:58):
a third-party resampler that is neither pinned nor installed here.  This module implements the standard rational
polyphase scheme — Kaiser(beta=5)-windowed sinc low-pass of half-length 10*max(up, down), unity DC gain times `up`,
centred output of ceil(n*up/down) samples — which is also what `scipy.signal.resample_poly` computes; the arithmetic runs
in libwseg: `wseg_resample_f32` for one signal, `wseg_resample_planar_f32` for the channels of a recording kept apart
([channels, n]: one launch, every row with the bits of the one-signal call).  The file path resamples through here:
wavio.DeviceIngest.resample, hence FilePipeline(sr=), load_wav_device(sr=), segment_files(sr=) and the CLI's --sr."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib


def design_taps(up, down, beta=5.0):
    """float32 FIR taps (already scaled by `up`) + half length, for the reduced ratio up/down."""
    max_rate = max(up, down)
    half_len = 10 * max_rate
    n = 2 * half_len + 1
    m = np.arange(n, dtype=np.float64) - half_len
    cutoff = 1.0 / max_rate
    h = cutoff * np.sinc(cutoff * m) * np.kaiser(n, beta)
    h /= h.sum()
    h = h.astype(np.float32)
    h *= np.float32(up)
    return h, half_len


def plan(n_in, sr_in, sr_out):
    g = math.gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    n_out = -(-n_in * up // down)
    taps, half_len = design_taps(up, down)
    pre_pad = down - half_len % down
    pre_remove = (half_len + pre_pad) // down
    return dict(up=up, down=down, n_out=n_out, taps=taps, pre_pad=pre_pad, pre_remove=pre_remove)


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
