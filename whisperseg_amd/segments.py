"""What the per-segment analyses of a recording's resident PCM share on the Python side (measure.py, patches.py, pitch.py): a row's
sample range, the recording's way to the device, and the argument checks and scratch of their `*_rows` launch functions."""
import math

import numpy as np

from . import _lib


def sample_bounds(onset, offset, sr, n):
    """(s0, s1) of a segment: half-sample rounding, clamped to the recording, never reversed."""
    s0 = min(max(int(math.floor(onset * sr + 0.5)), 0), n)
    s1 = max(s0, min(max(int(math.floor(offset * sr + 0.5)), 0), n))
    return s0, s1


def bounds_of(prediction, sr, n):
    """int64 [n_seg, 2]: sample_bounds of every row of a prediction dict."""
    rows = [sample_bounds(float(on), float(off), sr, n) for on, off in zip(prediction["onset"], prediction["offset"])]
    return np.asarray(rows, dtype=np.int64).reshape(-1, 2)


def device_pcm(audio, device):
    """numpy [n] (uploaded to `device`) or a tensor (a device tensor stays where it lies) -> contiguous float32 device tensor [n]."""
    import torch
    if torch.is_tensor(audio):
        pcm = audio.to(dtype=torch.float32).contiguous() if audio.is_cuda else audio.to(device=device, dtype=torch.float32).contiguous()
    else:
        pcm = torch.as_tensor(np.ascontiguousarray(audio, dtype=np.float32)).to(device)
    if pcm.dim() != 1:
        raise ValueError("audio must be one mono recording [n]")
    return pcm


def check_pcm(pcm, who):
    """WsegError unless `pcm` is what the launch function `who` takes: a contiguous float32 device tensor [n]."""
    import torch
    if not (torch.is_tensor(pcm) and pcm.is_cuda and pcm.dtype == torch.float32 and pcm.dim() == 1 and pcm.is_contiguous()):
        raise _lib.WsegError(f"{who} needs a contiguous float32 device tensor [n] (no CPU path)")


def check_out(out, shape, what, device):
    """`out` (WsegError unless it is a contiguous float32 device tensor of `shape`, `what` in words), or a new one on `device`."""
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not (out.is_cuda and out.dtype == torch.float32 and out.shape == tuple(shape) and out.is_contiguous()):
        raise _lib.WsegError(f"out must be a contiguous float32 device tensor {what}")
    return out


def new_scratch(nbytes, device):
    import torch
    return torch.empty(nbytes, dtype=torch.uint8, device=device)
