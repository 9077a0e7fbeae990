"""What the per-segment analyses of a recording's resident PCM share on the Python side (measure.py, patches.py, pitch.py) that is about
segments: a row's sample range and the recording's way to the device.  The argument checks, the outputs and the scratch of their
`*_rows` launch functions are resident.py's, as they are of every other analysis."""
import math

import numpy as np

from . import resident as RS


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
    """resident.resident of one mono recording [n]; ValueError for another rank."""
    pcm = RS.resident(audio, device)
    if pcm.dim() != 1:
        raise ValueError("audio must be one mono recording [n]")
    return pcm
