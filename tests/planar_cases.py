"""Expected values of the planar (channels kept apart) WAVE decode, shared by test_wav_planar_cpu.py and
test_ingest_planar_gpu.py: wav_cases.restate applied with channels=1 to the bytes of ONE channel picked out of the interleaved
data chunk on the host — a restatement independent of wavio.load_wav."""
import numpy as np

import wav_cases as WC


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def channel_bytes(data, fmt, channels, n_frames, c):
    code = WC.FORMATS.index(fmt) if isinstance(fmt, str) else int(fmt)
    b = np.frombuffer(bytes(data), np.uint8)[:n_frames * channels * WC.BYTES[code]].reshape(n_frames, channels, WC.BYTES[code])
    return b[:, c].tobytes()


def planes(data, fmt, channels, n_frames, first=0, count=None):
    """float32 [count, n_frames]: channels first .. first + count - 1 of the data chunk `data`."""
    count = channels - first if count is None else count
    rows = [WC.restate(channel_bytes(data, fmt, channels, n_frames, c), fmt, 1, n_frames) for c in range(first, first + count)]
    return np.stack(rows).astype(np.float32).reshape(count, n_frames)


def data_chunk(fmt, channels, n_frames, seed=0):
    """The data chunk WC.make_wav(fmt, channels, n_frames, seed) wraps."""
    rng = np.random.default_rng([seed, WC.FORMATS.index(fmt), channels, n_frames])
    return WC.sample_bytes(fmt, WC.random_samples(fmt, n_frames * channels, rng))
