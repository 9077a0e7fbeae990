"""In-memory RIFF/WAVE files of every sample format the ingest handles, and a numpy restatement of the arithmetic
wseg_pcm_to_mono_f32 is specified by (include/wseg.h), applied to the raw bytes of a data chunk.  Shared by
test_wav_raw_cpu.py and test_ingest_gpu.py."""
import struct

import numpy as np

FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")        # index = wseg_pcm_format
BYTES = (1, 2, 3, 4, 4, 8)
TAG_BITS = {"u8": (1, 8), "s16": (1, 16), "s24": (1, 24), "s32": (1, 32), "f32": (3, 32), "f64": (3, 64)}

# values planted in the first samples: integer extremes, s32 values that round on the way to float32, float64 values that tie
# between two float32s (2^-24 and 3 * 2^-24 above 1: half an ulp; round-to-nearest-even goes down resp. up), a float32 denormal,
# values beyond the float32 range (positive only: inf - inf in a frame would be a NaN), signed zeros.  No NaNs: payloads are
# not part of the contract.
SPECIAL = {
    "u8": [0, 255, 128, 127, 129, 1],
    "s16": [-32768, 32767, 0, -1, 1, 255, 256, -256],
    "s24": [-(1 << 23), (1 << 23) - 1, 0, -1, 1, 0x7FFF, 0x8000, -0x8000, 0x10000, -0x10001, 255, 256],
    "s32": [-(1 << 31), (1 << 31) - 1, 0, -1, 1, (1 << 24) + 1, (1 << 31) - 65, -(1 << 24) - 1, (1 << 24) + 3, (1 << 25) + 2, -(1 << 31) + 64],
    "f32": [0.0, -0.0, 1.0, -1.0, 1e-45, -1e-40, 3.4028234663852886e38, 0.1],
    "f64": [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24), 1e-40, -1e-45, 1e39, 1e300, 0.0, -0.0, 0.1, 1e-50, 3.4028235677973366e38],
}


def sample_bytes(fmt, values):
    """Little-endian bytes of integer / float sample values."""
    if fmt == "u8":
        return np.asarray(values, np.uint8).tobytes()
    if fmt == "s16":
        return np.asarray(values, "<i2").tobytes()
    if fmt == "s24":
        v = np.asarray(values, np.int64) & 0xFFFFFF
        return np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).tobytes()
    if fmt == "s32":
        return np.asarray(values, "<i4").tobytes()
    return np.asarray(values, "<f4" if fmt == "f32" else "<f8").tobytes()


def random_samples(fmt, n, rng, special=True):
    """n sample values of the format: random, the SPECIAL ones first."""
    if fmt in ("f32", "f64"):
        v = rng.uniform(-1, 1, n)
        v = v.astype(np.float32).astype(np.float64) if fmt == "f32" else v
    else:
        bits = TAG_BITS[fmt][1]
        lo, hi = (0, 256) if fmt == "u8" else (-(1 << (bits - 1)), 1 << (bits - 1))
        v = rng.integers(lo, hi, n, dtype=np.int64)
    if special:
        sp = np.asarray(SPECIAL[fmt], v.dtype)[:n]
        v[:len(sp)] = sp
    return v


def wav_bytes(fmt, channels, sr, data, extensible=False, junk_before_data=0):
    """A RIFF/WAVE file around the data chunk `data`; junk_before_data > 0 puts a chunk of that many bytes (odd sizes are
    padded, as RIFF demands) in front of it."""
    tag, bits = TAG_BITS[fmt]
    block = channels * bits // 8
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, sr, sr * block, block, bits)
    if extensible:
        body += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    chunks = b"fmt " + struct.pack("<I", len(body)) + body
    if junk_before_data:
        chunks += b"LIST" + struct.pack("<I", junk_before_data) + b"j" * junk_before_data + b"\x00" * (junk_before_data % 2)
    chunks += b"data" + struct.pack("<I", len(data)) + data + b"\x00" * (len(data) % 2)
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def make_wav(fmt, channels, n_frames, seed=0, sr=16000, **kw):
    rng = np.random.default_rng([seed, FORMATS.index(fmt), channels, n_frames])
    return wav_bytes(fmt, channels, sr, sample_bytes(fmt, random_samples(fmt, n_frames * channels, rng)), **kw)


def f32(x):
    return np.asarray(x, np.float32)


def restate(raw, fmt, channels, n_frames):
    """The specified arithmetic on the bytes of a data chunk -> float32 [n_frames].  Every step is a float32 operation written
    out on its own (no float64 intermediate except the one conversion of f64 samples and the int32 values of s32 on their way to
    ONE rounding)."""
    code = FORMATS.index(fmt) if isinstance(fmt, str) else int(fmt)
    b = np.frombuffer(bytes(raw), np.uint8)[:n_frames * channels * BYTES[code]].reshape(-1, BYTES[code]).astype(np.int64)
    word = sum(b[:, i] << (8 * i) for i in range(BYTES[code]))
    if code == 0:
        x = (word.astype(np.float32) - f32(128)) / f32(128)
    elif code == 1:
        x = (((word ^ 0x8000) - 0x8000).astype(np.float32)) / f32(32768)
    elif code == 2:
        x = (((word ^ 0x800000) - 0x800000).astype(np.float32)) / f32(1 << 23)
    elif code == 3:
        x = ((word ^ 0x80000000) - 0x80000000).astype(np.float32) * f32(2.0 ** -31)       # int64 -> float32: one rounding
    elif code == 4:
        x = word.astype(np.uint32).view(np.float32)
    else:
        with np.errstate(over="ignore"):
            x = word.astype(np.uint64).view(np.float64).astype(np.float32)
    x = x.reshape(n_frames, channels)
    if channels == 1:
        return x[:, 0].copy()
    col = [x[:, c] for c in range(channels)]
    with np.errstate(invalid="ignore", over="ignore"):
        if channels < 8:                             # left to right
            s = col[0]
            for c in range(1, channels):
                s = s + col[c]
        else:                                        # numpy's pairwise order: 8 strided partial sums, a tree, the rest one by one
            r = col[:8]
            c = 8
            while c < channels - channels % 8:
                r = [r[j] + col[c + j] for j in range(8)]
                c += 8
            s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            for c in range(c, channels):
                s = s + col[c]
        return (f32(0) + s) / f32(channels)          # the sum starts from +0: a frame of -0.0 samples gives +0.0
