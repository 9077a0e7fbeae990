"""In-memory RIFF/WAVE files of format tag 0x0011 (IMA / DVI ADPCM), their blocks — random bytes behind random valid headers, which
saturate both clamps of the arithmetic constantly, or a signal encoded by the stdlib's audioop.lin2adpcm — and the stdlib's decode of
them: audioop.adpcm2lin, an implementation of the IMA step and index arithmetic that shares nothing with whisperseg_amd.wavio.  It
takes the HIGH nibble of a byte first where WAVE stores the low one first, so bytes are nibble-swapped on the way in and out.  Shared
by test_ima_adpcm_cpu.py and test_ima_adpcm_gpu.py."""
import audioop
import struct

import numpy as np

TAG = 0x0011
SWAP = bytes(((b & 15) << 4) | (b >> 4) for b in range(256))


def block_frames(channels, block_bytes):
    return 2 * (block_bytes // channels - 4) + 1


def random_blocks(channels, block_bytes, n_blocks, seed=0, index_hi=89):
    """n_blocks blocks of random nibbles; every channel header a random int16 predictor, a step index in [0, index_hi) and a zero
    reserved byte."""
    rng = np.random.default_rng([seed, channels, block_bytes, n_blocks])
    b = rng.integers(0, 256, (n_blocks, block_bytes), dtype=np.uint8)
    head = b[:, :4 * channels].reshape(n_blocks, channels, 4)
    head[:, :, 2] = rng.integers(0, index_hi, (n_blocks, channels))
    head[:, :, 3] = 0
    return b.tobytes()


def encode(x, block_bytes):
    """int16 [n, channels] -> blocks (the last one padded with its last frame): per block and channel the header is the block's
    first sample and the step index the encoder arrived at, the rest audioop.lin2adpcm's nibbles, swapped."""
    n, channels = x.shape
    spb = block_frames(channels, block_bytes)
    n_blocks = -(-n // spb)
    if n_blocks * spb > n:
        x = np.concatenate([x, np.repeat(x[-1:], n_blocks * spb - n, axis=0)])
    index = [0] * channels
    out = bytearray()
    for blk in x.reshape(n_blocks, spb, channels):
        body = []
        for c in range(channels):
            first = int(blk[0, c])
            out += struct.pack("<hBB", first, index[c], 0)
            code, (_, index[c]) = audioop.lin2adpcm(blk[1:, c].astype("<i2").tobytes(), 2, (first, index[c]))
            body.append(np.frombuffer(code.translate(SWAP), np.uint8).reshape(-1, 4))
        out += np.stack(body, axis=1).tobytes()                       # [group, channel, 4 bytes]
    return bytes(out)


def audioop_decode(raw, channels, block_bytes):
    """-> int16 [n_blocks * spb, channels]: audioop.adpcm2lin run per (block, channel) on the channel's nibble-swapped bytes with
    the header as state (a header index above 88, which audioop refuses as a state, enters as 88)."""
    spb = block_frames(channels, block_bytes)
    n_blocks = len(raw) // block_bytes
    b = np.frombuffer(raw, np.uint8, n_blocks * block_bytes).reshape(n_blocks, block_bytes)
    out = np.empty((n_blocks, spb, channels), np.int16)
    for i in range(n_blocks):
        data = b[i, 4 * channels:].reshape(-1, channels, 4)
        for c in range(channels):
            pred, index = struct.unpack("<hB", b[i, 4 * c:4 * c + 3].tobytes())
            out[i, 0, c] = pred
            pcm, _ = audioop.adpcm2lin(data[:, c].tobytes().translate(SWAP), 2, (pred, min(index, 88)))
            out[i, 1:, c] = np.frombuffer(pcm, "<i2")
    return out.reshape(n_blocks * spb, channels)


def fmt_chunk(channels, sr, block_bytes, bits=4, samples_per_block="auto", tag=TAG):
    """The `fmt ` chunk; samples_per_block: "auto" — what the block size gives; an int — that value; None — no extension."""
    spb = block_frames(channels, block_bytes) if samples_per_block == "auto" else samples_per_block
    body = struct.pack("<HHIIHH", tag, channels, sr, sr * block_bytes // max(block_frames(channels, block_bytes), 1), block_bytes, bits)
    if spb is not None:
        body += struct.pack("<HH", 2, spb)
    return b"fmt " + struct.pack("<I", len(body)) + body


def wav_bytes(channels, sr, block_bytes, data, fact=None, trailing=b"", **fmt):
    """A RIFF/WAVE file around the blocks `data` (any length: a partial block or an odd byte count is written as it is, padded as
    RIFF demands); fact: the sample count of a `fact` chunk in front of the data, None for no such chunk; trailing: chunk bytes
    behind the data."""
    chunks = fmt_chunk(channels, sr, block_bytes, **fmt)
    if fact is not None:
        chunks += b"fact" + struct.pack("<II", 4, fact)
    chunks += b"data" + struct.pack("<I", len(data)) + data + b"\x00" * (len(data) % 2) + trailing
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def list_chunk(n):
    return b"LIST" + struct.pack("<I", n) + b"\x7f" * n + b"\x00" * (n % 2)


def make_wav(channels, block_bytes, n_blocks, seed=0, sr=16000, cut=0, **kw):
    """A file of random blocks; cut > 0: a `fact` chunk that cuts that many frames off the last block."""
    data = random_blocks(channels, block_bytes, n_blocks, seed)
    fact = n_blocks * block_frames(channels, block_bytes) - cut if cut else kw.pop("fact", None)
    return wav_bytes(channels, sr, block_bytes, data, fact=fact, **kw)


def floats(pcm, mono=True):
    """int16 [n, channels] -> what load_audio gives for it: / 2^15 in float32, numpy's float32 mean over a frame or the rows."""
    x = pcm.astype(np.float32) / np.float32(32768)
    if pcm.shape[1] == 1:
        return np.ascontiguousarray(x[:, 0])
    return x.mean(axis=1).astype(np.float32) if mono else np.ascontiguousarray(x.T)
