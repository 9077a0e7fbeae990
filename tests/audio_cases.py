"""In-memory AIFF / AIFF-C, AU, RF64 / BW64 and G.711 WAVE files, and a numpy restatement of the arithmetic
wseg_samples_to_mono_f32 is specified by (include/wseg.h) for the encodings 6..13, in the style of wav_cases (which it reuses for
0..5 and for the channel mean).  Shared by test_audio_containers_cpu.py and test_audio_ingest_gpu.py."""
import io
import math
import struct

import numpy as np

import wav_cases as WC

ENCODINGS = WC.FORMATS + ("s8", "s16be", "s24be", "s32be", "f32be", "f64be", "ulaw", "alaw")      # index = wseg_sample_encoding
BYTES = WC.BYTES + (1, 2, 3, 4, 4, 8, 1, 1)
NEW = ENCODINGS[6:]
SIBLING = {"s16be": "s16", "s24be": "s24", "s32be": "s32", "f32be": "f32", "f64be": "f64"}       # the same values, bytes reversed

# planted in the first samples: the extremes of every width; wav_cases.SPECIAL (byte-swapped by sample_bytes) for the big-endian
# encodings; all 256 codes for G.711
SPECIAL = dict({k: WC.SPECIAL[v] for k, v in SIBLING.items()}, s8=[-128, 127, 0, -1, 1, 64], ulaw=list(range(256)), alaw=list(range(256)))


def code_of(enc):
    return ENCODINGS.index(enc) if isinstance(enc, str) else int(enc)


def swap(data, width):
    """Every sample of `width` bytes reversed."""
    return np.frombuffer(bytes(data), np.uint8).reshape(-1, width)[:, ::-1].tobytes()


def sample_bytes(enc, values):
    """The bytes of integer / float sample values (G.711: the values are the codes) as the encoding stores them."""
    if enc in WC.FORMATS:
        return WC.sample_bytes(enc, values)
    if enc == "s8":
        return np.asarray(values, np.int8).tobytes()
    if enc in ("ulaw", "alaw"):
        return np.asarray(values, np.uint8).tobytes()
    return swap(WC.sample_bytes(SIBLING[enc], values), BYTES[code_of(enc)])


def random_samples(enc, n, rng, special=True):
    if enc in WC.FORMATS:
        return WC.random_samples(enc, n, rng, special)
    if enc in SIBLING:
        v = WC.random_samples(SIBLING[enc], n, rng, special=False)
    else:
        lo, hi = (-128, 128) if enc == "s8" else (0, 256)
        v = rng.integers(lo, hi, n, dtype=np.int64)
    if special:
        sp = np.asarray(SPECIAL[enc], v.dtype)[:n]
        v[:len(sp)] = sp
    return v


def random_data(enc, channels, n_frames, seed=0):
    rng = np.random.default_rng([seed, code_of(enc), channels, n_frames])
    return sample_bytes(enc, random_samples(enc, n_frames * channels, rng))


# ---- containers ---------------------------------------------------------------------------------------------------------------
def ext80(rate):
    """A positive number as the 80-bit extended float of an AIFF COMM chunk."""
    if isinstance(rate, int):
        e = rate.bit_length() - 1
        return struct.pack(">HQ", 16383 + e, rate << (63 - e))
    m, e = math.frexp(rate)
    return struct.pack(">HQ", 16383 + e - 1, int(m * 2.0 ** 64))


def _chunk_be(cid, body):
    return cid + struct.pack(">I", len(body)) + body + b"\x00" * (len(body) % 2)


def aiff_bytes(channels, sr, bits, data, n_frames=None, compression=None, ssnd_offset=0, comm_last=False, extra=b""):
    """FORM AIFF (compression None) or FORM AIFC (a four-cc) around the sample bytes `data`; n_frames: the COMM chunk's count
    (default: the whole frames of `data` at ceil(bits / 8) bytes a sample); ssnd_offset: bytes between the SSND header and the
    samples; comm_last: COMM behind SSND; extra: a chunk placed in front of both."""
    if n_frames is None:
        n_frames = len(data) // (channels * ((bits + 7) // 8))
    comm = struct.pack(">hIh", channels, n_frames, bits) + ext80(sr)
    if compression is not None:
        comm += compression + b"\x00\x00"        # an empty Pascal string, padded to even length
    comm = _chunk_be(b"COMM", comm)
    ssnd = _chunk_be(b"SSND", struct.pack(">II", ssnd_offset, 0) + b"\xA5" * ssnd_offset + data)
    fver = _chunk_be(b"FVER", struct.pack(">I", 0xA2805140)) if compression is not None else b""
    body = fver + extra + (ssnd + comm if comm_last else comm + ssnd)
    return b"FORM" + struct.pack(">I", 4 + len(body)) + (b"AIFF" if compression is None else b"AIFC") + body


AU_CODES = {"ulaw": 1, "s8": 2, "s16be": 3, "s24be": 4, "s32be": 5, "f32be": 6, "f64be": 7, "alaw": 27}


def au_bytes(encoding, channels, sr, data, size=None, annotation=b""):
    """A Sun/NeXT .snd file; encoding: the header's number (or one of AU_CODES' names); size None: len(data), else the header's
    value (0xFFFFFFFF: unknown); annotation: bytes between the 24-byte header and the samples."""
    number = AU_CODES[encoding] if isinstance(encoding, str) else encoding
    return struct.pack(">4s5I", b".snd", 24 + len(annotation), len(data) if size is None else size, number, sr, channels) + annotation + data


G711_TAG = {"alaw": 6, "ulaw": 7}


def wav_chunks(tag, bits, channels, sr, extensible=False):
    block = channels * bits // 8
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, sr, sr * block, block, bits)
    if extensible:
        body += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    return b"fmt " + struct.pack("<I", len(body)) + body


def g711_wav_bytes(enc, channels, sr, data, extensible=False):
    """A RIFF/WAVE file with format tag 6 (A-law) or 7 (u-law) at 8 bits."""
    chunks = wav_chunks(G711_TAG[enc], 8, channels, sr, extensible) + b"data" + struct.pack("<I", len(data)) + data + b"\x00" * (len(data) % 2)
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def rf64_bytes(fmt, channels, sr, data, riff_id=b"RF64", trailing=b"", ds64=True):
    """The RF64 / BW64 form of wav_cases.wav_bytes(fmt, ...): riff and data size fields 0xFFFFFFFF, the sizes in a ds64 chunk
    (ds64=False leaves it out), `trailing`: chunk bytes behind the samples."""
    tag, bits = WC.TAG_BITS[fmt]
    after = wav_chunks(tag, bits, channels, sr) + b"data" + struct.pack("<I", 0xFFFFFFFF) + data + b"\x00" * (len(data) % 2) + trailing
    d = b""
    if ds64:
        body = struct.pack("<QQQI", 4 + 8 + 28 + len(after), len(data), len(data) // (channels * bits // 8), 0)
        d = b"ds64" + struct.pack("<I", len(body)) + body
    return riff_id + struct.pack("<I", 0xFFFFFFFF) + b"WAVE" + d + after


def list_chunk(n):
    """A trailing LIST chunk of n payload bytes that would decode as loud samples."""
    return b"LIST" + struct.pack("<I", n) + b"\x7f\x80" * (n // 2) + b"\x7f" * (n % 2) + b"\x00" * (n % 2)


def container_bytes(enc, channels, sr, data):
    """A file of the encoding's usual container around the sample bytes: AIFF for signed big-endian PCM, AIFF-C for big-endian
    floats, AU for u-law, WAVE for A-law and the six wseg_pcm_format encodings."""
    if enc in WC.FORMATS:
        return WC.wav_bytes(enc, channels, sr, data)
    if enc in ("s8", "s16be", "s24be", "s32be"):
        return aiff_bytes(channels, sr, 8 * BYTES[code_of(enc)], data)
    if enc in ("f32be", "f64be"):
        return aiff_bytes(channels, sr, 8 * BYTES[code_of(enc)], data, compression=b"fl32" if enc == "f32be" else b"fl64")
    if enc == "ulaw":
        return au_bytes("ulaw", channels, sr, data)
    return g711_wav_bytes("alaw", channels, sr, data)


def make_audio(enc, channels, n_frames, seed=0, sr=16000):
    return container_bytes(enc, channels, sr, random_data(enc, channels, n_frames, seed))


class KeptBytesIO(io.BytesIO):
    """A BytesIO that survives the close() of the stdlib writers (aifc, sunau)."""

    def close(self):
        pass


# ---- the specified arithmetic -------------------------------------------------------------------------------------------------
def g711_tables():
    """(u-law, A-law) int16 tables of the stdlib."""
    import audioop
    codes = bytes(range(256))
    return np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2"), np.frombuffer(audioop.alaw2lin(codes, 2), "<i2")


def restate(raw, encoding, channels, n_frames):
    """wav_cases.restate for every wseg_sample_encoding: big-endian samples are byte-swapped and go through their sibling; s8 and
    G.711 become float32 samples by the header's arithmetic (x / 128; the int16 table, then x / 2^15), whose channel mean is that
    of the f32 encoding."""
    code = code_of(encoding)
    if code < 6:
        return WC.restate(raw, code, channels, n_frames)
    enc = ENCODINGS[code]
    raw = bytes(raw)[:n_frames * channels * BYTES[code]]
    if enc in SIBLING:
        return WC.restate(swap(raw, BYTES[code]), SIBLING[enc], channels, n_frames)
    b = np.frombuffer(raw, np.uint8).astype(np.int64)
    if enc == "s8":
        x = ((b ^ 0x80) - 0x80).astype(np.float32) / WC.f32(128)
    else:
        x = g711_tables()[0 if enc == "ulaw" else 1][b].astype(np.float32) / WC.f32(32768)
    return WC.restate(x.astype("<f4").tobytes(), "f32", channels, n_frames)


def restate_planar(raw, encoding, channels, n_frames):
    """-> float32 [channels, n_frames]: every sample converted, no mean (each channel as a one-channel recording)."""
    code = code_of(encoding)
    b = np.frombuffer(bytes(raw), np.uint8)[:n_frames * channels * BYTES[code]].reshape(n_frames, channels, BYTES[code])
    return np.stack([restate(b[:, c].tobytes(), code, 1, n_frames) for c in range(channels)])
