"""Audio file reader standing in for `librosa.load(path, sr=None)` (reference scripts/segment.py:48,61; librosa/soundfile are
not in the image): native sampling rate, float32 in [-1, 1), channels averaged to mono — or, with mono=False, kept apart as
`librosa.load(..., mono=False)` does for the reference's `channel_id` (segment_service.py:73-80, scripts/backend.py:279-282,
demo.py:76-78).
Containers (sniffed from the first 12 bytes; load_audio / scan_audio / read_audio_raw):
  RIFF/WAVE, RF64, BW64 — PCM 8/16/24/32-bit, IEEE float 32/64, G.711 A-law / u-law (tags 6 / 7), IMA / DVI ADPCM (tag 0x11,
      4 bits), WAVE_FORMAT_EXTENSIBLE; an RF64 / BW64 `ds64` chunk supplies the size of a `data` chunk whose own size field is
      0xFFFFFFFF (load_wav / scan_wav / read_wav_raw refuse everything else; _walk_wav is the one walk over the chunks)
  AIFF / AIFF-C — big-endian PCM of 1..32 bits (8-bit signed); compression NONE / twos / sowt / `raw ` / fl32 / fl64 / ulaw / alaw
  AU (.snd) — u-law, A-law, 8/16/24/32-bit linear, float 32/64
IMA ADPCM is the one compressed encoding that is read, and the one BLOCK codec: a block of nBlockAlign bytes holds, per channel, a
4-byte header (int16 predictor = the block's first sample, u8 step index, u8 reserved) and then groups of 4 bytes per channel, low
nibble first; decode_ima_adpcm is the definition (the standard's integer arithmetic, pinned against the stdlib's audioop.adpcm2lin).
Its frame count is the `fact` chunk's where there is one that the whole blocks can hold, else blocks x samples per block; bytes
behind the last whole block are dropped.  MS ADPCM (tag 2), AIFF-C `ima4`, Wave64 and FLAC are not read: nothing in the image
decodes them independently, so no test could pin their arithmetic.
Integer samples are divided by 2^(bits-1) of their container width, G.711 codes go through the standard's int16 expansion and ADPCM
through the standard's int16 predictor (then / 2^15), which is how libsndfile (behind librosa) produces its floats: equality with
it is by construction, not pinned by a test (soundfile is not in the image) — nor is libsndfile's treatment of `fact` and of a
partial last block.
load_wav / load_audio (one loader, _load, behind the container's header scan) keep the native rate; the device path
(load_wav_device, FilePipeline: one piece loop each, both over a FileOutput, which decodes through DeviceIngest.decode) takes `sr=`
and resamples on the GPU (whisperseg_amd.resample), all planes of a file at once and piece by piece as the file is read
(StreamResampler)."""
import collections
import io
import os
import queue
import struct
import threading

import numpy as np


# wseg_sample_encoding (include/wseg.h); 0..5 are wseg_pcm_format
PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32, PCM_F64 = range(6)
ENC_S8, ENC_S16BE, ENC_S24BE, ENC_S32BE, ENC_F32BE, ENC_F64BE, ENC_ULAW, ENC_ALAW = range(6, 14)
BYTES_PER_SAMPLE = (1, 2, 3, 4, 4, 8, 1, 2, 3, 4, 4, 8, 1, 1)
ENC_IMA_ADPCM = 14               # Python-side only: a block codec has no bytes per sample, and wseg_samples_to_* reject the code
MAX_CHANNELS = 64
STAGING_BYTES = 256 << 20        # one pinned staging buffer; a longer data chunk goes through in pieces
PLANAR_TILE_FRAMES = 1024        # kPlanarTile of csrc/wseg_ingest.hip: the frames a workgroup of wseg_samples_to_planar_f32 stages at a time
PLANAR_GRID_CAP = 2048           # kPlanarGridCap there: with more tiles than this the workgroups take a grid stride
ADPCM_GRID_CAP = 1024            # kAdpcmGridCap of csrc/wseg_ima_adpcm_plan.h: workgroups of the IMA ADPCM decode, floor(256 / channels) blocks each

WavRaw = collections.namedtuple("WavRaw", "data format channels sr n_frames")
# block_bytes / block_frames: bytes and frames of a block of a block codec (ENC_IMA_ADPCM; frame_bytes is 0 then), else 0
WavInfo = collections.namedtuple("WavInfo", "format channels sr n_frames frame_bytes offset block_bytes block_frames", defaults=(0, 0))

WAVE_IDS = (b"RIFF", b"RF64", b"BW64")


def _g711_tables():
    """The 256 int16 values of the u-law and A-law codes (ITU-T G.711's expansion; csrc/wseg_ingest.hip does the same arithmetic
    in registers)."""
    b = np.arange(256, dtype=np.int32)
    u = ~b & 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4)
    ulaw = np.where(u & 0x80, 0x84 - t, t - 0x84)
    a = b ^ 0x55
    seg = (a & 0x70) >> 4
    t = (a & 15) << 4
    t = np.where(seg > 0, (t + 0x108) << np.maximum(seg - 1, 0), t + 8)
    alaw = np.where(a & 0x80, t, -t)
    return ulaw.astype(np.int16), alaw.astype(np.int16)


ULAW_TO_S16, ALAW_TO_S16 = _g711_tables()


def _s24(raw, order):
    b = np.frombuffer(raw[: len(raw) // 3 * 3], np.uint8).reshape(-1, 3).astype(np.int32)
    lo, mid, hi = order
    v = b[:, lo] | (b[:, mid] << 8) | (b[:, hi] << 16)
    v = np.where(v >= 1 << 23, v - (1 << 24), v)
    return v.astype(np.float32) / float(1 << 23)


def _decode(raw, code):
    """Sample bytes of a wseg_sample_encoding -> float32 samples in file order: the definition of the arithmetic (bytes behind
    the last whole integer sample are dropped; float data must end with a sample)."""
    if code == PCM_U8:
        return (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0
    if code == ENC_S8:
        return np.frombuffer(raw, np.int8).astype(np.float32) / 128.0
    if code in (PCM_S16, ENC_S16BE):
        return np.frombuffer(raw[: len(raw) // 2 * 2], "<i2" if code == PCM_S16 else ">i2").astype(np.float32) / 32768.0
    if code in (PCM_S24, ENC_S24BE):
        return _s24(raw, (0, 1, 2) if code == PCM_S24 else (2, 1, 0))
    if code in (PCM_S32, ENC_S32BE):
        v = np.frombuffer(raw[: len(raw) // 4 * 4], "<i4" if code == PCM_S32 else ">i4")
        return (v.astype(np.float64) / float(1 << 31)).astype(np.float32)
    if code in (PCM_F32, PCM_F64, ENC_F32BE, ENC_F64BE):
        return np.frombuffer(raw, {PCM_F32: "<f4", PCM_F64: "<f8", ENC_F32BE: ">f4", ENC_F64BE: ">f8"}[code]).astype(np.float32)
    if code in (ENC_ULAW, ENC_ALAW):
        table = ULAW_TO_S16 if code == ENC_ULAW else ALAW_TO_S16
        return table[np.frombuffer(raw, np.uint8)].astype(np.float32) / 32768.0
    raise ValueError(f"unknown sample encoding {code}")


IMA_STEPS = np.array([
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157,
    173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707,
    1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635,
    13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], np.int32)
IMA_INDEX_STEPS = np.array([-1, -1, -1, -1, 2, 4, 6, 8], np.int32)


def ima_block_frames(channels, block_bytes, declared=None):
    """Frames of an IMA ADPCM block of `block_bytes` bytes: 2 * (block_bytes / channels - 4) + 1 (a header per channel, then whole
    groups of 4 bytes per channel); ValueError for a size no block can have, or when the header's wSamplesPerBlock (`declared`)
    says otherwise (libsndfile refuses such files too)."""
    if channels < 1 or block_bytes <= 4 * channels or (block_bytes - 4 * channels) % (4 * channels):
        raise ValueError(f"unsupported IMA ADPCM nBlockAlign {block_bytes} for {channels} channels (not a header and whole groups of "
                         f"4 bytes per channel)")
    spb = 2 * (block_bytes // channels - 4) + 1
    if declared is not None and declared != spb:
        raise ValueError(f"IMA ADPCM wSamplesPerBlock {declared} does not match the {spb} samples of a block of {block_bytes} bytes")
    return spb


def decode_ima_adpcm(raw, channels, block_bytes):
    """The whole blocks of `raw` (IMA / DVI ADPCM as WAVE lays it out, see the module's docstring) -> int16 [n_blocks * spb, channels]:
    the definition of the arithmetic, vectorised over blocks x channels with one loop over the spb - 1 steps of a chain.  Per nibble
    d: diff = step >> 3 (+ step if d & 4) (+ step >> 1 if d & 2) (+ step >> 2 if d & 1); the predictor moves down by it if d & 8,
    else up, and is clamped to int16; the step index moves by {-1,-1,-1,-1,2,4,6,8}[d & 7], clamped to 0..88 (a header's index above
    88 is taken as 88)."""
    spb = ima_block_frames(channels, block_bytes)
    n_blocks = len(raw) // block_bytes
    b = np.frombuffer(raw, np.uint8, n_blocks * block_bytes).reshape(n_blocks, block_bytes)
    head = b[:, :4 * channels].reshape(n_blocks, channels, 4)
    pred = head[:, :, :2].copy().view("<i2")[:, :, 0].astype(np.int32)
    index = np.minimum(head[:, :, 2].astype(np.int32), 88)
    data = b[:, 4 * channels:].reshape(n_blocks, (spb - 1) // 8, channels, 4)              # [block, group, channel, byte]
    nibbles = np.stack([data & 15, data >> 4], axis=-1).reshape(n_blocks, (spb - 1) // 8, channels, 8)      # low nibble first
    nibbles = nibbles.transpose(0, 1, 3, 2).reshape(n_blocks, spb - 1, channels).astype(np.int32)
    out = np.empty((n_blocks, spb, channels), np.int16)
    out[:, 0] = pred
    for k in range(spb - 1):
        d = nibbles[:, k]
        step = IMA_STEPS[index]
        diff = (step >> 3) + np.where(d & 4, step, 0) + np.where(d & 2, step >> 1, 0) + np.where(d & 1, step >> 2, 0)
        pred = np.clip(np.where(d & 8, pred - diff, pred + diff), -32768, 32767)
        index = np.clip(index + IMA_INDEX_STEPS[d & 7], 0, 88)
        out[:, k + 1] = pred
    return out.reshape(n_blocks * spb, channels)


def _channels(x, ch, mono):
    """Interleaved samples -> the mono mix (numpy's float32 mean over a frame), or with mono=False the rows of the channels."""
    if ch > 1 and not mono:
        x = x[: len(x) // ch * ch].reshape(-1, ch).T
    elif ch > 1:
        x = x[: len(x) // ch * ch].reshape(-1, ch).mean(axis=1).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def _pcm_format(tag, bits):
    """load_wav's dispatch on (format tag, width), with its errors."""
    if tag == 1:
        if bits not in (8, 16, 24, 32):
            raise ValueError(f"unsupported PCM width {bits}")
        return {8: PCM_U8, 16: PCM_S16, 24: PCM_S24, 32: PCM_S32}[bits]
    if tag == 3:
        return PCM_F32 if bits == 32 else PCM_F64
    if tag in (6, 7):
        if bits != 8:
            raise ValueError(f"unsupported G.711 width {bits}")
        return ENC_ALAW if tag == 6 else ENC_ULAW
    raise ValueError(f"unsupported WAVE format tag {tag}")


def _fmt_chunk(body):
    tag, ch, sr, _, _, bits = struct.unpack("<HHIIHH", body[:16])
    if tag == 0xFFFE and len(body) >= 26:
        tag = struct.unpack("<H", body[24:26])[0]
    return tag, ch, sr, bits


IMA_ADPCM_TAG = 0x0011


def _fmt_ima_adpcm(body):
    """The block fields of a tag-0x11 `fmt ` chunk -> (nBlockAlign, samples per block), checked: 4 bits per sample, and the
    extension's wSamplesPerBlock, where there is one, must be what the block size gives."""
    ch, block_bytes, bits = struct.unpack("<H", body[2:4])[0], struct.unpack("<H", body[12:14])[0], struct.unpack("<H", body[14:16])[0]
    if bits != 4:
        raise ValueError(f"unsupported IMA ADPCM width {bits}")
    declared = struct.unpack("<H", body[18:20])[0] if len(body) >= 20 and struct.unpack("<H", body[16:18])[0] >= 2 else None
    return block_bytes, ima_block_frames(max(int(ch), 1), block_bytes, declared)


def _ima_frames(data_bytes, block_bytes, spb, fact):
    """Frames of an IMA ADPCM data chunk: the `fact` chunk's count where the whole blocks can hold it, else all of theirs."""
    most = data_bytes // block_bytes * spb
    return fact if fact is not None and fact <= most else most


def _fact_chunk(body):
    return struct.unpack("<I", body[:4])[0] if len(body) >= 4 else None


def piece_bytes(info, n):
    """The bytes of `n` frames from the start of a piece of the file (a piece starts on a frame, of a block file on a block):
    n * frame_bytes, or for a block encoding the whole blocks that hold them, ceil(n / block_frames) * block_bytes."""
    if info.block_bytes:
        return -(-n // info.block_frames) * info.block_bytes
    return n * info.frame_bytes


def _ds64_data_size(body):
    """The `data` chunk's size of an RF64 / BW64 `ds64` chunk (riffSize u64, dataSize u64, sampleCount u64, tableLength u32,
    table...; little-endian), None when the chunk is too short to hold one."""
    return struct.unpack("<Q", body[8:16])[0] if len(body) >= 16 else None


def _walk_wav(f):
    """THE chunk walk of a RIFF/WAVE (RF64, BW64) file, seeking from header to header -> (tag, channels, sr, bits) of the `fmt `
    chunk, its body, the `fact` chunk's count (None without one), where the `data` chunk's bytes start and how many of them the
    file holds.  The last `fmt ` / `data` chunk counts, a chunk cut short by the end of the file is taken as far as it goes,
    an odd-sized chunk is followed by a pad byte, and the size of a `data` chunk that says 0xFFFFFFFF comes from the `ds64` chunk
    in front of it (the walk goes on behind the samples)."""
    header = f.read(12)
    if len(header) < 12 or header[:4] not in WAVE_IDS or header[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    end = f.seek(0, 2)
    pos, fmt, data, data_size, fmt_body, fact = 12, None, None, None, None, None
    while pos + 8 <= end:
        f.seek(pos)
        head = f.read(8)
        cid, size = head[:4], struct.unpack("<I", head[4:])[0]
        pos += 8
        if cid == b"fmt ":
            fmt_body = f.read(size)
            fmt = _fmt_chunk(fmt_body)
        elif cid == b"fact":
            fact = _fact_chunk(f.read(min(size, 4)))
        elif cid == b"ds64":
            data_size = _ds64_data_size(f.read(min(size, 16)))
        elif cid == b"data":
            if size == 0xFFFFFFFF and data_size is not None:
                size = data_size
            data = (pos, min(size, end - pos))
        pos += size + size % 2
    if fmt is None or data is None:
        raise ValueError("missing fmt or data chunk")
    tag, ch, sr, bits = fmt
    return tag, max(int(ch), 1), int(sr), bits, fmt_body, fact, data[0], data[1]


def _scan_wav_data(f):
    """The header scan of a WAVE file for a loader -> (WavInfo, the bytes of the data chunk to decode): ALL the file holds of it,
    not the whole frames alone, so that _decode refuses float data that ends inside a sample."""
    tag, ch, sr, bits, fmt_body, fact, offset, data_bytes = _walk_wav(f)
    if tag == IMA_ADPCM_TAG:
        block_bytes, spb = _fmt_ima_adpcm(fmt_body)
        return WavInfo(ENC_IMA_ADPCM, ch, sr, _ima_frames(data_bytes, block_bytes, spb, fact), 0, offset, block_bytes, spb), data_bytes
    code = _pcm_format(tag, bits)
    frame_bytes = ch * BYTES_PER_SAMPLE[code]
    return WavInfo(code, ch, sr, data_bytes // frame_bytes, frame_bytes, offset), data_bytes


def scan_wav(f):
    """The header scan of a WAVE file (seekable) without reading the samples -> WavInfo (offset: where the data chunk's bytes
    start; the samples are cut to whole frames, of an IMA ADPCM file to what `fact` and the whole blocks allow)."""
    return _scan_wav_data(f)[0]


# ---- AIFF / AIFF-C and AU: header scans; the samples are decoded by _decode (host) or the device entry points -----------------
AIFC_PCM_BE = (None, ENC_S8, ENC_S16BE, ENC_S24BE, ENC_S32BE)        # by sample width in bytes
AIFC_PCM_LE = (None, ENC_S8, PCM_S16, PCM_S24, PCM_S32)
AIFC_FIXED = {b"fl32": ENC_F32BE, b"FL32": ENC_F32BE, b"fl64": ENC_F64BE, b"FL64": ENC_F64BE,
              b"ulaw": ENC_ULAW, b"ULAW": ENC_ULAW, b"alaw": ENC_ALAW, b"ALAW": ENC_ALAW}
AU_ENCODINGS = {1: ENC_ULAW, 2: ENC_S8, 3: ENC_S16BE, 4: ENC_S24BE, 5: ENC_S32BE, 6: ENC_F32BE, 7: ENC_F64BE, 27: ENC_ALAW}


def _extended_to_rate(ten):
    """An 80-bit extended float (AIFF's sample rate) -> int, rounded to nearest; ValueError below 1 Hz and for inf / NaN."""
    exponent, mantissa = struct.unpack(">HQ", ten)
    e = (exponent & 0x7FFF) - 16383 - 63
    rate = 0
    if not exponent & 0x8000 and (exponent & 0x7FFF) != 0x7FFF and e > -128:
        rate = mantissa << e if e >= 0 else (mantissa + (1 << (-e - 1))) >> -e
    if rate < 1:
        raise ValueError("unsupported AIFF sample rate (below 1 Hz, or not a number)")
    return rate


def _info(code, ch, sr, declared, available, offset):
    if ch < 1:
        raise ValueError(f"unsupported channel count {ch}")
    frame_bytes = ch * BYTES_PER_SAMPLE[code]
    whole = max(available, 0) // frame_bytes
    return WavInfo(code, ch, int(sr), whole if declared is None else min(declared, whole), frame_bytes, offset)


def _scan_aiff(f):
    header = f.read(12)
    aifc = header[8:12] == b"AIFC"
    end = f.seek(0, 2)
    pos, comm, ssnd = 12, None, None
    while pos + 8 <= end:
        f.seek(pos)
        head = f.read(8)
        cid, size = head[:4], struct.unpack(">I", head[4:])[0]
        pos += 8
        if cid == b"COMM":
            comm = f.read(min(size, 22))
        elif cid == b"SSND":
            lead = f.read(8)
            if len(lead) < 8:
                raise ValueError("the SSND chunk is cut short")
            skip = struct.unpack(">I", lead[:4])[0]
            ssnd = (pos + 8 + skip, min(size, end - pos) - 8 - skip)
        pos += size + size % 2
    if comm is None or len(comm) < (22 if aifc else 18):
        raise ValueError("missing COMM chunk" if comm is None else "the COMM chunk is cut short")
    ch, frames, bits = struct.unpack(">hIh", comm[:8])
    sr = _extended_to_rate(comm[8:18])
    if ssnd is None:
        if frames:
            raise ValueError("missing SSND chunk")
        ssnd = (end, 0)
    kind = comm[18:22] if aifc else b"NONE"
    if kind in (b"NONE", b"twos", b"sowt", b"raw "):
        if not 1 <= bits <= 32:
            raise ValueError(f"unsupported PCM width {bits}")
        width = (bits + 7) // 8
        if kind == b"raw ":
            if width != 1:
                raise ValueError(f"unsupported PCM width {bits} for AIFF-C compression 'raw '")
            code = PCM_U8
        else:
            code = (AIFC_PCM_LE if kind == b"sowt" else AIFC_PCM_BE)[width]
    elif kind in AIFC_FIXED:
        code = AIFC_FIXED[kind]
    else:
        raise ValueError(f"unsupported AIFF-C compression {kind.decode('latin-1')!r}")
    return _info(code, ch, sr, frames, ssnd[1], ssnd[0])


def _scan_au(f):
    header = f.read(24)
    if len(header) < 24:
        raise ValueError("the AU header is cut short")
    _, offset, size, encoding, sr, ch = struct.unpack(">6I", header)
    if offset < 24:
        raise ValueError(f"AU data offset {offset} lies inside the header")
    if encoding not in AU_ENCODINGS:
        raise ValueError(f"unsupported AU encoding {encoding}")
    if sr < 1:
        raise ValueError("unsupported AU sample rate 0")
    end = f.seek(0, 2)
    available = end - offset if size == 0xFFFFFFFF else min(size, end - offset)
    return _info(AU_ENCODINGS[encoding], ch, sr, None, available, offset)


def _scan_audio_data(f):
    """_scan_wav_data for every container, sniffed from the first 12 bytes; of AIFF and AU the whole frames are the bytes to decode."""
    start = f.tell()
    header = f.read(12)
    f.seek(start)
    if header[:4] in WAVE_IDS:
        return _scan_wav_data(f)
    if header[:4] == b"FORM" and header[8:12] in (b"AIFF", b"AIFC"):
        info = _scan_aiff(f)
    elif header[:4] == b".snd":
        info = _scan_au(f)
    else:
        raise ValueError("unknown audio container (not RIFF/WAVE, RF64, BW64, AIFF, AIFF-C or AU)")
    return info, info.n_frames * info.frame_bytes


def scan_audio(f):
    """scan_wav for every container: the header walk over a seekable file without reading the samples -> WavInfo (format: a
    wseg_sample_encoding or ENC_IMA_ADPCM; offset: where the samples start in the file)."""
    return _scan_audio_data(f)[0]


def _opened(path_or_file):
    """-> (seekable binary file, whether it is ours to close)."""
    if isinstance(path_or_file, (str, bytes, os.PathLike)):
        return open(path_or_file, "rb"), True
    return (path_or_file if hasattr(path_or_file, "read") else io.BytesIO(path_or_file)), False


def _load(path_or_file, mono, scan_data):
    f, ours = _opened(path_or_file)
    try:
        info, nbytes = scan_data(f)
        f.seek(info.offset)
        raw = f.read(nbytes)
    finally:
        if ours:
            f.close()
    if info.format == ENC_IMA_ADPCM:
        x = decode_ima_adpcm(raw, info.channels, info.block_bytes)[:info.n_frames].astype(np.float32).reshape(-1) / 32768.0
    else:
        x = _decode(raw, info.format)
    return _channels(x, info.channels, mono), info.sr


def load_wav(path_or_file, mono=True):
    """-> (float32 mono ndarray, sampling_rate) of a RIFF/WAVE (RF64, BW64) file: a path, a seekable binary file or its bytes in a
    buffer.  mono=False: the channels kept apart, float32 [channels, n_frames] (C-contiguous) for a file of two or more channels
    and [n_frames] for a one-channel file; every sample converted as for the mono mix, before its mean."""
    return _load(path_or_file, mono, _scan_wav_data)


def load_audio(path_or_file, mono=True):
    """load_wav for every container scan_audio knows: with _decode and decode_ima_adpcm the definition of the arithmetic that the
    device path is held against."""
    return _load(path_or_file, mono, _scan_audio_data)


# ---- the same files, decoded on the GPU ----------------------------------------------------------------------------------
# load_audio above is the arithmetic's definition; what follows moves it to the device: read_wav_raw / read_audio_raw hand out
# the sample bytes untouched, libwseg's wseg_samples_to_mono_f32 widens and averages them with load_audio's float32 bits, and
# wseg_samples_to_planar_f32 widens the channels one asks for into planes (load_audio(mono=False)'s rows).
def _read_exact(f, view):
    got = 0
    while got < len(view):
        n = f.readinto(view[got:])
        if not n:
            raise ValueError("the file ended inside its data chunk")
        got += n


def _read_raw(path_or_file, into, scan):
    f, ours = _opened(path_or_file)
    try:
        info = scan(f)
        nbytes = piece_bytes(info, info.n_frames)
        if into is None:
            into = bytearray(nbytes)
        view = memoryview(into).cast("B")
        if len(view) < nbytes:
            raise ValueError(f"the data chunk holds {nbytes} bytes, the buffer {len(view)}")
        view = view[:nbytes]
        f.seek(info.offset)
        _read_exact(f, view)
    finally:
        if ours:
            f.close()
    return WavRaw(view, info.format, info.channels, info.sr, info.n_frames)


def read_wav_raw(path_or_file, into=None):
    """-> WavRaw(data, format, channels, sr, n_frames): the sample bytes of whole frames exactly as they sit in the data chunk
    (a uint8 memoryview of n_frames * channels * bytes-per-sample bytes; of an IMA ADPCM file the whole blocks that hold n_frames),
    `format` a wseg_sample_encoding code or ENC_IMA_ADPCM.  With `into` — a caller's writable buffer, e.g. pinned memory — the
    bytes are read straight into it and `data` is a view of its front."""
    return _read_raw(path_or_file, into, scan_wav)


def read_audio_raw(path_or_file, into=None):
    """read_wav_raw for every container scan_audio knows."""
    return _read_raw(path_or_file, into, scan_audio)


class DeviceIngest:
    """The device half of the ingest: pinned staging buffers, and `submit` = copy a filled buffer to the device and decode it
    there (`decode`, which submit, submit_planar and StreamResampler.submit all go through), stream-ordered on the current stream.
    Every call belongs to the thread that owns the device; a reader thread only ever writes into the arrays `acquire` handed out."""

    def __init__(self, device="cuda"):
        import torch
        from . import _lib
        self.torch, self._lib = torch, _lib
        self.lib = _lib.load(require_device=True)
        self.device = torch.device(device)
        self.buffers, self._pinned = [], {}

    def acquire(self, count, nbytes):
        """`count` pinned buffers of at least `nbytes` bytes (kept and re-used from call to call) -> writable uint8 arrays."""
        nbytes = -(-max(int(nbytes), 1) // 4096) * 4096
        if len(self.buffers) < count or self.buffers[0].numel() < nbytes:
            self.buffers = []        # let go of the old ones first
            self.buffers = [self.torch.empty(nbytes, dtype=self.torch.uint8, pin_memory=True) for _ in range(count)]
        views = [b.numpy()[:nbytes] for b in self.buffers[:count]]      # (a kept buffer may be longer than asked for)
        self._pinned = {v.ctypes.data: b for v, b in zip(views, self.buffers)}
        return views

    def new_output(self, n_frames):
        return self.torch.empty(int(n_frames), dtype=self.torch.float32, device=self.device)

    def new_planar_output(self, n_channels, n_frames):
        """The planes of `n_channels` channels: float32 [n_channels, n_frames]."""
        return self.torch.empty((int(n_channels), int(n_frames)), dtype=self.torch.float32, device=self.device)

    def submit(self, view, nbytes, info, out, frame0, n_frames):
        """Decode `n_frames` frames whose `nbytes` bytes sit at the front of buffer `view` into out[frame0 : frame0 + n_frames]
        -> an event that has completed once the copy out of the buffer has, i.e. once the buffer may be written again."""
        dst = out.data_ptr() + 4 * int(frame0)
        return self._submit(view, nbytes, n_frames, lambda raw: self.decode(info, None, raw.data_ptr(), n_frames, dst, 0))

    def submit_planar(self, view, nbytes, info, out, frame0, n_frames, first_channel):
        """submit for the planes of new_planar_output: channels first_channel .. first_channel + out.shape[0] - 1 of the piece go
        to out[:, frame0 : frame0 + n_frames] (the whole recording's frame count is the plane stride)."""
        sel, dst = (first_channel, out.shape[0]), out.data_ptr() + 4 * int(frame0)
        return self._submit(view, nbytes, n_frames, lambda raw: self.decode(info, sel, raw.data_ptr(), n_frames, dst, out.shape[1]))

    def decode(self, info, sel, raw, n_frames, dst, plane_stride):
        """THE choice among libwseg's four decode entry points, launched on the current stream -> the call's status.  `n_frames`
        frames from the start of a piece at device address `raw` go to float32 address `dst`: their mono mix for sel None
        (wseg_samples_to_mono_f32; the blocks of an IMA ADPCM file: wseg_ima_adpcm_to_mono_f32), else the sel[1] planes from
        channel sel[0] on, `plane_stride` floats apart (wseg_samples_to_planar_f32 / wseg_ima_adpcm_to_planar_f32)."""
        lib, n, channels = self.lib, int(n_frames), int(info.channels)
        if info.format == ENC_IMA_ADPCM:
            mono, planar = lib.wseg_ima_adpcm_to_mono_f32, lib.wseg_ima_adpcm_to_planar_f32
            piece = raw, -(-n // info.block_frames), int(info.block_bytes), channels, n
        else:
            mono, planar = lib.wseg_samples_to_mono_f32, lib.wseg_samples_to_planar_f32
            piece = raw, n, channels, int(info.format)
        if sel is None:
            return mono(*piece, dst, self._lib.stream_ptr())
        return planar(*piece, int(sel[0]), int(sel[1]), dst, int(plane_stride), self._lib.stream_ptr())

    def resample(self, out, sr_in, sr_out):
        """whisperseg_amd.resample.resample of a decoded tensor ([n_frames] or planes) on the current stream, i.e. behind the decode
        launches of the file's pieces: one launch whatever the number of planes."""
        from .resample import resample
        with self.torch.cuda.device(self.device):
            return resample(out, sr_in, sr_out, device=self.device)

    def open_resampled(self, info, sel, sr_out, piece_frames):
        """A StreamResampler for ONE file that goes through in pieces of at most `piece_frames` frames: the file at `sr_out`
        without its native-rate tensor.  sel: select_channels' answer (None: the mono mix)."""
        return StreamResampler(self, info, sel, sr_out, piece_frames)

    def _submit(self, view, nbytes, n_frames, decode):
        torch = self.torch
        with torch.cuda.device(self.device):
            event = torch.cuda.Event()
            if n_frames:
                # the kernel may read up to the next multiple of 16 bytes: the device copy is that long (and 16-byte aligned: torch
                # aligns its allocations to 512 bytes)
                raw = torch.empty(-(-nbytes // 16) * 16, dtype=torch.uint8, device=self.device)
                raw[:nbytes].copy_(self._pinned[view.ctypes.data][:nbytes], non_blocking=True)
                event.record()
                self._lib.check(decode(raw))
            else:
                event.record()
        return event

    @staticmethod
    def done(event, wait):
        if wait:
            event.synchronize()
        return event.query()


class StreamResampler:
    """One open file resampled piece by piece on the device (DeviceIngest.open_resampled).  It owns the file's output at the target
    rate — [n_out], or [planes, n_out] for a planar selection — and ONE segment buffer of resample.stream_capacity frames per plane
    (plus up to 3 floats in front and a stride rounded up to four: see below).
    submit(), per piece and in the file's order, on the current stream and without a host synchronisation: the frames the next
    outputs still need move to the front of the segment, the piece is decoded behind them (DeviceIngest.decode
    with the segment's stride as plane stride), and ONE wseg_resample_planar_range_f32 launch writes the
    outputs that have become computable, all planes at once (resample.stream_plan says which; a piece may add none).  Every output
    has the bits resample() gives it on the whole decoded recording.  result(): the output, once the last piece has been submitted.
    "The front" is 0 to 3 floats into the segment, such that the PIECE starts on a multiple of 16 bytes however many frames are
    retained: wseg_samples_to_mono_f32 stores 16 bytes per lane only to an aligned destination (dword stores otherwise), whereas the
    range call reads a segment of any alignment."""

    def __init__(self, ingest, info, sel, sr_out, piece_frames):
        from . import resample as R
        self.ingest, self.info, self.sel = ingest, info, sel
        self.plan = R.plan(info.n_frames, info.sr, sr_out)
        self.steps = R.stream_plan(info.n_frames, info.sr, sr_out, piece_frames)
        self.capacity = R.stream_capacity(info.sr, sr_out, piece_frames)
        planes = 1 if sel is None else sel[1]
        if planes > R.MAX_PLANES:
            raise ValueError(f"{planes} channels (one resample launch takes up to {R.MAX_PLANES})")
        self.out = ingest.new_output(self.plan["n_out"]) if sel is None else ingest.new_planar_output(planes, self.plan["n_out"])
        self.stride = -(-(self.capacity + 3) // 4) * 4       # (torch aligns the tensor itself to 512 bytes)
        self.segment = ingest.new_planar_output(planes, self.stride)
        self.taps = R._device_taps(self.plan, ingest.device)
        self.first = self.end = self.lead = 0    # the segment holds frames [first, end) of the recording, `lead` floats in
        self.pending = info.n_frames > 0

    def submit(self, view, nbytes, frame0, n_frames):
        """DeviceIngest.submit for the piece [frame0, frame0 + n_frames) -> the event after which `view` may be rewritten."""
        ingest, info, p, seg = self.ingest, self.info, self.plan, self.segment
        step = next(self.steps, None)
        if step is None or (step["frame0"], step["n"]) != (frame0, n_frames) or frame0 != self.end:
            raise ValueError(f"piece [{frame0}, {frame0} + {n_frames}) is not the next piece of the stream plan ({step})")
        kept = self.end - step["x_first"]
        src, lead = self.lead + step["x_first"] - self.first, -kept % 4
        if kept + n_frames > self.capacity:
            raise RuntimeError(f"{kept} retained frames + a piece of {n_frames} exceed the segment's {self.capacity}")

        def decode_and_resample(raw):
            status = ingest.decode(info, self.sel, raw.data_ptr(), n_frames, seg.data_ptr() + 4 * (lead + kept), self.stride)
            if status or not step["m_count"]:
                return status
            return ingest.lib.wseg_resample_planar_range_f32(
                seg.data_ptr() + 4 * lead, step["x_first"], kept + n_frames, self.stride, int(seg.shape[0]), int(info.n_frames),
                self.taps.data_ptr(), int(self.taps.numel()), p["up"], p["down"], p["pre_pad"], p["pre_remove"], self.out.data_ptr(),
                step["m_first"], step["m_count"], p["n_out"], ingest._lib.stream_ptr())

        with ingest.torch.cuda.device(ingest.device):
            if kept and src != lead:
                kept_frames = seg[:, src:src + kept]
                # the frames overlap their new place only when the history is longer than what came after it, i.e. with pieces
                # shorter than the ceil(n_taps / up) - 1 retained frames (tens to a thousand frames: test sizes, not staging buffers)
                seg[:, lead:lead + kept].copy_(kept_frames if src >= lead + kept else kept_frames.clone())
            event = ingest._submit(view, nbytes, n_frames, decode_and_resample)
        self.first, self.end, self.lead = step["x_first"], frame0 + n_frames, lead
        self.pending = self.end < info.n_frames
        return event

    def result(self):
        if self.pending:
            raise RuntimeError(f"result() after {self.end} of {self.info.n_frames} frames")
        return self.out


def chunk_plan(info, buffer_bytes, chunk_frames=None):
    """Frames per piece of a data chunk that goes through buffers of `buffer_bytes`: a multiple of a UNIT of 16 frames, so that
    every piece starts on a multiple of 16 bytes (and of 16 output floats) whatever the frame size.  Of a block file (IMA ADPCM)
    the unit is 16 BLOCKS: a multiple of 16 raw bytes, the block size being one of 4, and of 16 frames; such a file that fits the
    buffer whole is one piece even where the buffer holds fewer than 16 blocks."""
    blocks = bool(info.block_bytes)
    unit = 16 * info.block_frames if blocks else 16
    name, size = ("blocks", info.block_bytes) if blocks else ("frames", info.frame_bytes)
    fit = buffer_bytes // (16 * size) * unit
    if blocks and piece_bytes(info, info.n_frames) <= buffer_bytes:
        fit = max(fit, -(-max(info.n_frames, 1) // unit) * unit)
    if fit < unit:
        raise ValueError(f"a staging buffer of {buffer_bytes} bytes does not hold 16 {name} of {size} bytes")
    if chunk_frames is not None:
        if chunk_frames <= 0 or chunk_frames % unit:
            raise ValueError("chunk_frames must be a positive multiple of 16" + (f" blocks = {unit} frames" if blocks else ""))
        fit = min(fit, int(chunk_frames))
    return fit


def check_channels(info, name="wav"):
    if info.channels > MAX_CHANNELS:
        raise ValueError(f"{name}: {info.channels} channels (the device decode takes up to {MAX_CHANNELS})")


def select_channels(info, channel_id):
    """What a caller's `channel_id` asks of a file -> None: the mono decode (channel_id None, or a one-channel file, whose
    `channel_id` is ignored as upstream's `if len(audio.shape) == 2` does), else (first_channel, n_channels) for the planar
    decode: "all" is every channel (two or more, then), an int one channel by Python's indexing (IndexError when out of range):
    a selection of ONE plane is an integer's, which is what FileOutput.result picks the single row by."""
    if channel_id is None or info.channels == 1:
        return None
    if isinstance(channel_id, str):
        if channel_id != "all":
            raise ValueError(f"channel_id must be an integer, 'all' or None (got {channel_id!r})")
        return 0, info.channels
    k = int(channel_id)
    if not -info.channels <= k < info.channels:
        raise IndexError(f"channel_id {k} is out of range for a recording of {info.channels} channels")
    return k % info.channels, 1


def check_rate(sr):
    """A target rate: None (the native rate) or a positive integer -> None or int."""
    if sr is None:
        return None
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or sr <= 0:
        raise ValueError(f"sr must be a positive integer or None (got {sr!r})")
    return int(sr)


class FileOutput:
    """Where the pieces of ONE file go (load_wav_device and FilePipeline make one when a file's first piece is at hand, `target`
    the rate asked for and `piece_frames` that piece's frame count, a file's longest): the choice among the ingest's stream
    resampler — ingest.open_resampled(info, sel, target, piece_frames), for a file of frames that changes rate —, its mono output
    (sel None: new_output / submit) and its planes (new_planar_output / submit_planar).  submit() hands every piece on, in the
    file's order, and returns the event after which the piece's buffer may be rewritten.  result(), behind the last piece: the
    tensor at the target rate — [n] for the mono mix and for the one plane an integer channel_id selected (select_channels gives
    one plane to nothing else), otherwise the planes that were decoded.  An ingest without open_resampled has the file decoded
    whole at its native rate and result() calls ingest.resample(decoded, native, target) once, all its planes in one call."""

    def __init__(self, ingest, info, sel, target, piece_frames):
        self.ingest, self.info, self.sel, self.stream = ingest, info, sel, None
        self.rates = (info.sr, target) if target != info.sr and info.n_frames else None
        if self.rates and hasattr(ingest, "open_resampled"):
            self.stream = ingest.open_resampled(info, sel, target, piece_frames)
        elif sel is None:
            self.out = ingest.new_output(info.n_frames)
        else:
            self.out = ingest.new_planar_output(sel[1], info.n_frames)

    def submit(self, view, nbytes, frame0, n):
        if self.stream is not None:
            return self.stream.submit(view, nbytes, frame0, n)
        if self.sel is None:
            return self.ingest.submit(view, nbytes, self.info, self.out, frame0, n)
        return self.ingest.submit_planar(view, nbytes, self.info, self.out, frame0, n, self.sel[0])

    def result(self):
        out = self.out if self.stream is None else self.stream.result()
        if self.sel is not None and self.sel[1] == 1:
            out = out[0]
        if self.stream is None and self.rates:
            self.out = None                                   # (the native-rate tensor is let go of here)
            out = self.ingest.resample(out, *self.rates)
        return out


_INGEST = {}


def device_ingest(device="cuda"):
    """The DeviceIngest of `device`, made once and kept: its pinned staging buffers are re-used from call to call."""
    import torch
    key = str(torch.device(device))
    if key not in _INGEST:
        _INGEST[key] = DeviceIngest(device)
    return _INGEST[key]


def load_wav_device(path_or_file, device="cuda", chunk_frames=None, mono=True, channel_id=None, sr=None):
    """load_audio on the GPU (any container of scan_audio) -> (float32 device tensor [n_frames], sampling_rate), the same samples bit
    for bit: sample bytes -> pinned staging -> non_blocking copy -> DeviceIngest.decode on the current stream.  A data chunk larger
    than the staging buffer (or than `chunk_frames` frames, a multiple of 16: for tests) goes through in pieces.  An IMA ADPCM file
    goes through as its blocks, in pieces of a multiple of 16 blocks (`chunk_frames`: of 16 * block_frames).
    mono=False: load_wav(..., mono=False) as a device tensor ([channels, n_frames]; [n_frames] for a one-channel file), decoded to
    planes.  channel_id=k (implies mono=False): row k of that array, only that plane decoded; a one-channel file ignores it;
    negative k counts from the end, out of range raises IndexError.  channel_id="all" is mono=False.
    sr=N: `librosa.load(..., sr=N)` — every piece is resampled on the device as soon as it is decoded (StreamResampler: one launch
    per piece for all planes, the bits of resample() on the whole decoded file, which is never held at its native rate) and N is the
    rate returned; None, the native rate or a file of no frames: nothing is resampled."""
    sr = check_rate(sr)
    ingest = device_ingest(device)
    f, ours = _opened(path_or_file)
    try:
        info = scan_audio(f)
        check_channels(info)
        total = piece_bytes(info, info.n_frames)
        views = ingest.acquire(2, min(STAGING_BYTES, max(total, 16 * (info.block_bytes or info.frame_bytes))))
        step = chunk_plan(info, len(views[0]), chunk_frames)
        sel = select_channels(info, channel_id if channel_id is not None or mono else "all")
        target = info.sr if sr is None else sr
        output = FileOutput(ingest, info, sel, target, min(step, info.n_frames))
        events = [None, None]        # the next piece is read while the copy of the one before is in flight
        f.seek(info.offset)
        for i, frame0 in enumerate(range(0, info.n_frames, step)):
            n = min(step, info.n_frames - frame0)
            if events[i % 2] is not None:
                ingest.done(events[i % 2], wait=True)
            nbytes = piece_bytes(info, n)
            _read_exact(f, views[i % 2][:nbytes])
            events[i % 2] = output.submit(views[i % 2], nbytes, frame0, n)
        for event in events:         # the buffers belong to the next call
            if event is not None:
                ingest.done(event, wait=True)
    finally:
        if ours:
            f.close()
    return output.result(), target


def _named(exc, path):
    """`exc` again with the file's name in front (same type where the type takes a plain message)."""
    msg = f"{path}: {exc}"
    if isinstance(exc, OSError):
        return OSError(msg)
    try:
        return type(exc)(msg)
    except Exception:
        return RuntimeError(msg)


class FilePipeline:
    """Iterator over (float32 mono device tensor, sampling_rate) of `paths`, in order, with the file reads overlapped with
    whatever the consumer does between two items: ONE reader thread opens, parses and `readinto`s the buffers of a small pool
    (`n_buffers` x at most `buffer_bytes`; larger files go through in pieces), the consuming thread submits filled buffers to
    `ingest` (DeviceIngest, or anything with its acquire / new_output / submit / done) and gives a buffer back to the reader once
    the event of its submit has completed.  The reader makes no device call.  A reader error is raised by the consumer with the
    file's name; close() — also called when the iteration ends, fails or is abandoned — stops and joins the thread.
    `channel_id`: None — the mono mix, as above; an int — that channel of every multi-channel file ([n_frames]; one-channel files
    give their samples; out of range: IndexError with the file's name); "all" — what load_wav(p, mono=False) gives.  The planes
    come from the ingest's new_planar_output / submit_planar, which the mono mix never calls (FileOutput makes the choice, per file).
    `sr`: None — every file at its native rate; an int — the target rate of every file; a sequence with one entry per path (None
    entries: the native rate).  A file whose native rate differs from its target is yielded with the target rate.  An ingest with
    open_resampled (DeviceIngest) resamples it piece by piece — ingest.open_resampled(info, sel, target, piece_frames) when the
    file's first piece arrives, .submit(view, nbytes, frame0, n) for every piece in place of submit / submit_planar, .result()
    behind the last — so the file never exists at its native rate and the resampler runs while the reader reads on.  An ingest
    that offers only `resample` has the file decoded whole and resampled once its LAST piece has been submitted —
    ingest.resample(decoded, native, target), all its planes in one call — and the native-rate tensor is dropped there.  Neither
    is called otherwise (no `sr`, a file already at its target, a file of no frames), so an ingest without them serves a pipeline
    that never resamples."""

    def __init__(self, paths, ingest, buffer_bytes=STAGING_BYTES, n_buffers=2, channel_id=None, sr=None):
        self.paths, self.ingest, self.channel_id = list(paths), ingest, channel_id
        if sr is None or isinstance(sr, (int, np.integer)) and not isinstance(sr, bool):
            self.rates = [check_rate(sr)] * len(self.paths)
        elif isinstance(sr, (str, bytes)) or not hasattr(sr, "__len__"):
            raise ValueError(f"sr must be a positive integer, a sequence of them or None (got {sr!r})")
        else:
            if len(sr) != len(self.paths):
                raise ValueError(f"sr has {len(sr)} entries for {len(self.paths)} files")
            self.rates = [check_rate(v) for v in sr]
        sizes = [os.path.getsize(p) for p in self.paths if os.path.exists(p)]
        self.views = ingest.acquire(n_buffers, min(int(buffer_bytes), max(sizes + [16 * MAX_CHANNELS * 8]))) if self.paths else []
        self.free, self.filled = queue.Queue(), queue.Queue()
        for v in self.views:
            self.free.put(v)
        self.pending = collections.deque()       # (view, event) of submitted buffers, oldest first
        self.stop = threading.Event()
        self.thread = None
        if self.paths:
            self.thread = threading.Thread(target=self._read, name="wseg-wav-reader", daemon=True)
            self.thread.start()

    # ---- reader thread: host work only --------------------------------------------------------------------------------
    def _take_free(self):
        while not self.stop.is_set():
            try:
                return self.free.get(timeout=0.05)
            except queue.Empty:
                pass
        return None

    def _read(self):
        for index, path in enumerate(self.paths):
            try:
                with open(path, "rb") as f:
                    info = scan_audio(f)
                    check_channels(info, os.path.basename(path))
                    sel = select_channels(info, self.channel_id)
                    step = chunk_plan(info, len(self.views[0]))
                    f.seek(info.offset)
                    for frame0 in range(0, max(info.n_frames, 1), step):
                        n = min(step, info.n_frames - frame0)
                        view = self._take_free()
                        if view is None:
                            return
                        try:
                            _read_exact(f, view[:piece_bytes(info, n)])
                        except BaseException:
                            self.free.put(view)
                            raise
                        self.filled.put((index, info, view, frame0, n, sel))
            except BaseException as exc:
                self.filled.put((index, exc, None, 0, 0, None))
                return
        self.filled.put(None)

    # ---- consumer ---------------------------------------------------------------------------------------------------------
    def _reap(self, wait):
        """Give the reader back every submitted buffer whose copy has completed (wait: block for the oldest)."""
        while self.pending and self.ingest.done(self.pending[0][1], wait):
            self.free.put(self.pending.popleft()[0])
            wait = False

    def _next_item(self):
        while True:
            self._reap(False)
            try:
                return self.filled.get_nowait()
            except queue.Empty:
                pass
            if self.pending:
                self._reap(True)
            else:
                try:
                    return self.filled.get(timeout=0.05)
                except queue.Empty:
                    if not self.thread.is_alive() and self.filled.empty():
                        raise RuntimeError("the wav reader thread ended without a result")

    def __iter__(self):
        try:
            output = None
            while self.thread is not None:
                item = self._next_item()
                if item is None:
                    break
                index, info, view, frame0, n, sel = item
                if isinstance(info, BaseException):
                    raise _named(info, self.paths[index]) from info
                target = self.rates[index] if self.rates[index] is not None else info.sr
                if frame0 == 0:
                    output = FileOutput(self.ingest, info, sel, target, n)
                self.pending.append((view, output.submit(view, piece_bytes(info, n), frame0, n)))
                if frame0 + n >= info.n_frames:
                    yield output.result(), target
                    output = None
        finally:
            self.close()

    def close(self):
        self.stop.set()
        if self.thread is not None:
            self.thread.join()
            self.thread = None
        self._reap(bool(self.pending))
        while self.pending:
            self._reap(True)
