"""The host half of the GPU ingest, without a GPU: read_wav_raw hands out the bytes load_wav decodes (the arithmetic of
wseg_pcm_to_mono_f32, restated in numpy in wav_cases.restate, applied to them gives load_wav's float32 bits), and the file
pipeline behind SegmenterBase.segment_files keeps order, its buffer bound and its thread's life in hand."""
import hashlib
import io
import os
import struct
import threading

import numpy as np
import pytest

import audio_cases as AC
import ima_adpcm_cases as IC
import wav_cases as WC
from conftest import GOLDEN
from whisperseg_amd import wavio
from whisperseg_amd.wavio import load_wav, read_wav_raw


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check_raw_equals_load_wav(blob, fmt, channels, n_frames):
    raw = read_wav_raw(io.BytesIO(blob))
    assert (raw.format, raw.channels, raw.sr, raw.n_frames) == (WC.FORMATS.index(fmt), channels, 16000, n_frames)
    assert len(raw.data) == n_frames * channels * WC.BYTES[raw.format]
    want, sr = load_wav(io.BytesIO(blob))
    assert sr == raw.sr and want.dtype == np.float32 and want.shape == (n_frames,)
    got = WC.restate(raw.data, raw.format, raw.channels, raw.n_frames)
    assert np.array_equal(bits(got), bits(want))
    return raw


@pytest.mark.parametrize("channels", [1, 2, 3, 8, 9, 17, 64])
@pytest.mark.parametrize("fmt", WC.FORMATS)
def test_raw_bytes_and_restated_arithmetic_equal_load_wav(fmt, channels):
    """All six formats x 1 / 2 / 3 channels (and 8 / 9 / 17 / 64: numpy's mean sums 8 and more channels pairwise)."""
    n = 257
    blob = WC.make_wav(fmt, channels, n)
    raw = check_raw_equals_load_wav(blob, fmt, channels, n)
    assert bytes(raw.data) == blob[44:44 + len(raw.data)]              # the data chunk's bytes, untouched


def test_mean_of_negative_zero_frames_is_positive_zero():
    blob = WC.wav_bytes("f32", 2, 16000, WC.sample_bytes("f32", [-0.0, -0.0, -0.0, 0.0]))
    want, _ = load_wav(io.BytesIO(blob))
    raw = read_wav_raw(io.BytesIO(blob))
    assert bits(want).tolist() == [0, 0] == bits(WC.restate(raw.data, raw.format, 2, 2)).tolist()
    mono = WC.wav_bytes("f32", 1, 16000, WC.sample_bytes("f32", [-0.0]))
    assert bits(load_wav(io.BytesIO(mono))[0]).tolist() == [0x80000000] == bits(WC.restate(read_wav_raw(io.BytesIO(mono)).data, 4, 1, 1)).tolist()


@pytest.mark.parametrize("fmt", WC.FORMATS)
def test_extensible_tag_odd_chunk_and_ragged_end(fmt):
    rng = np.random.default_rng(5)
    data = WC.sample_bytes(fmt, WC.random_samples(fmt, 3 * 101, rng))
    check_raw_equals_load_wav(WC.wav_bytes(fmt, 3, 16000, data, extensible=True), fmt, 3, 101)
    check_raw_equals_load_wav(WC.wav_bytes(fmt, 3, 16000, data, junk_before_data=7), fmt, 3, 101)
    if fmt not in ("f32", "f64"):      # (load_wav itself refuses float data that ends inside a sample)
        check_raw_equals_load_wav(WC.wav_bytes(fmt, 3, 16000, data[:-1]), fmt, 3, 100)
    whole = len(data) - WC.BYTES[WC.FORMATS.index(fmt)]          # ends inside a frame, between two samples
    check_raw_equals_load_wav(WC.wav_bytes(fmt, 3, 16000, data[:whole]), fmt, 3, 100)
    # a data chunk whose header promises more than the file holds is taken as far as it goes
    blob = WC.wav_bytes(fmt, 3, 16000, data)
    cut = blob[:len(blob) - 2 * 3 * WC.BYTES[WC.FORMATS.index(fmt)] - len(data) % 2]
    check_raw_equals_load_wav(cut, fmt, 3, 99)


def test_into_fills_the_callers_buffer(tmp_path):
    blob = WC.make_wav("s24", 2, 1021)
    path = tmp_path / "a.wav"
    path.write_bytes(blob)
    plain = read_wav_raw(str(path))
    buf = np.full(8192, 0xEE, np.uint8)
    raw = read_wav_raw(str(path), into=buf)
    n = 1021 * 6
    assert raw[1:] == plain[1:] and bytes(raw.data) == bytes(plain.data) == bytes(buf[:n])
    assert (buf[n:] == 0xEE).all()
    with pytest.raises(ValueError):
        read_wav_raw(str(path), into=bytearray(n - 1))


def test_errors_are_load_wavs():
    cases = [b"RIFF\x00\x00\x00\x00WAVX", b"RIFF\x04\x00\x00\x00WAVE"]
    for offset, value in ((20, 2), (34, 12)):        # an ADPCM format tag; a 12-bit PCM width
        blob = bytearray(WC.wav_bytes("s16", 1, 16000, b"\x00\x00"))
        struct.pack_into("<H", blob, offset, value)
        cases.append(bytes(blob))
    for blob in cases:
        with pytest.raises(ValueError) as a:
            load_wav(io.BytesIO(blob))
        with pytest.raises(ValueError) as b:
            read_wav_raw(io.BytesIO(blob))
        assert str(a.value) == str(b.value)


def parent_load_wav(path):
    """load_wav as it stood before the device ingest was added, restated: the array it returns must not have changed."""
    with open(path, "rb") as f:
        blob = f.read()
    assert blob[:4] == b"RIFF" and blob[8:12] == b"WAVE"
    pos, fmt, raw = 12, None, None
    while pos + 8 <= len(blob):
        cid, size = blob[pos:pos + 4], struct.unpack("<I", blob[pos + 4:pos + 8])[0]
        body = blob[pos + 8:pos + 8 + size]
        pos += 8 + size + size % 2
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
        elif cid == b"data":
            raw = body
    tag, ch, sr, _, _, width = fmt
    assert (tag, width) == (1, 16)
    x = np.frombuffer(raw[: len(raw) // 2 * 2], "<i2").astype(np.float32) / 32768.0
    if ch > 1:
        x = x[: len(x) // ch * ch].reshape(-1, ch).mean(axis=1).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32), int(sr)


def test_load_wav_of_the_golden_recording_is_unchanged():
    path = os.path.join(GOLDEN, "meerkat_5s.wav")
    got, sr = load_wav(path)
    want, want_sr = parent_load_wav(path)
    assert sr == want_sr and got.dtype == np.float32 and len(got) > 1000
    assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(want.tobytes()).hexdigest()
    raw = read_wav_raw(path)
    assert np.array_equal(bits(WC.restate(raw.data, raw.format, raw.channels, raw.n_frames)), bits(got))


# ---- the folder pipeline against a stub segmenter and a host stand-in for the device half --------------------------------
class HostIngest:
    """wavio.DeviceIngest's interface on the host: buffers are numpy arrays, submit decodes with the numpy restatement, and an
    event completes only at its SECOND query (so buffers do stay out for a while)."""

    def __init__(self):
        self.acquired, self.out_now, self.out_max, self.submits = [], 0, 0, []

    def acquire(self, count, nbytes):
        self.acquired.append((count, nbytes))
        self.views = [np.zeros(nbytes, np.uint8) for _ in range(count)]
        return self.views

    def new_output(self, n_frames):
        return np.full(n_frames, np.nan, np.float32)

    def submit(self, view, nbytes, info, out, frame0, n_frames):
        assert any(view is v for v in self.views) and frame0 % 16 == 0 and nbytes == n_frames * info.frame_bytes <= len(view)
        out[frame0:frame0 + n_frames] = WC.restate(view[:nbytes], info.format, info.channels, n_frames)
        self.out_now += 1
        self.out_max = max(self.out_max, self.out_now)
        self.submits.append(n_frames)
        return {"queries": 0}

    def done(self, event, wait):
        event["queries"] += 1
        if wait or event["queries"] >= 2:
            if not event.get("released"):
                event["released"] = True
                self.out_now -= 1
            return True
        return False


def stub_segmenter(buffer_bytes):
    from whisperseg_amd.model import SegmenterBase

    class Stub(SegmenterBase):
        def __init__(self):
            super().__init__()
            self.host, self.ingest_buffer_bytes, self.kwargs = HostIngest(), buffer_bytes, None

        def ingest_backend(self):
            return self.host

        def segment_batch(self, audios, **kwargs):
            self.kwargs = kwargs
            return [dict(sr=sr, sha=hashlib.sha256(np.asarray(a).tobytes()).hexdigest(), n=len(a)) for a, sr in audios]

    return Stub()


def reader_threads():
    return [t for t in threading.enumerate() if t.name == "wseg-wav-reader"]


def folder(tmp_path):
    specs = [("s16", 2, 5000, 16000), ("s24", 1, 1021, 32000), ("f32", 3, 700, 48000), ("u8", 1, 0, 8000), ("s32", 5, 3333, 44100),
             ("f64", 2, 64, 16000)]
    paths = []
    for i, (fmt, ch, n, sr) in enumerate(specs):
        p = tmp_path / f"{i}_{fmt}.wav"
        p.write_bytes(WC.make_wav(fmt, ch, n, seed=i, sr=sr))
        paths.append(str(p))
    return paths


def test_segment_files_pipeline_keeps_order_and_its_buffer_bound(tmp_path):
    paths = folder(tmp_path)
    want = [dict(sr=sr, sha=hashlib.sha256(a.tobytes()).hexdigest(), n=len(a)) for a, sr in map(load_wav, paths)]
    for buffer_bytes in (1 << 20, 8192):             # whole files; pieces of at most 8 KiB (a multiple of 16 frames each)
        seg = stub_segmenter(buffer_bytes)
        assert seg.segment_files(paths, num_trials=2) == want
        assert seg.kwargs == {"num_trials": 2}
        count, nbytes = seg.host.acquired[0]
        assert len(seg.host.acquired) == 1 and count == 2 and nbytes <= buffer_bytes
        assert 1 <= seg.host.out_max <= 2 and seg.host.out_now == 0
        assert not reader_threads()
    assert len(seg.host.submits) > len(paths)     # the small pool cut the larger files into pieces
    assert seg.segment_files(paths) == want          # again on the same segmenter
    assert not reader_threads()


def test_segment_files_raises_a_readers_error_with_the_files_name(tmp_path):
    paths = folder(tmp_path)
    with open(paths[2], "r+b") as f:
        f.seek(8)
        f.write(b"JUNK")
    seg = stub_segmenter(1 << 20)
    with pytest.raises(ValueError, match="2_f32.wav.*not a RIFF/WAVE file"):
        seg.segment_files(paths)
    assert not reader_threads() and seg.host.out_now == 0
    with pytest.raises(OSError, match="nowhere.wav"):
        seg.segment_files(paths[:2] + [str(tmp_path / "nowhere.wav")])
    assert not reader_threads()
    # a consumer that gives up half way leaves no thread either
    pipe = wavio.FilePipeline(paths[:2] + paths[3:], HostIngest(), buffer_bytes=8192)
    it = iter(pipe)
    next(it)
    it.close()
    assert not reader_threads()


def test_segment_files_of_nothing():
    seg = stub_segmenter(1 << 20)
    assert seg.segment_files([]) == [] and seg.host.acquired == [] and not reader_threads()


# ---- the piece plan, as a table ---------------------------------------------------------------------------------------------------
NO_16 = "chunk_frames must be a positive multiple of 16"
MIB3 = (3 << 20) + 5
# (frame_bytes, buffer_bytes, [chunk_plan for chunk_frames None / 16 / 40 / 0]); a str: the ValueError's message
FRAME_PLANS = [
    (1, 15, ["a staging buffer of 15 bytes does not hold 16 frames of 1 bytes"] * 4),
    (1, 16, [16, 16, NO_16, NO_16]),
    (1, MIB3, [3145728, 16, NO_16, NO_16]),
    (6, 95, ["a staging buffer of 95 bytes does not hold 16 frames of 6 bytes"] * 4),
    (6, 96, [16, 16, NO_16, NO_16]),
    (6, MIB3, [524288, 16, NO_16, NO_16]),
    (512, 8191, ["a staging buffer of 8191 bytes does not hold 16 frames of 512 bytes"] * 4),
    (512, 8192, [16, 16, NO_16, NO_16]),
    (512, MIB3, [6144, 16, NO_16, NO_16]),
]
# (channels, block_bytes, blocks in the file, frames cut off the last, buffer_bytes, [chunk_plan for chunk_frames None / 16 blocks /
# 24 blocks / 0]); the files of 5 blocks fit a buffer of 5 blocks whole
BLOCK_PLANS = [
    (1, 256, 100000, 0, 4095, ["a staging buffer of 4095 bytes does not hold 16 blocks of 256 bytes"] * 4),
    (1, 256, 100000, 0, 4096, [8080, 8080] + [NO_16 + " blocks = 8080 frames"] * 2),
    (1, 256, 100000, 0, MIB3, [6205440, 8080] + [NO_16 + " blocks = 8080 frames"] * 2),
    (2, 2048, 100000, 0, 32767, ["a staging buffer of 32767 bytes does not hold 16 blocks of 2048 bytes"] * 4),
    (2, 2048, 100000, 0, 32768, [32656, 32656] + [NO_16 + " blocks = 32656 frames"] * 2),
    (2, 2048, 100000, 0, MIB3, [3134976, 32656] + [NO_16 + " blocks = 32656 frames"] * 2),
    (64, 512, 100000, 0, 8191, ["a staging buffer of 8191 bytes does not hold 16 blocks of 512 bytes"] * 4),
    (64, 512, 100000, 0, 8192, [144, 144] + [NO_16 + " blocks = 144 frames"] * 2),
    (64, 512, 100000, 0, MIB3, [55296, 144] + [NO_16 + " blocks = 144 frames"] * 2),
    (2, 2048, 5, 0, 10239, ["a staging buffer of 10239 bytes does not hold 16 blocks of 2048 bytes"] * 4),
    (2, 2048, 5, 0, 10240, [32656, 32656] + [NO_16 + " blocks = 32656 frames"] * 2),
    (2, 2048, 5, 100, 10239, ["a staging buffer of 10239 bytes does not hold 16 blocks of 2048 bytes"] * 4),
    (2, 2048, 5, 100, 10240, [32656, 32656] + [NO_16 + " blocks = 32656 frames"] * 2),
]


def plans(info, buffer_bytes, chunk_frames):
    got = []
    for c in chunk_frames:
        try:
            got.append(wavio.chunk_plan(info, buffer_bytes, c))
        except ValueError as exc:
            got.append(str(exc))
    return got


def test_chunk_plan_table():
    """Values and messages of chunk_plan as it stood with one body for frames and one for blocks."""
    for frame_bytes, buffer_bytes, want in FRAME_PLANS:
        info = wavio.WavInfo(wavio.PCM_S16, 1, 16000, 10 ** 9, frame_bytes, 44)
        assert plans(info, buffer_bytes, (None, 16, 40, 0)) == want, (frame_bytes, buffer_bytes)
    for channels, block_bytes, n_blocks, cut, buffer_bytes, want in BLOCK_PLANS:
        spb = wavio.ima_block_frames(channels, block_bytes)
        info = wavio.WavInfo(wavio.ENC_IMA_ADPCM, channels, 16000, n_blocks * spb - cut, 0, 60, block_bytes, spb)
        assert plans(info, buffer_bytes, (None, 16 * spb, 24 * spb, 0)) == want, (channels, block_bytes, n_blocks, cut, buffer_bytes)


# ---- one chunk walk: load_wav, read_wav_raw and scan_wav on awkward files ---------------------------------------------------------
def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + b"\x00" * (len(body) % 2)


def riff(*chunks):
    return b"RIFF" + struct.pack("<I", 4 + sum(map(len, chunks))) + b"WAVE" + b"".join(chunks)


def awkward_files():
    """name -> (file, the WavInfo of its scan, the bytes read_wav_raw hands out)."""
    rng = np.random.default_rng(11)
    s16 = WC.sample_bytes("s16", WC.random_samples("s16", 3 * 50, rng))
    f32 = WC.sample_bytes("f32", WC.random_samples("f32", 2 * 20, rng))
    blocks = IC.random_blocks(2, 72, 3)
    fmt = AC.wav_chunks(1, 16, 3, 16000)
    return {
        "two fmt chunks": (riff(AC.wav_chunks(1, 24, 2, 8000), fmt, chunk(b"data", s16)), wavio.WavInfo(1, 3, 16000, 50, 6, 68), s16),
        "two data chunks": (riff(fmt, chunk(b"data", s16[:60]), chunk(b"data", s16)), wavio.WavInfo(1, 3, 16000, 50, 6, 112), s16),
        "an odd chunk before data": (WC.wav_bytes("s16", 3, 16000, s16, junk_before_data=7), wavio.WavInfo(1, 3, 16000, 50, 6, 60), s16),
        "ds64 and a trailing chunk": (AC.rf64_bytes("s16", 3, 16000, s16, trailing=AC.list_chunk(301)), wavio.WavInfo(1, 3, 16000, 50, 6, 80), s16),
        "fact after data": (IC.wav_bytes(2, 11025, 72, blocks, trailing=chunk(b"fact", struct.pack("<I", 2 * 65 + 7))),
                            wavio.WavInfo(wavio.ENC_IMA_ADPCM, 2, 11025, 2 * 65 + 7, 0, 48, 72, 65), blocks),
        "float data that ends inside a sample": (WC.wav_bytes("f32", 2, 16000, f32[:-1]), wavio.WavInfo(4, 2, 16000, 19, 8, 44), f32[:19 * 8]),
    }


@pytest.mark.parametrize("name", list(awkward_files()))
def test_load_wav_read_wav_raw_and_scan_wav_agree_on_awkward_files(name):
    blob, info, data = awkward_files()[name]
    assert wavio.scan_wav(io.BytesIO(blob)) == info == wavio.scan_audio(io.BytesIO(blob))
    raw = read_wav_raw(io.BytesIO(blob))
    assert tuple(raw[1:]) == tuple(info[:4]) and bytes(raw.data) == data == blob[info.offset:info.offset + len(data)]
    if info.format == wavio.ENC_IMA_ADPCM:
        restated = IC.floats(IC.audioop_decode(bytes(raw.data), raw.channels, info.block_bytes)[:raw.n_frames])
    else:
        restated = WC.restate(raw.data, raw.format, raw.channels, raw.n_frames)
    assert restated.shape == (info.n_frames,)
    for loader in (load_wav, wavio.load_audio):
        if name == "float data that ends inside a sample":       # the loaders refuse it; the raw path gives the whole frames
            with pytest.raises(ValueError, match="multiple of element size"):
                loader(io.BytesIO(blob))
            continue
        want, sr = loader(io.BytesIO(blob))
        assert sr == info.sr and np.array_equal(bits(want), bits(restated))
        planes = loader(io.BytesIO(blob), mono=False)[0]
        assert planes.shape == (info.channels, info.n_frames) and np.array_equal(bits(planes.mean(axis=0).astype(np.float32)), bits(want))


def test_awkward_files_fail_with_one_message():
    s16 = WC.sample_bytes("s16", [1, 2, 3, 4])
    fmt = AC.wav_chunks(1, 16, 1, 16000)
    cases = [(riff(fmt, AC.wav_chunks(2, 4, 1, 16000), chunk(b"data", s16)), "unsupported WAVE format tag 2"),      # the LAST fmt chunk counts
             (riff(fmt, AC.wav_chunks(1, 12, 1, 16000), chunk(b"data", s16)), "unsupported PCM width 12"),
             (riff(chunk(b"data", s16), chunk(b"fact", b"\x04\x00\x00\x00")), "missing fmt or data chunk"),
             (riff(fmt, chunk(b"LIST", b"data" + s16)), "missing fmt or data chunk"),
             (riff(fmt, chunk(b"data", s16))[:8] + b"WAVX", "not a RIFF/WAVE file")]
    for blob, text in cases:
        for call in (load_wav, read_wav_raw, wavio.scan_wav, wavio.load_audio):
            with pytest.raises(ValueError) as exc:
                call(io.BytesIO(blob))
            assert str(exc.value) == text, call
