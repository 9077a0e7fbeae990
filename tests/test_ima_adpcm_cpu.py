"""IMA ADPCM WAVE files (format tag 0x0011) without a GPU: wavio.decode_ima_adpcm — the host definition the kernel is compared with
in test_ima_adpcm_gpu.py — against the stdlib's audioop.adpcm2lin, the header scan (block geometry, `fact`, partial blocks, malformed
headers), the piece plan of a block file by brute force, and the file pipeline over a host stand-in for the device half."""
import io
import os
import struct

import numpy as np
import pytest

import ima_adpcm_cases as IC
from conftest import GOLDEN
from oracle.resample import resample_poly_ref
from test_wav_planar_cpu import PlanarHostIngest, equal_items, reader_threads
from whisperseg_amd import wavio
from whisperseg_amd.wavio import decode_ima_adpcm, load_audio, load_wav, scan_audio

PER_CHANNEL = (8, 36, 256, 1024)         # block bytes per channel: 9 (the minimum), 65, 505 and 2041 samples per block
CHANNELS = (1, 2, 3, 8, 9)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def load(blob, **kw):
    return load_audio(io.BytesIO(blob), **kw)


# ---- 1. the host definition against audioop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("per_channel", PER_CHANNEL)
def test_decode_equals_audioop_on_random_blocks(per_channel, channels):
    block_bytes = per_channel * channels
    n_blocks = 5 if per_channel < 256 else 2
    raw = IC.random_blocks(channels, block_bytes, n_blocks, seed=1)
    got = decode_ima_adpcm(raw, channels, block_bytes)
    want = IC.audioop_decode(raw, channels, block_bytes)
    assert got.dtype == np.int16 and got.shape == (n_blocks * IC.block_frames(channels, block_bytes), channels)
    assert np.array_equal(got, want)
    assert (got == 32767).any() and (got == -32768).any()           # random nibbles run into both clamps
    # the floats of a file around these blocks: / 2^15, numpy's mean
    blob = IC.wav_bytes(channels, 16000, block_bytes, raw)
    mono, sr = load(blob)
    assert sr == 16000 and np.array_equal(bits(mono), bits(IC.floats(want)))
    planes = load(blob, mono=False)[0]
    assert planes.flags["C_CONTIGUOUS"] and np.array_equal(bits(planes), bits(IC.floats(want, mono=False)))
    assert np.array_equal(bits(load_wav(io.BytesIO(blob))[0]), bits(mono))
    assert decode_ima_adpcm(raw + b"\x01" * (block_bytes - 1), channels, block_bytes).shape == got.shape      # whole blocks only
    assert decode_ima_adpcm(b"", channels, block_bytes).shape == (0, channels)


@pytest.mark.parametrize("per_channel", PER_CHANNEL)
def test_decode_equals_audioop_on_an_encoded_recording(per_channel):
    x, sr = load_wav(os.path.join(GOLDEN, "meerkat_5s.wav"))
    pcm = np.round(x * 32768).astype(np.int16)
    for channels in (1, 2):
        sig = np.stack([pcm, pcm[::-1]], axis=1)[:, :channels]
        raw = IC.encode(sig, per_channel * channels)
        got = decode_ima_adpcm(raw, channels, per_channel * channels)
        assert np.array_equal(got, IC.audioop_decode(raw, channels, per_channel * channels))
        for c in range(channels):                                       # it IS the recording, at 4 bits a sample
            assert np.corrcoef(got[:len(sig), c].astype(np.float64), sig[:, c].astype(np.float64))[0, 1] > 0.9
        assert np.array_equal(got[::IC.block_frames(channels, per_channel * channels)], sig[::IC.block_frames(channels, per_channel * channels)])


def test_a_header_index_above_88_is_88():
    raw = bytearray(IC.random_blocks(2, 72, 4, seed=3))
    at88 = bytearray(raw)
    for blk in range(4):
        for c in range(2):
            raw[blk * 72 + 4 * c + 2] = (89, 100, 200, 255)[(blk + c) % 4]
            at88[blk * 72 + 4 * c + 2] = 88
    want = IC.audioop_decode(bytes(at88), 2, 72)
    assert np.array_equal(decode_ima_adpcm(bytes(raw), 2, 72), want)
    assert np.array_equal(IC.audioop_decode(bytes(raw), 2, 72), want)


# ---- 2. the scan ------------------------------------------------------------------------------------------------------------------
def test_scan_gives_the_block_geometry_and_the_frame_count():
    channels, block_bytes, spb = 2, 72, 65
    data = IC.random_blocks(channels, block_bytes, 7)
    full = decode_ima_adpcm(data, channels, block_bytes)
    for kw, frames in (({}, 7 * spb), ({"fact": 7 * spb - 1}, 7 * spb - 1), ({"fact": 6 * spb + 1}, 6 * spb + 1), ({"fact": 0}, 0),
                       ({"fact": 7 * spb + 1}, 7 * spb),                    # more than the blocks hold: all of theirs
                       ({"samples_per_block": None}, 7 * spb), ({"trailing": IC.list_chunk(301)}, 7 * spb)):
        blob = IC.wav_bytes(channels, 11025, block_bytes, data, **kw)
        info = scan_audio(io.BytesIO(blob))
        assert info == wavio.WavInfo(wavio.ENC_IMA_ADPCM, channels, 11025, frames, 0, info.offset, block_bytes, spb), kw
        assert blob[info.offset:info.offset + len(data)] == data
        x, sr = load(blob, mono=False)
        assert sr == 11025 and np.array_equal(bits(x), bits(IC.floats(full[:frames], mono=False))), kw
    # a partial trailing block is dropped, with or without an odd byte count; `fact` is held against the WHOLE blocks
    for extra in (1, 35, 71):
        blob = IC.wav_bytes(channels, 11025, block_bytes, data + b"\x77" * extra, fact=7 * spb + 3)
        assert scan_audio(io.BytesIO(blob)).n_frames == 7 * spb
        assert np.array_equal(bits(load(blob, mono=False)[0]), bits(IC.floats(full, mono=False)))
    raw = wavio.read_audio_raw(io.BytesIO(IC.wav_bytes(channels, 11025, block_bytes, data, fact=6 * spb + 1)))
    assert (raw.format, raw.channels, raw.n_frames, bytes(raw.data)) == (14, channels, 6 * spb + 1, data)
    assert wavio.ENC_IMA_ADPCM == 14 and len(wavio.BYTES_PER_SAMPLE) == 14
    assert wavio.WavInfo(1, 2, 16000, 10, 4, 44) == wavio.WavInfo(1, 2, 16000, 10, 4, 44, 0, 0)
    # an extensible header around the tag reads the same
    body = struct.pack("<HHIIHH", 0xFFFE, 1, 8000, 4055, 256, 4) + struct.pack("<HHI", 22, 505, 0) + struct.pack("<H", 0x11) + bytes(14)
    mono = IC.random_blocks(1, 256, 2)
    blob = b"RIFF" + struct.pack("<I", 4 + 8 + len(body) + 8 + len(mono)) + b"WAVE" + b"fmt " + struct.pack("<I", len(body)) + body + \
        b"data" + struct.pack("<I", len(mono)) + mono
    assert scan_audio(io.BytesIO(blob))[:4] == (14, 1, 8000, 1010)


def test_malformed_headers_are_refused_by_both_walks():
    data = IC.random_blocks(2, 72, 2)
    cases = [(IC.wav_bytes(2, 8000, 72, data, samples_per_block=64), "wSamplesPerBlock 64 does not match the 65 samples"),
             (IC.wav_bytes(2, 8000, 76, data), "unsupported IMA ADPCM nBlockAlign 76 for 2 channels"),
             (IC.wav_bytes(2, 8000, 8, data, samples_per_block=None), "unsupported IMA ADPCM nBlockAlign 8 for 2 channels"),
             (IC.wav_bytes(2, 8000, 72, data, bits=3), "unsupported IMA ADPCM width 3"),
             (IC.wav_bytes(2, 8000, 72, data, tag=2), "unsupported WAVE format tag 2")]
    for blob, text in cases:
        for call in (load, lambda v: scan_audio(io.BytesIO(v)), lambda v: wavio.read_wav_raw(io.BytesIO(v))):
            with pytest.raises(ValueError, match=text):
                call(blob)


def test_duration_and_rate_come_from_the_scan(tmp_path):
    from whisperseg_amd import audio_utils
    spb = IC.block_frames(1, 256)
    for name, kw, frames in (("a.wav", {}, 40 * spb), ("b.wav", {"cut": 5}, 40 * spb - 5)):
        path = tmp_path / name
        path.write_bytes(IC.make_wav(1, 256, 40, sr=8000, **kw))
        assert audio_utils.get_sampling_rate(str(path)) == 8000
        assert audio_utils.get_audio_duration(str(path)) == frames / 8000


# ---- 3. the piece plan ------------------------------------------------------------------------------------------------------------
def test_piece_plan_of_a_block_file_by_brute_force():
    for channels, block_bytes, n_blocks, cut in ((1, 256, 100, 0), (2, 72, 37, 64), (3, 24, 16, 1), (1, 8, 33, 8), (2, 2048, 5, 100)):
        spb = IC.block_frames(channels, block_bytes)
        info = scan_audio(io.BytesIO(IC.make_wav(channels, block_bytes, n_blocks, cut=cut)))
        assert info.n_frames == n_blocks * spb - cut
        assert [wavio.piece_bytes(info, n) for n in (0, 1, spb, spb + 1, 16 * spb)] == [0, block_bytes, block_bytes, 2 * block_bytes, 16 * block_bytes]
        for buffer_bytes in (16 * block_bytes, 16 * block_bytes + 15, 50 * block_bytes, 1 << 20):
            for chunk_frames in (None, 16 * spb, 32 * spb):
                step = wavio.chunk_plan(info, buffer_bytes, chunk_frames)
                assert step % (16 * spb) == 0 and step > 0
                covered, byte0 = 0, 0
                for frame0 in range(0, info.n_frames, step):
                    n = min(step, info.n_frames - frame0)
                    nbytes = wavio.piece_bytes(info, n)
                    assert frame0 == covered and frame0 % 16 == 0 and byte0 % 16 == 0 and byte0 == frame0 // spb * block_bytes
                    assert nbytes <= buffer_bytes and nbytes == -(-n // spb) * block_bytes
                    if frame0 + n < info.n_frames:
                        assert n == step and n % (16 * spb) == 0
                    else:                                               # the last piece carries the `fact`-cut frame count
                        assert frame0 + n == n_blocks * spb - cut and byte0 + nbytes == n_blocks * block_bytes
                    covered, byte0 = covered + n, byte0 + nbytes
                assert covered == info.n_frames
        with pytest.raises(ValueError, match="multiple of 16 blocks"):
            wavio.chunk_plan(info, 1 << 20, 16 * spb + 16)
        if n_blocks > 15:
            with pytest.raises(ValueError, match="does not hold 16 blocks"):
                wavio.chunk_plan(info, 15 * block_bytes, None)
    # a file that fits the buffer whole is one piece, however few blocks the buffer holds
    info = scan_audio(io.BytesIO(IC.make_wav(2, 2048, 5)))
    assert wavio.chunk_plan(info, 5 * 2048) >= info.n_frames
    # sample encodings plan as before
    pcm = wavio.WavInfo(1, 2, 16000, 1000, 4, 44)
    assert wavio.chunk_plan(pcm, 4096) == 1024 and wavio.piece_bytes(pcm, 48) == 192


# ---- 4. the file pipeline over a host stand-in ------------------------------------------------------------------------------------
class AdpcmHostIngest(PlanarHostIngest):
    """PlanarHostIngest decoding block files with audioop (ima_adpcm_cases.audioop_decode), and a `resample` that is the oracle's —
    there is no open_resampled, so the pipeline takes its resample-only fallback."""

    def check(self, view, nbytes, info, frame0, n_frames):
        assert info.format == wavio.ENC_IMA_ADPCM and info.frame_bytes == 0
        assert frame0 % (16 * info.block_frames) == 0 and nbytes == wavio.piece_bytes(info, n_frames) <= len(view)
        return IC.audioop_decode(bytes(view[:nbytes]), info.channels, info.block_bytes)[:n_frames]

    def submit(self, view, nbytes, info, out, frame0, n_frames):
        self.calls.append(("submit", frame0, n_frames))
        out[frame0:frame0 + n_frames] = IC.floats(self.check(view, nbytes, info, frame0, n_frames))
        return {"queries": 0}

    def submit_planar(self, view, nbytes, info, out, frame0, n_frames, first_channel):
        self.calls.append(("submit_planar", frame0, n_frames, first_channel, out.shape[0]))
        planes = IC.floats(self.check(view, nbytes, info, frame0, n_frames), mono=False).reshape(info.channels, n_frames)
        out[:, frame0:frame0 + n_frames] = planes[first_channel:first_channel + out.shape[0]]
        return {"queries": 0}

    def resample(self, out, sr_in, sr_out):
        self.calls.append(("resample", out.shape, sr_in, sr_out))
        return resampled(out, sr_in, sr_out)


def resampled(a, sr_in, sr_out):
    if sr_in == sr_out or not a.shape[-1]:
        return a
    return resample_poly_ref(a, sr_in, sr_out) if a.ndim == 1 else np.stack([resample_poly_ref(r, sr_in, sr_out) for r in a])


@pytest.fixture(scope="module")
def adpcm_folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("adpcm")
    files = [("0_stereo.wav", IC.make_wav(2, 72, 90, seed=1, sr=16000, cut=7)),
             ("1_three.wav", IC.make_wav(3, 108, 41, seed=2, sr=8000, trailing=IC.list_chunk(77))),
             ("2_short.wav", IC.make_wav(2, 512, 3, seed=3, sr=16000)),
             ("3_nine.wav", IC.wav_bytes(9, 32000, 72, IC.random_blocks(9, 72, 50, seed=4) + b"\x55" * 13))]
    paths = []
    for name, blob in files:
        (d / name).write_bytes(blob)
        paths.append(str(d / name))
    return paths


def test_pipeline_over_adpcm_files(adpcm_folder):
    paths = adpcm_folder
    mono = [load_audio(p) for p in paths]
    planar = [load_audio(p, mono=False) for p in paths]
    assert [a.shape[0] for a, _ in mono] == [90 * 65 - 7, 41 * 65, 3 * 505, 50 * 9]
    host = AdpcmHostIngest()
    equal_items(list(wavio.FilePipeline(paths, host, buffer_bytes=2048)), mono)
    assert sum(c[0] == "submit" for c in host.calls) > 2 * len(paths)          # in pieces (the short file whole: 3 blocks)
    equal_items(list(wavio.FilePipeline(paths, AdpcmHostIngest(), buffer_bytes=2048, channel_id=1)), [(a[1], sr) for a, sr in planar])
    equal_items(list(wavio.FilePipeline(paths, AdpcmHostIngest(), buffer_bytes=2048, channel_id="all")), planar)
    host = AdpcmHostIngest()
    got = list(wavio.FilePipeline(paths, host, buffer_bytes=2048, sr=16000))
    equal_items(got, [(resampled(a, sr, 16000), 16000) for a, sr in mono])
    assert [c[2:] for c in host.calls if c[0] == "resample"] == [(8000, 16000), (32000, 16000)]
    equal_items(list(wavio.FilePipeline(paths, AdpcmHostIngest(), sr=16000, channel_id="all")),
                [(resampled(a, sr, 16000), 16000) for a, sr in planar])
    equal_items(list(wavio.FilePipeline(paths, AdpcmHostIngest())), mono)     # whole files
    assert not reader_threads()


def test_pipeline_names_the_block_file_its_buffers_cannot_hold(adpcm_folder, tmp_path):
    big = tmp_path / "big_blocks.wav"
    big.write_bytes(IC.make_wav(2, 2048, 17))
    with pytest.raises(ValueError, match=r"big_blocks\.wav.*16 blocks of 2048 bytes"):
        list(wavio.FilePipeline(adpcm_folder[:1] + [str(big)], AdpcmHostIngest(), buffer_bytes=8192))
    assert not reader_threads()
