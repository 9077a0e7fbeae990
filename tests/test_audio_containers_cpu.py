"""The containers and sample encodings beyond little-endian RIFF/WAVE PCM, without a GPU: AIFF / AIFF-C, AU, RF64 / BW64 and
G.711 files read by whisperseg_amd.wavio (load_audio / scan_audio / read_audio_raw) against the stdlib's own readers and writers
(aifc, sunau, audioop), the numpy restatement of the device arithmetic (audio_cases.restate) against load_audio, and the file
pipeline over a folder that mixes the containers.  Every comparison is bit equality."""
import aifc
import audioop
import io
import os
import struct
import sunau
import sys

import numpy as np
import pytest

import audio_cases as AC
import wav_cases as WC
from conftest import ROOT
from oracle.resample import resample_poly_ref
from test_wav_planar_cpu import PlanarHostIngest, equal_items, reader_threads
from whisperseg_amd import wavio
from whisperseg_amd.wavio import load_audio, load_wav, read_audio_raw, scan_audio


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def load(blob, **kw):
    return load_audio(io.BytesIO(blob), **kw)


def ints_be(data, width):
    """Signed big-endian integers of `width` bytes, as aifc / sunau hand frames out."""
    b = np.frombuffer(data, np.uint8).reshape(-1, width).astype(np.int64)
    v = sum(b[:, i] << (8 * (width - 1 - i)) for i in range(width))
    return (v ^ (1 << (8 * width - 1))) - (1 << (8 * width - 1))


def rows(x, channels):
    """Interleaved float32 samples -> what load_audio(mono=False) returns."""
    return x if channels == 1 else np.ascontiguousarray(x.reshape(-1, channels).T)


# ---- G.711 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["ulaw", "alaw"])
def test_g711_wave_files_decode_to_the_audioop_tables(enc):
    codes = bytes(range(256))
    lin = audioop.ulaw2lin(codes, 2) if enc == "ulaw" else audioop.alaw2lin(codes, 2)
    table = np.frombuffer(lin, "<i2")
    assert (table.min(), table.max()) == ((-32124, 32124) if enc == "ulaw" else (-32256, 32256))
    want = table.astype(np.float32) / np.float32(32768)
    for extensible in (False, True):
        x, sr = load(AC.g711_wav_bytes(enc, 1, 8000, codes, extensible=extensible))
        assert sr == 8000 and same(x, want)
        assert same(load_wav(io.BytesIO(AC.g711_wav_bytes(enc, 1, 8000, codes, extensible=extensible)))[0], want)
    stereo, _ = load(AC.g711_wav_bytes(enc, 2, 8000, codes), mono=False)
    assert same(stereo, rows(want, 2))
    info = scan_audio(io.BytesIO(AC.g711_wav_bytes(enc, 2, 8000, codes)))
    assert info == wavio.WavInfo(AC.code_of(enc), 2, 8000, 128, 2, 44)
    if enc == "ulaw":
        assert want[0x7F] == 0 and want[0xFF] == 0
    else:
        assert table[0x55] == -8 and table[0xD5] == 8


def test_g711_at_another_width_is_refused_by_both_walks():
    blob = bytearray(AC.g711_wav_bytes("ulaw", 1, 8000, b"\x00\x00"))
    struct.pack_into("<H", blob, 34, 16)
    with pytest.raises(ValueError, match="unsupported G.711 width 16") as a:
        load_wav(io.BytesIO(bytes(blob)))
    with pytest.raises(ValueError) as b:
        wavio.read_wav_raw(io.BytesIO(bytes(blob)))
    assert str(a.value) == str(b.value)


# ---- AIFF ---------------------------------------------------------------------------------------------------------------------
def aifc_written(width, channels, sr, frames, comptype=None):
    f = AC.KeptBytesIO()
    w = aifc.open(f, "wb")
    w.setnchannels(channels)
    w.setsampwidth(width)
    w.setframerate(sr)
    if comptype is not None:
        w.setcomptype(comptype, comptype)
    w.writeframes(frames)
    w.close()
    return f.getvalue()


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_aiff_files_written_by_aifc(width, channels):
    enc = ("s8", "s16be", "s24be", "s32be")[width - 1]
    for n, sr in ((0, 8000), (1, 22050), (5, 44100), (1021, 250000)):
        blob = aifc_written(width, channels, sr, AC.random_data(enc, channels, n, seed=3))
        r = aifc.open(io.BytesIO(blob), "rb")
        assert r.getnframes() == n and r.getsampwidth() == width
        ints = ints_be(r.readframes(n), width)
        want = ints.astype(np.float32) / np.float32(2.0 ** (8 * width - 1))
        x, got_sr = load(blob, mono=False)
        assert got_sr == r.getframerate() == sr
        assert same(x, rows(want, channels)), (width, channels, n)
        mono, _ = load(blob)
        assert same(mono, AC.restate(AC.random_data(enc, channels, n, seed=3), enc, channels, n))
        info = scan_audio(io.BytesIO(blob))
        assert (info.format, info.channels, info.sr, info.n_frames, info.frame_bytes) == (AC.code_of(enc), channels, sr, n, channels * width)
    if n:
        assert want.min() == -1.0       # the planted extreme reached the comparison


def test_aiff_built_by_hand():
    data = AC.random_data("s24be", 1, 101)          # 303 bytes: an odd-length SSND
    want, _ = load(AC.aiff_bytes(1, 32000, 24, data))
    assert want.shape == (101,) and want[0] == -1.0
    for blob in (AC.aiff_bytes(1, 32000, 24, data, ssnd_offset=6),
                 AC.aiff_bytes(1, 32000, 24, data, comm_last=True),
                 AC.aiff_bytes(1, 32000, 24, data, comm_last=True, ssnd_offset=6, extra=b"NAME" + struct.pack(">I", 3) + b"abc\x00")):
        x, sr = load(blob)
        assert sr == 32000 and same(x, want)
        assert bytes(read_audio_raw(io.BytesIO(blob)).data) == data
    assert scan_audio(io.BytesIO(AC.aiff_bytes(1, 32000, 24, data, ssnd_offset=6))).offset == 12 + 26 + 8 + 8 + 6
    # the header's count and the bytes present: the smaller wins
    assert same(load(AC.aiff_bytes(1, 32000, 24, data, n_frames=40))[0], want[:40])
    assert same(load(AC.aiff_bytes(1, 32000, 24, data[:-4], n_frames=101))[0], want[:99])
    # a 12-bit sample sits left-justified in two bytes; rates that are no integers round to nearest
    x, sr = load(AC.aiff_bytes(2, 22050.5, 12, AC.random_data("s16be", 2, 9)), mono=False)
    assert sr == 22051 and same(x, AC.restate_planar(AC.random_data("s16be", 2, 9), "s16be", 2, 9))
    assert load(AC.aiff_bytes(1, 11024.25, 16, b"\x00\x00"))[1] == 11024
    with pytest.raises(ValueError, match="sample rate"):
        load(AC.aiff_bytes(1, 0.25, 16, b"\x00\x00"))


# ---- AIFF-C -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["ulaw", "alaw"])
def test_aifc_g711_files_written_by_aifc(enc):
    lin = np.arange(-32768, 32768, 37, dtype="<i2").tobytes()               # aifc compresses 16-bit frames itself
    lin = lin[:len(lin) // 12 * 12]
    for channels in (1, 2, 3):
        blob = aifc_written(2, channels, 8000, lin, comptype=enc.upper().encode())
        codes = audioop.lin2ulaw(lin, 2) if enc == "ulaw" else audioop.lin2alaw(lin, 2)
        back = audioop.ulaw2lin(codes, 2) if enc == "ulaw" else audioop.alaw2lin(codes, 2)
        assert aifc.open(io.BytesIO(blob), "rb").readframes(1 << 20) == back
        want = np.frombuffer(back, "<i2").astype(np.float32) / np.float32(32768)
        x, sr = load(blob, mono=False)
        assert sr == 8000 and same(x, rows(want, channels))
        assert scan_audio(io.BytesIO(blob)).format == AC.code_of(enc)
    for kind in (enc.encode(), enc.upper().encode()):
        x, _ = load(AC.aiff_bytes(1, 8000, 8, bytes(range(256)), compression=kind))
        assert same(x, AC.g711_tables()[enc == "alaw"].astype(np.float32) / np.float32(32768))


@pytest.mark.parametrize("fmt,kind", [("s16", b"sowt"), ("s24", b"sowt"), ("s32", b"sowt"), ("s16", b"NONE"), ("s24", b"twos"), ("s32", b"NONE"),
                                      ("f32", b"fl32"), ("f32", b"FL32"), ("f64", b"fl64"), ("f64", b"FL64")])
def test_aifc_by_hand_carries_the_data_chunk_of_a_wave_file(fmt, kind):
    for channels in (1, 3):
        wav = WC.make_wav(fmt, channels, 257)
        data = bytes(wavio.read_wav_raw(io.BytesIO(wav)).data)
        width = WC.BYTES[WC.FORMATS.index(fmt)]
        blob = AC.aiff_bytes(channels, 16000, 8 * width, data if kind == b"sowt" else AC.swap(data, width), compression=kind)
        for mono in (True, False):
            with np.errstate(over="ignore"):
                got, want = load(blob, mono=mono), load_wav(io.BytesIO(wav), mono=mono)
            assert got[1] == want[1] and same(got[0], want[0]), (fmt, kind, channels, mono)


def test_aifc_raw_is_unsigned_and_sowt_bytes_are_signed():
    data = WC.sample_bytes("u8", WC.SPECIAL["u8"])
    x, _ = load(AC.aiff_bytes(1, 8000, 8, data, compression=b"raw "))
    assert same(x, load_wav(io.BytesIO(WC.wav_bytes("u8", 1, 8000, data)))[0]) and x[0] == -1.0 and x[2] == 0.0
    s, _ = load(AC.aiff_bytes(1, 8000, 8, AC.sample_bytes("s8", AC.SPECIAL["s8"]), compression=b"sowt"))
    assert s.tolist() == [-1.0, 127 / 128, 0.0, -1 / 128, 1 / 128, 0.5]


# ---- AU -----------------------------------------------------------------------------------------------------------------------
def sunau_written(width, channels, sr, frames, comptype="NONE"):
    f = AC.KeptBytesIO()
    w = sunau.open(f, "wb")
    w.setnchannels(channels)
    w.setsampwidth(width)
    w.setframerate(sr)
    w.setcomptype(comptype, "")
    w.writeframes(frames)
    w.close()
    return f.getvalue()


@pytest.mark.parametrize("channels", [1, 2, 4])              # (the channel counts sunau writes)
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_au_linear_files_written_by_sunau(width, channels):
    enc = ("s8", "s16be", "s24be", "s32be")[width - 1]
    for n in (0, 5, 1021):
        data = AC.random_data(enc, channels, n, seed=4)
        blob = sunau_written(width, channels, 44100, data)
        r = sunau.open(io.BytesIO(blob), "rb")
        assert r.getnframes() == n
        want = ints_be(r.readframes(n), width).astype(np.float32) / np.float32(2.0 ** (8 * width - 1))
        x, sr = load(blob, mono=False)
        assert sr == 44100 and same(x, rows(want, channels))
        assert scan_audio(io.BytesIO(blob)).format == AC.code_of(enc)


def test_au_ulaw_written_by_sunau_and_the_hand_built_encodings():
    lin = np.arange(-32768, 32768, 41, dtype="<i2").tobytes()
    blob = sunau_written(2, 1, 8000, lin, comptype="ULAW")                  # sunau compresses 16-bit frames itself
    back = audioop.ulaw2lin(audioop.lin2ulaw(lin, 2), 2)
    assert sunau.open(io.BytesIO(blob), "rb").readframes(1 << 20) == back
    assert same(load(blob)[0], np.frombuffer(back, "<i2").astype(np.float32) / np.float32(32768))
    assert same(load(AC.au_bytes("alaw", 1, 8000, bytes(range(256))))[0], AC.g711_tables()[1].astype(np.float32) / np.float32(32768))
    for fmt, enc in (("f32", "f32be"), ("f64", "f64be")):
        wav = WC.make_wav(fmt, 2, 65)
        data = AC.swap(bytes(wavio.read_wav_raw(io.BytesIO(wav)).data), AC.BYTES[AC.code_of(enc)])
        with np.errstate(over="ignore"):
            got, want = load(AC.au_bytes(enc, 2, 16000, data)), load_wav(io.BytesIO(wav))
        assert got[1] == 16000 and same(got[0], want[0])


def test_au_unknown_size_and_annotation():
    data = AC.random_data("s16be", 2, 33)
    want, _ = load(AC.au_bytes("s16be", 2, 48000, data))
    assert want.shape == (33,)
    assert same(load(AC.au_bytes("s16be", 2, 48000, data, size=0xFFFFFFFF))[0], want)
    note = AC.au_bytes("s16be", 2, 48000, data, annotation=b"recorded at dusk")
    assert scan_audio(io.BytesIO(note)).offset == 40 and same(load(note)[0], want)
    assert same(load(AC.au_bytes("s16be", 2, 48000, data + b"\x01\x02\x03", size=0xFFFFFFFF))[0], want)      # cut inside a frame
    assert same(load(AC.au_bytes("s16be", 2, 48000, data + b"\x7f" * 8, size=len(data)))[0], want)            # bytes behind the size


# ---- RF64 / BW64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("riff_id", [b"RF64", b"BW64"])
def test_rf64_with_a_trailing_chunk_equals_the_plain_riff_file(riff_id):
    for fmt, channels, n in (("s16", 2, 1021), ("s24", 1, 333), ("f32", 3, 64), ("u8", 1, 77)):
        wav = WC.make_wav(fmt, channels, n)
        data = bytes(wavio.read_wav_raw(io.BytesIO(wav)).data)
        blob = AC.rf64_bytes(fmt, channels, 16000, data, riff_id=riff_id, trailing=AC.list_chunk(301))
        for mono in (True, False):
            got, want = load(blob, mono=mono), load_wav(io.BytesIO(wav), mono=mono)
            assert got[1] == want[1] and same(got[0], want[0]), (fmt, mono)
            assert same(load_wav(io.BytesIO(blob), mono=mono)[0], want[0])
        raw = read_audio_raw(io.BytesIO(blob))
        assert bytes(raw.data) == data and raw.n_frames == n
        assert scan_audio(io.BytesIO(blob)).offset == 12 + 36 + 24 + 8
    # without a ds64 the size is taken as far as the file goes, as before
    wav = WC.make_wav("s16", 1, 50)
    data = bytes(wavio.read_wav_raw(io.BytesIO(wav)).data)
    assert same(load(AC.rf64_bytes("s16", 1, 16000, data, riff_id=riff_id, ds64=False))[0], load_wav(io.BytesIO(wav))[0])
    assert len(load(AC.rf64_bytes("s16", 1, 16000, data, riff_id=riff_id, ds64=False, trailing=AC.list_chunk(20)))[0]) == 50 + 14


# ---- raw reads ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3, 8, 9])
@pytest.mark.parametrize("enc", AC.ENCODINGS)
def test_raw_bytes_and_restated_arithmetic_equal_load_audio(enc, channels):
    n = 257
    data = AC.random_data(enc, channels, n)
    width = AC.BYTES[AC.code_of(enc)]
    for blob, frames in ((AC.container_bytes(enc, channels, 16000, data), n),
                         (AC.container_bytes(enc, channels, 16000, data[:len(data) - width]), n - 1)):
        raw = read_audio_raw(io.BytesIO(blob))
        assert (raw.format, raw.channels, raw.sr, raw.n_frames) == (AC.code_of(enc), channels, 16000, frames)
        assert bytes(raw.data) == data[:frames * channels * width] and wavio.BYTES_PER_SAMPLE[raw.format] == width
        with np.errstate(over="ignore"):
            want, sr = load(blob)
            planar, _ = load(blob, mono=False)
        assert sr == 16000 and want.shape == (frames,)
        assert same(AC.restate(raw.data, raw.format, channels, frames), want)
        assert same(rows(np.ascontiguousarray(AC.restate_planar(raw.data, raw.format, channels, frames).T).reshape(-1), channels), planar)
    assert len(wavio.BYTES_PER_SAMPLE) == 14 == len(AC.BYTES) and tuple(wavio.BYTES_PER_SAMPLE) == AC.BYTES


def test_special_values_are_in_the_cases():
    for enc in AC.NEW:
        raw = read_audio_raw(io.BytesIO(AC.make_audio(enc, 1, 300)))
        assert bytes(raw.data).startswith(AC.sample_bytes(enc, AC.SPECIAL[enc]))
    assert bytes(read_audio_raw(io.BytesIO(AC.make_audio("s16be", 1, 8))).data)[:4] == b"\x80\x00\x7f\xff"
    with np.errstate(over="ignore"):
        x, _ = load(AC.make_audio("f64be", 1, 64))
    assert x[1] == np.float32(1 + 2.0 ** -22) and np.isinf(x[5])
    x, _ = load(AC.make_audio("s32be", 1, 64))
    assert x[0] == -1.0 and x[5] == np.float32(2.0 ** -7) and x[6] == np.float32(1 - 2.0 ** -24)
    assert sorted(set(bytes(read_audio_raw(io.BytesIO(AC.make_audio("alaw", 2, 128))).data))) == list(range(256))


def test_into_fills_the_callers_buffer(tmp_path):
    path = tmp_path / "a.aiff"
    path.write_bytes(AC.make_audio("s24be", 2, 1021))
    plain = read_audio_raw(str(path))
    buf = np.full(8192, 0xEE, np.uint8)
    raw = read_audio_raw(str(path), into=buf)
    assert raw[1:] == plain[1:] and bytes(raw.data) == bytes(plain.data) == bytes(buf[:1021 * 6]) and (buf[1021 * 6:] == 0xEE).all()


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_errors_are_the_same_from_both_readers():
    no_comm = b"FORM" + struct.pack(">I", 4 + 16 + 2) + b"AIFF" + b"SSND" + struct.pack(">III", 10, 0, 0) + b"\x00\x00"
    cases = [(AC.aiff_bytes(1, 8000, 16, b"\x00\x00", compression=b"ima4"), "ima4"),
             (AC.au_bytes(23, 1, 8000, b"\x00\x00"), "23"),
             (no_comm, "COMM"),
             (b"OggS" + b"\x00" * 60, "container"),
             (b"FORM\x00\x00\x00\x048SVX", "container"),
             (b".snd" + b"\x00" * 8, "AU header"),
             (AC.aiff_bytes(1, 8000, 40, b"\x00" * 5), "width 40"),
             (b"", "container")]
    for blob, word in cases:
        with pytest.raises(ValueError, match=word) as a:
            load(blob)
        with pytest.raises(ValueError) as b:
            read_audio_raw(io.BytesIO(blob))
        with pytest.raises(ValueError) as c:
            scan_audio(io.BytesIO(blob))
        assert str(a.value) == str(b.value) == str(c.value), blob[:16]
    for blob in (b"RIFF\x00\x00\x00\x00JUNK" + b"\x00" * 32, b"RF64\xff\xff\xff\xffWAVX"):
        for call in (load, lambda v: read_audio_raw(io.BytesIO(v)), lambda v: load_wav(io.BytesIO(v))):
            with pytest.raises(ValueError, match="^not a RIFF/WAVE file$"):
                call(blob)
    # the WAVE-only functions stay WAVE-only
    for call in (lambda v: load_wav(io.BytesIO(v)), lambda v: wavio.read_wav_raw(io.BytesIO(v)), lambda v: wavio.scan_wav(io.BytesIO(v))):
        with pytest.raises(ValueError, match="^not a RIFF/WAVE file$"):
            call(AC.make_audio("s16be", 1, 4))
    # pinned before: MS-ADPCM and 12-bit PCM
    for offset, value, text in ((20, 2, "unsupported WAVE format tag 2"), (34, 12, "unsupported PCM width 12")):
        blob = bytearray(WC.wav_bytes("s16", 1, 16000, b"\x00\x00"))
        struct.pack_into("<H", blob, offset, value)
        with pytest.raises(ValueError, match=text):
            load(bytes(blob))


# ---- the file pipeline over a folder of mixed containers ----------------------------------------------------------------------
class MixedHostIngest(PlanarHostIngest):
    """PlanarHostIngest decoding with audio_cases' restatements (every encoding), and a `resample` that is the oracle's."""

    def submit(self, view, nbytes, info, out, frame0, n_frames):
        assert frame0 % 16 == 0 and nbytes == n_frames * info.frame_bytes <= len(view)
        self.calls.append(("submit", frame0, n_frames))
        out[frame0:frame0 + n_frames] = AC.restate(view[:nbytes], info.format, info.channels, n_frames)
        return {"queries": 0}

    def submit_planar(self, view, nbytes, info, out, frame0, n_frames, first_channel):
        assert frame0 % 16 == 0 and nbytes == n_frames * info.frame_bytes <= len(view) and out.ndim == 2
        self.calls.append(("submit_planar", frame0, n_frames, first_channel, out.shape[0]))
        out[:, frame0:frame0 + n_frames] = AC.restate_planar(view[:nbytes], info.format, info.channels, n_frames)[first_channel:first_channel + out.shape[0]]
        return {"queries": 0}

    def resample(self, out, sr_in, sr_out):
        self.calls.append(("resample", out.shape, sr_in, sr_out))
        return resampled(out, sr_in, sr_out)


def resampled(a, sr_in, sr_out):
    if sr_in == sr_out or not a.shape[-1]:
        return a
    return resample_poly_ref(a, sr_in, sr_out) if a.ndim == 1 else np.stack([resample_poly_ref(r, sr_in, sr_out) for r in a])


@pytest.fixture(scope="module")
def mixed_folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("mixed")
    wav = WC.make_wav("s16", 2, 3000, seed=5, sr=16000)
    files = [("0.wav", wav),
             ("1_s24.aiff", AC.make_audio("s24be", 2, 2100, seed=1, sr=32000)),
             ("2_ulaw.aifc", AC.aiff_bytes(3, 8000, 8, AC.random_data("ulaw", 3, 4500, seed=2), compression=b"ulaw")),
             ("3_s16.au", AC.au_bytes("s16be", 2, 16000, AC.random_data("s16be", 2, 2500, seed=3), annotation=b"four" * 4)),
             ("4_rf64.wav", AC.rf64_bytes("s16", 2, 16000, bytes(wavio.read_wav_raw(io.BytesIO(wav)).data), trailing=AC.list_chunk(9001)))]
    paths = []
    for name, blob in files:
        (d / name).write_bytes(blob)
        paths.append(str(d / name))
    return paths


def test_pipeline_over_mixed_containers(mixed_folder):
    paths = mixed_folder
    mono = [load_audio(p) for p in paths]
    planar = [load_audio(p, mono=False) for p in paths]
    assert same(mono[4][0], mono[0][0]) and [sr for _, sr in mono] == [16000, 32000, 8000, 16000, 16000]
    host = MixedHostIngest()
    equal_items(list(wavio.FilePipeline(paths, host, buffer_bytes=8192)), mono)
    assert sum(c[0] == "submit" for c in host.calls) >= 2 * len(paths)          # every file went through in pieces
    assert not reader_threads()
    equal_items(list(wavio.FilePipeline(paths, MixedHostIngest(), buffer_bytes=8192, channel_id=1)), [(a[1], sr) for a, sr in planar])
    equal_items(list(wavio.FilePipeline(paths, MixedHostIngest(), buffer_bytes=8192, channel_id="all")), planar)
    assert not reader_threads()
    host = MixedHostIngest()
    got = list(wavio.FilePipeline(paths, host, buffer_bytes=8192, sr=16000))
    equal_items(got, [(resampled(a, sr, 16000), 16000) for a, sr in mono])
    assert [c[2:] for c in host.calls if c[0] == "resample"] == [(32000, 16000), (8000, 16000)]
    got = list(wavio.FilePipeline(paths, MixedHostIngest(), buffer_bytes=8192, sr=16000, channel_id="all"))
    equal_items(got, [(resampled(a, sr, 16000), 16000) for a, sr in planar])
    assert not reader_threads()
    # whole files give the same items
    equal_items(list(wavio.FilePipeline(paths, MixedHostIngest())), mono)
    assert not reader_threads()


def test_pipeline_names_the_file_it_cannot_read(mixed_folder, tmp_path):
    bad = tmp_path / "x.aifc"
    bad.write_bytes(AC.aiff_bytes(1, 8000, 16, b"\x00\x00", compression=b"ima4"))
    with pytest.raises(ValueError, match=r"x\.aifc.*ima4"):
        list(wavio.FilePipeline(mixed_folder[:2] + [str(bad)], MixedHostIngest()))
    assert not reader_threads()


# ---- callers ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    return segment


def test_cli_audio_ext_argument(cli, tmp_path):
    p = cli.build_parser()
    assert p.parse_args(["--audio_folder", "d"]).audio_ext is None
    assert p.parse_args(["--audio_ext", "wav", "aiff", "aifc", "au"]).audio_ext == ["wav", "aiff", "aifc", "au"]
    with pytest.raises(SystemExit):
        p.parse_args(["--audio_ext"])
    assert cli.folder_patterns(None) == ["*.wav", "*.WAV"]                    # today's two globs, in today's order
    assert cli.folder_patterns(["aiff", "au"]) == ["*.aiff", "*.AIFF", "*.au", "*.AU"]
    assert cli.folder_patterns([".Wav"]) == ["*.wav", "*.WAV"]


def test_cli_stdin_goes_through_load_audio(cli, monkeypatch):
    blob = AC.make_audio("s24be", 2, 100)

    class Stdin:
        buffer = io.BytesIO(blob)

    monkeypatch.setattr(sys, "stdin", Stdin)
    audio, sr = cli.stdin_wav()
    assert sr == 16000 and same(audio, load(blob)[0])
    Stdin.buffer = io.BytesIO(blob)
    audio, _ = cli.stdin_wav(channel_id=1)
    assert same(audio, load(blob, mono=False)[0][1])


def test_sampling_rate_and_duration_from_the_header_alone(tmp_path):
    import audio_utils as shim
    from whisperseg_amd import audio_utils
    assert shim.get_sampling_rate is audio_utils.get_sampling_rate and shim.get_audio_duration is audio_utils.get_audio_duration
    cases = [("a.wav", WC.make_wav("s16", 2, 4000, sr=16000), 16000, 0.25),
             ("b.aiff", AC.make_audio("s24be", 3, 1000, sr=250000), 250000, 0.004),
             ("c.au", AC.au_bytes("ulaw", 1, 8000, bytes(12000), size=0xFFFFFFFF), 8000, 1.5)]
    for name, blob, sr, seconds in cases:
        path = tmp_path / name
        path.write_bytes(blob)
        assert audio_utils.get_sampling_rate(str(path)) == sr
        assert audio_utils.get_audio_duration(str(path)) == seconds
    # no sample is read: a file whose samples are missing answers the same from its header
    path = tmp_path / "d.aiff"
    path.write_bytes(AC.aiff_bytes(1, 44100, 16, b"", n_frames=0))
    assert audio_utils.get_sampling_rate(str(path)) == 44100 and audio_utils.get_audio_duration(str(path)) == 0.0
    (tmp_path / "e.bin").write_bytes(b"\x00" * 64)
    with pytest.raises(ValueError, match="container"):
        audio_utils.get_sampling_rate(str(tmp_path / "e.bin"))
