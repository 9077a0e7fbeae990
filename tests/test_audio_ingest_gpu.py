"""The sample encodings beyond little-endian WAVE PCM decoded on the GPU (wseg_samples_to_mono_f32 /
wseg_samples_to_planar_f32, encodings 6..13) equal whisperseg_amd.wavio.load_audio bit for bit — itself pinned against the stdlib's
readers by test_audio_containers_cpu.py — and write nothing but the floats they address; the callers on top (load_wav_device,
segment_files, the CLI's --audio_ext) give on AIFF, AIFF-C, AU and RF64 files what the host path gives."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_cases as AC
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd.wavio import PLANAR_TILE_FRAMES as T, load_audio, load_wav, load_wav_device, read_audio_raw, read_wav_raw

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
FRAMES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1021, 4099)      # edges of the 4-frame lane group, the wave, the workgroup
PLANAR_FRAMES = (15, 16, 17, T - 1, T, T + 1, 2 * T + 1)                # the pass and tile edges
SENTINEL = -12345.5


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def device_raw(data):
    """The sample bytes in a device allocation rounded up to 16 bytes (torch aligns allocations to 512)."""
    n = len(data)
    raw = torch.zeros(max(16, -(-n // 16) * 16), dtype=torch.uint8, device="cuda")
    raw[:n] = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()
    assert raw.data_ptr() % 16 == 0
    return raw


_WANT = {}


def case(enc, channels, n):
    """-> (file bytes, load_audio's mono array, its planes [channels, n]) of one random file, computed once."""
    key = (enc, channels, n)
    if key not in _WANT:
        blob = AC.make_audio(enc, channels, n)
        with np.errstate(over="ignore", invalid="ignore"):
            mono, planes = load_audio(io.BytesIO(blob))[0], load_audio(io.BytesIO(blob), mono=False)[0].reshape(channels, n)
        mono.setflags(write=False)
        planes.setflags(write=False)
        _WANT[key] = blob, mono, planes
    return _WANT[key]


def decode_mono(lib, enc, channels, n, guard=16):
    """Decode a file's samples to mono between two sentinel regions of `guard` floats; compare with load_audio's bits."""
    from whisperseg_amd import _lib
    blob, want, _ = case(enc, channels, n)
    raw = read_audio_raw(io.BytesIO(blob))
    assert (raw.format, raw.channels, raw.n_frames) == (AC.code_of(enc), channels, n)
    buf = torch.full((n + 2 * guard,), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(lib.wseg_samples_to_mono_f32(device_raw(raw.data).data_ptr(), n, channels, raw.format, buf.data_ptr() + 4 * guard,
                                            _lib.stream_ptr()))
    host = buf.cpu().numpy()
    assert (host[:guard] == SENTINEL).all() and (host[guard + n:] == SENTINEL).all(), (enc, channels, n)
    got = host[guard:guard + n]
    assert np.array_equal(bits(got), bits(want)), (enc, channels, n, np.flatnonzero(bits(got) != bits(want))[:8])


@pytest.mark.parametrize("channels", [1, 2, 3, 5])
@pytest.mark.parametrize("enc", AC.NEW)
def test_mono_kernel_equals_load_audio(gpu_lib, enc, channels):
    for n in FRAMES:
        decode_mono(gpu_lib, enc, channels, n)


@pytest.mark.parametrize("enc", AC.NEW)
def test_mono_kernel_from_8_channels_on_and_unaligned_out(gpu_lib, enc):
    """numpy's mean sums 8 and more channels pairwise; the kernel follows it.  Also: an `out` three floats off a 16-byte boundary."""
    for channels, n in ((8, 257), (9, 66), (17, 65), (64, 67)):
        decode_mono(gpu_lib, enc, channels, n, guard=5)
    decode_mono(gpu_lib, enc, 2, 1021, guard=3)
    decode_mono(gpu_lib, enc, 1, 1021, guard=3)


def decode_planes(lib, enc, channels, n, first, count, lead):
    """Channels first .. first + count - 1 into planes n + 7 floats apart, the first `lead` floats behind a 16-byte boundary (the
    stride moves the others), inside a buffer of sentinels; planes' bits are load_audio(mono=False)'s rows, the rest is untouched."""
    from whisperseg_amd import _lib
    blob, _, planes = case(enc, channels, n)
    raw = read_audio_raw(io.BytesIO(blob))
    stride, tail = n + 7, 9
    buf = torch.full((4 + lead + (count - 1) * stride + n + tail,), SENTINEL, dtype=torch.float32, device="cuda")
    base = 4 + lead
    assert (buf.data_ptr() + 4 * base) % 16 == 4 * (lead % 4)
    _lib.check(lib.wseg_samples_to_planar_f32(device_raw(raw.data).data_ptr(), n, channels, raw.format, first, count,
                                              buf.data_ptr() + 4 * base, stride, _lib.stream_ptr()))
    host = buf.cpu().numpy()
    addressed = np.zeros(len(host), bool)
    for c in range(count):
        lo = base + c * stride
        addressed[lo:lo + n] = True
        got, want = host[lo:lo + n], planes[first + c]
        assert np.array_equal(bits(got), bits(want)), (enc, channels, n, first + c, lead, np.flatnonzero(bits(got) != bits(want))[:8])
    assert (bits(host[~addressed]) == bits(np.float32(SENTINEL))).all(), (enc, channels, n, lead)


@pytest.mark.parametrize("shape", [(2, 0, 2), (3, 1, 1), (8, 2, 5), (9, 0, 9), (64, 63, 1)])
@pytest.mark.parametrize("enc", AC.NEW)
def test_planar_kernel_equals_load_audio(gpu_lib, enc, shape):
    channels, first, count = shape
    for i, n in enumerate(PLANAR_FRAMES):
        decode_planes(gpu_lib, enc, channels, n, first, count, lead=i % 4)
    for lead in range(4):                      # every offset from a 16-byte boundary at one size
        decode_planes(gpu_lib, enc, channels, 17, first, count, lead)


def test_expected_values_hold_the_planted_ones():
    """What the kernels are compared with carries the extremes, the byte-swapped special values and all 256 G.711 codes."""
    for enc in AC.NEW:
        blob, mono, planes = case(enc, 1, 1021)
        assert bytes(read_audio_raw(io.BytesIO(blob)).data).startswith(AC.sample_bytes(enc, AC.SPECIAL[enc]))
        assert np.array_equal(bits(mono), bits(planes[0])) and np.array_equal(bits(mono), bits(AC.restate(read_audio_raw(io.BytesIO(blob)).data, enc, 1, 1021)))
    assert case("s8", 1, 1021)[1][:2].tolist() == [-1.0, 127 / 128]
    assert case("s24be", 1, 1021)[1][0] == -1.0 and case("s32be", 1, 1021)[1][6] == np.float32(1 - 2.0 ** -24)
    assert np.isinf(case("f64be", 1, 1021)[1][5]) and case("f64be", 1, 1021)[1][1] == np.float32(1 + 2.0 ** -22)
    assert case("ulaw", 1, 1021)[1][0] == -32124 / 32768 and case("alaw", 1, 1021)[1][0x55] == -8 / 32768


def test_argument_checks_of_the_new_entry_points(gpu_lib):
    lib = gpu_lib
    raw = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda")
    r, o = raw.data_ptr(), out.data_ptr()
    mono = lambda *a: lib.wseg_samples_to_mono_f32(*a, None)
    planar = lambda *a: lib.wseg_samples_to_planar_f32(*a, None)
    assert mono(r, 0, 2, 12, o) == 0 and planar(r, 0, 2, 7, 0, 2, o, 0) == 0          # no frames: nothing is launched
    #            raw  n  ch enc out
    for args, word in (((None, 4, 1, 7, o), "raw"), ((r + 4, 4, 1, 7, o), "raw"), ((r, 4, 1, 7, None), "out"), ((r, 4, 1, 7, o + 2), "out"),
                       ((r, 4, 0, 7, o), "channels"), ((r, 4, 65, 7, o), "channels"), ((r, 4, 1, 14, o), "encoding"), ((r, 4, 1, -1, o), "encoding"),
                       ((r, -1, 1, 7, o), "n_frames")):
        assert mono(*args) == -1, args
        assert word in lib.wseg_last_error().decode() and "wseg_samples_to_mono_f32" in lib.wseg_last_error().decode(), (args, lib.wseg_last_error())
    #            raw  n  ch enc first count out stride
    for args, word in (((None, 4, 2, 13, 0, 2, o, 8), "raw"), ((r + 4, 4, 2, 13, 0, 2, o, 8), "raw"), ((r, 4, 2, 13, 0, 2, None, 8), "out"),
                       ((r, 4, 2, 13, 0, 2, o + 2, 8), "out"), ((r, 4, 0, 13, 0, 1, o, 8), "channels"), ((r, 4, 65, 13, 0, 2, o, 8), "channels"),
                       ((r, 4, 2, 14, 0, 2, o, 8), "encoding"), ((r, 4, 2, -1, 0, 2, o, 8), "encoding"), ((r, -1, 2, 13, 0, 2, o, 8), "n_frames"),
                       ((r, 4, 2, 13, 2, 1, o, 8), "first_channel"), ((r, 4, 2, 13, -1, 1, o, 8), "first_channel"),
                       ((r, 4, 2, 13, 1, 2, o, 8), "n_out_channels"), ((r, 4, 2, 13, 0, 0, o, 8), "n_out_channels"),
                       ((r, 4, 2, 13, 0, 2, o, 3), "plane_stride")):
        assert planar(*args) == -1, args
        assert word in lib.wseg_last_error().decode() and "wseg_samples_to_planar_f32" in lib.wseg_last_error().decode(), (args, lib.wseg_last_error())
    # the old entry points go on rejecting every code from 6 on
    assert lib.wseg_pcm_to_mono_f32(r, 4, 1, 6, o, None) == -1 and "format" in lib.wseg_last_error().decode()
    assert lib.wseg_pcm_to_planar_f32(r, 4, 2, 13, 0, 2, o, 8, None) == -1 and "format" in lib.wseg_last_error().decode()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()                                        # nothing was written on rejection
    # codes 0..5 are wseg_pcm_format: the same kernel, the same bits
    blob = WC.make_wav("s24", 3, 257)
    data = read_wav_raw(io.BytesIO(blob))
    got = torch.empty(257, dtype=torch.float32, device="cuda")
    assert mono(device_raw(data.data).data_ptr(), 257, 3, 2, got.data_ptr()) == 0
    assert np.array_equal(bits(got.cpu().numpy()), bits(load_wav(io.BytesIO(blob))[0]))


def test_load_wav_device_on_aiff_and_au(gpu_lib, tmp_path):
    from whisperseg_amd.resample import resample
    files = {"s24_stereo.aiff": AC.make_audio("s24be", 2, 1021, sr=44100),
             "ulaw.au": AC.au_bytes("ulaw", 1, 8000, AC.random_data("ulaw", 1, 1021), annotation=b"note" * 3)}
    for name, blob in files.items():
        path = tmp_path / name
        path.write_bytes(blob)
        want, sr = load_audio(str(path))
        for kw in ({}, {"chunk_frames": 48}):
            got, got_sr = load_wav_device(str(path), **kw)
            assert got_sr == sr and got.is_cuda and got.dtype == torch.float32
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (name, kw)
            planes, _ = load_wav_device(str(path), mono=False, **kw)
            assert np.array_equal(bits(planes.cpu().numpy()), bits(load_audio(str(path), mono=False)[0])), (name, kw)
            resampled, rate = load_wav_device(str(path), sr=16000, **kw)
            expect = resample(torch.from_numpy(want).cuda(), sr, 16000)
            assert rate == 16000 and torch.equal(resampled.view(torch.int32), expect.view(torch.int32)), (name, kw)
    row, _ = load_wav_device(str(tmp_path / "s24_stereo.aiff"), channel_id=1, chunk_frames=48)
    assert np.array_equal(bits(row.cpu().numpy()), bits(load_audio(str(tmp_path / "s24_stereo.aiff"), mono=False)[0][1]))
    with pytest.raises(ValueError, match="ima4"):
        load_wav_device(io.BytesIO(AC.aiff_bytes(1, 8000, 16, b"\x00\x00", compression=b"ima4")))


def rewrapped(d, stem, fmt, sr, data):
    """The samples of one little-endian data chunk as WAVE, AIFF, AIFF-C sowt, AU and RF64 with a trailing chunk."""
    width = WC.BYTES[WC.FORMATS.index(fmt)]
    (d / (stem + "_a.wav")).write_bytes(WC.wav_bytes(fmt, 1, sr, data))
    (d / (stem + "_b.aiff")).write_bytes(AC.aiff_bytes(1, sr, 8 * width, AC.swap(data, width)))
    (d / (stem + "_c.aifc")).write_bytes(AC.aiff_bytes(1, sr, 8 * width, data, compression=b"sowt"))
    (d / (stem + "_d.au")).write_bytes(AC.au_bytes(AC.ENCODINGS[6 + width - 1], 1, sr, AC.swap(data, width), annotation=b"meerkat\x00"))
    (d / (stem + "_e_rf64.wav")).write_bytes(AC.rf64_bytes(fmt, 1, sr, data, trailing=AC.list_chunk(40001)))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """meerkat_5s.wav as it is, and its samples re-wrapped: AIFF s16, AIFF-C sowt, AU s16, RF64 with a trailing chunk.  With the
    fixture model the recording gives no rows at 16 kHz (tests/test_ingest_planar_gpu.py), so the same signal at 32 kHz as s24 —
    which does — goes through the same five wrappings."""
    from scipy.signal import resample_poly
    d = tmp_path_factory.mktemp("containers")
    src = os.path.join(GOLDEN, "meerkat_5s.wav")
    with open(src, "rb") as f:
        (d / "meerkat.wav").write_bytes(f.read())
    raw = read_wav_raw(src)
    assert (raw.format, raw.channels, raw.sr) == (1, 1, TM.SR)
    rewrapped(d, "m16", "s16", raw.sr, bytes(raw.data))
    x2 = resample_poly(load_wav(src)[0], 2, 1)
    q = np.clip(np.round(x2 * (1 << 23)), -(1 << 23), (1 << 23) - 1).astype(np.int64)
    rewrapped(d, "m32", "s24", 2 * raw.sr, WC.sample_bytes("s24", q))
    return str(d)


def test_segment_files_and_cli_on_every_container(gpu_lib, folder, tmp_path):
    from whisperseg_amd.model import WhisperSegmenter
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        from segment import folder_patterns, table, write_csv
    finally:
        sys.path.pop(0)
    import glob
    exts = ["wav", "aiff", "aifc", "au"]
    paths = [p for pattern in folder_patterns(exts) for p in glob.glob(folder + "/" + pattern)]       # the CLI's order
    names = [os.path.basename(p) for p in paths]
    assert len(paths) == 11 and [os.path.splitext(n)[1] for n in names[5:]] == [".aiff"] * 2 + [".aifc"] * 2 + [".au"] * 2
    seg = WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")
    want = seg.segment_batch((load_audio(p) for p in paths), spec_time_step=TM.STS)
    by_name = dict(zip(names, want))
    original = seg.segment_batch([load_wav(os.path.join(GOLDEN, "meerkat_5s.wav"))], spec_time_step=TM.STS)[0]
    for name, w in by_name.items():                                                                   # the samples are identical
        assert w == (by_name["m32_a.wav"] if name.startswith("m32") else original), name
    print("rows per file:", {n: len(w["onset"]) for n, w in by_name.items()})
    assert len(by_name["m32_a.wav"]["onset"]) >= 1                                                    # not vacuous
    assert seg.segment_files(paths, spec_time_step=TM.STS) == want
    seg.ingest_buffer_bytes = 64 * 1024                                                               # every file in pieces
    assert seg.segment_files(paths, spec_time_step=TM.STS) == want
    text = io.StringIO()
    write_csv(*table(want, names), text)
    out = tmp_path / "containers.csv"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "segment.py"), "--model_path", MODEL_DIR, "--audio_folder", folder,
                           "--csv_save_path", str(out), "--spec_time_step", str(TM.STS), "--audio_ext"] + exts,
                          env=dict(os.environ, WHISPERSEG_AMD_DTYPE="f32"))
    assert out.read_text() == text.getvalue() and len(out.read_text().splitlines()) == 1 + 5 * len(by_name["m32_a.wav"]["onset"]) + 6 * len(original["onset"])
