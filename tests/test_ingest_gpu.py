"""WAVE samples decoded on the GPU (wseg_pcm_to_mono_f32) equal whisperseg_amd.wavio.load_wav bit for bit, and the callers on
top — load_wav_device, SegmenterBase.segment_files, the CLI's folder mode — give what the host path gives."""
import glob
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd.wavio import load_wav, load_wav_device, read_wav_raw

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
FRAMES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1021, 4099)      # edges of the 4-frame lane group, the wave, the workgroup
SENTINEL = -12345.5


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def device_raw(data):
    """The data chunk's bytes in a device allocation rounded up to 16 bytes (torch aligns allocations to 512)."""
    n = len(data)
    raw = torch.zeros(max(16, -(-n // 16) * 16), dtype=torch.uint8, device="cuda")
    raw[:n] = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()
    assert raw.data_ptr() % 16 == 0
    return raw


def decode_on_device(lib, blob, guard=16):
    """-> (float32 host array, load_wav's array) of an in-memory file; `out` sits between two sentinel regions of `guard` floats."""
    from whisperseg_amd import _lib
    raw = read_wav_raw(io.BytesIO(blob))
    dev = device_raw(raw.data)
    buf = torch.full((raw.n_frames + 2 * guard,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[guard:guard + raw.n_frames]
    _lib.check(lib.wseg_pcm_to_mono_f32(dev.data_ptr(), raw.n_frames, raw.channels, raw.format, out.data_ptr(), _lib.stream_ptr()))
    host = buf.cpu().numpy()
    assert (host[:guard] == SENTINEL).all() and (host[guard + raw.n_frames:] == SENTINEL).all()
    return host[guard:guard + raw.n_frames], load_wav(io.BytesIO(blob))[0]


@pytest.mark.parametrize("channels", [1, 2, 3, 5])
@pytest.mark.parametrize("fmt", WC.FORMATS)
def test_kernel_equals_load_wav(gpu_lib, fmt, channels):
    for n in FRAMES:
        got, want = decode_on_device(gpu_lib, WC.make_wav(fmt, channels, n))
        assert got.shape == want.shape == (n,)
        assert np.array_equal(bits(got), bits(want)), (fmt, channels, n, np.flatnonzero(bits(got) != bits(want))[:8])


@pytest.mark.parametrize("fmt", WC.FORMATS)
def test_kernel_equals_load_wav_from_8_channels_on(gpu_lib, fmt):
    """numpy's mean sums 8 and more channels pairwise; the kernel follows it.  Also: an `out` that is not 16-byte aligned."""
    for channels, n in ((8, 257), (9, 66), (17, 65), (24, 7), (64, 67)):
        got, want = decode_on_device(gpu_lib, WC.make_wav(fmt, channels, n), guard=5)
        assert np.array_equal(bits(got), bits(want)), (fmt, channels, n)
    got, want = decode_on_device(gpu_lib, WC.make_wav(fmt, 2, 1021), guard=3)
    assert np.array_equal(bits(got), bits(want)), fmt


def test_special_values_are_in_the_cases():
    """The planted values reach the comparison: extremes, s32 values that round, float64 ties, a denormal, a value beyond the range."""
    for fmt in WC.FORMATS:
        x, _ = load_wav(io.BytesIO(WC.make_wav(fmt, 1, 64)))
        raw = read_wav_raw(io.BytesIO(WC.make_wav(fmt, 1, 64)))
        assert bytes(raw.data).startswith(WC.sample_bytes(fmt, WC.SPECIAL[fmt]))
        assert x[0] == {"u8": -1.0, "s16": -1.0, "s24": -1.0, "s32": -1.0, "f32": 0.0, "f64": 1.0}[fmt]
    x, _ = load_wav(io.BytesIO(WC.make_wav("f64", 1, 64)))
    assert x[1] == np.float32(1 + 2.0 ** -22) and np.isinf(x[5]) and 0 < x[3] < np.finfo(np.float32).tiny
    x, _ = load_wav(io.BytesIO(WC.make_wav("s32", 1, 64)))
    assert x[5] == np.float32(2.0 ** -7) and x[6] == np.float32(1 - 2.0 ** -24)      # 2^24 + 1 and 2^31 - 65 both rounded


def test_no_frames_and_invalid_arguments(gpu_lib):
    lib = gpu_lib
    raw = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.full((8,), SENTINEL, dtype=torch.float32, device="cuda")
    call = lambda r, n, ch, fmt, o: lib.wseg_pcm_to_mono_f32(r, n, ch, fmt, o, None)
    assert call(raw.data_ptr(), 0, 2, 1, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    for args, word in (((None, 4, 1, 1, out.data_ptr()), "raw"), ((raw.data_ptr() + 4, 4, 1, 1, out.data_ptr()), "raw"),
                       ((raw.data_ptr(), 4, 1, 1, None), "out"), ((raw.data_ptr(), 4, 0, 1, out.data_ptr()), "channels"),
                       ((raw.data_ptr(), 4, 65, 1, out.data_ptr()), "channels"), ((raw.data_ptr(), 4, 1, 6, out.data_ptr()), "format"),
                       ((raw.data_ptr(), 4, 1, -1, out.data_ptr()), "format"), ((raw.data_ptr(), -1, 1, 1, out.data_ptr()), "n_frames")):
        assert call(*args) == -1, args
        assert word in lib.wseg_last_error().decode(), (args, lib.wseg_last_error())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


def test_load_wav_device_in_pieces(gpu_lib, tmp_path):
    path = tmp_path / "s24_stereo.wav"
    path.write_bytes(WC.make_wav("s24", 2, 1021, sr=44100))
    want, sr = load_wav(str(path))
    whole, sr_a = load_wav_device(str(path))
    pieces, sr_b = load_wav_device(str(path), chunk_frames=48)
    assert sr == sr_a == sr_b == 44100 and whole.is_cuda and whole.dtype == torch.float32
    assert np.array_equal(bits(whole.cpu().numpy()), bits(want)) and np.array_equal(bits(pieces.cpu().numpy()), bits(want))
    empty, _ = load_wav_device(io.BytesIO(WC.make_wav("s16", 2, 0)))
    assert empty.shape == (0,)
    with pytest.raises(ValueError, match="unsupported PCM width"):
        blob = bytearray(WC.make_wav("s16", 1, 4))
        blob[34] = 12
        load_wav_device(io.BytesIO(bytes(blob)))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """meerkat_5s.wav as is, the same signal as s16 stereo, s24 mono at twice the rate and f32 at three times the rate: three
    front-end configurations (16 / 32 / 48 kHz) that pool into one decode."""
    from scipy.signal import resample_poly
    d = tmp_path_factory.mktemp("wavs")
    src = os.path.join(GOLDEN, "meerkat_5s.wav")
    x, sr = load_wav(src)
    assert sr == TM.SR
    with open(src, "rb") as f:
        (d / "a_meerkat.wav").write_bytes(f.read())
    q = lambda v, full: np.clip(np.round(v * full), -full, full - 1).astype(np.int64)
    stereo = np.stack([q(x, 32768), q(0.5 * x, 32768)], axis=1).reshape(-1)
    (d / "b_s16_stereo.wav").write_bytes(WC.wav_bytes("s16", 2, sr, WC.sample_bytes("s16", stereo)))
    x2 = resample_poly(x, 2, 1)
    (d / "c_s24_mono.WAV").write_bytes(WC.wav_bytes("s24", 1, 2 * sr, WC.sample_bytes("s24", q(x2, 1 << 23))))
    x3 = resample_poly(x, 3, 1).astype(np.float32)
    (d / "d_f32.wav").write_bytes(WC.wav_bytes("f32", 1, 3 * sr, WC.sample_bytes("f32", x3), junk_before_data=7))
    return str(d)


def test_segment_files_and_cli_equal_the_host_path(gpu_lib, folder, tmp_path):
    from whisperseg_amd.model import WhisperSegmenter
    seg = WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")
    paths = glob.glob(folder + "/*.wav") + glob.glob(folder + "/*.WAV")        # the CLI's order
    assert len(paths) == 4
    want = seg.segment_batch((load_wav(p) for p in paths), spec_time_step=TM.STS)
    assert sum(len(w["onset"]) for w in want) >= 4
    assert seg.segment_files(paths, spec_time_step=TM.STS) == want
    assert seg.segment_files(paths, spec_time_step=TM.STS) == want             # again: the pinned buffers are re-used
    seg.ingest_buffer_bytes = 64 * 1024                                        # every file in pieces
    assert seg.segment_files(paths, spec_time_step=TM.STS) == want
    one, sr = load_wav_device(paths[1])
    assert seg.segment(one, sr, spec_time_step=TM.STS) == want[1]
    # the CLI's folder mode writes the rows of the host path
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        from segment import write_csv
    finally:
        sys.path.pop(0)
    rows = [(os.path.basename(p), on, off, c) for p, w in zip(paths, want) for on, off, c in zip(w["onset"], w["offset"], w["cluster"])]
    text = io.StringIO()
    write_csv(["filename", "onset", "offset", "cluster"], rows, text)
    out = tmp_path / "folder.csv"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "segment.py"), "--model_path", MODEL_DIR, "--audio_folder", folder,
                           "--csv_save_path", str(out), "--spec_time_step", str(TM.STS)], env=dict(os.environ, WHISPERSEG_AMD_DTYPE="f32"))
    assert out.read_text() == text.getvalue()
