"""The channels of a recording decoded to planes on the GPU (wseg_pcm_to_planar_f32) equal the host definition bit for bit —
wavio.load_wav(mono=False), itself pinned by test_wav_planar_cpu.py — and write nothing but the floats they address; the callers
on top (load_wav_device, segment_channels, segment_files, the CLI's --channel_id) give what the host-picked channels give."""
import glob
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import planar_cases as PC
import wav_cases as WC
from conftest import GOLDEN, ROOT
from planar_cases import bits
from tools import tiny_model as TM
from whisperseg_amd.wavio import PLANAR_GRID_CAP, PLANAR_TILE_FRAMES as T, load_wav, load_wav_device

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
FRAMES = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, 1021, T - 1, T, T + 1, 2 * T + 3)
SENTINEL = -12345.5
LEAD, TAIL = 5, 9                    # sentinel floats in front of the first plane (which is then not 16-byte aligned) and behind the last


def device_raw(data):
    """The data chunk's bytes in a device allocation rounded up to 16 bytes (torch aligns allocations to 512)."""
    n = len(data)
    raw = torch.zeros(max(16, -(-n // 16) * 16), dtype=torch.uint8, device="cuda")
    raw[:n] = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()
    assert raw.data_ptr() % 16 == 0
    return raw


def decode_planes(lib, fmt, channels, n, first=0, count=None, seed=0):
    """Decode channels first .. first + count - 1 of a random data chunk into planes n + 7 floats apart inside a buffer of
    sentinels; check the planes' bits and that every float outside them still holds the sentinel."""
    from whisperseg_amd import _lib
    count = channels - first if count is None else count
    data = PC.data_chunk(fmt, channels, n, seed)
    stride = n + 7
    buf = torch.full((LEAD + (count - 1) * stride + n + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
    assert (buf.data_ptr() + 4 * LEAD) % 16 != 0
    _lib.check(lib.wseg_pcm_to_planar_f32(device_raw(data).data_ptr(), n, channels, WC.FORMATS.index(fmt), first, count,
                                          buf.data_ptr() + 4 * LEAD, stride, _lib.stream_ptr()))
    host = buf.cpu().numpy()
    want = PC.planes(data, fmt, channels, n, first, count)
    addressed = np.zeros(len(host), bool)
    for c in range(count):
        lo = LEAD + c * stride
        addressed[lo:lo + n] = True
        got = host[lo:lo + n]
        assert np.array_equal(bits(got), bits(want[c])), (fmt, channels, n, first + c, np.flatnonzero(bits(got) != bits(want[c]))[:8])
    assert (bits(host[~addressed]) == bits(np.float32(SENTINEL))).all(), (fmt, channels, n, np.flatnonzero((host != SENTINEL) & ~addressed)[:8])


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8, 9, 64])
@pytest.mark.parametrize("fmt", WC.FORMATS)
def test_kernel_equals_the_host_definition(gpu_lib, fmt, channels):
    for n in FRAMES:
        decode_planes(gpu_lib, fmt, channels, n)


@pytest.mark.parametrize("fmt", WC.FORMATS)
def test_sub_ranges_of_channels(gpu_lib, fmt):
    for channels, first, count in ((3, 1, 1), (5, 2, 3), (64, 63, 1), (1, 0, 1)):
        for n in (5, 257, T + 1):
            decode_planes(gpu_lib, fmt, channels, n, first, count, seed=1)


def test_expected_values_are_load_wavs():
    """The restatement the kernel is compared with is the host definition (CPU side: test_wav_planar_cpu.py), planted values included."""
    for fmt in WC.FORMATS:
        blob = WC.make_wav(fmt, 3, 65)
        got, _ = load_wav(io.BytesIO(blob), mono=False)
        assert np.array_equal(bits(got), bits(PC.planes(PC.data_chunk(fmt, 3, 65), fmt, 3, 65)))


def test_grid_stride_wraps(gpu_lib):
    """More tiles than the launch has workgroups: u8 mono, 2 MiB."""
    decode_planes(gpu_lib, "u8", 1, PLANAR_GRID_CAP * T + 5)


def test_no_frames_and_invalid_arguments(gpu_lib):
    lib = gpu_lib
    raw = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda")
    r, o = raw.data_ptr(), out.data_ptr()
    call = lambda *a: lib.wseg_pcm_to_planar_f32(*a, None)
    assert call(r, 0, 2, 1, 0, 2, o, 0) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    #            raw    n  ch fmt first count out stride
    for args, word in (((None, 4, 2, 1, 0, 2, o, 8), "raw"), ((r + 4, 4, 2, 1, 0, 2, o, 8), "raw"),
                       ((r, 4, 2, 1, 0, 2, None, 8), "out"), ((r, 4, 2, 1, 0, 2, o + 2, 8), "out"),
                       ((r, 4, 0, 1, 0, 1, o, 8), "channels"), ((r, 4, 65, 1, 0, 2, o, 8), "channels"),
                       ((r, 4, 2, 6, 0, 2, o, 8), "format"), ((r, 4, 2, -1, 0, 2, o, 8), "format"),
                       ((r, -1, 2, 1, 0, 2, o, 8), "n_frames"),
                       ((r, 4, 2, 1, 2, 1, o, 8), "first_channel"), ((r, 4, 2, 1, -1, 1, o, 8), "first_channel"),
                       ((r, 4, 2, 1, 1, 2, o, 8), "n_out_channels"), ((r, 4, 2, 1, 0, 0, o, 8), "n_out_channels"),
                       ((r, 4, 2, 1, 0, 3, o, 8), "n_out_channels"),
                       ((r, 4, 2, 1, 0, 2, o, 3), "plane_stride"), ((r, 4, 2, 1, 0, 2, o, -8), "plane_stride")):
        assert call(*args) == -1, args
        assert word in lib.wseg_last_error().decode(), (args, lib.wseg_last_error())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert call(r, 4, 2, 1, 1, 1, o + 4, -8) == 0          # one plane: plane_stride is ignored
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[1:5] == 0).all() and host[0] == SENTINEL and (host[5:] == SENTINEL).all()


def test_load_wav_device_planar_and_channel_id(gpu_lib, tmp_path):
    for fmt, channels, n, sr in (("s24", 5, 1021, 44100), ("s16", 2, 4099, 16000)):
        path = tmp_path / f"{fmt}_{channels}.wav"
        path.write_bytes(WC.make_wav(fmt, channels, n, sr=sr))
        want, want_sr = load_wav(str(path), mono=False)
        assert want.shape == (channels, n)
        for kw in ({}, {"chunk_frames": 48}):
            got, got_sr = load_wav_device(str(path), mono=False, **kw)
            assert got_sr == want_sr == sr and got.is_cuda and got.dtype == torch.float32 and got.is_contiguous()
            assert got.shape == want.shape and np.array_equal(bits(got.cpu().numpy()), bits(want))
            for k in (0, channels - 1, -1, -channels):
                row, _ = load_wav_device(str(path), channel_id=k, **kw)
                assert row.shape == (n,) and np.array_equal(bits(row.cpu().numpy()), bits(want[k])), (fmt, k, kw)
            mix, _ = load_wav_device(str(path), **kw)                                # the default is the mono mix, as before
            assert np.array_equal(bits(mix.cpu().numpy()), bits(load_wav(str(path))[0]))
        for k in (channels, -channels - 1):
            with pytest.raises(IndexError):
                load_wav_device(str(path), channel_id=k)
    mono = WC.make_wav("s24", 1, 1021)
    want, _ = load_wav(io.BytesIO(mono))
    for kw in ({"channel_id": 3}, {"mono": False}, {"channel_id": 3, "chunk_frames": 48}):
        got, _ = load_wav_device(io.BytesIO(mono), **kw)                             # a one-channel file ignores channel_id
        assert got.shape == (1021,) and np.array_equal(bits(got.cpu().numpy()), bits(want))
    empty, _ = load_wav_device(io.BytesIO(WC.make_wav("s16", 3, 0)), mono=False)
    assert empty.shape == (3, 0)


def test_load_wav_device_channel_id_all_gives_every_plane(gpu_lib):
    """channel_id="all" is mono=False: the planes of load_wav(mono=False), not the first of them — from a sample file in five
    pieces (the last one ragged), from an IMA ADPCM file whose `fact` count cuts the last block, and resampled piece by piece."""
    import ima_adpcm_cases as IC
    from whisperseg_amd.resample import resample
    s16 = WC.make_wav("s16", 3, 300)
    adpcm = IC.make_wav(2, 256, 5, cut=100)
    for blob, kw, shape in ((s16, {"chunk_frames": 64}, (3, 300)), (adpcm, {"chunk_frames": 16 * IC.block_frames(2, 256)}, (2, 5 * 249 - 100))):
        want, sr = load_wav(io.BytesIO(blob), mono=False)
        assert want.shape == shape
        got, got_sr = load_wav_device(io.BytesIO(blob), channel_id="all", **kw)
        planes, _ = load_wav_device(io.BytesIO(blob), mono=False, **kw)
        assert got_sr == sr and got.shape == shape and np.array_equal(bits(got.cpu().numpy()), bits(want))
        assert torch.equal(got.view(torch.int32), planes.view(torch.int32))
    want = resample(torch.from_numpy(load_wav(io.BytesIO(s16), mono=False)[0]).cuda(), 16000, 32000)
    got, got_sr = load_wav_device(io.BytesIO(s16), channel_id="all", sr=32000, chunk_frames=64)
    planes, _ = load_wav_device(io.BytesIO(s16), mono=False, sr=32000, chunk_frames=64)
    assert got_sr == 32000 and got.shape == want.shape == (3, 600)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got.view(torch.int32), planes.view(torch.int32))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """meerkat_5s.wav as is; s16 stereo: the signal, and the signal reversed in time; s24 x 3 channels at twice the rate: the
    signal, silence, the signal at half amplitude."""
    from scipy.signal import resample_poly
    d = tmp_path_factory.mktemp("channels")
    src = os.path.join(GOLDEN, "meerkat_5s.wav")
    x, sr = load_wav(src)
    assert sr == TM.SR
    with open(src, "rb") as f:
        (d / "a_meerkat.wav").write_bytes(f.read())
    q = lambda v, full: np.clip(np.round(v * full), -full, full - 1).astype(np.int64)
    stereo = np.stack([q(x, 32768), q(x[::-1], 32768)], axis=1).reshape(-1)
    (d / "b_s16_stereo.wav").write_bytes(WC.wav_bytes("s16", 2, sr, WC.sample_bytes("s16", stereo)))
    x2 = resample_poly(x, 2, 1)
    three = np.stack([q(x2, 1 << 23), np.zeros(len(x2), np.int64), q(0.5 * x2, 1 << 23)], axis=1).reshape(-1)
    (d / "c_s24_three.WAV").write_bytes(WC.wav_bytes("s24", 3, 2 * sr, WC.sample_bytes("s24", three)))
    return str(d)


def test_segment_files_channels_and_cli_equal_the_host_path(gpu_lib, folder, tmp_path):
    """With the fixture model the meerkat signal at 16 kHz gives no rows forwards or reversed, so the stereo file's two channels give
    the SAME (empty) result — the reference decode in float32 on the host says so too: no rows for either channel, four rows
    (two of cluster c, two of a) for their mono mix.  That channels differ from each other is therefore asserted on the
    three-channel file (5 rows for the signal at 32 kHz, none for silence, 7 for the half-amplitude signal), that they differ from
    the mono mix on the stereo file."""
    from whisperseg_amd.model import WhisperSegmenter
    seg = WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")
    kw = dict(spec_time_step=TM.STS)
    paths = glob.glob(folder + "/*.wav") + glob.glob(folder + "/*.WAV")          # the CLI's order
    assert len(paths) == 3
    planar = [load_wav(p, mono=False) for p in paths]
    assert sorted(a.ndim for a, _ in planar) == [1, 2, 2]
    per_channel = [[seg.segment(row, sr, **kw) for row in (a if a.ndim == 2 else [a])] for a, sr in planar]
    assert [seg.segment_channels(a, sr, **kw) for a, sr in planar] == per_channel
    device_audio, sr = load_wav_device(paths[-1], mono=False)
    assert seg.segment_channels(device_audio, sr, **kw) == per_channel[-1]
    # not vacuous: channels give different rows from each other (the three-channel file) and from the mono mix (the stereo file)
    stereo = next(i for i, p in enumerate(paths) if p.endswith("b_s16_stereo.wav"))
    three = next(i for i, p in enumerate(paths) if p.endswith("c_s24_three.WAV"))
    mix = seg.segment(*load_wav(paths[stereo]), **kw)
    assert mix["onset"] and mix not in per_channel[stereo]
    sig, silence, half = per_channel[three]
    assert sig["onset"] and half["onset"] and not silence["onset"] and sig != half
    picked = seg.segment_batch(((a if a.ndim == 1 else a[1], sr) for a, sr in planar), **kw)
    assert picked == [g[min(1, len(g) - 1)] for g in per_channel]
    for buffer_bytes in (seg.ingest_buffer_bytes, 64 * 1024):                     # whole files; every file in pieces
        seg.ingest_buffer_bytes = buffer_bytes
        assert seg.segment_files(paths, channel_id=1, **kw) == picked
        assert seg.segment_files(paths, channel_id="all", **kw) == per_channel
    # the CLI's folder mode with --channel_id all writes those rows
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        from segment import table, write_csv
    finally:
        sys.path.pop(0)
    text = io.StringIO()
    columns, rows = table(per_channel, [os.path.basename(p) for p in paths], all_channels=True)
    assert columns == ["filename", "channel", "onset", "offset", "cluster"] and len({r[:2] for r in rows}) >= 2
    write_csv(columns, rows, text)
    out = tmp_path / "channels.csv"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "segment.py"), "--model_path", MODEL_DIR, "--audio_folder", folder,
                           "--csv_save_path", str(out), "--spec_time_step", str(TM.STS), "--channel_id", "all"],
                          env=dict(os.environ, WHISPERSEG_AMD_DTYPE="f32"))
    assert out.read_text() == text.getvalue()
