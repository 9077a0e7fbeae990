"""IMA ADPCM blocks decoded on the GPU (wseg_ima_adpcm_to_mono_f32 / wseg_ima_adpcm_to_planar_f32) equal the host definition
whisperseg_amd.wavio.decode_ima_adpcm — pinned against the stdlib's audioop by test_ima_adpcm_cpu.py — bit for bit as float32, and
write nothing but the floats they address; the callers on top (load_wav_device, segment_files, the CLI) give on tag-0x11 WAVE files
what the host path gives."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ima_adpcm_cases as IC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import wavio
from whisperseg_amd.wavio import ADPCM_GRID_CAP, decode_ima_adpcm, load_audio, load_wav, load_wav_device

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
PER_CHANNEL = (8, 36, 256, 1024)          # block bytes per channel: 1, 8, 63 and 255 data dwords — one slice, two, three passes, ten
CHANNELS = (1, 2, 3, 5, 8, 9, 64)
GUARD = 8
NAN_BITS = np.float32(np.nan).view(np.uint32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def device_raw(data):
    """The blocks in a device allocation rounded up to 16 bytes (torch aligns allocations to 512)."""
    n = len(data)
    raw = torch.zeros(max(16, -(-n // 16) * 16), dtype=torch.uint8, device="cuda")
    raw[:n] = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()
    assert raw.data_ptr() % 16 == 0
    return raw


_CASES = {}


def case(per_channel, channels, n_blocks, seed=0):
    """-> (blocks, device copy, decode_ima_adpcm's int16 [n_blocks * spb, channels]) of random blocks, computed once; blocks are
    independent, so a prefix of the blocks decodes to the prefix of the frames."""
    key = (per_channel, channels, n_blocks, seed)
    if key not in _CASES:
        data = IC.random_blocks(channels, per_channel * channels, n_blocks, seed)
        pcm = decode_ima_adpcm(data, channels, per_channel * channels)
        pcm.setflags(write=False)
        _CASES[key] = data, device_raw(data), pcm
    return _CASES[key]


def block_counts(channels):
    group = 256 // channels
    return sorted({1, max(group - 1, 1), group, group + 1})


def run_mono(lib, per_channel, channels, n_blocks, cut, lead, of=None):
    """n_blocks blocks (of the case `of`, default its own) with `cut` frames off the last one -> out `lead` floats behind a 16-byte
    boundary, between NaN guards."""
    from whisperseg_amd import _lib
    block_bytes, spb = per_channel * channels, IC.block_frames(channels, per_channel * channels)
    _, raw, pcm = case(per_channel, channels, of or n_blocks)
    n = n_blocks * spb - cut
    buf = torch.full((4 + lead + n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    base = 4 + lead
    assert (buf.data_ptr() + 4 * base) % 16 == 4 * (lead % 4)
    _lib.check(lib.wseg_ima_adpcm_to_mono_f32(raw.data_ptr(), n_blocks, block_bytes, channels, n, buf.data_ptr() + 4 * base, _lib.stream_ptr()))
    host = buf.cpu().numpy()
    what = (per_channel, channels, n_blocks, cut, lead)
    assert (bits(host[:base]) == NAN_BITS).all() and (bits(host[base + n:]) == NAN_BITS).all(), what
    want = IC.floats(pcm[:n])
    got = host[base:base + n]
    assert np.array_equal(bits(got), bits(want)), (what, np.flatnonzero(bits(got) != bits(want))[:8])


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("per_channel", PER_CHANNEL)
def test_mono_kernel_equals_the_host_definition(gpu_lib, per_channel, channels):
    spb = IC.block_frames(channels, per_channel * channels)
    most = block_counts(channels)[-1]
    i = 0
    for n_blocks in block_counts(channels):
        for cut in (0, 1, spb - 1):                       # spb - 1: one frame is left of the last block
            run_mono(gpu_lib, per_channel, channels, n_blocks, cut, lead=i % 4, of=most)
            i += 1
    for lead in range(4):                                 # every offset from a 16-byte boundary at one size
        run_mono(gpu_lib, per_channel, channels, 2, 3, lead, of=most)


def run_planar(lib, per_channel, channels, n_blocks, cut, first, count, lead, of=None):
    """Channels first .. first + count - 1 into planes an odd number of floats apart, the first `lead` floats behind a 16-byte
    boundary, inside a buffer of NaNs: the planes are the host definition's, everything else is untouched."""
    from whisperseg_amd import _lib
    block_bytes, spb = per_channel * channels, IC.block_frames(channels, per_channel * channels)
    _, raw, pcm = case(per_channel, channels, of or n_blocks)
    n = n_blocks * spb - cut
    stride = n + 7 + n % 2                                # odd, and longer than a plane: guards between the planes
    base = 4 + lead
    buf = torch.full((base + (count - 1) * stride + n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.wseg_ima_adpcm_to_planar_f32(raw.data_ptr(), n_blocks, block_bytes, channels, n, first, count, buf.data_ptr() + 4 * base,
                                                stride, _lib.stream_ptr()))
    host = buf.cpu().numpy()
    what = (per_channel, channels, n_blocks, cut, first, count, lead)
    addressed = np.zeros(len(host), bool)
    want = pcm[:n].astype(np.float32) / np.float32(32768)
    for c in range(count):
        lo = base + c * stride
        addressed[lo:lo + n] = True
        got = host[lo:lo + n]
        assert np.array_equal(bits(got), bits(want[:, first + c])), (what, c, np.flatnonzero(bits(got) != bits(want[:, first + c]))[:8])
    assert (bits(host[~addressed]) == NAN_BITS).all(), what


def selections(channels):
    """All channels, one middle channel, the last two."""
    return sorted({(0, channels), (channels // 2, 1), (max(channels - 2, 0), min(channels, 2))})


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("per_channel", PER_CHANNEL)
def test_planar_kernel_equals_the_host_definition(gpu_lib, per_channel, channels):
    spb = IC.block_frames(channels, per_channel * channels)
    most = block_counts(channels)[-1]
    i = 0
    for first, count in selections(channels):
        for n_blocks in block_counts(channels):
            cut = (0, 1, spb - 1)[i % 3]
            run_planar(gpu_lib, per_channel, channels, n_blocks, cut, first, count, lead=i % 4, of=most)
            i += 1
    first, count = selections(channels)[-1]
    for cut in (0, 1, spb - 1):
        for lead in range(4):
            run_planar(gpu_lib, per_channel, channels, 2, cut, first, count, lead, of=most)


@pytest.mark.parametrize("channels", [1, 2, 64])
def test_more_groups_than_the_grid_take_the_stride(gpu_lib, channels):
    n_blocks = ADPCM_GRID_CAP * (256 // channels) + 3                   # of 8 bytes per channel: 2 MiB of blocks
    run_mono(gpu_lib, 8, channels, n_blocks, cut=2, lead=1)
    if channels > 1:
        run_planar(gpu_lib, 8, channels, n_blocks, 2, channels - 1, 1, lead=3)


def test_argument_checks(gpu_lib):
    lib = gpu_lib
    raw = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((1024,), float("nan"), dtype=torch.float32, device="cuda")
    r, o = raw.data_ptr(), out.data_ptr()
    mono = lambda *a: lib.wseg_ima_adpcm_to_mono_f32(*a, None)
    planar = lambda *a: lib.wseg_ima_adpcm_to_planar_f32(*a, None)
    assert mono(r, 0, 72, 2, 0, o) == 0 and planar(r, 0, 72, 2, 0, 0, 2, o, 0) == 0          # no blocks: nothing is launched
    #            raw blocks bytes ch frames out            (72 bytes, 2 channels: 65 frames a block)
    for args, word in (((None, 2, 72, 2, 130, o), "raw"), ((r + 4, 2, 72, 2, 130, o), "raw"), ((r, 2, 72, 2, 130, None), "out"),
                       ((r, 2, 72, 2, 130, o + 2), "out"), ((r, 2, 72, 0, 130, o), "channels"), ((r, 2, 72 * 65, 65, 130, o), "channels"),
                       ((r, 2, 8, 2, 2, o), "block_bytes"), ((r, 2, 76, 2, 130, o), "block_bytes"), ((r, 2, 70, 2, 130, o), "block_bytes"),
                       ((r, 2, 131080, 2, 130, o), "block_bytes"), ((r, 2, 0, 2, 130, o), "block_bytes"), ((r, 2, -72, 2, 130, o), "block_bytes"),
                       ((r, -1, 72, 2, 130, o), "n_blocks"), ((r, 1 << 46, 72, 2, 130, o), "n_blocks"),
                       ((r, 2, 72, 2, 131, o), "n_frames"), ((r, 2, 72, 2, 65, o), "n_frames"), ((r, 2, 72, 2, 0, o), "n_frames"),
                       ((r, 2, 72, 2, -1, o), "n_frames"), ((r, 0, 72, 2, 1, o), "n_frames")):
        assert mono(*args) == -1, args
        assert word in lib.wseg_last_error().decode() and "wseg_ima_adpcm_to_mono_f32" in lib.wseg_last_error().decode(), (args, lib.wseg_last_error())
    #            raw blocks bytes ch frames first count out stride
    for args, word in (((None, 2, 72, 2, 130, 0, 2, o, 200), "raw"), ((r + 8, 2, 72, 2, 130, 0, 2, o, 200), "raw"),
                       ((r, 2, 72, 2, 130, 0, 2, None, 200), "out"), ((r, 2, 72, 2, 130, 0, 2, o + 1, 200), "out"),
                       ((r, 2, 72, 0, 130, 0, 1, o, 200), "channels"), ((r, 2, 72, 65, 130, 0, 2, o, 200), "channels"),
                       ((r, 2, 76, 2, 130, 0, 2, o, 200), "block_bytes"), ((r, 2, 8, 2, 2, 0, 2, o, 200), "block_bytes"),
                       ((r, -1, 72, 2, 130, 0, 2, o, 200), "n_blocks"), ((r, 2, 72, 2, 131, 0, 2, o, 200), "n_frames"),
                       ((r, 2, 72, 2, 65, 0, 2, o, 200), "n_frames"), ((r, 2, 72, 2, 130, 2, 1, o, 200), "first_channel"),
                       ((r, 2, 72, 2, 130, -1, 1, o, 200), "first_channel"), ((r, 2, 72, 2, 130, 1, 2, o, 200), "n_out_channels"),
                       ((r, 2, 72, 2, 130, 0, 0, o, 200), "n_out_channels"), ((r, 2, 72, 2, 130, 0, 2, o, 129), "plane_stride")):
        assert planar(*args) == -1, args
        assert word in lib.wseg_last_error().decode() and "wseg_ima_adpcm_to_planar_f32" in lib.wseg_last_error().decode(), (args, lib.wseg_last_error())
    # the sample entry points go on rejecting the Python-side code of a block file
    assert lib.wseg_samples_to_mono_f32(r, 4, 1, wavio.ENC_IMA_ADPCM, o, None) == -1 and "encoding" in lib.wseg_last_error().decode()
    assert lib.wseg_samples_to_planar_f32(r, 4, 2, wavio.ENC_IMA_ADPCM, 0, 2, o, 8, None) == -1 and "encoding" in lib.wseg_last_error().decode()
    torch.cuda.synchronize()
    assert (bits(out.cpu().numpy()) == NAN_BITS).all()                                       # nothing was written on rejection


def test_load_wav_device_on_adpcm_files(gpu_lib, tmp_path):
    from whisperseg_amd.resample import resample
    x, _ = load_wav(os.path.join(GOLDEN, "meerkat_5s.wav"))
    pcm = np.round(x[:30000] * 32768).astype(np.int16)
    spb = IC.block_frames(2, 512)
    files = {"noise3.wav": (IC.make_wav(3, 108, 70, seed=1, sr=11025, cut=9), IC.block_frames(3, 108)),
             "meerkat2.wav": (IC.wav_bytes(2, 11025, 512, IC.encode(np.stack([pcm, pcm[::-1]], axis=1), 512), fact=len(pcm),
                                           trailing=IC.list_chunk(333)), spb)}
    for name, (blob, frames) in files.items():
        path = tmp_path / name
        path.write_bytes(blob)
        want, sr = load_audio(str(path))
        planes = load_audio(str(path), mono=False)[0]
        assert sr == 11025 and len(want) == (70 * frames - 9 if name == "noise3.wav" else len(pcm))
        for kw in ({}, {"chunk_frames": 16 * frames}):
            got, got_sr = load_wav_device(str(path), **kw)
            assert got_sr == sr and got.is_cuda and got.dtype == torch.float32
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (name, kw)
            got, _ = load_wav_device(str(path), mono=False, **kw)
            assert np.array_equal(bits(got.cpu().numpy()), bits(planes)), (name, kw)
            row, _ = load_wav_device(str(path), channel_id=-1, **kw)
            assert np.array_equal(bits(row.cpu().numpy()), bits(planes[-1])), (name, kw)
            resampled, rate = load_wav_device(str(path), sr=16000, **kw)         # through StreamResampler
            expect = resample(torch.from_numpy(want).cuda(), sr, 16000)
            assert rate == 16000 and torch.equal(resampled.view(torch.int32), expect.view(torch.int32)), (name, kw)
            resampled, _ = load_wav_device(str(path), sr=16000, channel_id=-2, **kw)
            expect = resample(torch.from_numpy(planes[-2].copy()).cuda(), sr, 16000)
            assert torch.equal(resampled.view(torch.int32), expect.view(torch.int32)), (name, kw)
        with pytest.raises(ValueError, match="multiple of 16 blocks"):
            load_wav_device(str(path), chunk_frames=16 * frames + 16)
    with pytest.raises(ValueError, match="unsupported WAVE format tag 2"):
        load_wav_device(io.BytesIO(IC.make_wav(1, 256, 2, tag=2)))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """ADPCM copies of the two golden recordings (mono, blocks of 256 and 1024 bytes, the second with a `fact` chunk), and the
    meerkat clip at 32 kHz — where the fixture model finds segments in it (tests/test_audio_ingest_gpu.py) — as a stereo ADPCM file
    whose second channel is the clip reversed."""
    from scipy.signal import resample_poly
    d = tmp_path_factory.mktemp("adpcm_folder")
    for name, block_bytes, fact in (("meerkat_5s.wav", 256, False), ("zebra_finch_g17y2U-f00007.wav", 1024, True)):
        x, sr = load_wav(os.path.join(GOLDEN, name))
        pcm = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)[:, None]
        (d / ("a_" + name)).write_bytes(IC.wav_bytes(1, sr, block_bytes, IC.encode(pcm, block_bytes), fact=len(pcm) if fact else None))
    x, sr = load_wav(os.path.join(GOLDEN, "meerkat_5s.wav"))
    pcm = np.clip(np.round(resample_poly(x, 2, 1) * 32768), -32768, 32767).astype(np.int16)
    (d / "b_meerkat_32k_stereo.wav").write_bytes(IC.wav_bytes(2, 2 * sr, 2048, IC.encode(np.stack([pcm, pcm[::-1]], axis=1), 2048), fact=len(pcm)))
    return str(d)


def test_segment_files_and_cli_on_adpcm_files(gpu_lib, folder, tmp_path):
    from whisperseg_amd.model import WhisperSegmenter
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        from segment import folder_patterns, table, write_csv
    finally:
        sys.path.pop(0)
    import glob
    paths = [p for pattern in folder_patterns(None) for p in glob.glob(folder + "/" + pattern)]         # the CLI's order
    names = [os.path.basename(p) for p in paths]
    assert len(paths) == 3
    for p in paths:
        with open(p, "rb") as f:
            assert wavio.scan_audio(f).format == wavio.ENC_IMA_ADPCM
    seg = WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")
    want = seg.segment_batch((load_audio(p) for p in paths), spec_time_step=TM.STS)
    print("rows per file:", {n: len(w["onset"]) for n, w in zip(names, want)})
    assert sum(len(w["onset"]) for w in want) >= 1                                                    # not vacuous
    assert seg.segment_files(paths, spec_time_step=TM.STS) == want
    seg.ingest_buffer_bytes = 64 * 1024                                                               # the two longer files in pieces
    assert seg.segment_files(paths, spec_time_step=TM.STS) == want
    text = io.StringIO()
    write_csv(*table(want, names), text)
    out = tmp_path / "adpcm.csv"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "segment.py"), "--model_path", MODEL_DIR, "--audio_folder", folder,
                           "--csv_save_path", str(out), "--spec_time_step", str(TM.STS)], env=dict(os.environ, WHISPERSEG_AMD_DTYPE="f32"))
    assert out.read_text() == text.getvalue()
