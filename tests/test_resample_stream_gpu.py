"""A recording resampled piece by piece on the device: wseg_resample_planar_range_f32 on the minimal segment of every range gives
the bits of the whole-recording call and writes nothing else; load_wav_device(sr=) and FilePipeline(sr=) — now streamed, without a
native-rate tensor and without DeviceIngest.resample — give what resample() of the decoded file gives, bit for bit, down to
16-frame pieces with a filter history longer than a piece; segment_files on top of it equals resampling by hand."""
import glob
import io
import os

import numpy as np
import pytest
import torch

import wav_cases as WC
from conftest import GOLDEN
from test_resample_planar_gpu import LEAD, RATIOS, SENTINEL, TAIL, UNSTAGED, folder, lengths, planar, signal, taps  # noqa: F401
from tools import tiny_model as TM
from whisperseg_amd import wavio
from whisperseg_amd.resample import plan, resample, stream_plan
from whisperseg_amd.wavio import load_wav_device

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")


# ---- 1. a range from its minimal segment ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("sr_in,sr_out", RATIOS + UNSTAGED)
def test_ranges_from_minimal_segments_have_the_bits_of_the_whole_call(gpu_lib, sr_in, sr_out, planes):
    from whisperseg_amd import _lib
    tile, sizes = lengths(sr_in, sr_out)
    for n_in in [max(sizes)] + ([1] if (sr_in, sr_out) == (8000, 16000) else []):
        p = plan(n_in, sr_in, sr_out)
        n_out, n_taps, up = p["n_out"], len(p["taps"]), p["up"]
        x = signal(planes, n_in, seed=n_in + planes)
        want = planar(gpu_lib, x, p)                                             # the whole call
        m = np.arange(n_out, dtype=np.int64)
        c = (m + p["pre_remove"]) * p["down"] - p["pre_pad"]
        k_lo, k_hi = np.maximum(0, -(-(c - n_taps + 1) // up)), np.minimum(c // up, n_in - 1)
        ys = n_out + 2 + n_out % 2                                               # an odd stride, longer than the planes
        ybuf = torch.full((LEAD + planes * ys + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
        written = torch.zeros_like(ybuf, dtype=torch.bool)
        rows = lambda t: t[LEAD:LEAD + planes * ys].view(planes, ys)
        hp = taps(p)
        cuts = sorted({0, n_out} | {b for b in (1, tile - 1, tile + 1) if b < n_out})
        assert n_in == 1 or len(cuts) >= 4
        for i, (m0, m1) in enumerate(zip(cuts, cuts[1:])):
            k0, k1 = int(k_lo[m0]), int(k_hi[m1 - 1])
            frames = max(k1 - k0 + 1, 0)
            lead = 1 + 2 * (i % 2)                                               # an odd float offset into a fresh buffer
            xs = frames + 3
            xbuf = torch.full((lead + planes * xs + TAIL,), float("nan"), dtype=torch.float32, device="cuda")
            xbuf[lead:lead + planes * xs].view(planes, xs)[:, :frames] = torch.from_numpy(np.ascontiguousarray(x[:, k0:k0 + frames])).cuda()
            before = ybuf.clone()
            _lib.check(gpu_lib.wseg_resample_planar_range_f32(
                xbuf.data_ptr() + 4 * lead, k0, frames, xs, planes, n_in, hp.data_ptr(), n_taps, up, p["down"], p["pre_pad"], p["pre_remove"],
                ybuf.data_ptr() + 4 * LEAD, m0, m1 - m0, ys, _lib.stream_ptr()))
            here = torch.zeros_like(written)
            rows(here)[:, m0:m1] = True
            assert torch.equal(ybuf[~here].view(torch.int32), before[~here].view(torch.int32)), (n_in, m0, m1)      # nothing else written
            written |= here
        assert bool((ybuf[~written] == SENTINEL).all()) and int(written.sum()) == planes * n_out
        got = rows(ybuf)[:, :n_out].contiguous()
        assert not bool(torch.isnan(got).any())
        bad = torch.nonzero(got.view(torch.int32) != want)
        assert not len(bad), (n_in, n_out, tile, cuts, bad[:8].tolist())
        # no output: nothing launched, nothing written
        before = ybuf.clone()
        _lib.check(gpu_lib.wseg_resample_planar_range_f32(xbuf.data_ptr() + 4 * lead, k0, frames, xs, planes, n_in, hp.data_ptr(), n_taps, up,
                                                          p["down"], p["pre_pad"], p["pre_remove"], ybuf.data_ptr() + 4 * LEAD, m1, 0, ys,
                                                          _lib.stream_ptr()))
        assert torch.equal(ybuf.view(torch.int32), before.view(torch.int32))


# ---- 2. load_wav_device(sr=) in pieces ----------------------------------------------------------------------------------------------
def finite_wav(fmt, channels, n_frames, sr, seed):
    rng = np.random.default_rng(seed)
    return WC.wav_bytes(fmt, channels, sr, WC.sample_bytes(fmt, WC.random_samples(fmt, n_frames * channels, rng, special=fmt != "f64")))


MONO_3000 = finite_wav("s16", 1, 3000, 16000, seed=5)


def declared_at(blob, sr):
    """The same file with another rate in its header."""
    return WC.wav_bytes("s16", 1, sr, wavio.read_wav_raw(io.BytesIO(blob)).data.tobytes())


FILES = {
    "s16 stereo 32k": (finite_wav("s16", 2, 5003, 32000, seed=1), 16000, ({}, {"mono": False}, {"channel_id": -1})),
    "s24 x3 48k": (finite_wav("s24", 3, 4099, 48000, seed=2), 16000, ({}, {"mono": False}, {"channel_id": -1})),
    "f64 x5 44.1k": (finite_wav("f64", 5, 3001, 44100, seed=3), 16000, ({}, {"mono": False}, {"channel_id": -1})),
    # a filter history of 187 resp. 1 133 frames: longer than a 16-frame piece, most of which emit nothing
    "s16 mono 300k": (declared_at(MONO_3000, 300000), 16000, ({},)),
    "s16 mono 2.5M": (declared_at(MONO_3000, 2500000), 44100, ({},)),
}


@pytest.mark.parametrize("name", list(FILES))
def test_load_wav_device_in_pieces_equals_resampling_the_decoded_file(gpu_lib, name):
    blob, target, kws = FILES[name]
    for kw in kws:
        native, sr = load_wav_device(io.BytesIO(blob), **kw)
        assert sr != target
        want = resample(native, sr, target)
        for chunk_frames in (16, 4096, None):
            got, got_sr = load_wav_device(io.BytesIO(blob), sr=target, chunk_frames=chunk_frames, **kw)
            assert got_sr == target and got.shape == want.shape and got.is_contiguous()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, kw, chunk_frames)
    if "mono" in name:
        steps = list(stream_plan(3000, sr, target, 16))
        assert any(s["frame0"] + s["n"] - s["keep_from"] > 16 for s in steps) and sum(s["m_count"] == 0 for s in steps) > 10


# ---- 3. no native-rate copy, no DeviceIngest.resample ---------------------------------------------------------------------------------
def test_a_streamed_file_never_exists_at_its_native_rate(gpu_lib, folder, monkeypatch):  # noqa: F811
    n = 1 << 20
    rng = np.random.default_rng(9)
    blob = WC.wav_bytes("s16", 4, 48000, rng.integers(-32768, 32768, 4 * n, dtype=np.int64).astype("<i2").tobytes())
    kw = dict(mono=False, sr=16000, chunk_frames=16384)
    load_wav_device(io.BytesIO(blob[:44 + 8 * 4096]), **kw)                      # warm: the taps and the library are on the device
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got, sr = load_wav_device(io.BytesIO(blob), **kw)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("peak rise %.2f MiB (output %.2f MiB, native planes 16 MiB)" % (rise / 2 ** 20, got.numel() * 4 / 2 ** 20))
    assert sr == 16000 and got.shape == (4, 349526)
    assert rise < 4 * n * 4                                                       # below the native-rate planes alone
    native, _ = load_wav_device(io.BytesIO(blob), mono=False)
    assert torch.equal(got.view(torch.int32), resample(native, 48000, 16000).view(torch.int32))
    del native

    def never(self, *a, **k):
        raise AssertionError("DeviceIngest.resample on the streamed path")

    paths = sorted(glob.glob(folder + "/*"))
    assert len(paths) == 3
    loads = {"all": dict(mono=False), None: {}, 0: dict(channel_id=0)}
    want = {k: [resample(a, sr, 16000) for a, sr in (load_wav_device(p, **kw_load) for p in paths)] for k, kw_load in loads.items()}
    monkeypatch.setattr(wavio.DeviceIngest, "resample", never)
    again, _ = load_wav_device(io.BytesIO(blob), **kw)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    for channel_id in loads:
        items = list(wavio.FilePipeline(paths, wavio.device_ingest(), buffer_bytes=64 * 1024, sr=16000, channel_id=channel_id))
        assert [sr for _, sr in items] == [16000] * 3
        for (a, _), w in zip(items, want[channel_id]):
            assert a.shape == w.shape and torch.equal(a.view(torch.int32), w.view(torch.int32)), channel_id


# ---- 4. segment_files ---------------------------------------------------------------------------------------------------------------
def test_segment_files_streamed_equals_resampling_by_hand(gpu_lib, folder):  # noqa: F811
    from whisperseg_amd.model import WhisperSegmenter
    seg = WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")
    kw = dict(spec_time_step=TM.STS)
    paths = glob.glob(folder + "/*.wav") + glob.glob(folder + "/*.WAV")
    assert len(paths) == 3
    planes = [load_wav_device(p, mono=False) for p in paths]
    per_channel = [seg.segment_channels(resample(a, sr, 16000), 16000, **kw) for a, sr in planes]
    assert any(r["onset"] for g in per_channel for r in g)                       # not vacuous
    seg.ingest_buffer_bytes = 16 * 1024                                           # every file in pieces
    assert seg.segment_files(paths, sr=16000, channel_id="all", **kw) == per_channel
