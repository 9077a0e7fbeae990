"""All planes of a recording resampled in one launch (wseg_resample_planar_f32) have the bits of the one-signal kernel
(wseg_resample_f32, the definition of the arithmetic) run on each plane on the same device, write nothing but the floats they
address, and agree with the CPU oracle; the callers on top — resample() of [channels, n], load_wav_device(sr=), segment_files(sr=),
the CLI's --sr — give what resampling each decoded file by hand gives."""
import glob
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wav_cases as WC
from conftest import GOLDEN, ROOT
from oracle.resample import resample_poly_ref
from tools import tiny_model as TM
from whisperseg_amd.resample import PLANAR_GRID_CAP, launch_plan, plan, resample
from whisperseg_amd.wavio import load_wav, load_wav_device

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
RATIOS = [(48000, 16000), (44100, 16000), (16000, 44100), (32000, 48000), (300000, 250000), (300000, 16000), (250000, 44100),
          (8000, 16000)]
# ... and two ratios beyond the issue's table, for the branches those never take: a window too long to stage even for the smallest
# tile (x read from global memory), without and with a tap table too long to stage as well
UNSTAGED = [(300000, 4000), (2500000, 44100)]
SENTINEL = -12345.5
LEAD, TAIL = 1, 9                    # guard floats in front of the first plane (a base offset of one float) and behind the last


def signal(planes, n, seed):
    """Seeded normal samples with stretches of +0.0, -0.0 and denormals and single +-3e38 written in (no inf / NaN)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((planes, n)).astype(np.float32)
    for p in range(planes):
        for k, fill in enumerate((np.float32(0.0), np.float32(-0.0), None)):
            if n >= 8:
                lo = int(rng.integers(0, n - n // 8))
                hi = lo + max(1, n // 8 if k < 2 else n // 16)
                x[p, lo:hi] = fill if fill is not None else (rng.integers(1, 1 << 22, hi - lo).astype(np.uint32)
                                                             | (rng.integers(0, 2, hi - lo).astype(np.uint32) << 31)).view(np.float32)
        if n >= 2:
            i, j = rng.choice(n, 2, replace=False)
            x[p, i], x[p, j] = np.float32(3e38), np.float32(-3e38)
    if n == 1 and planes > 1:
        x[1, 0] = np.float32(-0.0)
    return x


_TABLES = {}


def taps(p):
    """The taps on the device, once per ratio: both kernels read the same array."""
    key = (p["up"], p["down"])
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(p["taps"]).cuda()
    return _TABLES[key]


def parent(lib, x, p):
    """The yardstick: wseg_resample_f32 on every plane (contiguous copies) -> int32 bits [planes, n_out]."""
    from whisperseg_amd import _lib
    h = taps(p)
    rows = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    y = torch.full((x.shape[0], p["n_out"]), SENTINEL, dtype=torch.float32, device="cuda")
    for c in range(x.shape[0]):
        _lib.check(lib.wseg_resample_f32(rows[c].data_ptr(), x.shape[1], h.data_ptr(), len(p["taps"]), p["up"], p["down"], p["pre_pad"],
                                         p["pre_remove"], y[c].data_ptr(), p["n_out"], _lib.stream_ptr()))
    return y.view(torch.int32)


def planar(lib, x, p, x_pad=0, y_pad=0):
    """wseg_resample_planar_f32 with x as rows x_pad floats longer than the planes, one float into a larger buffer, and y in a
    buffer of sentinels with rows y_pad floats longer than n_out -> int32 bits [planes, n_out]; every guard float is checked."""
    from whisperseg_amd import _lib
    planes, n_in = x.shape
    n_out = p["n_out"]
    xs, ys = n_in + x_pad, n_out + y_pad
    xbuf = torch.full((LEAD + planes * xs + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
    xrows = xbuf[LEAD:LEAD + planes * xs].view(planes, xs)
    xrows[:, :n_in] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    before = xbuf.clone()
    ybuf = torch.full((LEAD + planes * ys + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
    hp = taps(p)
    _lib.check(lib.wseg_resample_planar_f32(xbuf.data_ptr() + 4 * LEAD, n_in, xs, planes, hp.data_ptr(), len(p["taps"]), p["up"], p["down"],
                                            p["pre_pad"], p["pre_remove"], ybuf.data_ptr() + 4 * LEAD, n_out, ys, _lib.stream_ptr()))
    yrows = ybuf[LEAD:LEAD + planes * ys].view(planes, ys)
    guards = torch.ones_like(ybuf, dtype=torch.bool)
    guards[LEAD:LEAD + planes * ys].view(planes, ys)[:, :n_out] = False
    assert bool((ybuf[guards] == SENTINEL).all()), "a guard float of y was written"
    assert torch.equal(xbuf.view(torch.int32), before.view(torch.int32))
    return yrows[:, :n_out].contiguous().view(torch.int32)


def n_in_for(n_out, up, down):
    """The input length whose output length is n_out (up <= down), or the nearest reachable one above it (up > down: output
    lengths come in steps of up / down)."""
    n_in = (n_out - 1) * down // up + 1                          # the shortest input with at least n_out outputs
    got = -(-n_in * up // down)
    assert n_out <= got < n_out + -(-up // down)
    return n_in


def lengths(sr_in, sr_out):
    tile = launch_plan(3000, sr_in, sr_out)["tile"]
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    sizes = sorted({1, 2, 300} | {n_in_for(t, up, down) for t in (tile - 1, tile, tile + 1, 3 * tile + 17)})
    if (sr_in, sr_out) in UNSTAGED:                              # (56 inputs per output: 3 * tile + 17 outputs would need 44 000)
        sizes = [n for n in sizes if n <= 20000]
    return tile, sizes


# ---- 1. bit equality with the one-signal kernel ---------------------------------------------------------------------------------
def test_the_ratios_take_every_branch():
    staged = {(lp["x_staged"], lp["taps_staged"]) for lp in (launch_plan(3000, a, b) for a, b in RATIOS + UNSTAGED)}
    assert staged == {(1, 1), (1, 0), (0, 1), (0, 0)}


@pytest.mark.parametrize("planes", [1, 2, 5, 64])
@pytest.mark.parametrize("sr_in,sr_out", RATIOS + UNSTAGED)
def test_planes_have_the_bits_of_the_one_signal_kernel(gpu_lib, sr_in, sr_out, planes):
    tile, sizes = lengths(sr_in, sr_out)
    assert tile % 64 == 0 and max(sizes) <= 20000
    for n_in in sizes:
        p = plan(n_in, sr_in, sr_out)
        x = signal(planes, n_in, seed=n_in + planes)
        want = parent(gpu_lib, x, p)
        got = planar(gpu_lib, x, p)
        bad = torch.nonzero(got != want)
        assert got.shape == want.shape == (planes, p["n_out"]) and not len(bad), (n_in, p["n_out"], tile, bad[:8].tolist())


# ---- 2. layout: rows of a larger tensor, odd strides, guards ------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RATIOS + UNSTAGED)
def test_odd_strides_and_offsets_write_only_the_addressed_floats(gpu_lib, sr_in, sr_out):
    for n_in in (1, 300, 2999):
        p = plan(n_in, sr_in, sr_out)
        x = signal(3, n_in, seed=7 + n_in)
        want = parent(gpu_lib, x, p)
        for x_pad, y_pad in ((1, 1), (4, 3), (2, 2)):
            x_pad += (n_in + x_pad + 1) % 2                      # both strides odd
            y_pad += (p["n_out"] + y_pad + 1) % 2
            assert (n_in + x_pad) % 2 == 1 and (p["n_out"] + y_pad) % 2 == 1 and y_pad > 0
            assert torch.equal(planar(gpu_lib, x, p, x_pad, y_pad), want), (n_in, x_pad, y_pad)


# ---- 3. against the CPU oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RATIOS + UNSTAGED)
def test_three_planes_match_the_oracle(gpu_lib, sr_in, sr_out):
    n_in = 1 if (sr_in, sr_out) == (8000, 16000) else 3000
    x = np.random.default_rng(n_in + sr_in).standard_normal((3, n_in)).astype(np.float32)
    got = resample(x, sr_in, sr_out, device="cuda:0").cpu().numpy()
    for row, y in zip(x, got):
        want = resample_poly_ref(row, sr_in, sr_out)
        err = float(np.max(np.abs(y - want)))
        print(f"{sr_in} -> {sr_out}: max error {err:.3g}, max |want| {np.abs(want).max():.3g}")
        assert y.shape == want.shape and err <= 2e-5 * max(1.0, np.abs(want).max())


# ---- 4. more tiles than the grid cap ------------------------------------------------------------------------------------------------
def test_grid_stride_beyond_the_cap(gpu_lib):
    tile = launch_plan(1, 16000, 8000)["tile"]
    n_in = 2 * (PLANAR_GRID_CAP * tile + 3 * tile + 5)
    p = plan(n_in, 16000, 8000)
    assert -(-p["n_out"] // tile) > PLANAR_GRID_CAP + 3
    x = np.random.default_rng(1).standard_normal((1, n_in)).astype(np.float32)
    assert torch.equal(planar(gpu_lib, x, p), parent(gpu_lib, x, p))


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------------
def test_empty_signals_and_rejected_arguments(gpu_lib):
    from whisperseg_amd import _lib
    lib = gpu_lib
    p = plan(300, 48000, 16000)
    hp = taps(p)
    x = torch.from_numpy(signal(2, 300, 3)).cuda()
    y = torch.full((2, 120), SENTINEL, dtype=torch.float32, device="cuda")

    def call(xp, n_in, xs, planes, tp, yp, n_out, ys, n_taps=len(p["taps"]), up=p["up"], down=p["down"]):
        return lib.wseg_resample_planar_f32(xp, n_in, xs, planes, tp, n_taps, up, down, p["pre_pad"], p["pre_remove"], yp, n_out, ys,
                                            _lib.stream_ptr())

    xp, tp, yp = x.data_ptr(), hp.data_ptr(), y.data_ptr()
    for args, word in (((xp, 300, 300, 0, tp, yp, 100, 120), "n_planes"), ((xp, 300, 300, 65, tp, yp, 100, 120), "n_planes"),
                       ((xp, 300, 299, 2, tp, yp, 100, 120), "stride"), ((xp, 300, 300, 2, tp, yp, 100, 99), "stride"),
                       ((None, 300, 300, 2, tp, yp, 100, 120), "pointer"), ((xp, 300, 300, 2, None, yp, 100, 120), "pointer"),
                       ((xp, 300, 300, 2, tp, None, 100, 120), "pointer"), ((xp, -1, 300, 2, tp, yp, 100, 120), "negative"),
                       ((xp, 300, 300, 2, tp, yp, -1, 120), "negative")):
        assert call(*args) == -1, args
        assert word in lib.wseg_last_error().decode(), (args, lib.wseg_last_error())
    assert call(xp, 300, 300, 2, tp, yp, 100, 120, up=0) == -1 and call(xp, 300, 300, 2, tp, yp, 100, 120, n_taps=0) == -1
    assert call(xp, 300, 300, 2, tp, yp, 0, 120) == 0                              # no output: nothing launched
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    assert call(xp, 0, 300, 2, tp, yp + 4, 100, 120) == 0                          # no input: zeros, and only where a plane is
    torch.cuda.synchronize()
    host = y.cpu().numpy()
    assert (host[:, 1:101] == 0).all() and (host[:, 0] == SENTINEL).all() and (host[0, 101:] == SENTINEL).all() and (host[1, 101:] == SENTINEL).all()
    y.fill_(SENTINEL)
    assert call(xp, 0, 0, 1, tp, yp + 4, 7, 0) == 0                                # one plane: the strides are ignored
    torch.cuda.synchronize()
    host = y.cpu().numpy().reshape(-1)
    assert (host[1:8] == 0).all() and host[0] == SENTINEL and (host[8:] == SENTINEL).all()
    assert resample(np.zeros((3, 0), np.float32), 48000, 16000, device="cuda:0").shape == (3, 0)


# ---- 6. resample() ------------------------------------------------------------------------------------------------------------------
def test_resample_dispatches_on_the_rank(gpu_lib, monkeypatch):
    calls = []
    for name in ("wseg_resample_f32", "wseg_resample_planar_f32"):
        fn = getattr(gpu_lib, name)
        monkeypatch.setattr(gpu_lib, name, lambda *a, _fn=fn, _name=name: (calls.append(_name), _fn(*a))[1])
    n = 2999
    x = signal(3, n, 11)
    rows = [resample(r, 44100, 16000, device="cuda:0") for r in x]
    assert calls == ["wseg_resample_f32"] * 3 and all(r.shape == (1089,) for r in rows)
    want = torch.stack(rows).view(torch.int32)
    wide = np.full((3, n + 5), SENTINEL, np.float32)
    wide[:, 2:2 + n] = x
    on_device = torch.from_numpy(wide).cuda()
    for audio in (x, wide[:, 2:2 + n], on_device[:, 2:2 + n], np.ascontiguousarray(x.T).T, torch.from_numpy(x).cuda()):
        del calls[:]
        got = resample(audio, 44100, 16000, device="cuda:0")
        assert calls == ["wseg_resample_planar_f32"], calls                        # ONE launch for all rows
        assert got.shape == (3, 1089) and got.is_contiguous() and torch.equal(got.view(torch.int32), want)
    # views numpy gives negative strides are copied, as the 1-D path always copied them
    del calls[:]
    flipped = resample(x[::-1, ::-1], 44100, 16000, device="cuda:0")
    assert calls == ["wseg_resample_planar_f32"]
    for c in range(3):
        del calls[:]
        row = resample(x[2 - c, ::-1], 44100, 16000, device="cuda:0")
        assert calls == ["wseg_resample_f32"] and torch.equal(row.view(torch.int32), flipped[c].view(torch.int32))
    assert not torch.equal(flipped.view(torch.int32), want)
    del calls[:]
    one = resample(x[:1], 44100, 16000, device="cuda:0")
    assert one.shape == (1, 1089) and torch.equal(one.view(torch.int32), want[:1]) and calls == ["wseg_resample_planar_f32"]
    del calls[:]
    same = resample(on_device[:, 2:2 + n], 16000, 16000, device="cuda:0")         # equal rates: a clone, of either shape
    assert same.shape == (3, n) and same.data_ptr() != on_device.data_ptr() and np.array_equal(same.cpu().numpy().view(np.uint32), x.view(np.uint32))
    assert resample(x[0], 16000, 16000, device="cuda:0").shape == (n,) and not calls
    with pytest.raises(ValueError):
        resample(np.zeros((65, 10), np.float32), 48000, 16000, device="cuda:0")
    with pytest.raises(ValueError):
        resample(np.zeros((2, 2, 10), np.float32), 48000, 16000, device="cuda:0")


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """meerkat_5s.wav as is (16 kHz, one channel); s16 stereo at 32 kHz: the signal, and the signal reversed in time; s24 x 3
    channels at 48 kHz: the signal, silence, the mean of the signal and its reverse (which at 16 kHz gives rows with the fixture
    model where the signal alone gives none: test_ingest_planar_gpu.py)."""
    from scipy.signal import resample_poly
    d = tmp_path_factory.mktemp("rates")
    src = os.path.join(GOLDEN, "meerkat_5s.wav")
    x, sr = load_wav(src)
    assert sr == TM.SR == 16000
    with open(src, "rb") as f:
        (d / "a_meerkat.wav").write_bytes(f.read())
    q = lambda v, full: np.clip(np.round(v * full), -full, full - 1).astype(np.int64)
    x2, x3 = resample_poly(x, 2, 1), resample_poly(x, 3, 1)
    stereo = np.stack([q(x2, 32768), q(x2[::-1], 32768)], axis=1).reshape(-1)
    (d / "b_s16_stereo_32k.wav").write_bytes(WC.wav_bytes("s16", 2, 2 * sr, WC.sample_bytes("s16", stereo)))
    three = np.stack([q(x3, 1 << 23), np.zeros(len(x3), np.int64), q(0.5 * (x3 + x3[::-1]), 1 << 23)], axis=1).reshape(-1)
    (d / "c_s24_three_48k.WAV").write_bytes(WC.wav_bytes("s24", 3, 3 * sr, WC.sample_bytes("s24", three)))
    return str(d)


def test_load_wav_device_resamples_what_it_decoded(gpu_lib, folder):
    for path in sorted(glob.glob(folder + "/*")):
        for kw in ({}, {"mono": False}, {"channel_id": -1}, {"mono": False, "chunk_frames": 4096}):
            native, sr = load_wav_device(path, **kw)
            got, got_sr = load_wav_device(path, sr=16000, **kw)
            assert got_sr == 16000 and got.ndim == native.ndim
            want = native if sr == 16000 else torch.stack([resample(r, sr, 16000) for r in native]) if native.ndim == 2 else resample(native, sr, 16000)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (path, kw)
            same, same_sr = load_wav_device(path, sr=sr, **kw)
            assert same_sr == sr and torch.equal(same.view(torch.int32), native.view(torch.int32))
    empty, sr = load_wav_device(io.BytesIO(WC.make_wav("s16", 3, 0, sr=48000)), mono=False, sr=16000)
    assert empty.shape == (3, 0) and sr == 16000
    for bad in (0, -1, "16k", 16000.0):
        with pytest.raises(ValueError):
            load_wav_device(sorted(glob.glob(folder + "/*"))[0], sr=bad)


def test_segment_files_and_cli_at_a_target_rate_equal_resampling_by_hand(gpu_lib, folder, tmp_path):
    from whisperseg_amd.model import WhisperSegmenter
    seg = WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")
    kw = dict(spec_time_step=TM.STS)
    paths = glob.glob(folder + "/*.wav") + glob.glob(folder + "/*.WAV")          # the CLI's order
    assert len(paths) == 3
    mixes = [load_wav_device(p) for p in paths]
    assert sorted(sr for _, sr in mixes) == [16000, 32000, 48000]
    by_hand = seg.segment_batch([resample(a, sr, 16000) for a, sr in mixes], 16000, **kw)
    planes = [load_wav_device(p, mono=False) for p in paths]
    assert sorted(a.shape[0] if a.ndim == 2 else 1 for a, _ in planes) == [1, 2, 3]
    per_channel = [seg.segment_channels(resample(a, sr, 16000), 16000, **kw) for a, sr in planes]
    assert any(r["onset"] for r in by_hand) and any(r["onset"] for g in per_channel for r in g)      # not vacuous: rows on both sides
    assert by_hand != seg.segment_batch(iter(mixes), **kw)                        # ... and the rate matters
    for buffer_bytes in (seg.ingest_buffer_bytes, 64 * 1024):                     # whole files; every file in pieces
        seg.ingest_buffer_bytes = buffer_bytes
        assert seg.segment_files(paths, sr=16000, **kw) == by_hand
        assert seg.segment_files(paths, sr=16000, channel_id="all", **kw) == per_channel
        assert seg.segment_files(paths, sr=[16000] * 3, channel_id=0, **kw) == [g[0] for g in per_channel]
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        from segment import table, write_csv
    finally:
        sys.path.pop(0)
    text = io.StringIO()
    columns, rows = table(per_channel, [os.path.basename(p) for p in paths], all_channels=True)
    assert rows
    write_csv(columns, rows, text)
    out = tmp_path / "rates.csv"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "segment.py"), "--model_path", MODEL_DIR, "--audio_folder", folder,
                           "--csv_save_path", str(out), "--spec_time_step", str(TM.STS), "--channel_id", "all", "--sr", "16000"],
                          env=dict(os.environ, WHISPERSEG_AMD_DTYPE="f32"))
    assert out.read_text() == text.getvalue()
