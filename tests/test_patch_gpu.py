"""Per-segment log-mel patches on the GPU (wseg_patches_f32, whisperseg_amd/csrc/wseg_patch.hip) against the host definition
whisperseg_amd.patches.patches_host, from the kernel pair up to segment(patches=W) and the CLI's --patches.

What may differ from the definition, and by how much, is worked out in tests/patch_cases.py (above SPREAD): every value by four
times the measured cost of the fp32 transform and the float32 bank plus 2 ulp of the expected float32, no entry left out.  The
shapes are the smallest at which the kernel can go wrong: one second per rate, a few dozen segments, every width that changes how
frames fall into work items."""
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

import golden_inputs as GI
import measure_cases as MC
import patch_cases as PC
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import measure as M
from whisperseg_amd import patches as P
from whisperseg_amd.audio_utils import get_n_fft_given_sr

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
FIXTURE_WAVS = [os.path.join(GOLDEN, "meerkat_5s.wav"), os.path.join(GOLDEN, "zebra_finch_g17y2U-f00007.wav")]
GUARD = 64                            # NaN samples in front of and behind the recording
PATCH_GUARD = 0x7fc12345              # the bits of the guard patches: a NaN no kernel writes


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def guarded(x):
    """-> (whole tensor, the recording inside it): NaN guards in front and behind."""
    whole = torch.full((len(x) + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    whole[GUARD:GUARD + len(x)] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return whole, whole[GUARD:GUARD + len(x)]


def device_patches(x, bounds, sr, width, low=0, high=None):
    """The launch pair on a guarded recording into patches held between guard patches -> float32 [n_seg, 80, width]; every value
    must be finite and the guards must survive."""
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    _, pcm = guarded(x)
    held = torch.from_numpy(np.full((len(bounds) + 2, 80, width), PATCH_GUARD, np.uint32).view(np.float32)).cuda()
    P.patch_rows(pcm, bounds, P.device_tables(sr, low, high, pcm.device), width, out=held[1:len(bounds) + 1])
    host = held.cpu().numpy()
    assert (bits(host[0]) == PATCH_GUARD).all() and (bits(host[-1]) == PATCH_GUARD).all()
    assert np.isfinite(host[1:-1]).all()
    return host[1:-1]


def check(got, x, bounds, sr, width, low=0, high=None, spread=None, what=""):
    """Every entry of `got` against the definition on (x, bounds) -> the largest error / tolerance ratio."""
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    want = P.patches_host(x, sr, MC.prediction(bounds, sr, len(x)), width=width, min_frequency=low, max_frequency=high)
    assert got.dtype == np.float32 and got.shape == want.shape == (len(bounds), 80, width), (what, got.shape, want.shape)
    if not len(bounds):
        return 0.0
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / PC.tolerance(want, sr, spread)
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{what} sr={sr} W={width}: {len(bounds)} patches, largest error {err.max():.3g}, {ratio.max():.3f} of its tolerance (patch, filter, column {worst})")
    assert (ratio <= 1).all(), (what, sr, width, worst, float(got[worst]), float(want[worst]), float(ratio.max()))
    return float(ratio.max())


@functools.lru_cache(maxsize=None)
def case(sr, width):
    """recording(sr), rows_for(sr, width) and the device's patches for them: computed once, shared, never modified."""
    x, bounds = MC.recording(sr), PC.rows_for(sr, width)
    return x, bounds, device_patches(x, bounds, sr, width)


@pytest.mark.parametrize("sr", PC.RATES)
def test_kernel_against_the_definition(gpu_lib, sr):
    """All five n_fft (16, 8, 4, 2 and 1 frames a work item); widths that divide an item, exceed it and straddle it; L = 0, 1,
    W - 1, W, W + 1 and odd lengths; segments at sample 0 and up to sample n, empty ones at 0 and at n, overlapping and silent ones;
    a recording shorter than a frame; guards around samples and patches."""
    worst = 0.0
    for width in PC.widths(sr):
        x, bounds, got = case(sr, width)
        worst = max(worst, check(got, x, bounds, sr, width, what="paths"))
    short = PC.short_recording(sr)
    assert len(short) == PC.SHORT_N < get_n_fft_given_sr(sr)
    for width in (1, 5, 32):
        worst = max(worst, check(device_patches(short, PC.short_rows(), sr, width), short, PC.short_rows(), sr, width, what="n=100"))
    print(f"n_fft {get_n_fft_given_sr(sr)}: largest error / tolerance {worst:.3f}")
    # silence is -1.5 everywhere, on the device too
    quiet = device_patches(MC.silence(3000), [(0, 3000), (5, 5), (2999, 3000)], sr, 3)
    assert (quiet == -1.5).all()
    # the public call, from numpy and from the resident tensor, gives those bits
    width = 5
    x, bounds, got = case(sr, width)
    pred = MC.prediction(bounds, sr, len(x))
    for audio in (x, guarded(x)[1]):
        assert np.array_equal(bits(P.patches(audio, sr, pred, width=width)), bits(got))


def test_bands_and_empty_filters(gpu_lib):
    """min_frequency = 2000 and 0 at 16 kHz against the definition; and the band 0 .. 1000 Hz, whose filters are narrower than a bin:
    many hold no bin (count 0 in the device tables) and sit at the patch's floor."""
    sr, width = PC.BAND_RATE, PC.BAND_WIDTH
    x, bounds = MC.recording(sr), PC.rows_for(sr, PC.BAND_WIDTH)
    check(device_patches(x, bounds, sr, width, low=PC.BAND_MIN_FREQUENCY), x, bounds, sr, width, low=PC.BAND_MIN_FREQUENCY, what="from 2000 Hz")
    check(case(sr, width)[2], x, bounds, sr, width, what="from 0 Hz")
    (nx, nrows, nwidth, low, high), = PC.narrow_cases()
    got = device_patches(nx, nrows, sr, nwidth, low=low, high=high)
    check(got, nx, nrows, sr, nwidth, low=low, high=high, spread=PC.NARROW_SPREAD, what="0 .. 1000 Hz")
    empty = np.flatnonzero(P.filterbank(sr, get_n_fft_given_sr(sr), low, high).sum(axis=0) == 0)
    assert len(empty) >= 10 and (P.device_tables(sr, low, high).mel_count.cpu().numpy()[empty] == 0).all()
    assert (got[:, empty, :] == got[:, empty[:1], :1]).all()                    # one floor per patch


def test_same_bits_on_every_run_and_for_every_grid(gpu_lib, monkeypatch):
    wide = case(400000, 64)                         # 43 segments x 64 columns, one frame an item: a grid of 3 strides 900 times
    small = case(16000, 5)                          # 16 frames an item: items straddle segments
    many = MC.random_segments(16000, 16000, 257)
    x16 = MC.recording(16000)
    first_many = device_patches(x16, many, 16000, 32)
    for (x, bounds, first), sr, width in ((wide, 400000, 64), (small, 16000, 5)):
        assert np.array_equal(bits(device_patches(x, bounds, sr, width)), bits(first))
    for cap in ("3", "1"):
        monkeypatch.setenv("WSEG_PATCH_GRID", cap)
        assert np.array_equal(bits(device_patches(wide[0], wide[1], 400000, 64)), bits(wide[2])), cap
        assert np.array_equal(bits(device_patches(small[0], small[1], 16000, 5)), bits(small[2])), cap
        assert np.array_equal(bits(device_patches(x16, many, 16000, 32)), bits(first_many)), cap


def test_a_segment_does_not_depend_on_its_company(gpu_lib, monkeypatch):
    """n_seg = 0 / 1 / 257 / 1 000; one segment alone, among 257 and among 1 000 has the same bits, at a width that puts several
    segments into one work item (5) and at one that gives a segment two items (32); blocks of rows give the bits of one call."""
    sr = 16000
    x = MC.recording(sr)
    thousand = MC.random_segments(sr, len(x), 1000)
    some = MC.random_segments(sr, len(x), 257).copy()
    some[100] = thousand[500]
    for width in (5, 32):
        assert device_patches(x, np.zeros((0, 2), np.int64), sr, width).shape == (0, 80, width)
        assert P.patches(x, sr, {"onset": [], "offset": []}, width=width).shape == (0, 80, width)
        alone = device_patches(x, thousand[500:501], sr, width)
        among_some = device_patches(x, some, sr, width)
        among_all = device_patches(x, thousand, sr, width)
        assert alone.shape == (1, 80, width) and among_some.shape == (257, 80, width) and among_all.shape == (1000, 80, width)
        assert np.array_equal(bits(alone[0]), bits(among_some[100])) and np.array_equal(bits(alone[0]), bits(among_all[500]))
        # three blocks of rows: the public call cuts them, every row keeps its bits
        pred = MC.prediction(thousand, sr, len(x))
        whole = P.patches(x, sr, pred, width=width)
        assert np.array_equal(bits(whole), bits(among_all))
        monkeypatch.setattr(P, "PATCH_BLOCK_BYTES", 80 * width * 4 * 334)
        assert np.array_equal(bits(P.patches(x, sr, pred, width=width)), bits(whole))
        monkeypatch.undo()


def test_invalid_calls_are_refused_before_a_launch(gpu_lib):
    from whisperseg_amd import _lib
    sr = 16000
    x = MC.recording(sr)
    pred = MC.prediction([(10, 900)], sr, len(x))
    with pytest.raises(ValueError, match="k_lo"):
        P.patches(x, sr, pred, min_frequency=7000, max_frequency=6000)
    with pytest.raises(ValueError, match="width"):
        P.patches(x, sr, pred, width=257)
    pcm = guarded(x)[1]
    tables = P.device_tables(sr, 0, None, pcm.device)
    with pytest.raises(_lib.WsegError, match="bounds"):
        P.patch_rows(pcm, [(10, len(x) + 1)], tables, 8)
    with pytest.raises(ValueError, match="width"):
        P.patch_rows(pcm, [(10, 900)], tables, 0)
    with pytest.raises(_lib.WsegError, match="out"):
        P.patch_rows(pcm, [(10, 900)], tables, 8, out=torch.empty((1, 80, 9), device="cuda"))
    with pytest.raises(_lib.WsegError):
        P.patch_rows(torch.from_numpy(x), [(10, 900)], tables, 8)               # no CPU path


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seg():
    from whisperseg_amd.model import WhisperSegmenter
    return WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")


def s16(v):
    return np.clip(np.round(np.asarray(v, np.float64) * 32768), -32768, 32767).astype(np.int64)


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    """A recording of the fixture model's own signal family as an s16 file (the model finds rows in it, whatever it makes of the
    two field recordings), then the two fixture recordings."""
    tiny = tmp_path_factory.mktemp("patch") / "tiny.wav"
    tiny.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", s16(GI.tiny_recording(3, 2)))))
    return [str(tiny)] + FIXTURE_WAVS


ROW_KEYS = ("onset", "offset", "cluster")
KW = dict(spec_time_step=TM.STS)
WIDTH = 32


def rows_of(pred):
    return {k: pred[k] for k in ROW_KEYS}


def same_predictions(a, b):
    """Two lists of patches=W prediction dicts: the same keys, rows and picture bits."""
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert list(p) == list(q) and {k: v for k, v in p.items() if k != "patch"} == {k: v for k, v in q.items() if k != "patch"}
        assert p["patch"].shape == q["patch"].shape and np.array_equal(bits(p["patch"]), bits(q["patch"]))


def check_prediction(seg, pred, plain, audio, sr, what, min_frequency=None):
    """A patches=WIDTH prediction: the plain call's rows plus "patch", which is patches() on the same PCM bit for bit and the
    definition on its samples within tolerance."""
    low = seg.resolve_segmentation_params(min_frequency, TM.STS, None, None, None)[0]
    assert list(pred)[:3] == list(ROW_KEYS) and list(pred)[-1] == "patch" and rows_of(pred) == plain, what
    patch = pred["patch"]
    assert isinstance(patch, np.ndarray) and patch.dtype == np.float32 and patch.shape == (len(plain["onset"]), 80, WIDTH), what
    assert np.array_equal(bits(patch), bits(P.patches(audio, sr, plain, width=WIDTH, min_frequency=low))), what
    host = audio.cpu().numpy() if torch.is_tensor(audio) else audio
    check(patch, host, M.bounds_of(plain, sr, len(host)), sr, WIDTH, low=low, what=what)


def test_segment_with_patches(gpu_lib, seg, wavs):
    from whisperseg_amd.wavio import load_wav
    total = 0
    for path in wavs:
        x, sr = load_wav(path)
        plain = seg.segment(x, sr, **KW)
        assert set(plain) == set(ROW_KEYS)
        pred = seg.segment(x, sr, patches=WIDTH, **KW)
        assert list(pred) == list(ROW_KEYS) + ["patch"]
        check_prediction(seg, pred, plain, x, sr, os.path.basename(path))
        total += len(plain["onset"])
        # with the measurements as well: both sets of keys, the columns of the measure=True-only call, the same pictures
        both, measured = seg.segment(x, sr, measure=True, patches=WIDTH, **KW), seg.segment(x, sr, measure=True, **KW)
        assert list(both) == list(ROW_KEYS) + list(M.COLUMNS) + ["patch"]
        assert all(np.array_equal(bits(both[c]), bits(measured[c])) for c in M.COLUMNS) and rows_of(measured) == plain
        assert rows_of(both) == plain and np.array_equal(bits(both["patch"]), bits(pred["patch"]))
        if path == wavs[0]:
            assert len(plain["onset"]) >= 3          # not vacuous: the fixture model finds rows in its own signal family
            high = seg.segment(x, sr, patches=WIDTH, min_frequency=2000, **KW)      # the band starts at the call's min_frequency
            check_prediction(seg, high, seg.segment(x, sr, min_frequency=2000, **KW), x, sr, "min_frequency=2000", min_frequency=2000)
    assert total >= 3


def test_segment_files_and_batch_with_patches(gpu_lib, seg, wavs, tmp_path):
    from whisperseg_amd.wavio import load_wav, load_wav_device
    per_file = [seg.segment(*load_wav(p), patches=WIDTH, **KW) for p in wavs]
    same_predictions(seg.segment_files(wavs, patches=WIDTH, **KW), per_file)
    same_predictions(seg.segment_batch([load_wav(p) for p in wavs], patches=WIDTH, **KW), per_file)
    assert [rows_of(p) for p in per_file] == seg.segment_files(wavs, **KW)
    # at a second rate the pictures are taken at the TARGET rate, on the resampled samples
    rate = 24000
    at_rate = seg.segment_files(wavs, sr=rate, patches=WIDTH, **KW)
    for path, pred in zip(wavs, at_rate):
        audio, sr = load_wav_device(path, sr=rate)
        assert sr == rate
        check_prediction(seg, pred, seg.segment(audio, rate, **KW), audio, rate, f"sr={rate} " + os.path.basename(path))
    # every channel of a two-channel file, each on its own plane
    x, sr = load_wav(wavs[0])
    two = tmp_path / "two.wav"
    two.write_bytes(WC.wav_bytes("s16", 2, sr, WC.sample_bytes("s16", np.stack([s16(x), s16(0.5 * x[::-1])], axis=1).reshape(-1))))
    planes, _ = load_wav(str(two), mono=False)
    got = seg.segment_files([str(two)], channel_id="all", patches=WIDTH, **KW)
    assert len(got) == 1 and len(got[0]) == 2
    same_predictions(got[0], seg.segment_channels(planes, sr, patches=WIDTH, **KW))
    for c, pred in enumerate(got[0]):
        check_prediction(seg, pred, seg.segment(planes[c], sr, **KW), planes[c], sr, f"channel {c}")
    assert got[0][0]["onset"] and rows_of(got[0][0]) != rows_of(got[0][1])
    at_rate = seg.segment_files([str(two)], channel_id="all", sr=rate, patches=WIDTH, **KW)
    planes_at_rate, sr = load_wav_device(str(two), mono=False, sr=rate)
    for c, pred in enumerate(at_rate[0]):
        check_prediction(seg, pred, seg.segment(planes_at_rate[c], rate, **KW), planes_at_rate[c].contiguous(), rate, f"sr={rate} channel {c}")


def test_cli_patches(gpu_lib, seg, wavs, tmp_path, monkeypatch):
    from whisperseg_amd.wavio import load_wav
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    monkeypatch.setenv("WHISPERSEG_AMD_DTYPE", "f32")
    path = wavs[0]
    x, sr = load_wav(path)
    base = ["--model_path", MODEL_DIR, "--audio_path", path, "--spec_time_step", str(TM.STS)]
    plain_csv, full_csv, npz = tmp_path / "plain.csv", tmp_path / "full.csv", tmp_path / "patches.npz"
    segment.main(base + ["--csv_save_path", str(plain_csv)])
    segment.main(base + ["--csv_save_path", str(full_csv), "--patches", "8", "--patches_save_path", str(npz)])
    assert full_csv.read_bytes() == plain_csv.read_bytes()
    want = seg.segment(x, sr, patches=8, **KW)
    text = io.StringIO()
    segment.write_csv(*segment.table([want]), text)
    assert plain_csv.read_text() == text.getvalue() and want["onset"]
    with np.load(npz) as arch:
        assert set(arch.files) == {"patch", "onset", "offset", "cluster"}
        assert arch["patch"].dtype == np.float32 and np.array_equal(bits(arch["patch"]), bits(want["patch"]))
        assert arch["onset"].tolist() == want["onset"] and arch["offset"].tolist() == want["offset"]
        assert arch["cluster"].tolist() == [str(c) for c in want["cluster"]]
    # folder mode with every channel: the archive carries the CSV's filename and channel columns, row for row
    folder = tmp_path / "wavs"
    folder.mkdir()
    (folder / "two.wav").write_bytes(WC.wav_bytes("s16", 2, sr, WC.sample_bytes("s16", np.stack([s16(x), s16(0.5 * x[::-1])], axis=1).reshape(-1))))
    (folder / "one.wav").write_bytes(open(path, "rb").read())
    args = ["--model_path", MODEL_DIR, "--audio_folder", str(folder), "--spec_time_step", str(TM.STS), "--channel_id", "all"]
    a_csv, b_csv, b_npz = tmp_path / "a.csv", tmp_path / "b.csv", tmp_path / "b.npz"
    segment.main(args + ["--csv_save_path", str(a_csv)])
    segment.main(args + ["--csv_save_path", str(b_csv), "--patches", "8", "--patches_save_path", str(b_npz)])
    assert a_csv.read_bytes() == b_csv.read_bytes()
    lines = [ln.split(",") for ln in b_csv.read_text().splitlines()]
    assert lines[0] == ["filename", "channel", "onset", "offset", "cluster"] and len(lines) > 3
    with np.load(b_npz) as arch:
        assert arch["patch"].shape == (len(lines) - 1, 80, 8) and np.isfinite(arch["patch"]).all()
        for i, (name, channel, onset, offset, cluster) in enumerate(lines[1:]):
            assert (arch["filename"][i], int(arch["channel"][i]), repr(float(arch["onset"][i])), repr(float(arch["offset"][i])), arch["cluster"][i]) == \
                (name, int(channel), onset, offset, cluster)
        first = np.flatnonzero(arch["filename"] == "one.wav")
        assert len(first) == len(want["onset"]) and np.array_equal(bits(arch["patch"][first]), bits(want["patch"]))
