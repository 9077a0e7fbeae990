"""The pitch contour on the GPU (wseg_pitch_frames_f64, whisperseg_amd/csrc/wseg_pitch.hip) against the host definition
whisperseg_amd.pitch.frames_host, from the kernel up to segment(pitch=True) and the CLI's --pitch.

There is no tolerance anywhere: the kernel takes the definition's float64 steps (+ - x / and comparisons, correctly rounded on both
sides) in the definition's order, so all three columns of every frame must have the definition's BITS, on every case of
tests/pitch_cases.py, for every grid."""
import ctypes as C
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

import golden_inputs as GI
import pitch_cases as PC
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import measure as M
from whisperseg_amd import pitch as P

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
GUARD = 64                            # NaN samples in front of and behind the recording; guard rows / words around out and scratch
ROW_GUARD = 0x7fc12345                # the bits of the guard words: a NaN no kernel writes
BYTE_GUARD = 0xa5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_frames(case):
    """The launch on a guarded recording, into rows held between guard rows, with guard bytes behind the scratch -> float32
    [total_frames, 3]; every guard must survive."""
    from whisperseg_amd import _lib
    lib = _lib.load(require_device=True)
    x = np.array(case.x, dtype=np.float32)                   # (a writable copy: the cases are read-only)
    whole = torch.full((len(x) + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    whole[GUARD:GUARD + len(x)] = torch.from_numpy(x).cuda()
    pcm = whole[GUARD:GUARD + len(x)]
    bounds = np.ascontiguousarray(case.bounds, dtype=np.int64).reshape(-1, 2)
    offsets = P.frame_offsets_of(bounds, case.tau_max, case.hop)
    total = int(offsets[-1])
    held = torch.from_numpy(np.full((total + 2 * GUARD, 3), ROW_GUARD, np.uint32).view(np.float32)).cuda()
    nbytes = P.scratch_bytes(bounds, case.tau_max, case.hop)
    scratch = torch.full((nbytes + 256,), BYTE_GUARD, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wseg_pitch_frames_f64(pcm.data_ptr(), len(x), bounds.ctypes.data_as(C.c_void_p), len(bounds), case.tau_min, case.tau_max,
                                         case.hop, float(case.threshold), scratch.data_ptr(), nbytes, held[GUARD:].data_ptr(),
                                         _lib.stream_ptr()))
    host = held.cpu().numpy()
    assert (bits(host[:GUARD]) == ROW_GUARD).all() and (bits(host[GUARD + total:]) == ROW_GUARD).all(), case.name
    assert (scratch[nbytes:].cpu().numpy() == BYTE_GUARD).all(), case.name
    return host[GUARD:GUARD + total]


@functools.lru_cache(maxsize=None)
def device(index):
    """The device's frames of all_cases()[index] under the default grid: computed once, shared, never modified."""
    got = device_frames(PC.all_cases()[index])
    got.setflags(write=False)
    return got


def assert_same_bits(got, index, what=""):
    case = PC.all_cases()[index]
    want, offsets = PC.expected(index)
    assert got.shape == want.shape, (case.name, what)
    wrong = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    if len(wrong):
        f = int(wrong[0])
        seg = int(np.searchsorted(offsets, f, side="right")) - 1
        raise AssertionError(f"{case.name} {what}: {len(wrong)} of {len(want)} frames differ; the first is frame {f} (segment {seg} "
                             f"{case.bounds[seg].tolist()}): device {got[f].tolist()}, definition {want[f].tolist()}")


@pytest.mark.parametrize("index", range(len(PC.all_cases())), ids=[c.name for c in PC.all_cases()])
def test_the_device_has_the_definitions_bits(gpu_lib, index):
    """Every case: five lag ranges (one candidate .. 2048 lags), every structural length, ten signal families, three thresholds, a
    threshold that equals a d' value, one where the prefix sum's order decides, exact-fit segments clean and poisoned, 300 random
    segments."""
    assert_same_bits(device(index), index)


def test_neighbouring_samples_never_leak(gpu_lib):
    """x[s0 - 1] and x[s1] set to NaN: every frame keeps the bits of the clean run (and out and scratch keep their guards)."""
    names = [c.name for c in PC.all_cases()]
    pairs = [(i, names.index("poisoned " + n)) for i, n in enumerate(names) if "poisoned " + n in names]
    assert len(pairs) == 4
    for clean, poisoned in pairs:
        assert np.isnan(PC.all_cases()[poisoned].x).any() and np.isfinite(device(clean)).all()
        assert np.array_equal(bits(device(clean)), bits(device(poisoned))), names[clean]


def test_same_bits_on_every_run_and_for_every_grid(gpu_lib, monkeypatch):
    chosen = [PC.index_of("300 random segments"), PC.index_of("lags 8..257"), PC.index_of("lags 8..2048"), PC.index_of("lags 2..3")]
    for index in chosen:
        assert np.array_equal(bits(device_frames(PC.all_cases()[index])), bits(device(index)))
    for cap in ("3", "1"):
        monkeypatch.setenv("WSEG_PITCH_GRID", cap)
        for index in chosen:
            assert_same_bits(device_frames(PC.all_cases()[index]), index, what=f"grid {cap}")


def test_public_calls(gpu_lib):
    sr = 16000
    rng = np.random.default_rng(PC.SEED + 77)
    x = np.concatenate([PC.synthetic("missing", 310.0, sr, 6000, rng, True), np.zeros(3000, np.float32),
                        PC.synthetic("tone", 1234.5, sr, 6000, rng, False)])
    pred = PC.prediction([(10, 5000), (6100, 8900), (9100, 15000), (100, 300), (7, 7)], sr, len(x))
    for kw in ({}, {"f_min": 100.0, "f_max": 2500.0, "threshold": 0.15, "hop": 37}):
        want = P.pitch_host(x, sr, pred, contour=True, **kw)
        for audio in (x, torch.from_numpy(x).cuda(), torch.from_numpy(x)):
            got = P.pitch(audio, sr, pred, contour=True, **kw)
            assert list(got) == list(P.COLUMNS) + list(P.CONTOUR_KEYS)
            for c in P.COLUMNS:
                assert got[c].dtype == np.float32 and np.array_equal(bits(got[c]), bits(want[c])), (c, kw)
            for key in P.CONTOUR_KEYS:
                assert len(got[key]) == 5 and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[key], want[key])), key
        assert list(P.pitch(x, sr, pred, **kw)) == list(P.COLUMNS)
    assert abs(want["f0_mean"][2] / 1234.5 - 1) < 0.01 and np.isnan(want["f0_mean"][1]) and np.isnan(want["aperiodicity"][3])
    plain = P.pitch_host(x, sr, pred)
    assert abs(plain["f0_mean"][0] / 310 - 1) < 2e-3          # the missing fundamental, not a partial
    assert all(len(v) == 0 for v in P.pitch(x, sr, {"onset": [], "offset": []}).values())
    # the launch itself: the device contour and the host offsets
    pcm = torch.from_numpy(x).cuda()
    frames, offsets = P.pitch_rows(pcm, [(10, 5000), (7, 7)], 8, 256, 128)
    assert frames.is_cuda and frames.shape == (int(offsets[-1]), 3) and list(offsets) == [0, 1 + (4990 - 512) // 128, 35]
    frames, offsets = P.pitch_rows(pcm, np.zeros((0, 2), np.int64), 8, 256, 128)
    assert frames.shape == (0, 3) and list(offsets) == [0]


def test_invalid_calls_are_refused_before_a_launch(gpu_lib):
    from whisperseg_amd import _lib
    sr = 16000
    x = np.zeros(4000, np.float32)
    pred = PC.prediction([(10, 3000)], sr, len(x))
    for kw in (dict(f_min=5.0), dict(f_min=4000, f_max=3000), dict(threshold=1.0), dict(threshold=0.0), dict(hop=0)):
        with pytest.raises(ValueError):
            P.pitch(x, sr, pred, **kw)
    pcm = torch.from_numpy(x).cuda()
    for args, word in ((([(10, 4001)], 8, 256, 128), "bounds"), (([(9, 8)], 8, 256, 128), "bounds"), (([(10, 3000)], 1, 256, 128), "tau_min"),
                       (([(10, 3000)], 8, 8, 128), "tau_m"), (([(10, 3000)], 8, 2049, 128), "tau_max"), (([(10, 3000)], 8, 256, 0), "hop"),
                       (([(10, 3000)], 8, 256, 128, 1.0), "threshold"), (([(10, 3000)], 8, 256, 128, float("nan")), "threshold")):
        with pytest.raises(_lib.WsegError, match=word):
            P.pitch_rows(pcm, *args)
    with pytest.raises(_lib.WsegError):
        P.pitch_rows(torch.from_numpy(x), [(10, 3000)], 8, 256, 128)          # no CPU path
    with pytest.raises(_lib.WsegError, match="out"):
        P.pitch_rows(pcm, [(10, 3000)], 8, 256, 128, out=torch.empty((3, 3), dtype=torch.float32, device="cuda"))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seg():
    from whisperseg_amd.model import WhisperSegmenter
    return WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")


def s16(v):
    return np.clip(np.round(np.asarray(v, np.float64) * 32768), -32768, 32767).astype(np.int64)


@pytest.fixture(scope="module")
def wav(tmp_path_factory):
    """A recording of the fixture model's own signal family as an s16 file: the model finds rows in it."""
    tiny = tmp_path_factory.mktemp("pitch") / "tiny.wav"
    tiny.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", s16(GI.tiny_recording(3, 2)))))
    return str(tiny)


ROW_KEYS = ("onset", "offset", "cluster")
KW = dict(spec_time_step=TM.STS)


def test_segment_with_pitch(gpu_lib, seg, wav):
    from whisperseg_amd.wavio import load_wav
    x, sr = load_wav(wav)
    plain = seg.segment(x, sr, **KW)
    assert set(plain) == set(ROW_KEYS) and len(plain["onset"]) >= 3
    pred = seg.segment(x, sr, pitch=True, **KW)
    assert list(pred) == list(ROW_KEYS) + list(P.COLUMNS) and {k: pred[k] for k in ROW_KEYS} == plain
    want = P.pitch_host(x, sr, plain)
    for c in P.COLUMNS:
        assert isinstance(pred[c], list) and len(pred[c]) == len(plain["onset"])
        assert np.array_equal(bits(np.float32(pred[c])), bits(want[c])), c
    # a range, a threshold and the contours
    opts = {"f_min": 2.5 * sr / 512, "f_max": sr / 10, "threshold": 0.2, "contour": True}
    full = seg.segment(x, sr, pitch=opts, **KW)
    want = P.pitch_host(x, sr, plain, **opts)
    assert list(full) == list(ROW_KEYS) + list(P.COLUMNS) + list(P.CONTOUR_KEYS)
    assert all(np.array_equal(bits(np.float32(full[c])), bits(want[c])) for c in P.COLUMNS)
    assert all(np.array_equal(a, b, equal_nan=True) for key in P.CONTOUR_KEYS for a, b in zip(full[key], want[key]))
    assert sum(len(a) for a in full["f0_contour"]) > 0
    # with the other two keywords: the same rows as each keyword alone, the PCM held once
    every = seg.segment(x, sr, measure=True, patches=8, pitch=True, **KW)
    measured, pictured = seg.segment(x, sr, measure=True, **KW), seg.segment(x, sr, patches=8, **KW)
    assert set(every) == set(ROW_KEYS) | set(M.COLUMNS) | set(P.COLUMNS) | {"patch"}
    assert all(every[k] == pred[k] for k in ROW_KEYS)
    assert all(np.array_equal(bits(np.float32(every[c])), bits(np.float32(pred[c]))) for c in P.COLUMNS)
    assert all(np.array_equal(bits(np.float32(every[c])), bits(np.float32(measured[c]))) for c in M.COLUMNS)
    assert np.array_equal(every["patch"], pictured["patch"])
    # the other entry points, and a channel's plane
    assert seg.segment_batch([(x, sr)], pitch=True, **KW)[0].keys() == pred.keys()
    batch = seg.segment_batch([(x, sr), (x[::-1].copy(), sr)], pitch=True, **KW)
    files = seg.segment_files([wav], pitch=True, **KW)
    for other in (batch[0], files[0]):
        assert {k: other[k] for k in ROW_KEYS} == plain
        assert all(np.array_equal(bits(np.float32(other[c])), bits(np.float32(pred[c]))) for c in P.COLUMNS)
    planes = np.stack([x, 0.5 * x[::-1]]).astype(np.float32)
    per_channel = seg.segment_channels(planes, sr, pitch=True, **KW)
    assert all(np.array_equal(bits(np.float32(per_channel[0][c])), bits(np.float32(pred[c]))) for c in P.COLUMNS)
    rows1 = {k: per_channel[1][k] for k in ROW_KEYS}
    want1 = P.pitch_host(planes[1], sr, rows1)
    assert all(np.array_equal(bits(np.float32(per_channel[1][c])), bits(want1[c])) for c in P.COLUMNS)
    # a bad range fails before anything runs
    for bad in ({"f_min": 5.0}, {"threshold": 2}, {"hop": 3}, "yes"):
        with pytest.raises(ValueError):
            seg.segment(x, sr, pitch=bad, **KW)
        with pytest.raises(ValueError):
            seg.segment_batch([(x, sr)], pitch=bad, **KW)


def test_cli_pitch(gpu_lib, seg, wav, tmp_path, monkeypatch):
    from whisperseg_amd.wavio import load_wav
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    monkeypatch.setenv("WHISPERSEG_AMD_DTYPE", "f32")
    x, sr = load_wav(wav)
    base = ["--model_path", MODEL_DIR, "--audio_path", wav, "--spec_time_step", str(TM.STS)]
    plain_csv, full_csv, both_csv, archive = tmp_path / "plain.csv", tmp_path / "full.csv", tmp_path / "both.csv", tmp_path / "f0.npz"
    segment.main(base + ["--csv_save_path", str(plain_csv)])
    segment.main(base + ["--csv_save_path", str(full_csv), "--pitch", "--pitch_save_path", str(archive)])
    segment.main(base + ["--csv_save_path", str(both_csv), "--measure", "--pitch", "--pitch_threshold", "0.2"])
    plain = seg.segment(x, sr, **KW)
    text = io.StringIO()
    segment.write_csv(["onset", "offset", "cluster"], list(zip(plain["onset"], plain["offset"], plain["cluster"])), text)
    assert plain_csv.read_text() == text.getvalue() and plain["onset"]          # byte for byte what the existing path writes
    full = seg.segment(x, sr, pitch={"contour": True}, **KW)
    text = io.StringIO()
    segment.write_csv(*segment.table([full], pitch=True), text)
    lines = full_csv.read_text().splitlines()
    assert full_csv.read_text() == text.getvalue()
    assert lines[0] == "onset,offset,cluster," + ",".join(P.COLUMNS) and len(lines) == 1 + len(plain["onset"])
    assert [ln.split(",")[:3] for ln in lines] == [ln.split(",") for ln in plain_csv.read_text().splitlines()]
    lines = both_csv.read_text().splitlines()
    assert lines[0] == "onset,offset,cluster," + ",".join(M.COLUMNS + P.COLUMNS) and len(lines) == 1 + len(plain["onset"])
    assert [ln.split(",")[:3] for ln in lines] == [ln.split(",") for ln in plain_csv.read_text().splitlines()]
    saved = np.load(str(archive))
    assert set(saved.files) == {"f0", "aperiodicity", "frame_time", "frame_offsets", "onset", "offset", "cluster"}
    want = P.pitch_host(x, sr, plain, contour=True)
    assert saved["frame_offsets"].dtype == np.int64 and len(saved["frame_offsets"]) == len(plain["onset"]) + 1
    assert np.array_equal(np.diff(saved["frame_offsets"]), [len(a) for a in want["f0_contour"]]) and saved["frame_offsets"][-1] > 0
    assert np.array_equal(saved["f0"], np.concatenate(want["f0_contour"]), equal_nan=True)
    assert np.array_equal(saved["aperiodicity"], np.concatenate(want["aperiodicity_contour"]))
    assert np.array_equal(saved["frame_time"], np.concatenate(want["frame_time"]))
    assert list(saved["onset"]) == plain["onset"] and list(saved["offset"]) == plain["offset"] and list(saved["cluster"]) == [str(c) for c in plain["cluster"]]
