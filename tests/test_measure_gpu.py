"""Per-segment measurements on the GPU (wseg_measure_segments_f32, whisperseg_amd/csrc/wseg_measure.hip) against the host
definition whisperseg_amd.measure.measure_host, from the kernel pair up to segment(measure=True) and the CLI's --measure.

What may differ from the definition, and by how much, is worked out in tests/measure_cases.py (above SPREAD): the time-domain
columns not at all (rms by one float32 ulp: both sides take sqrt(mean) of a float64 sum of exact squares, whose relative error is
far below 2^-24, and round once), the spectral columns by four times the measured cost of an fp32 FFT plus the output's ulps,
and the peak bin must be a near-maximiser of the definition's float64 spectrum."""
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

import golden_inputs as GI
import measure_cases as MC
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import measure as M
from whisperseg_amd.audio_utils import get_n_fft_given_sr

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
FIXTURE_WAVS = [os.path.join(GOLDEN, "meerkat_5s.wav"), os.path.join(GOLDEN, "zebra_finch_g17y2U-f00007.wav")]
GUARD = 64                            # NaN samples in front of and behind the recording
ROW_GUARD = 0x7fc12345                # the bits of the guard rows: a NaN no kernel writes


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def guarded(x):
    """-> (whole tensor, the recording inside it): NaN guards in front and behind."""
    whole = torch.full((len(x) + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    whole[GUARD:GUARD + len(x)] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return whole, whole[GUARD:GUARD + len(x)]


def device_rows(x, bounds, sr, min_frequency=0):
    """The launch pair on a guarded recording into rows held between guard rows -> raw float32 [n_seg, 8]; the guards must survive."""
    n_fft = get_n_fft_given_sr(sr)
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    _, pcm = guarded(x)
    held = torch.from_numpy(np.full((len(bounds) + 2, 8), ROW_GUARD, np.uint32).view(np.float32)).cuda()
    M.measure_rows(pcm, bounds, n_fft, *M.band_bins(sr, n_fft, min_frequency), out=held[1:len(bounds) + 1])
    host = held.cpu().numpy()
    assert (bits(host[0]) == ROW_GUARD).all() and (bits(host[-1]) == ROW_GUARD).all()
    return host[1:-1]


def device_columns(x, bounds, sr, min_frequency=0):
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    return M.columns_from_rows(device_rows(x, bounds, sr, min_frequency), bounds[:, 1] - bounds[:, 0], sr, get_n_fft_given_sr(sr))


def check(got, x, bounds, sr, min_frequency=0, what=""):
    """Every column of `got` against the definition on (x, bounds); prints the largest error / tolerance ratio per column."""
    n_fft = get_n_fft_given_sr(sr)
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    want = M.measure_host(x, sr, MC.prediction(bounds, sr, len(x)), min_frequency=min_frequency)
    k_lo, k_hi = M.band_bins(sr, n_fft, min_frequency)
    for name in M.COLUMNS:
        assert got[name].dtype == np.float32 and got[name].shape == (len(bounds),), name
        assert np.array_equal(np.isnan(got[name]), np.isnan(want[name])), (what, name, np.flatnonzero(np.isnan(got[name]) != np.isnan(want[name])))
    ok = ~np.isnan(want["rms"])
    assert np.array_equal(bits(got["peak_amplitude"][ok]), bits(want["peak_amplitude"][ok])), (what, "peak_amplitude")
    assert np.array_equal(got["zero_crossing_rate"][ok], want["zero_crossing_rate"][ok]), (what, "zero_crossing_rate")
    rms_ulps = np.abs(got["rms"][ok].astype(np.float64) - want["rms"][ok]) / np.spacing(want["rms"][ok])
    assert (rms_ulps <= 1).all(), (what, "rms", rms_ulps.max())
    spectral = np.flatnonzero(~np.isnan(want["peak_frequency"]))
    worst_peak = 0.0
    for i in spectral:
        k = int(round(float(got["peak_frequency"][i]) * n_fft / sr))
        assert k_lo <= k <= k_hi and got["peak_frequency"][i] == np.float32(k * sr / n_fft), (what, i, got["peak_frequency"][i])
        band = M.power_spectrum(x, int(bounds[i, 0]), int(bounds[i, 1]), n_fft)[k_lo:k_hi + 1]
        worst_peak = max(worst_peak, 1 - band[k - k_lo] / band.max())
        assert band[k - k_lo] >= (1 - MC.PEAK_TAU) * band.max(), (what, i, k, band[k - k_lo] / band.max())
    ratios = {}
    for name in MC.SPREAD_COLUMNS:
        err = np.abs(got[name][spectral].astype(np.float64) - want[name][spectral])
        tol = MC.tolerance(name, want[name][spectral], sr)
        ratios[name] = float((err / tol).max()) if len(err) else 0.0
        unit = 1.0 if name == "spectral_entropy" else sr / n_fft
        print(f"{what} sr={sr} {name}: largest error {float((err / unit).max()) if len(err) else 0:.3g} (bins / absolute), {ratios[name]:.3f} of its tolerance")
        assert (err <= tol).all(), (what, name, int(np.argmax(err / tol)), float((err / tol).max()))
    print(f"{what} sr={sr}: {len(bounds)} segments, {len(spectral)} with a spectrum; rms within {rms_ulps.max() if ok.any() else 0:.2f} ulp; "
          f"peak bin short of the maximum by {worst_peak:.2e} (allowed {MC.PEAK_TAU:.2e})")
    return want


@functools.lru_cache(maxsize=None)
def case(sr):
    """recording(sr), segments(sr) and the device's columns for them: computed once, shared, never modified."""
    x, bounds = MC.recording(sr), MC.segments(sr)
    return x, bounds, device_columns(x, bounds, sr)


@pytest.mark.parametrize("sr", MC.RATES)
def test_every_path_at_every_rate(gpu_lib, sr):
    """All five n_fft; 1 and 7 samples, one frame -+ 1, the second frame, the seam of two chunks at 63 / 64 / 65 frames, a dozen
    random lengths; odd starts, s0 = 0, s1 = n, overlapping, empty and silent segments; guards around samples and rows."""
    x, bounds, got = case(sr)
    n_fft = get_n_fft_given_sr(sr)
    frames = [M.frame_count(int(s1 - s0), n_fft) for s0, s1 in bounds]
    assert {0, 1, 2, 3, 63, 64, 65} <= set(frames) and bounds[:, 0].min() == 0 and bounds[:, 1].max() == len(x)
    want = check(got, x, bounds, sr, what="paths")
    empty, silent = len(bounds) - 2, len(bounds) - 1
    assert all(np.isnan(want[c][empty]) for c in M.COLUMNS)
    assert want["rms"][silent] == 0 and np.isnan(want["peak_frequency"][silent]) and np.isnan(got["spectral_entropy"][silent])
    # the public call, from numpy and from the resident tensor, gives those bits
    pred = MC.prediction(bounds, sr, len(x))
    for audio in (x, guarded(x)[1]):
        again = M.measure(audio, sr, pred)
        assert list(again) == list(M.COLUMNS) and all(np.array_equal(bits(again[c]), bits(got[c])) for c in M.COLUMNS)


@pytest.mark.parametrize("n_seg", MC.RANDOM_COUNTS)
def test_segment_counts(gpu_lib, n_seg):
    sr, low = MC.RANDOM_RATE, MC.RANDOM_MIN_FREQUENCY
    x = MC.recording(sr)
    bounds = MC.random_segments(sr, len(x), n_seg)
    got = device_columns(x, bounds, sr, min_frequency=low)
    assert all(got[c].shape == (n_seg,) for c in M.COLUMNS)
    check(got, x, bounds, sr, min_frequency=low, what=f"n_seg={n_seg}")
    if n_seg == 0:
        assert all(len(v) == 0 for v in M.measure(x, sr, {"onset": [], "offset": []}).values())


@pytest.mark.parametrize("sr", MC.RATES)
def test_neighbouring_samples_never_leak(gpu_lib, sr):
    """x[s0 - 1] and x[s1] set to NaN, then to +inf: every row keeps the bits of the clean run."""
    x = MC.recording(sr)
    bounds = MC.spaced_segments(sr)
    clean = device_rows(x, bounds, sr)
    assert np.isfinite(clean[:, :3]).all()
    for poison in (np.nan, np.inf):
        y = x.copy()
        y[bounds[:, 0] - 1] = poison
        y[bounds[:, 1]] = poison
        assert np.array_equal(bits(device_rows(y, bounds, sr)), bits(clean)), poison


def test_same_bits_on_every_run_and_for_every_grid(gpu_lib, monkeypatch):
    sr = 400000                                     # 37 segments, 45 chunks: a grid of 3 strides fifteen times
    x, bounds, _ = case(sr)
    first = device_rows(x, bounds, sr)
    assert np.array_equal(bits(device_rows(x, bounds, sr)), bits(first))
    many = MC.random_segments(16000, 16000, 257)
    first_many = device_rows(MC.recording(16000), many, 16000)
    for cap in ("3", "1"):
        monkeypatch.setenv("WSEG_MEASURE_GRID", cap)
        assert np.array_equal(bits(device_rows(x, bounds, sr)), bits(first)), cap
        assert np.array_equal(bits(device_rows(MC.recording(16000), many, 16000)), bits(first_many)), cap


def test_invalid_calls_are_refused_before_a_launch(gpu_lib):
    from whisperseg_amd import _lib
    sr = 16000
    x = MC.recording(sr)
    pred = MC.prediction([(10, 900)], sr, len(x))
    with pytest.raises(ValueError, match="k_lo"):
        M.measure(x, sr, pred, min_frequency=7000, max_frequency=6000)
    pcm = guarded(x)[1]
    with pytest.raises(_lib.WsegError, match="bounds"):
        M.measure_rows(pcm, [(10, len(x) + 1)], 512, 1, 256)
    with pytest.raises(_lib.WsegError, match="k_hi"):
        M.measure_rows(pcm, [(10, 900)], 512, 1, 257)
    with pytest.raises(_lib.WsegError, match="n_fft"):
        M.measure_rows(pcm, [(10, 900)], 500, 1, 250)
    with pytest.raises(_lib.WsegError):
        M.measure_rows(torch.from_numpy(x), [(10, 900)], 512, 1, 256)          # no CPU path


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
    tiny = tmp_path_factory.mktemp("measure") / "tiny.wav"
    tiny.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", s16(GI.tiny_recording(3, 2)))))
    return [str(tiny)] + FIXTURE_WAVS


ROW_KEYS = ("onset", "offset", "cluster")
KW = dict(spec_time_step=TM.STS)


def split(pred):
    """(the three row columns, the eight measured ones as float32 arrays) of a measure=True prediction."""
    assert list(pred) == list(ROW_KEYS) + list(M.COLUMNS)
    assert all(isinstance(pred[c], list) and len(pred[c]) == len(pred["onset"]) for c in M.COLUMNS)
    return {k: pred[k] for k in ROW_KEYS}, {c: np.asarray(pred[c], dtype=np.float32) for c in M.COLUMNS}


def check_prediction(pred, plain, x, sr, min_frequency, what):
    rows, cols = split(pred)
    assert rows == plain, what
    check(cols, x, M.bounds_of(rows, sr, len(x)), sr, min_frequency=min_frequency, what=what)


def test_segment_with_measure(gpu_lib, seg, wavs):
    from whisperseg_amd.wavio import load_wav
    total = 0
    for path in wavs:
        x, sr = load_wav(path)
        plain = seg.segment(x, sr, **KW)
        assert set(plain) == set(ROW_KEYS)
        pred = seg.segment(x, sr, measure=True, **KW)
        check_prediction(pred, plain, x, sr, 0, os.path.basename(path))
        total += len(plain["onset"])
        if plain["onset"]:                           # the band starts at the recording's min_frequency
            high = seg.segment(x, sr, measure=True, min_frequency=2000, **KW)
            check_prediction(high, seg.segment(x, sr, min_frequency=2000, **KW), x, sr, 2000, "min_frequency=2000")
            low = split(high)[1]["freq_05"]
            assert (low[~np.isnan(low)] >= 2000 - sr / get_n_fft_given_sr(sr)).all()
        if path == wavs[0]:
            assert len(plain["onset"]) >= 3          # not vacuous: the fixture model finds rows in its own signal family
    assert total >= 3


def test_segment_files_and_batch_with_measure(gpu_lib, seg, wavs, tmp_path):
    from whisperseg_amd.wavio import load_wav, load_wav_device
    per_file = [seg.segment(*load_wav(p), measure=True, **KW) for p in wavs]
    assert seg.segment_files(wavs, measure=True, **KW) == per_file
    assert seg.segment_batch([load_wav(p) for p in wavs], measure=True, **KW) == per_file
    assert [{k: p[k] for k in ROW_KEYS} for p in per_file] == seg.segment_files(wavs, **KW)
    # at a second rate the columns are measured at the TARGET rate, on the resampled samples
    rate = 24000
    at_rate = seg.segment_files(wavs, sr=rate, measure=True, **KW)
    for path, pred in zip(wavs, at_rate):
        audio, sr = load_wav_device(path, sr=rate)
        assert sr == rate
        check_prediction(pred, seg.segment(audio, rate, **KW), audio.cpu().numpy(), rate, 0, f"sr={rate} " + os.path.basename(path))
    # every channel of a two-channel file, each measured on its own plane
    x, sr = load_wav(wavs[0])
    two = tmp_path / "two.wav"
    two.write_bytes(WC.wav_bytes("s16", 2, sr, WC.sample_bytes("s16", np.stack([s16(x), s16(0.5 * x[::-1])], axis=1).reshape(-1))))
    planes, _ = load_wav(str(two), mono=False)
    got = seg.segment_files([str(two)], channel_id="all", measure=True, **KW)
    assert len(got) == 1 and len(got[0]) == 2
    assert got[0] == seg.segment_channels(planes, sr, measure=True, **KW)
    for c, pred in enumerate(got[0]):
        check_prediction(pred, seg.segment(planes[c], sr, **KW), planes[c], sr, 0, f"channel {c}")
    assert got[0][0]["onset"] and got[0][0] != got[0][1]


def test_cli_measure(gpu_lib, seg, wavs, tmp_path, monkeypatch):
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
    plain_csv, full_csv = tmp_path / "plain.csv", tmp_path / "full.csv"
    segment.main(base + ["--csv_save_path", str(plain_csv)])
    segment.main(base + ["--csv_save_path", str(full_csv), "--measure"])
    plain = seg.segment(x, sr, **KW)
    text = io.StringIO()
    segment.write_csv(["onset", "offset", "cluster"], list(zip(plain["onset"], plain["offset"], plain["cluster"])), text)
    assert plain_csv.read_text() == text.getvalue() and plain["onset"]          # byte for byte what the existing path writes
    full = seg.segment(x, sr, measure=True, **KW)
    text = io.StringIO()
    segment.write_csv(*segment.table([full], measure=True), text)
    lines = full_csv.read_text().splitlines()
    assert full_csv.read_text() == text.getvalue()
    assert lines[0] == "onset,offset,cluster," + ",".join(M.COLUMNS) and len(lines) == 1 + len(plain["onset"])
    assert [ln.split(",")[:3] for ln in lines] == [ln.split(",") for ln in plain_csv.read_text().splitlines()]
