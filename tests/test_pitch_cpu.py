"""The host definition of the pitch contour (whisperseg_amd/pitch.py) against its plain restatement, its own conventions and
signals whose fundamental is known; no GPU.  The device test (tests/test_pitch_gpu.py) compares the kernel with this definition
bit for bit, so what is checked here is that the definition is what it says and that it finds the pitch."""
import os
import sys

import numpy as np
import pytest

import pitch_cases as PC
from conftest import GOLDEN, ROOT
from whisperseg_amd import measure as M
from whisperseg_amd import pitch as P
from whisperseg_amd.audio_utils import get_n_fft_given_sr


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_definition_has_the_bits_of_the_plain_double_loop():
    """Every case with tau_max <= 65, every segment: frames_host (numpy, vectorised over lags and frames) == frames_plain (Python
    floats, one lag and one term at a time, its own frame count and prefix sum)."""
    checked = 0
    for index, c in enumerate(PC.all_cases()):
        if c.tau_max > 65:
            continue
        frames, offsets = PC.expected(index)
        for (s0, s1), first, last in zip(c.bounds, offsets[:-1], offsets[1:]):
            plain = P.frames_plain(c.x, int(s0), int(s1), c.tau_min, c.tau_max, c.hop, c.threshold)
            assert len(plain) == last - first, (c.name, s0, s1)
            if "poisoned" not in c.name:
                assert np.isfinite(plain).all()
            assert np.array_equal(bits(plain), bits(frames[first:last])), (c.name, s0, s1)
            checked += len(plain)
    assert checked > 3000


def test_the_order_is_immaterial_on_int16_pcm():
    """On int16-derived PCM every term and every partial sum of d, scaled by 2^30, is an integer below 2^53: the chain's d equals
    numpy's pairwise ((a - b) ** 2).sum() bit for bit — and the chain's order shows in no bit there."""
    for tau_max in (65, 257, 2048):
        x = PC.signal("int16_noise", tau_max, 2 * tau_max + 3)
        assert np.array_equal(x * 32768, np.round(x * 32768)) and np.abs(x * 32768).max() <= 3000
        frames = np.stack([x[j:j + 2 * tau_max] for j in (0, 3)])
        d = P.difference(frames, tau_max)
        x64 = frames.astype(np.float64)
        for f in range(2):
            for tau in (0, 1, 2, tau_max // 2, tau_max - 1, tau_max):
                assert d[f, tau] == ((x64[f, :tau_max] - x64[f, tau:tau + tau_max]) ** 2).sum()
        assert (d * 2.0 ** 30 == np.round(d * 2.0 ** 30)).all() and (d * 2.0 ** 30).max() < 2.0 ** 53


def test_frame_counts():
    for tau_min, tau_max in PC.LAGS:
        hop = PC.HOPS[tau_max]
        lengths = PC.structural_lengths(tau_max, hop)
        assert [P.frame_count(v, tau_max, hop) for v in lengths] == [0, 1, 1, 2, 0, 4]
        for length in lengths + [1, 2 * tau_max + 7 * hop + hop // 2]:
            walked = sum(1 for t in range(0, max(0, length), hop) if t + 2 * tau_max <= length)      # frames by their starts
            assert P.frame_count(length, tau_max, hop) == walked
    c = PC.structural_case(8, 65)
    _, offsets = PC.expected(PC.index_of(c.name))
    assert list(np.diff(offsets)[:6]) == [0, 1, 1, 2, 0, 4] and offsets[0] == 0
    assert np.array_equal(offsets, P.frame_offsets_of(c.bounds, c.tau_max, c.hop))
    assert c.bounds[:, 0].min() == 0 and c.bounds[:, 1].max() == len(c.x)
    # hop = 1 and a hop longer than the frame
    assert P.frame_count(20, 8, 1) == 5 and P.frame_count(100, 8, 50) == 2 and P.frame_count(15, 8, 1) == 0


def test_neighbouring_samples_never_leak():
    cases = PC.all_cases()
    pairs = [(i, i + 1) for i, c in enumerate(cases[:-1]) if cases[i + 1].name == "poisoned " + c.name]
    assert len(pairs) == len(PC.LAGS) - 1
    for clean, poisoned in pairs:
        assert np.isnan(cases[poisoned].x).sum() == 2 * len(cases[poisoned].bounds)
        assert np.isfinite(PC.expected(clean)[0]).all()
        assert np.array_equal(bits(PC.expected(clean)[0]), bits(PC.expected(poisoned)[0]))
        # the last frame of every segment ends at s1, the first starts at s0
        c = cases[clean]
        assert ((c.bounds[:, 1] - c.bounds[:, 0] - 2 * c.tau_max) % c.hop == 0).all()


def test_conventions_and_what_the_cases_hold():
    for tau_min, tau_max in PC.LAGS[:-1]:
        c = PC.structural_case(tau_min, tau_max)
        frames, offsets = PC.expected(PC.index_of(c.name))
        per = 6                                      # segments per signal
        for name in ("silence", "dc"):
            s = PC.SIGNALS.index(name)
            got = frames[offsets[per * s]:offsets[per * (s + 1)]]
            assert len(got) == 8 and np.array_equal(got, np.tile(np.float32([tau_min, 1, 0]), (8, 1))), (name, tau_max)
        s = PC.SIGNALS.index("edge_dip")             # the dip at the last candidate
        got = frames[offsets[per * s]:offsets[per * (s + 1)]]
        assert (got[:, 2] == 1).all() and (np.abs(got[:, 0] - (tau_max - 1)) <= 0.5).all(), tau_max
    # a descent of several lags behind the first lag under the threshold; clamped shifts; both kinds of frames
    descents, clamped = 0, 0
    for index, c in enumerate(PC.all_cases()):
        frames, offsets = PC.expected(index)
        clamped += int((np.abs(frames[:, 0] - np.round(frames[:, 0])) == 0.5).sum())
        for (s0, s1), first, last in zip(c.bounds, offsets[:-1], offsets[1:]):
            if last > first and frames[first, 2] == 1 and c.tau_max >= 64 and np.isfinite(c.x[s0:s1]).all():
                dn = P.normalised_difference(c.x[None, s0:s0 + 2 * c.tau_max], c.tau_max)[0]
                start = c.tau_min + int(np.flatnonzero(dn[c.tau_min:c.tau_max] < c.threshold)[0])
                descents += int(round(float(frames[first, 0])) - start >= 3)
    assert descents >= 10 and clamped >= 3
    tie, order = PC.threshold_cases()
    for c in (tie, order):
        dn = P.normalised_difference(c.x[None, :], c.tau_max)[0]
        assert (dn[c.tau_min:c.tau_max] == c.threshold).sum() >= (c is tie)
    dn = P.normalised_difference(tie.x[None, :], tie.tau_max)[0]
    at = int(np.flatnonzero(dn[tie.tau_min:tie.tau_max] == tie.threshold)[0]) + tie.tau_min
    assert not (dn[tie.tau_min:at] <= tie.threshold).any()            # a `<=` would stop at `at`; `<` does not
    got = P.pick(dn, tie.tau_min, tie.tau_max, tie.threshold)
    assert not (got[2] == 1 and abs(got[0] - at) <= 0.5 and dn[at + 1] >= dn[at])
    d = P.difference(order.x[None, :], order.tau_max)
    assert not np.array_equal(P.pick(P.normalise(d)[0], order.tau_min, order.tau_max, order.threshold),
                              P.pick(PC.normalise_sequential(d)[0], order.tau_min, order.tau_max, order.threshold))


def test_columns_and_contours():
    sr = 16000
    x = np.concatenate([PC.synthetic("tone", 440.0, sr, 4000, np.random.default_rng(0), False), np.zeros(4000, np.float32),
                        (0.2 * np.random.default_rng(1).standard_normal(4000)).astype(np.float32)])
    pred = PC.prediction([(100, 3900), (4100, 7900), (8100, 11900), (20, 400), (3000, 5000)], sr, len(x))
    out = P.pitch_host(x, sr, pred, contour=True)
    assert list(out) == list(P.COLUMNS) + list(P.CONTOUR_KEYS)
    assert all(out[c].dtype == np.float32 and out[c].shape == (5,) for c in P.COLUMNS)
    assert abs(out["f0_mean"][0] / 440 - 1) < 2e-3 and out["voiced_fraction"][0] == 1 and out["aperiodicity"][0] < 0.01
    assert out["f0_min"][0] <= out["f0_first"][0] <= out["f0_max"][0] and out["f0_min"][0] <= out["f0_last"][0] <= out["f0_max"][0]
    for row in (1, 2):                               # silence, noise: frames, none voiced
        assert out["voiced_fraction"][row] == 0 and all(np.isnan(out[c][row]) for c in P.COLUMNS[:5]) and out["aperiodicity"][row] > 0.5
    assert out["aperiodicity"][1] == 1
    assert all(np.isnan(out[c][3]) for c in P.COLUMNS) and len(out["f0_contour"][3]) == 0      # shorter than a frame
    assert 0 < out["voiced_fraction"][4] < 1         # the tone's end and the silence behind it
    f0 = out["f0_contour"][4]
    assert f0.dtype == np.float32 and np.isnan(f0).any() and np.isfinite(f0).any()
    assert np.array_equal(np.isfinite(f0), out["aperiodicity_contour"][4] < 0.1)
    assert np.allclose(out["frame_time"][4], (3000 + 128 * np.arange(len(f0)) + 256) / sr, rtol=0, atol=1e-12)
    # the means are sequential float64 sums in frame order
    frames, offsets = P.frames_host(x, M.bounds_of(pred, sr, len(x)), 8, 256, 128)
    acc = 0.0
    for v in frames[offsets[0]:offsets[1], 0]:
        acc += sr / float(v)
    assert out["f0_mean"][0] == np.float32(acc / (offsets[1] - offsets[0]))
    merged = P.with_columns(pred, out)
    assert list(merged) == ["onset", "offset"] + list(P.COLUMNS) + list(P.CONTOUR_KEYS) and isinstance(merged["f0_mean"], list)
    assert list(P.pitch_host(x, sr, {"onset": [], "offset": []})) == list(P.COLUMNS)


def test_invalid_ranges_thresholds_and_hops_are_refused():
    assert P.lag_range(16000) == (8, 256) and P.lag_range(250000) == (8, 2048) and P.lag_range(16000, 100, 4000) == (4, 160)
    assert P.lag_range(16000, f_max=16000) == (2, 256)
    x = np.zeros(4000, np.float32)
    pred = {"onset": [0.0], "offset": [0.2]}
    for kw in (dict(f_min=5.0), dict(f_min=4000, f_max=3000), dict(f_min=0), dict(f_max=-1.0),
               dict(f_max=float("nan")), dict(threshold=0.0), dict(threshold=1.0), dict(threshold=float("nan")), dict(hop=0), dict(hop=-3),
               dict(hop=2.5)):
        with pytest.raises(ValueError):
            P.pitch_host(x, 16000, pred, **kw)
    with pytest.raises(ValueError):
        P.pitch_host(np.zeros((2, 100), np.float32), 16000, pred)
    for bad in ((1, 64, 16, 0.1), (2, 2, 16, 0.1), (2, 2049, 16, 0.1), (64, 8, 16, 0.1), (2, 64, 0, 0.1), (2, 64, 2 ** 31, 0.1), (2, 64, 16, 1.5)):
        with pytest.raises(ValueError):
            P.frames_host(x, [(0, 4000)], *bad)
    with pytest.raises(ValueError, match="bounds"):
        P.frames_host(x, [(0, 4001)], 2, 64, 16)
    # the segmenter's keyword
    assert P.options(True) == {} and P.options({"f_min": 200, "contour": True}, 16000) == {"f_min": 200, "contour": True}
    for bad in (False, 1, "yes", {"fmin": 3}, {"threshold": 1}, {"f_min": -1}, {"f_min": 500, "f_max": 400}):
        with pytest.raises(ValueError):
            P.options(bad)
    with pytest.raises(ValueError, match="lags"):
        P.options({"f_min": 5}, 16000)
    from whisperseg_amd.model import SegmenterBase
    assert SegmenterBase._holds_pcm(False, None) is False and SegmenterBase._holds_pcm(False, None, True, 16000) is True
    with pytest.raises(ValueError, match="lags"):
        SegmenterBase._holds_pcm(True, 8, {"f_min": 5}, 16000)
    from whisperseg_amd import dist
    for name in ("segment_distributed", "segment_batch_distributed"):
        with pytest.raises(ValueError, match="pitch"):
            dist._refuse_measure({"pitch": True}, name)


def cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    return segment


def test_cli_flags(capsys):
    segment = cli()
    base = ["--model_path", "m", "--csv_save_path", "o.csv"]
    args = segment.parse_args(base)
    assert args.pitch is False and segment.pitch_keyword(args) is None
    assert segment.pitch_keyword(segment.parse_args(base + ["--pitch"])) is True
    args = segment.parse_args(base + ["--pitch", "--pitch_min_hz", "300", "--pitch_threshold", "0.2", "--pitch_save_path", "p.npz"])
    assert segment.pitch_keyword(args) == {"f_min": 300.0, "threshold": 0.2, "contour": True}
    for extra in (["--pitch_min_hz", "300"], ["--pitch_max_hz", "300"], ["--pitch_threshold", "0.2"], ["--pitch_save_path", "p.npz"],
                  ["--pitch", "--pitch_min_hz", "0"], ["--pitch", "--pitch_max_hz", "-5"], ["--pitch", "--pitch_min_hz", "nan"],
                  ["--pitch", "--pitch_min_hz", "400", "--pitch_max_hz", "300"], ["--pitch", "--pitch_threshold", "0"],
                  ["--pitch", "--pitch_threshold", "1"], ["--pitch", "--pitch_save_path", "p.txt"]):
        with pytest.raises(SystemExit) as e:
            segment.main(base + extra)                       # refused by argparse, before a model is looked for
        assert e.value.code == 2 and "pitch" in capsys.readouterr().err, extra
    # the table carries the columns behind the measurements; the archive follows the table's row order
    a = {"onset": [0.5, 1.25], "offset": [0.75, 1.5], "cluster": ["a", "b"], **{c: [1.0, 2.0] for c in P.COLUMNS},
         "f0_contour": [np.float32([100, np.nan]), np.float32([])], "aperiodicity_contour": [np.float32([0.01, 0.9]), np.float32([])],
         "frame_time": [np.array([0.51, 0.52]), np.array([])]}
    c = {"onset": [0.1], "offset": [0.2], "cluster": ["c"], **{k: [3.0] for k in P.COLUMNS}, "f0_contour": [np.float32([7, 8, 9])],
         "aperiodicity_contour": [np.float32([0.1, 0.2, 0.3])], "frame_time": [np.array([0.11, 0.12, 0.13])]}
    columns, rows = segment.table([[a, c], [c, a]], ["x.wav", "y.wav"], True, pitch=True)
    assert columns == ["filename", "channel", "onset", "offset", "cluster"] + list(P.COLUMNS) and len(rows) == 6
    arch = segment.pitch_archive([[a, c], [c, a]], ["x.wav", "y.wav"], True)
    assert set(arch) == {"f0", "aperiodicity", "frame_time", "frame_offsets", "filename", "channel", "onset", "offset", "cluster"}
    assert arch["frame_offsets"].dtype == np.int64 and list(arch["frame_offsets"]) == [0, 2, 2, 5, 8, 10, 10]
    assert all(arch[k].shape == (10,) for k in ("f0", "aperiodicity", "frame_time"))
    assert np.array_equal(arch["f0"][2:8], np.float32([7, 8, 9, 7, 8, 9])) and np.isnan(arch["f0"][1]) and arch["frame_time"][8] == 0.51
    assert [tuple(arch[k][i].item() for k in columns[:5]) for i in range(6)] == [r[:5] for r in rows]
    assert list(segment.pitch_archive([])["frame_offsets"]) == [0]
    plain = {k: a[k] for k in ("onset", "offset", "cluster")}
    assert segment.table([a]) == segment.table([plain])


# ---- accuracy against signals whose fundamental is known (a check of the definition, not a device tolerance) -----------------------
# Bounds: 0.01 for tones — the parabola's bias at eight samples a period; a numpy prototype of this definition measured 0.0068 /
# 0.0072 at 16 / 32 kHz — and 1.0e-3 for stacks with f <= sr / 32 (prototype: 6.2e-4).  What the bounds must keep excluding is an
# octave error (0.5) and a whole-sample error (1 / period >= 1 / 256).
@pytest.mark.parametrize("sr", (16000, 32000))
def test_tones_are_found(sr):
    rng = np.random.default_rng(PC.SEED + sr)
    n_fft = get_n_fft_given_sr(sr)
    n = 3 * n_fft
    worst = 0.0
    for f in rng.uniform(2.1 * sr / n_fft, 0.98 * sr / 8, 60):
        for noisy in (False, True):
            x = PC.synthetic("tone", f, sr, n, rng, noisy)
            out = P.pitch_host(x, sr, PC.prediction([(0, n)], sr, n), contour=True)
            assert out["voiced_fraction"][0] == 1, (f, noisy)
            err = float(np.abs(out["f0_contour"][0].astype(np.float64) / f - 1).max())
            worst = max(worst, err)
            assert err <= 0.01, (f, noisy, err)
    print(f"sr={sr}: 120 tones, worst |f0 / f - 1| = {worst:.4f}")


@pytest.mark.parametrize("sr", (16000, 32000))
def test_harmonic_stacks_give_the_fundamental_not_the_loudest_partial(sr):
    rng = np.random.default_rng(PC.SEED + 3 * sr)
    n_fft = get_n_fft_given_sr(sr)
    n = 3 * n_fft
    worst, off_peak = 0.0, 0
    for kind in ("stack", "missing"):
        for f in rng.uniform(2.1 * sr / n_fft, sr / 32, 30):
            x = PC.synthetic(kind, f, sr, n, rng, False)
            pred = PC.prediction([(0, n)], sr, n)
            out = P.pitch_host(x, sr, pred, contour=True)
            assert out["voiced_fraction"][0] == 1, (kind, f)
            err = float(np.abs(out["f0_contour"][0].astype(np.float64) / f - 1).max())
            worst = max(worst, err)
            assert err <= 1.0e-3, (kind, f, err)
            if kind == "missing":                    # measure's peak names a partial, not the fundamental
                peak = float(M.measure_host(x, sr, pred)["peak_frequency"][0])
                assert abs(peak / f - 1) > 0.1, (f, peak)
                off_peak += 1
    assert off_peak == 30
    print(f"sr={sr}: 60 stacks, worst |f0 / f - 1| = {worst:.2e}")


def test_noise_is_unvoiced():
    sr = 16000
    x = (0.2 * np.random.default_rng(PC.SEED).standard_normal(sr)).astype(np.float32)
    out = P.pitch_host(x, sr, PC.prediction([(0, sr)], sr, sr))
    assert out["voiced_fraction"][0] == 0 and np.isnan(out["f0_mean"][0]) and out["aperiodicity"][0] > 0.5


def test_recordings_have_voiced_frames():
    """The first 5 s of each golden recording.  Recorded when the test was written: meerkat_5s.wav (16 kHz) 622 frames, 38 voiced,
    median f0 513.7 Hz; zebra_finch_g17y2U-f00007.wav (32 kHz) 1247 frames, 155 voiced, median f0 1397.5 Hz.  The tone and stack
    tests above measured 0.0078 / 0.0078 (tones, 16 / 32 kHz) and 6.8e-4 / 5.6e-4 (stacks) as their worst errors."""
    from whisperseg_amd.wavio import load_wav
    for name in ("meerkat_5s.wav", "zebra_finch_g17y2U-f00007.wav"):
        x, sr = load_wav(os.path.join(GOLDEN, name))
        x = x[:5 * sr]
        out = P.pitch_host(x, sr, PC.prediction([(0, len(x))], sr, len(x)), contour=True)
        f0 = out["f0_contour"][0]
        voiced = f0[np.isfinite(f0)]
        print(f"{name}: sr={sr}, {len(f0)} frames, {len(voiced)} voiced, median f0 {np.median(voiced):.1f} Hz")
        assert len(voiced) >= 10 and 2 * sr / get_n_fft_given_sr(sr) <= np.median(voiced) <= sr / 8
