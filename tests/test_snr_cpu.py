"""The signal-to-noise definition (whisperseg_amd/snr.py) on the host: the frame ranges against a plainly written second
statement, known answers of snr_host, the conventions of a zero floor, the rank against numpy's quantile, the tolerance constants of
the device tests and the CLI's flags.  No GPU."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import measure_cases as MC
import snr_cases as SC
from conftest import ROOT
from whisperseg_amd import snr as S
from whisperseg_amd.audio_utils import get_n_fft_given_sr


# ---- frame ranges -------------------------------------------------------------------------------------------------------------------
def ranges_plain(s0, s1, n, n_fft, context_samples, q):
    """The definition once more, by looking at every frame: (j0, j1, w0, w1, r), or None where the recording has no frame."""
    hop = n_fft // 4
    starts = [t for t in range(0, n, hop) if t + n_fft <= n]
    if not starts:
        return None
    inside = [j for j, t in enumerate(starts) if s0 <= t and t + n_fft <= s1]
    if not inside:
        centre = (s0 + s1) // 2
        best = None
        for j, t in enumerate(starts):                       # the nearest frame centre; of two equally near ones the later
            d = abs(t + n_fft // 2 - centre)
            if best is None or d <= best[0]:
                best = (d, j)
        inside = [best[1]]
    j0, j1 = inside[0], inside[-1] + 1
    if context_samples is None:
        window = list(range(len(starts)))
    else:
        c = 0
        while c * hop < context_samples:
            c += 1
        window = [j for j in range(len(starts)) if j0 - c <= j < j1 + c]
    length = len(window)
    r = 0
    while r + 1 <= length - 1 and r + 1 <= q * (length - 1):
        r += 1
    return j0, j1, window[0], window[-1] + 1, r


@pytest.mark.parametrize("sr", (16000, 96000))
def test_frame_ranges_against_a_plain_loop(sr):
    n_fft = get_n_fft_given_sr(sr)
    hop = n_fft // 4
    rng = np.random.default_rng(SC.SEED + sr)
    for n in (n_fft - 1, n_fft, n_fft + hop - 1, n_fft + hop, n_fft + 9 * hop + 5):
        rows = [(0, 0), (0, 1), (0, min(n, hop)), (0, n), (n, n), (n - 1, n), (max(0, n - n_fft), n), (max(0, n - n_fft - 1), n),
                (n // 2, n // 2), (n // 2, n // 2 + 3), (hop, min(n, hop + n_fft)), (hop - 1, min(n, hop + n_fft)),
                (min(n, hop + 1), min(n, hop + n_fft + 1)), (1, max(1, n - 1))]
        for _ in range(40):
            a, b = sorted(int(v) for v in rng.integers(0, n + 1, 2))
            rows.append((a, b))
            rows.append((a, min(n, a + int(rng.integers(0, n_fft)))))          # shorter than a frame
        bounds = np.asarray(rows, dtype=np.int64)
        for q in (0.0, 0.1, 0.5, 1.0):
            for context in (None, 0.0, 1.5 * hop / sr, 3 * hop / sr, 0.05):
                table, windows = S.frame_ranges(bounds, n, n_fft, sr, q, context)
                assert table.dtype == windows.dtype == np.int64 and table.shape == (len(rows), 3)
                samples = None if context is None else int(np.floor(context * sr + 0.5))
                for (s0, s1), (j0, j1, w) in zip(rows, table):
                    want = ranges_plain(s0, s1, n, n_fft, samples, q)
                    if want is None:
                        assert len(windows) == 0 and (j0, j1, w) == (0, 0, 0)
                    else:
                        assert (j0, j1, *windows[w]) == want, (n, s0, s1, q, context)
                if context is None and len(windows):
                    assert len(windows) == 1                                    # one window for the whole recording


def test_frame_count_and_whole_frames_only():
    for sr in SC.RATES:
        n_fft = get_n_fft_given_sr(sr)
        hop = n_fft // 4
        assert [S.frame_count(n, n_fft) for n in (0, n_fft - 1, n_fft, n_fft + hop - 1, n_fft + hop)] == [0, 0, 1, 1, 2]
    x = SC.recording(16000)[:512 + 128 + 100]
    poisoned = np.concatenate([x, np.full(512, np.nan, np.float32)])
    assert np.array_equal(S.frame_energy_host(x, 16000), S.frame_energy_host(poisoned[:len(x)], 16000))
    assert len(S.frame_energy_host(x, 16000)) == 2 and len(S.frame_energy_host(x[:511], 16000)) == 0


# ---- known answers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", SC.RATES)
def test_a_full_scale_sine_is_zero_db(sr):
    n_fft = get_n_fft_given_sr(sr)
    n = 12 * n_fft
    pred = MC.prediction([(n_fft, 9 * n_fft)], sr, n)
    for amplitude, want in ((1.0, 0.0), (0.5, 20 * np.log10(0.5))):
        got = S.snr_host(MC.tone(sr, n_fft // 8, n, amplitude), sr, pred, min_frequency=500)
        assert abs(got["signal_level_db"][0] - want) < 0.01 and abs(want - (0.0 if amplitude == 1.0 else -6.02)) < 0.01
        assert abs(got["snr_db"][0]) < 0.01 and abs(got["peak_snr_db"][0]) < 0.01           # the tone is its own floor


def test_the_floor_follows_the_noise():
    sr, n = 16000, 32000
    tone = MC.tone(sr, 64, n, 0.5).astype(np.float64)
    tone[:20000] = 0.0                                       # the call: the last 12 000 samples
    noise = np.random.default_rng(SC.SEED).standard_normal(n)
    pred = MC.prediction([(20480, 31000)], sr, n)
    levels = [S.snr_host((tone + a * noise).astype(np.float32), sr, pred) for a in (1e-4, 1e-3, 1e-2)]
    for low, high in zip(levels, levels[1:]):
        assert abs((high["noise_level_db"][0] - low["noise_level_db"][0]) - 20.0) < 0.01
        assert abs((low["snr_db"][0] - high["snr_db"][0]) - 20.0) < 0.05          # (the noise adds a little to S as well)
    assert abs(levels[0]["signal_level_db"][0] - 20 * np.log10(0.5)) < 0.01
    assert levels[1]["peak_snr_db"][0] >= levels[1]["snr_db"][0] > 40


def test_conventions_of_a_zero_floor_and_of_empty_rows():
    sr, n = 16000, 16000
    x = np.zeros(n, np.float32)
    x[12000:14000] = MC.tone(sr, 40, 2000, 0.25)
    pred = MC.prediction([(12000, 14000), (2000, 4000), (5000, 5000)], sr, n)
    got = S.snr_host(x, sr, pred)
    assert np.isneginf(got["noise_level_db"][:2]).all()                      # N == 0: log10(0)
    assert np.isposinf(got["snr_db"][0]) and np.isposinf(got["peak_snr_db"][0]) and np.isfinite(got["signal_level_db"][0])
    assert np.isneginf(got["signal_level_db"][1]) and np.isnan(got["snr_db"][1]) and np.isnan(got["peak_snr_db"][1])      # 0 / 0
    assert all(np.isnan(got[c][2]) for c in S.COLUMNS)                       # an empty row
    assert all(got[c].dtype == np.float32 and got[c].shape == (3,) for c in S.COLUMNS) and list(got) == list(S.COLUMNS)
    short = S.snr_host(x[:300], sr, MC.prediction([(0, 300)], sr, 300))       # J == 0
    assert all(np.isnan(short[c][0]) for c in S.COLUMNS)
    kept = S.snr_host(x, sr, pred, track=True)
    assert list(kept) == list(S.COLUMNS) + list(S.TRACK_KEYS) and kept["hop"] == 128 and kept["n_fft"] == 512
    assert np.array_equal(kept["frame_energy"], S.frame_energy_host(x, sr)) and kept["frame_energy"].dtype == np.float32
    # a NaN frame sorts last: the floor of a window with few NaN frames stays a number
    bad = SC.recording(sr).copy()
    bad[100] = np.nan
    got = S.snr_host(bad, sr, MC.prediction([(8000, 9000)], sr, n))
    assert np.isfinite(got["noise_level_db"][0]) and np.isfinite(got["snr_db"][0])
    for kw in (dict(quantile=-0.1), dict(quantile=1.5), dict(quantile=None), dict(context=-1.0), dict(context=float("inf")),
               dict(min_frequency=9000)):
        with pytest.raises(ValueError):
            S.snr_host(x, sr, pred, **kw)
    for bad in ("yes", {"hop": 3}, {"quantile": 2}, {"context": -1}, {"max_frequency": 0}):
        with pytest.raises(ValueError):
            S.options(bad)
    assert S.options(True) == {} and S.options({"quantile": 0.5, "track": True}) == {"quantile": 0.5, "track": True}
    with pytest.raises(ValueError):
        S.options({"max_frequency": 10.0}, 16000, 0)                          # no bin below 10 Hz


def test_the_rank_is_numpys_lower_quantile():
    rng = np.random.default_rng(SC.SEED + 1)
    for J in (1, 2, 3, 257):
        track = (rng.standard_normal(J) ** 2).astype(np.float32)
        for q in (0.0, 0.1, 0.25, 0.5, 0.9, 0.999, 1.0):
            table = np.array([[0, 1, 0]], np.int64)
            windows = np.array([[0, J, SC.rank(q, J)]], np.int64)
            assert S.rows_host(track, table, windows)[0, 2] == np.quantile(track, q, method="lower"), (J, q)
            _, made = S.frame_ranges([(0, 512)], 512 + 128 * (J - 1), 512, 16000, q, None)
            assert made.tolist() == windows.tolist()


# ---- the tolerances of the device tests ---------------------------------------------------------------------------------------------
def test_tolerance_constants_are_the_measured_spread():
    for sr in SC.RATES:
        got = SC.fp32_spread(sr)
        print(sr, got)
        assert SC.FP32_SPREAD[sr] / 4 <= got <= 2 * SC.FP32_SPREAD[sr], (sr, got)


def test_the_intervals_are_narrow_on_noise_only_frames():
    """Rows inside the zeroed stretch of the recording hold the white-noise floor alone; so do the frames the 10 % quantile falls
    on.  In the full band and in the band from 500 Hz the interval of their level is narrower than 0.01 dB."""
    for sr in SC.RATES:
        lo_s, hi_s = int(MC.SILENT[0] * sr), int(MC.SILENT[1] * sr)
        bounds = np.array([(lo_s, hi_s), (lo_s + 3, hi_s - 5)], np.int64)
        for band in (0, 1):
            for context in (None, 0.2):
                lo, hi = SC.column_intervals(sr, band, bounds, 0.1, context)
                for c in ("signal_level_db", "noise_level_db"):
                    print(sr, band, context, c, (hi[c] - lo[c]).max())
                    assert np.isfinite(lo[c]).all() and ((hi[c] - lo[c]) < 0.01).all(), (sr, band, c)
                want = S.snr_host(SC.recording(sr), sr, MC.prediction(bounds, sr, sr), *SC.bands(sr)[band], 0.1, context)
                assert all(((lo[c] <= want[c]) & (want[c] <= hi[c])).all() for c in S.COLUMNS)      # the definition lies inside


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    return segment


def test_cli_flags(capsys):
    segment = cli()
    base = ["--model_path", "m", "--audio_path", "a.wav", "--csv_save_path", "o.csv"]
    args = segment.parse_args(base)
    assert args.snr is False and segment.snr_keyword(args) is None
    assert segment.snr_keyword(segment.parse_args(base + ["--snr"])) is True
    assert segment.snr_keyword(segment.parse_args(base + ["--snr", "--snr_quantile", "0.25", "--snr_context", "2"])) == {"quantile": 0.25, "context": 2.0}
    assert segment.snr_keyword(segment.parse_args(base + ["--snr", "--snr_save_path", "t.npz"])) == {"track": True}
    for bad, word in ((["--snr_quantile", "0.2"], "needs --snr"), (["--snr_context", "1"], "needs --snr"), (["--snr_save_path", "t.npz"], "needs --snr"),
                      (["--snr", "--snr_quantile", "1.5"], "[0, 1]"), (["--snr", "--snr_quantile", "-0.1"], "[0, 1]"),
                      (["--snr", "--snr_context", "-1"], "non-negative"), (["--snr", "--snr_context", "inf"], "non-negative"),
                      (["--snr", "--snr_save_path", "t.npy"], ".npz")):
        with pytest.raises(SystemExit):
            segment.parse_args(base + bad)
        assert word in capsys.readouterr().err, bad


def test_cli_table_and_archive():
    segment = cli()
    from whisperseg_amd.measure import COLUMNS as MEASURE
    from whisperseg_amd.pitch import COLUMNS as PITCH
    res = {"onset": [0.5, 1.25], "offset": [0.75, 1.5], "cluster": ["a", "b"]}
    plain = io.StringIO()
    segment.write_csv(*segment.table([res]), plain)
    assert plain.getvalue() == "onset,offset,cluster\n0.5,0.75,a\n1.25,1.5,b\n"          # without the flag: what it was
    full = dict(res, **{c: [1.0, 2.0] for c in MEASURE + PITCH + S.COLUMNS}, frame_energy=np.arange(3, dtype=np.float32), hop=128, n_fft=512)
    columns, rows = segment.table([full], measure=True, pitch=True, snr=True)
    assert columns == ["onset", "offset", "cluster"] + list(MEASURE) + list(PITCH) + list(S.COLUMNS) and len(rows) == 2
    columns, _ = segment.table([[full, full]], names=["f.wav"], all_channels=True, snr=True)
    assert columns == ["filename", "channel", "onset", "offset", "cluster"] + list(S.COLUMNS)
    saved = segment.snr_archive([[full, dict(full, frame_energy=np.zeros(0, np.float32))]], all_channels=True)
    assert saved["frame_energy"].tolist() == [0.0, 1.0, 2.0] and saved["frame_offsets"].tolist() == [0, 3, 3]
    assert saved["hop"].tolist() == [128, 128] and saved["n_fft"].tolist() == [512, 512] and saved["frame_offsets"].dtype == np.int64


# ---- the plan -----------------------------------------------------------------------------------------------------------------------
def test_plan_check_program_under_the_sanitizer(tmp_path):
    """tools/snr_plan_check.cpp sweeps the plan over the limits; built with -fsanitize=undefined it must exit 0 and print ok."""
    exe = tmp_path / "snr_plan_check"
    subprocess.run(["c++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "snr_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_the_split_constant_is_the_plans():
    with open(os.path.join(ROOT, "whisperseg_amd", "csrc", "wseg_snr_plan.h")) as f:
        assert f"constexpr int kSnrSplit = {S.SPLIT};" in f.read()


def test_host_queries_need_no_device():
    from whisperseg_amd import _lib
    lib = _lib.load()
    assert [lib.wseg_frame_energy_frames(n, 512) for n in (0, 511, 512, 639, 640)] == [0, 0, 1, 1, 2]
    assert lib.wseg_frame_energy_frames(1000, 500) == -1 and b"n_fft" in lib.wseg_last_error()
    table, windows = np.array([[0, 2, 0], [1, 3, 1], [2, 2, 0]], np.int64), np.array([[0, 5, 2], [0, 5, 2]], np.int64)
    assert S.scratch_bytes(5, table, windows) % 256 == 0
    for t, w, word in ((table, [[0, 5, 5]], "rank"), (table, [[0, 5, -1]], "rank"), (table, [[3, 3, 0]], "rank"), (table, [[0, 6, 0]], "windows"),
                       ([[0, 6, 0]], windows, "bounds"), ([[2, 1, 0]], windows, "bounds"), ([[0, 1, 2]], windows, "window of row")):
        with pytest.raises(_lib.WsegError, match=word):
            S.scratch_bytes(5, t, w)
