"""whisperseg_amd/measure.py on the host: the definition's known answers and conventions, the host plan of the device path
(wseg_measure_scratch_bytes: no device needed), the CLI's --measure and that measure=False leaves everything as it was."""
import inspect
import io
import math
import os
import sys

import numpy as np
import pytest

import measure_cases as MC
from conftest import ROOT
from whisperseg_amd import measure as M
from whisperseg_amd.audio_utils import get_n_fft_given_sr



@pytest.fixture(scope="module", autouse=True)
def library():
    """The plan tests reach the host arithmetic through libwseg (no device): built here if it is not yet (a no-op otherwise)."""
    from whisperseg_amd import build
    build.build(verbose=False)


def one(x, sr, s0, s1, **kw):
    """measure_host of one segment given in samples -> {column: float}."""
    got = M.measure_host(x, sr, MC.prediction([(s0, s1)], sr, len(x)), **kw)
    assert tuple(got) == M.COLUMNS and all(v.dtype == np.float32 and v.shape == (1,) for v in got.values())
    return {k: v[0] for k, v in got.items()}


def test_columns_and_ladder():
    assert M.COLUMNS == ("peak_amplitude", "rms", "zero_crossing_rate", "peak_frequency", "centroid_frequency", "freq_05", "freq_95",
                         "spectral_entropy")
    assert [get_n_fft_given_sr(sr) for sr in MC.RATES] == [512, 1024, 2048, 4096, 8192]
    from oracle.frontend import hann_periodic
    assert np.array_equal(M.hann_periodic(512), hann_periodic(512))


@pytest.mark.parametrize("sr", MC.RATES)
def test_a_tone_at_a_bin_centre(sr):
    n_fft = get_n_fft_given_sr(sr)
    for k in (3, n_fft // 8 + 1, n_fft // 2 - 5):
        x = MC.tone(sr, k, 6 * n_fft)
        got = one(x, sr, 17, 17 + 4 * n_fft + 123)
        assert got["peak_frequency"] == np.float32(k * sr / n_fft)
        assert abs(got["centroid_frequency"] - k * sr / n_fft) <= 0.5 * sr / n_fft
        assert got["freq_05"] < got["centroid_frequency"] < got["freq_95"]
        assert got["spectral_entropy"] < 0.2


def test_white_noise_in_a_band():
    sr, n_fft = 48000, 1024
    x = MC.white_noise(sr // 2)
    lo, hi = 6000, 18000
    got = one(x, sr, 1, len(x) - 1, min_frequency=lo, max_frequency=hi)
    k_lo, k_hi = M.band_bins(sr, n_fft, lo, hi)
    assert (k_lo, k_hi) == (128, 384)
    few = 4 * sr / n_fft
    assert got["spectral_entropy"] > 0.9
    assert abs(got["freq_05"] - (lo + 0.05 * (hi - lo))) <= few and abs(got["freq_95"] - (lo + 0.95 * (hi - lo))) <= few
    assert abs(got["centroid_frequency"] - 0.5 * (lo + hi)) <= few
    assert lo <= got["peak_frequency"] <= hi


def test_time_domain_columns():
    sr = 16000
    period = 10                                                         # samples: a sign change every 5
    x = np.where((np.arange(4000) // (period // 2)) % 2 == 0, 0.25, -0.75).astype(np.float32)
    s0, s1 = 1003, 3003                                                 # 2000 samples: pairs (i - 1, i) for i in (s0, s1)
    got = one(x, sr, s0, s1)
    crossings = sum(1 for i in range(s0 + 1, s1) if (x[i] < 0) != (x[i - 1] < 0))
    assert crossings == len([i for i in range(s0 + 1, s1) if i % 5 == 0]) == 400
    assert got["zero_crossing_rate"] == np.float32(crossings / ((s1 - s0) / sr))
    assert got["peak_amplitude"] == np.float32(0.75)
    y = MC.chirps(sr, sr)
    got = one(y, sr, 101, 9000)
    seg = y[101:9000]
    assert got["peak_amplitude"].tobytes() == np.abs(seg).max().tobytes()
    assert got["rms"] == np.float32(np.sqrt(np.mean(seg.astype(np.float64) ** 2)))
    # x[s0 - 1] is never looked at: a sign change in front of the segment is not counted
    z = np.array([-1, 1, 1, -1, -1], np.float32)
    assert one(z, sr, 1, 5)["zero_crossing_rate"] == np.float32(1 / (4 / sr))


def test_sample_bounds():
    sb = M.sample_bounds
    assert sb(0.0, 1.0, 16000, 20000) == (0, 16000)
    assert sb(2.5 / 16000, 3.49 / 16000, 16000, 100) == (3, 3)           # floor(x + 0.5): 2.5 -> 3, 3.49 -> 3
    assert sb(1.4999 / 16000, 7.5 / 16000, 16000, 100) == (1, 8)
    assert sb(-1.0, 0.5, 1000, 100) == (0, 100)                          # clamped at 0 and at n
    assert sb(0.2, 5.0, 1000, 100) == (100, 100)
    assert sb(0.05, 0.02, 1000, 100) == (50, 50)                         # offset < onset: empty at the onset
    assert M.frame_count(0, 512) == 0 and M.frame_count(1, 512) == M.frame_count(512, 512) == 1
    assert M.frame_count(513, 512) == 2 and M.frame_count(640, 512) == 2 and M.frame_count(641, 512) == 3


def test_conventions():
    sr = 16000
    x = MC.recording(sr)
    pred = MC.prediction([(500, 500), (int(MC.SILENT[0] * sr) + 3, int(MC.SILENT[0] * sr) + 300), (901, 902), (100, 2000)], sr, len(x))
    x[901] = 0.5
    got = M.measure_host(x, sr, pred)
    rows = np.stack([got[c] for c in M.COLUMNS], axis=1)
    assert np.isnan(rows[0]).all()                                       # empty: eight NaN
    assert np.isnan(rows[1, 3:]).all() and list(rows[1, :3]) == [0, 0, 0]        # silence
    assert np.isnan(rows[2, 3:]).all() and list(rows[2, :3]) == [0.5, 0.5, 0]    # one sample: w[0] = 0
    assert np.isfinite(rows[3]).all()
    with pytest.raises(ValueError, match="k_lo"):
        M.measure_host(x, sr, pred, min_frequency=7000, max_frequency=6000)
    with pytest.raises(ValueError):
        M.measure_host(x, sr, pred, min_frequency=7990, max_frequency=7995)      # no bin centre inside
    assert all(len(v) == 0 and v.dtype == np.float32 for v in M.measure_host(x, sr, {"onset": [], "offset": []}).values())
    quiet = M.measure_host(MC.silence(4000), sr, MC.prediction([(0, 4000), (7, 2000)], sr, 4000))
    assert all(np.isnan(quiet[c]).all() for c in M.COLUMNS[3:]) and all((quiet[c] == 0).all() for c in M.COLUMNS[:3])


def test_band_arithmetic():
    assert M.band_bins(16000, 512) == (1, 256)                           # min_frequency 0: DC is never in the band
    assert M.band_bins(16000, 512, 0, 1e9) == (1, 256)                   # max_frequency above sr / 2 is clipped
    assert M.band_bins(16000, 512, 31.25, 62.5) == (1, 2)
    assert M.band_bins(250000, 4096, 35000) == (math.ceil(35000 * 4096 / 250000), 2048)
    with pytest.raises(ValueError):
        M.band_bins(16000, 512, 31.26, 62.49)                            # ceil -> 2, floor -> 1


def brute_chunks(length, n_fft):
    """Frames counted one by one: frame j exists if it is the first one or the frame before it did not reach the segment's end."""
    if length == 0:
        return 0
    hop, j = n_fft // 4, 1
    while (j - 1) * hop + n_fft < length:
        j += 1
    return -(-j // M.CHUNK_FRAMES)


@pytest.mark.parametrize("n_fft", [512, 1024, 2048, 4096, 8192])
def test_plan_against_a_brute_force_count(n_fft):
    """wseg_measure_scratch_bytes is host arithmetic: (3 n_seg + 1) int64 padded to 256 bytes, then n_fft / 2 + 4 doubles a chunk."""
    hop = n_fft // 4
    table = lambda n_seg: -(-(3 * n_seg + 1) * 8 // 256) * 256
    chunk = (n_fft // 2 + 4) * 8
    lengths = [0, 1, 7]
    for centre in (n_fft, n_fft + hop, 64 * hop + n_fft - hop, 128 * hop + n_fft - hop):
        lengths += [centre - 1, centre, centre + 1]
    for length in lengths:
        assert M.scratch_bytes([(5, 5 + length)], n_fft) == table(1) + brute_chunks(length, n_fft) * chunk, length
        assert M.frame_count(length, n_fft) <= brute_chunks(length, n_fft) * M.CHUNK_FRAMES
    bounds = [(3 * i, 3 * i + length) for i, length in enumerate(lengths)]
    assert M.scratch_bytes(bounds, n_fft) == table(len(bounds)) + sum(brute_chunks(v, n_fft) for v in lengths) * chunk
    assert brute_chunks(64 * hop + n_fft - hop, n_fft) == 1 and brute_chunks(64 * hop + n_fft - hop + 1, n_fft) == 2
    big = 1 << 40                                                        # frames
    assert M.scratch_bytes([(0, n_fft + (big - 1) * hop)], n_fft) == table(1) + (big // 64) * chunk


def test_plan_rejects_invalid_input():
    from whisperseg_amd import _lib
    lib = _lib.load()
    for bounds, n_fft, word in (([(5, 4)], 512, "bounds"), ([(-1, 4)], 512, "bounds"), ([(0, 4)], 768, "n_fft"), ([(0, 4)], 256, "n_fft"),
                                ([(0, (1 << 52) + 1)], 512, "bounds"), ([(0, 1 << 48)] * 200, 512, "chunks")):
        with pytest.raises(_lib.WsegError, match=word):
            M.scratch_bytes(bounds, n_fft)
    assert lib.wseg_measure_scratch_bytes(None, -1, 512) == 0 and b"n_seg" in lib.wseg_last_error()
    assert lib.wseg_measure_scratch_bytes(None, 0, 512) == 256           # no segments: the one-entry table, no error
    # the launch entry point validates on the host too, before it touches a device: band, bounds against n, scratch
    b = np.array([[0, 600]], np.int64)
    call = lambda n, k_lo, k_hi, scratch_bytes: lib.wseg_measure_segments_f32(None, n, b.ctypes.data, 1, 512, k_lo, k_hi, None, None, None,
                                                                              scratch_bytes, None, None)
    assert call(599, 1, 256, 0) != 0 and b"bounds" in lib.wseg_last_error()
    assert call(600, 0, 256, 0) != 0 and b"k_lo" in lib.wseg_last_error()
    assert call(600, 5, 4, 0) != 0 and b"k_lo" in lib.wseg_last_error()
    assert call(600, 1, 257, 0) != 0 and b"k_hi" in lib.wseg_last_error()
    assert call(-1, 1, 256, 0) != 0
    assert lib.wseg_measure_segments_f32(None, 0, None, 0, 512, 1, 256, None, None, None, 0, None, None) == 0      # n_seg == 0: nothing to do


def test_tolerance_constants_are_the_measured_spread():
    """The constants the device tests multiply by four are what the float32 run of the definition gives on this host (same order
    of magnitude: pocketfft's vector width differs between CPUs), and that run never moves a peak bin."""
    for sr in MC.RATES:
        *cols, power, moved = MC.fp32_spread(sr)
        print(sr, cols, power, moved)
        assert moved == 0
        assert power <= 2 * MC.POWER_SPREAD
        for got, const in zip(cols, MC.SPREAD[get_n_fft_given_sr(sr)]):
            assert const / 4 <= got <= 2 * const, (sr, got, const)


def cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    return segment


def test_cli_flag_and_header():
    segment = cli()
    p = segment.build_parser()
    assert p.parse_args(["--model_path", "m", "--csv_save_path", "o.csv"]).measure is False
    assert p.parse_args(["--model_path", "m", "--csv_save_path", "o.csv", "--measure"]).measure is True
    plain = {"onset": [0.5, 1.25], "offset": [0.75, 1.5], "cluster": ["a", "b"]}
    cols = {name: np.array([i + 0.5, i + 0.25], np.float32) for i, name in enumerate(M.COLUMNS)}
    full = M.with_columns(plain, cols)
    assert set(plain) == {"onset", "offset", "cluster"} and list(full)[:3] == ["onset", "offset", "cluster"] and list(full)[3:] == list(M.COLUMNS)
    assert all(isinstance(v, list) and len(v) == 2 and isinstance(v[0], float) for k, v in full.items() if k in M.COLUMNS)
    columns, rows = segment.table([full], ["a.wav"], measure=True)
    assert columns == ["filename", "onset", "offset", "cluster"] + list(M.COLUMNS)
    assert rows[1] == ("a.wav", 1.25, 1.5, "b") + tuple(i + 0.25 for i in range(8))
    # without the flag the text is what it was, whether or not the dicts carry the columns
    before, after, with_flag = io.StringIO(), io.StringIO(), io.StringIO()
    segment.write_csv(*segment.table([plain], ["a.wav"]), before)
    segment.write_csv(*segment.table([full], ["a.wav"]), after)
    segment.write_csv(columns, rows, with_flag)
    assert before.getvalue() == after.getvalue() == "filename,onset,offset,cluster\na.wav,0.5,0.75,a\na.wav,1.25,1.5,b\n"
    assert with_flag.getvalue().splitlines()[0] == "filename,onset,offset,cluster," + ",".join(M.COLUMNS)
    assert with_flag.getvalue().splitlines()[1].startswith("a.wav,0.5,0.75,a,0.5,1.5,2.5,")


def test_keyword_off_changes_nothing():
    """measure defaults to False everywhere; with it off, segment() hands get_sliced_audios_features the arguments it always did
    (a subclass with the old signature keeps working) and returns exactly the three keys; the distributed entry points refuse it."""
    from whisperseg_amd import dist, model, postprocess
    for fn in (model.SegmenterBase.segment, model.SegmenterBase.segment_batch):
        assert inspect.signature(fn).parameters["measure"].default is False

    class Stub(model.SegmenterBase):
        def get_sliced_audios_features(self, audio, sr, min_frequency, spec_time_step, num_trials):      # the signature before the keyword
            return [(0, 0.0, None, 1.0)]

        def generate_segment_text(self, sliced, *args, **kwargs):
            return ["text"] * len(sliced)

        def parse_generation(self, texts, sliced, *args):
            return {"onset": [0.1, 0.1, 0.4], "offset": [0.2, 0.2, 0.6], "cluster": ["a", "a", "b"]}

    stub = Stub()
    raw = stub.parse_generation(None, None)
    want = postprocess.drop_consecutive_duplicates(postprocess.correct_fft_blur(dict(raw), 512, 16000))
    got = stub.segment(np.zeros(16000, np.float32), 16000)
    assert got == want and set(got) == {"onset", "offset", "cluster"}
    assert stub.segment_batch([np.zeros(16000, np.float32)], 16000) == [want]
    assert stub.segment_channels(np.zeros((2, 16000), np.float32), 16000) == [want, want]
    for fn, args in ((dist.segment_distributed, (stub, None, 16000)), (dist.segment_batch_distributed, (stub, [], 16000))):
        with pytest.raises(ValueError, match="measure"):
            fn(*args, measure=True)
