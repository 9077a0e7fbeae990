"""whisperseg_amd/patches.py on the host: the definition against the reference-pinned oracle front-end, its known answers and
conventions, the tolerance constants of the device tests, the host plan of the device path (wseg_patches_scratch_bytes and the
validation of wseg_patches_f32: no device needed), the CLI's flags and that patches=None leaves everything as it was."""
import inspect
import os
import sys

import numpy as np
import pytest

import measure_cases as MC
import patch_cases as PC
from conftest import ROOT
from whisperseg_amd import patches as P
from whisperseg_amd.audio_utils import get_n_fft_given_sr


@pytest.fixture(scope="module", autouse=True)
def library():
    """The plan tests reach the host arithmetic through libwseg (no device): built here if it is not yet (a no-op otherwise)."""
    from whisperseg_amd import build
    build.build(verbose=False)


def one(x, sr, s0, s1, width, **kw):
    got = P.patches_host(x, sr, MC.prediction([(s0, s1)], sr, len(x)), width=width, **kw)
    assert got.dtype == np.float32 and got.shape == (1, 80, width)
    return got[0]


@pytest.mark.parametrize("sr,hop,first,width", [(16000, 40, 100, 32), (48000, 96, 200, 16)])
def test_definition_against_the_oracle_front_end(sr, hop, first, width):
    """Column centres laid on the oracle's frame grid: s0 = first hop - hop / 2, L = width hop gives t_c = (first + c) hop, the
    centres of the oracle's reflect-centred frames first .. first + width - 1, far from the window's ends (where the oracle
    reflects and the definition pads with zeros).  Un-normalised, 4 ref - 4 is the oracle's log10 mel on every entry above its
    window clamp; the two must agree within 2e-6: the oracle's complex64 spectrum costs <= 1.1e-7, its float32 log10 <= 4.8e-7 at
    |v| < 8, its float32 normalised value times 4 another <= 4.8e-7 — 1.1e-6 together, and headroom below 2x."""
    from oracle.frontend import logmel_window
    x = MC.recording(sr)
    n_fft = get_n_fft_given_sr(sr)
    ref = logmel_window(x, sr, hop / sr)
    assert first * hop > n_fft and (first + width) * hop < len(x) - n_fft
    s0, length = first * hop - hop // 2, width * hop
    centres = P.column_centres(s0, s0 + length, width)
    assert np.array_equal(centres, (first + np.arange(width)) * hop)
    v = P.log_mel_columns(x, centres, n_fft, P.filterbank(sr, n_fft))
    window = ref[:, first:first + width].astype(np.float64)
    above = window > ref.max() - 2.0 + 1e-6                      # strictly above the oracle's clamp (max - 8, normalised: max - 2)
    assert above.mean() >= 0.9, above.mean()
    err = np.abs(4.0 * window - 4.0 - v)[above]
    print(f"sr={sr}: {above.sum()} of {above.size} entries compared, largest difference {err.max():.3g} (allowed 2e-6)")
    assert err.max() <= 2e-6
    assert np.array_equal(one(x, sr, s0, s0 + length, width), P.normalise(v))


@pytest.mark.parametrize("sr", PC.RATES)
def test_a_tone_at_a_bin_centre(sr):
    """Every column has its largest row at a filter whose triangle contains the tone's bin."""
    n_fft = get_n_fft_given_sr(sr)
    fb = P.filterbank(sr, n_fft)
    for k in (n_fft // 8 + 1, n_fft // 2 - 5):
        x = MC.tone(sr, k, 6 * n_fft)
        patch = one(x, sr, n_fft + 17, 4 * n_fft + 140, 7)
        assert (fb[k, patch.argmax(axis=0)] > 0).all(), (sr, k, patch.argmax(axis=0))


def test_shapes_and_edge_cases():
    sr, n_fft = 16000, 512
    x = MC.recording(sr)
    # L == 0: every column is the one frame centred on s0
    flat = one(x, sr, 3000, 3000, 6)
    assert (flat == flat[:, :1]).all() and np.isfinite(flat).all() and flat.max() > 0
    # L < W: columns share centres as the integers fall
    assert list(P.column_centres(50, 53, 6)) == [50, 50, 51, 51, 52, 52]
    assert list(P.column_centres(50, 50, 3)) == [50, 50, 50] and list(P.column_centres(0, 8, 2)) == [2, 6]
    # silence: -1.5 everywhere, a frame that reaches outside the recording included
    assert (P.patches_host(MC.silence(300), sr, MC.prediction([(0, 300), (7, 7)], sr, 300), width=4) == -1.5).all()
    quiet = int(MC.SILENT[0] * sr) + n_fft // 2
    assert (one(x, sr, quiet + 1, quiet + 200, 5) == -1.5).all()
    # a filter that holds no bin sits at the floor: from 0 Hz to sr / 2 the bank has none (every filter spans two bins or more), in
    # the band 0 .. 1000 Hz the filters are narrower than a bin and many are empty
    assert (P.filterbank(sr, n_fft).sum(axis=0) > 0).all()
    fb = P.filterbank(sr, n_fft, *PC.NARROW_BAND)
    empty = np.flatnonzero(fb.sum(axis=0) == 0)
    assert 10 <= len(empty) < 80
    s0, s1, width = 4001, 9000, 8
    v = P.log_mel_columns(x, P.column_centres(s0, s1, width), n_fft, fb)
    floor = np.float32((max(-10.0, v.max() - 8.0) + 4.0) / 4.0)
    narrow = dict(zip(("min_frequency", "max_frequency"), PC.NARROW_BAND))
    assert (one(x, sr, s0, s1, width, **narrow)[empty] == floor).all() and v.max() > -2
    # frames reach outside the recording on both sides and read zeros there: no NaN, and a recording shorter than a frame works
    short = PC.short_recording(sr)
    got = P.patches_host(short, sr, MC.prediction(PC.short_rows(), sr, len(short)), width=5)
    assert got.shape == (len(PC.short_rows()), 80, 5) and np.isfinite(got).all()
    # no rows
    none = P.patches_host(x, sr, {"onset": [], "offset": []}, width=9)
    assert none.shape == (0, 80, 9) and none.dtype == np.float32
    # what is refused before anything runs
    pred = MC.prediction([(10, 900)], sr, len(x))
    for width in (0, 257, -1, 2.5, None):
        with pytest.raises(ValueError, match="width"):
            P.patches_host(x, sr, pred, width=width)
    with pytest.raises(ValueError, match="k_lo"):
        P.patches_host(x, sr, pred, min_frequency=7000, max_frequency=6000)
    with pytest.raises(ValueError):
        P.patches_host(x, sr, pred, min_frequency=7990, max_frequency=7995)       # no bin centre inside
    with pytest.raises(ValueError, match="mono"):
        P.patches_host(np.zeros((2, 100), np.float32), sr, pred)
    # the float32 yardstick keeps the transform in single precision (the assertion inside log_mel_columns) and stays close
    a, b = one(x, sr, s0, s1, 32), one(x, sr, s0, s1, 32, fft_dtype=np.float32)
    assert 0 < np.abs(a.astype(np.float64) - b).max() <= 2 * PC.SPREAD[n_fft]


@pytest.mark.parametrize("sr", PC.RATES)
def test_tolerance_constants_are_the_measured_spread(sr):
    """The constant the device tests multiply by four is at least what the float32 run of the definition costs on this host over
    exactly the cases they compare, and at most twice it."""
    got, const = PC.fp32_spread(sr), PC.SPREAD[get_n_fft_given_sr(sr)]
    print(f"sr={sr}: measured spread {got:.3g}, constant {const:.3g}")
    assert got <= const <= 2 * got, (sr, got, const)
    if sr == PC.BAND_RATE:
        got = PC.fp32_spread(sr, PC.narrow_cases())
        print(f"the narrow band: measured spread {got:.3g}, constant {PC.NARROW_SPREAD:.3g}")
        assert got <= PC.NARROW_SPREAD <= 2 * got


def test_the_cases_hold_what_they_promise():
    for sr in PC.RATES:
        n_fft = get_n_fft_given_sr(sr)
        for width in PC.widths(sr):
            rows = PC.rows_for(sr, width)
            lengths = set((rows[:, 1] - rows[:, 0]).tolist())
            assert {0, 1, width - 1, width, width + 1, 1001} <= lengths
            assert (rows[:, 0] >= 0).all() and (rows[:, 1] <= sr).all() and (rows[:, 0] <= rows[:, 1]).all()
            assert rows[:, 0].min() == 0 and rows[:, 1].max() == sr and any(s0 == sr for s0, _ in rows)
        assert PC.SHORT_N < n_fft
    assert PC.widths(16000)[-1] == PC.widths(400000)[-1] == 256 and 256 not in PC.widths(48000)


def test_plan_through_the_library():
    """wseg_patches_scratch_bytes is host arithmetic: (s0, s1) int64 pairs padded to 256 bytes, then one uint32 a segment padded to
    256 bytes; the launch entry point validates on the host, before it touches a device, and names the argument."""
    import ctypes as C
    from whisperseg_amd import _lib
    lib = _lib.load()
    pad = lambda b: max(256, -(-b // 256) * 256)
    for n_seg in (0, 1, 16, 17, 64, 65, 1000, 100000, 2 ** 31 - 1):
        assert P.scratch_bytes(n_seg, 80, 32) == pad(16 * n_seg) + pad(4 * n_seg), n_seg
    assert P.scratch_bytes(5, 1, 1) == P.scratch_bytes(5, 96, 256) == 512
    for args, word in (((-1, 80, 32), "n_seg"), ((1, 0, 32), "n_mels"), ((1, 97, 32), "n_mels"), ((1, 80, 0), "width"), ((1, 80, 257), "width")):
        with pytest.raises(_lib.WsegError, match=word):
            P.scratch_bytes(*args)
    b = np.array([[0, 600]], np.int64)

    def call(n_fft=512, n=600, n_seg=1, width=32, n_mels=80, desc=True, bounds=b):
        d = _lib.LogmelDesc(n_fft=n_fft, hop=1, n_mels=n_mels, n_cols=256)       # null tables: never reached by an invalid call
        return lib.wseg_patches_f32(C.byref(d) if desc else None, None, n, bounds.ctypes.data if bounds is not None else None, n_seg, width,
                                    None, 0, None, None)

    for kw, word in ((dict(n_fft=768), b"n_fft"), (dict(n_fft=256), b"n_fft"), (dict(n_seg=-1), b"n_seg"), (dict(n=599), b"bounds"),
                     (dict(width=0), b"width"), (dict(width=257), b"width"), (dict(n_mels=97), b"n_mels"), (dict(n=-1), b"n is"),
                     (dict(desc=False), b"d is"), (dict(bounds=None), b"bounds_host"), (dict(bounds=np.array([[5, 4]], np.int64)), b"bounds"),
                     (dict(bounds=np.array([[-1, 4]], np.int64)), b"bounds")):
        assert call(**kw) != 0 and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())
    assert call() != 0 and b"d must" in lib.wseg_last_error()                    # a valid plan, then the tables are missed
    assert call(n_seg=0, bounds=None) == 0                                       # n_seg == 0: nothing to do


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
    assert args.patches is None and args.patches_save_path is None
    args = segment.parse_args(base + ["--patches", "32", "--patches_save_path", "p.npz"])
    assert args.patches == 32 and args.patches_save_path == "p.npz"
    for extra in (["--patches", "32"], ["--patches_save_path", "p.npz"], ["--patches", "0", "--patches_save_path", "p.npz"],
                  ["--patches", "257", "--patches_save_path", "p.npz"], ["--patches", "8", "--patches_save_path", "p.txt"]):
        with pytest.raises(SystemExit) as e:
            segment.main(base + extra)                       # refused by argparse, before a model is looked for
        assert e.value.code == 2 and "patches" in capsys.readouterr().err
    # the archive follows the table's row order and carries the table's identifying columns
    a = {"onset": [0.5, 1.25], "offset": [0.75, 1.5], "cluster": ["a", "b"], "patch": np.arange(2 * 80 * 3, dtype=np.float32).reshape(2, 80, 3)}
    c = {"onset": [0.1], "offset": [0.2], "cluster": ["c"], "patch": -np.ones((1, 80, 3), np.float32)}
    arch = segment.patch_archive([[a, c], [c, a]], ["x.wav", "y.wav"], True)
    columns, rows = segment.table([[a, c], [c, a]], ["x.wav", "y.wav"], True)
    assert columns == ["filename", "channel", "onset", "offset", "cluster"] and set(arch) == set(columns) | {"patch"}
    assert [tuple(arch[k][i].item() for k in columns) for i in range(len(rows))] == rows
    assert arch["patch"].shape == (6, 80, 3) and np.array_equal(arch["patch"][2], c["patch"][0]) and np.array_equal(arch["patch"][4:], a["patch"])
    assert set(segment.patch_archive([a])) == {"patch", "onset", "offset", "cluster"}
    assert segment.patch_archive([], ["x.wav"][:0], width=7)["patch"].shape == (0, 80, 7)
    # the CSV is the table's, whether or not the dicts carry the pictures
    plain = {k: v for k, v in a.items() if k != "patch"}
    assert segment.table([a]) == segment.table([plain])


def test_keyword_off_changes_nothing():
    """patches defaults to None everywhere; with it absent, segment() hands get_sliced_audios_features the arguments it always did and
    returns exactly the three keys; a value that is no width is refused before any work; the distributed entry points refuse it."""
    from whisperseg_amd import dist, model, postprocess
    for fn in (model.SegmenterBase.segment, model.SegmenterBase.segment_batch):
        assert inspect.signature(fn).parameters["patches"].default is None

    class Stub(model.SegmenterBase):
        def get_sliced_audios_features(self, audio, sr, min_frequency, spec_time_step, num_trials):      # the signature before the keywords
            return [(0, 0.0, None, 1.0)]

        def generate_segment_text(self, sliced, *args, **kwargs):
            return ["text"] * len(sliced)

        def parse_generation(self, texts, sliced, *args):
            return {"onset": [0.1, 0.1, 0.4], "offset": [0.2, 0.2, 0.6], "cluster": ["a", "a", "b"]}

    stub = Stub()
    want = postprocess.drop_consecutive_duplicates(postprocess.correct_fft_blur(dict(stub.parse_generation(None, None)), 512, 16000))
    got = stub.segment(np.zeros(16000, np.float32), 16000)
    assert got == want and set(got) == {"onset", "offset", "cluster"}
    assert stub.segment_batch([np.zeros(16000, np.float32)], 16000) == [want]
    assert stub.segment_channels(np.zeros((2, 16000), np.float32), 16000) == [want, want]
    for bad in (0, 257, 2.5, "32", True):
        with pytest.raises(ValueError, match="width"):
            stub.segment(np.zeros(16000, np.float32), 16000, patches=bad)
        with pytest.raises(ValueError, match="width"):
            stub.segment_batch([np.zeros(16000, np.float32)], 16000, patches=bad)
    for fn, args in ((dist.segment_distributed, (stub, None, 16000)), (dist.segment_batch_distributed, (stub, [], 16000))):
        with pytest.raises(ValueError, match="patches"):
            fn(*args, patches=32)
