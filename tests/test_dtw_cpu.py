"""whisperseg_amd/dtw.py on the host: the definition against its plain-loop restatement and against the Euclidean definition at
band 0, its symmetry and its monotony in the band, its conventions, that the float cases of the device tests prove something (their
share of decided rows), the host plan of the device path (wseg_dtw_scratch_bytes and the validation of the launching entries: no
device needed), the plan-check program under the host undefined-behaviour sanitizer and the CLI's --neighbors_metric /
--neighbors_band flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dtw_cases as DC
from conftest import ROOT
from whisperseg_amd import dtw as DW
from whisperseg_amd import neighbors as NB


@pytest.fixture(scope="module", autouse=True)
def library():
    """The plan tests reach the host arithmetic through libwseg (no device): built here if it is not yet (a no-op otherwise)."""
    from whisperseg_amd import build
    build.build(verbose=False)


def float_pair_rows(c, t, n=6):
    return np.random.default_rng([DC.SEED, c, t, n, 3]).uniform(-1.5, 0.5, (n, c * t)).astype(np.float32)


def test_definition_by_hand():
    """One channel, three steps: q = [0, 1, 3], x = [0, 0, 1].  The costs are (q_a - x_b)^2; with the full band the best path is
    (0,0) (0,1) (1,2) (2,2): 0 + 0 + 0 + 4; with band 0 only the diagonal is left: 0 + 1 + 4."""
    q, x = np.array([[0, 1, 3]], np.float32), np.array([[0, 0, 1]], np.float32)
    assert DW.dtw_host(q, x, 1, 2).tolist() == [[4.0]] and DW.dtw_host(q, x, 1, 1).tolist() == [[4.0]] and DW.dtw_host(q, x, 1, 0).tolist() == [[5.0]]
    cost = DW.cost_host(q, x, 1, 1)[0, 0]
    assert cost[:2, :2].tolist() == [[0, 0], [1, 1]] and np.isposinf(cost[0, 2]) and np.isposinf(cost[2, 0]) and cost[2, 2] == 4
    # two channels, time fastest: row[ch * T + t]
    q2, x2 = np.array([[0, 1, 3, 2, 2, 2]], np.float32), np.array([[0, 0, 1, 2, 2, 0]], np.float32)
    # the second channel adds 4 to every cost of column b = 2: the best path is now the diagonal's end, (0,0) (0,1) (1,1) (2,2):
    # 0 + 0 + 1 + 8
    assert DW.dtw_host(q2, x2, 2, 2).tolist() == [[9.0]]
    assert DW.dtw_plain(q2[0], x2[0], 2, 2) == 9.0
    assert DW.check_band(None, 32) == 4 and DW.check_band(None, 1) == 0 and DW.check_band(None, 2) == 1 and DW.check_band(None, 64) == 8
    index, distance = DW.dtw_neighbors_host(np.concatenate([q, x, q]), None, 2, 1, 2)
    assert index.tolist() == [[2, 1], [0, 2], [0, 1]] and distance.tolist() == [[0, 4], [4, 4], [0, 4]]


def test_band_zero_is_the_euclidean_definition():
    for n, c, t, k in ((64, 16, 8, 4), (200, 1, 1, 15), (50, 3, 5, 64)):
        rows = DC.integer_rows(n, c * t)
        got, want = DW.dtw_neighbors_host(rows, None, k, c, 0), NB.neighbors_host(rows, None, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (n, c, t)
    q, x, _ = DC.cross_case()
    got, want = DW.dtw_neighbors_host(q, x, 15, 9, 0), NB.neighbors_host(q, x, 15)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("shape", ((1, 1, 0), (3, 5, 4), (7, 20, 3), (2, 64, 1)), ids=lambda s: "x".join(map(str, s)))
def test_host_equals_the_plain_loop(shape):
    """The numpy statement and the loop over Python floats give the same float64 bits, and so do the pair list and float32."""
    c, t, r = shape
    rows = float_pair_rows(c, t)
    dist = DW.dtw_host(rows, rows, c, r)
    plain = np.array([[DW.dtw_plain(rows[i], rows[j], c, r) for j in range(len(rows))] for i in range(len(rows))])
    assert dist.dtype == np.float64 and np.array_equal(dist.view(np.uint64), plain.view(np.uint64))
    pairs = np.array([(i, j) for i in range(len(rows)) for j in range(len(rows))])
    got = DW.dtw_pairs_host(rows, rows, pairs, c, r)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), dist.astype(np.float32).ravel().view(np.uint32))
    assert DW.dtw_pairs_host(rows, rows, np.zeros((0, 2), np.int64), c, r).shape == (0,)


def test_symmetry_and_monotony_in_the_band():
    for c, t in ((3, 5), (7, 20), (2, 64), (16, 8)):
        rows = float_pair_rows(c, t, 8)
        before = None
        for r in range(t):
            dist = DW.dtw_host(rows, rows, c, r)
            assert np.array_equal(dist.view(np.uint64), dist.T.copy().view(np.uint64)), (c, t, r)
            assert (np.diag(dist) == 0).all()
            assert before is None or (dist <= before).all(), (c, t, r)
            before = dist
        a, b = DW.dtw_host(rows[:3], rows[3:], c, 1), DW.dtw_host(rows[3:], rows[:3], c, 1)
        assert np.array_equal(a, b.T)


def test_warped_twins():
    """A row one step late is at distance exactly 0 once the band lets the path step aside, and further than 0 under band 0."""
    rows, n = DC.twin_rows(), DC.TWINS["n"]
    for band in (1, 2):
        ref = DC.reference("twins", band)
        assert (ref.distance[:, 0] == 0).all() and (ref.dist[np.arange(n), n + np.arange(n)] == 0).all()
    ref = DC.reference("twins", 0)
    assert (ref.dist[np.arange(n), n + np.arange(n)] > 0).all() and not np.array_equal(rows[:n], rows[n:])


def test_invalid_input_is_refused():
    x = DC.integer_rows(5, 12)
    for k in (0, 65, 2.5, None, True):
        with pytest.raises(ValueError, match="k must"):
            DW.dtw_neighbors_host(x, None, k, 3, 1)
    for channels in (0, 129, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="channels must"):
            DW.dtw_neighbors_host(x, None, 2, channels, 1)
        with pytest.raises(ValueError, match="channels must"):
            DW.dtw_host(x, x, channels, 1)
    for band in (-1, 4, 2.5, True, "1"):
        with pytest.raises(ValueError, match="band must"):
            DW.dtw_neighbors_host(x, None, 2, 3, band)
        with pytest.raises(ValueError, match="band must"):
            DW.dtw_plain(x[0], x[1], 3, band)
        with pytest.raises(ValueError, match="band must"):
            DW.dtw_pairs_host(x, x, np.zeros((0, 2), np.int64), 3, band)
    with pytest.raises(ValueError, match="multiple of channels"):
        DW.dtw_neighbors_host(x, None, 2, 5, 1)
    with pytest.raises(ValueError, match="multiple of channels"):
        DW.dtw_host(np.zeros((3, 0), np.float32), np.zeros((3, 0), np.float32), 1, 0)
    with pytest.raises(ValueError, match="T = D / channels must"):
        DW.dtw_neighbors_host(np.zeros((3, 130), np.float32), None, 2, 2, 1)
    with pytest.raises(ValueError, match="same D"):
        DW.dtw_neighbors_host(x, x[:, :9], 2, 3, 1)
    with pytest.raises(ValueError, match="2-D"):
        DW.dtw_neighbors_host(x[0], None, 2, 3, 1)
    with pytest.raises(ValueError, match="2-D"):
        DW.dtw_host(x, x[None], 3, 1)
    for pairs in ([[0, 5]], [[5, 0]], [[-1, 0]], [[0, 1, 2]], [0, 1], [[0.5, 1.0]]):
        with pytest.raises(ValueError, match="pairs must"):
            DW.dtw_pairs_host(x, x, np.array(pairs), 3, 1)
    # the conventions of neighbors_host: fewer candidates than k, no candidates, no queries
    index, distance = DW.dtw_neighbors_host(x, None, 8, 3, 1)
    assert (index[:, 4:] == -1).all() and np.isposinf(distance[:, 4:]).all() and (index[:, :4] >= 0).all()
    index, distance = DW.dtw_neighbors_host(x, np.zeros((0, 12), np.float32), 2, 3, 1)
    assert index.shape == (5, 2) and (index == -1).all() and np.isposinf(distance).all()
    index, distance = DW.dtw_neighbors_host(np.zeros((0, 12), np.float32), x, 2, 3, 1)
    assert index.shape == distance.shape == (0, 2) and index.dtype == np.int32 and distance.dtype == np.float32


@pytest.mark.parametrize("shape", DC.FLOAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_float_cases_prove_something(shape):
    """At least 90 % of a float case's rows are decided by the definition alone, and the definition satisfies its own contract."""
    ref = DC.reference("float", *shape)
    share = float(ref.decided().mean())
    print(f"(C, T, N, band, k) = {shape}: {100 * share:.1f} % of the rows decided; median tau {np.median(ref.tau):.3g}, "
          f"median k-th distance {np.median(ref.sorted[:, ref.k - 1]):.3g}")
    assert share >= DC.MIN_DECIDED
    assert DC.check_contract(ref, ref.index, ref.distance, "the definition") == share


def test_the_cases_hold_what_they_promise():
    for n, c, t, band, k in DC.INTEGER_SHAPES:
        x = DC.integer_rows(n, c * t)
        assert x.shape == (n, c * t) and x.dtype == np.float32 and np.array_equal(x, np.round(x)) and x.min() >= -3 and x.max() <= 3
        assert 1 <= k <= 64 and 1 <= c <= 128 and 1 <= t <= 64 and 0 <= band < t and (2 * t - 1) * 36 * c < 2 ** 24
    assert {(c, t, band, k) for _, c, t, band, k in DC.INTEGER_SHAPES} >= {(128, 64, 63, 64)}
    q, x, which = DC.cross_case()
    assert q.shape == (37, 81) and x.shape == (500, 81) and len(which) == 10 and all(np.array_equal(q[i], x[j]) for i, j in which.items())
    rows = DC.twin_rows()
    n, c, t = DC.TWINS["n"], DC.TWINS["c"], DC.TWINS["t"]
    cols = rows.reshape(2 * n, c, t)
    assert np.array_equal(cols[:n, :, -1], cols[:n, :, -2]) and np.array_equal(cols[n:, :, 1:], cols[:n, :, :-1]) and np.array_equal(cols[n:, :, 0], cols[:n, :, 0])


def test_plan_through_the_library():
    """wseg_dtw_scratch_bytes is host arithmetic (no device), monotone in m, n and k, 0 / WsegError for invalid input; the launching
    entry points validate on the host, before they touch a device, and name the argument."""
    from whisperseg_amd import _lib
    lib = _lib.load()
    pad = lambda b: max(256, -(-b // 256) * 256)
    for m, n, c, t, k in ((1, 1, 1, 1, 1), (64, 64, 16, 8, 15), (65, 1000, 80, 32, 15), (1000, 100000, 80, 33, 64), (2 ** 31 - 1, 2 ** 31 - 1, 128, 64, 64)):
        seqs = 4 if t <= 32 else 2
        m4, nt = -(-m // 4) * 4, -(-n // seqs)
        assert DW.scratch_bytes(m, n, c, t, k) == pad(4 * m * t) + pad(4 * n * t) + pad(min(m4 * nt, m4 + 4 * 2048) * (k + 8) * 8), (m, n, c, t, k)
    assert DW.scratch_bytes(0, 0, 1, 1, 1) == 3 * 256 and DW.scratch_bytes(10, 10, 1, 8, 15) == DW.scratch_bytes(10, 10, 128, 8, 15)
    sizes = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000, 4097, 100000, 131073, 10 ** 7, 2 ** 31 - 1)
    for other in (1, 4, 5, 5000, 2 ** 31 - 1):
        for t in (1, 32, 33, 64):
            for k in (1, 15, 64):
                by_m = [DW.scratch_bytes(s, other, 80, t, k) for s in sizes]
                by_n = [DW.scratch_bytes(other, s, 80, t, k) for s in sizes]
                assert by_m == sorted(by_m) and by_n == sorted(by_n), (other, t, k)
            by_k = [DW.scratch_bytes(other, 70000, 80, t, k) for k in range(1, 65)]
            assert by_k == sorted(by_k) and by_k[0] < by_k[-1]
        by_t = [DW.scratch_bytes(other, 70000, 80, t, 15) for t in range(1, 65)]
        assert by_t == sorted(by_t)
    for args, word in (((-1, 5, 8, 4, 3), "m must"), ((5, -1, 8, 4, 3), "n must"), ((2 ** 31, 5, 8, 4, 3), "m must"), ((5, 2 ** 31, 8, 4, 3), "n must"),
                       ((5, 5, 0, 4, 3), "channels must"), ((5, 5, 129, 4, 3), "channels must"), ((5, 5, 8, 0, 3), "steps must"),
                       ((5, 5, 8, 65, 3), "steps must"), ((5, 5, 8, 4, 0), "k must"), ((5, 5, 8, 4, 65), "k must")):
        assert lib.wseg_dtw_scratch_bytes(*args) == 0 and word.encode() in lib.wseg_last_error(), args
        with pytest.raises(_lib.WsegError, match=word):
            DW.scratch_bytes(*args)

    def call(m=5, n=5, c=8, t=4, band=1, k=3, exclude=0, q=64, x=64, scratch=None, nbytes=0, index=64, distance=64):      # (pointers never dereferenced: every call is refused)
        return lib.wseg_dtw_knn_f32(q, m, x, n, c, t, band, k, exclude, scratch, nbytes, index, distance, None)

    for kw, word in ((dict(k=0), b"k must"), (dict(k=65), b"k must"), (dict(c=0), b"channels must"), (dict(c=129), b"channels must"),
                     (dict(t=0), b"steps must"), (dict(t=65), b"steps must"), (dict(band=-1), b"band must"), (dict(band=4), b"band must"),
                     (dict(m=-1), b"m must"), (dict(n=-1), b"n must"), (dict(m=2 ** 31), b"m must"), (dict(exclude=2), b"exclude_same_index"),
                     (dict(q=None), b"queries"), (dict(q=66), b"queries"), (dict(x=None), b"corpus"), (dict(x=65), b"corpus"),
                     (dict(index=None), b"index_out"), (dict(distance=None), b"distance_out"), (dict(), b"scratch"),
                     (dict(scratch=260, nbytes=1 << 30), b"scratch"), (dict(scratch=256, nbytes=8), b"scratch")):
        assert call(**kw) != 0 and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())
    assert call(m=0, q=None, x=None, index=None, distance=None) == 0                 # m == 0: nothing to do, nothing looked at

    def pairs(m=5, n=5, c=8, t=4, band=1, q=64, x=64, p=64, count=3, out=64):
        return lib.wseg_dtw_pairs_f64(q, m, x, n, c, t, band, p, count, out, None)

    for kw, word in ((dict(c=0), b"channels must"), (dict(c=129), b"channels must"), (dict(t=65), b"steps must"), (dict(band=-1), b"band must"),
                     (dict(band=4), b"band must"), (dict(m=-1), b"m must"), (dict(n=2 ** 31), b"n must"), (dict(count=-1), b"pair count"),
                     (dict(m=0), b"rows on both sides"), (dict(q=None), b"queries"), (dict(x=66), b"corpus"), (dict(p=None), b"pairs"),
                     (dict(p=65), b"pairs"), (dict(out=None), b"out must")):
        assert pairs(**kw) != 0 and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())
    assert pairs(count=0, q=None, x=None, p=None, out=None) == 0                     # no pair: nothing to do, nothing looked at


def test_plan_check_program_under_the_sanitizer(tmp_path):
    """tools/dtw_plan_check.cpp sweeps the plan over the limits; built with -fsanitize=undefined it must exit 0."""
    exe = tmp_path / "dtw_plan_check"
    subprocess.run(["c++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "dtw_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])


def test_patch_dtw_neighbors_input_errors():
    good = {"onset": [0.1, 0.2], "offset": [0.15, 0.3], "cluster": ["a", "b"], "patch": np.zeros((2, 80, 4), np.float32)}
    plain = {k: v for k, v in good.items() if k != "patch"}
    for bad in ([plain], [good, plain], [[good, plain]]):
        with pytest.raises(ValueError, match="patch"):
            DW.patch_dtw_neighbors(bad, 3)
    with pytest.raises(ValueError, match="different sizes"):
        DW.patch_dtw_neighbors([good, dict(good, patch=np.zeros((2, 80, 5), np.float32))], 3)
    with pytest.raises(ValueError, match="up to 64 columns"):
        DW.patch_dtw_neighbors([dict(good, patch=np.zeros((2, 80, 65), np.float32))], 3)
    for k in (0, 65, 2.5):
        with pytest.raises(ValueError, match="k must"):
            DW.patch_dtw_neighbors([good], k)
    none = DW.patch_dtw_neighbors([], 3)
    assert none["neighbor_index"].shape == none["neighbor_distance"].shape == (0, 3) and none["neighbor_index"].dtype == np.int32


def test_cli_flags(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    base = ["--model_path", "m", "--csv_save_path", "o.csv"]
    saved = base + ["--patches", "8", "--patches_save_path", "p.npz"]
    args = segment.parse_args(saved + ["--neighbors", "3"])
    assert args.neighbors_metric == "euclidean" and args.neighbors_band is None
    args = segment.parse_args(saved + ["--neighbors", "3", "--neighbors_metric", "dtw"])
    assert args.neighbors_metric == "dtw" and args.neighbors_band is None
    args = segment.parse_args(saved + ["--embed", "2", "--neighbors_metric", "dtw", "--neighbors_band", "0"])
    assert args.neighbors_metric == "dtw" and args.neighbors_band == 0
    assert segment.parse_args(base + ["--patches", "64", "--patches_save_path", "p.npz", "--neighbors", "3", "--neighbors_metric", "dtw"]).patches == 64
    for extra, word in ((saved + ["--neighbors_metric", "dtw"], "neighbors_metric"),                       # neither --neighbors nor --embed
                        (saved + ["--neighbors_metric", "euclidean"], "neighbors_metric"),
                        (saved + ["--clusters", "5", "--neighbors_metric", "dtw"], "neighbors_metric"),
                        (saved + ["--neighbors_band", "2"], "neighbors_band"),
                        (saved + ["--neighbors", "3", "--neighbors_band", "2"], "neighbors_band"),          # a band without dtw
                        (saved + ["--neighbors", "3", "--neighbors_metric", "euclidean", "--neighbors_band", "2"], "neighbors_band"),
                        (saved + ["--neighbors", "3", "--neighbors_metric", "dtw", "--neighbors_band", "8"], "neighbors_band"),      # 0 .. W - 1
                        (saved + ["--neighbors", "3", "--neighbors_metric", "dtw", "--neighbors_band", "-1"], "neighbors_band"),
                        (saved + ["--neighbors", "3", "--neighbors_metric", "cosine"], "neighbors_metric"),
                        (base + ["--patches", "65", "--patches_save_path", "p.npz", "--neighbors", "3", "--neighbors_metric", "dtw"], "patches")):
        with pytest.raises(SystemExit) as e:
            segment.main(extra)                              # refused by argparse, before a model is looked for
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
