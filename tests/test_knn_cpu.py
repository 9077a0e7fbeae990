"""whisperseg_amd/neighbors.py on the host: the definition on a hand-computed example, its tie rule and conventions, that the float
cases of the device tests prove something (their share of decided rows), the host plan of the device path (wseg_knn_scratch_bytes
and the validation of wseg_knn_f32: no device needed), patch_neighbors' input errors and the CLI's --neighbors flag."""
import os
import sys

import numpy as np
import pytest

import knn_cases as KC
from conftest import ROOT
from whisperseg_amd import neighbors as NB


@pytest.fixture(scope="module", autouse=True)
def library():
    """The plan tests reach the host arithmetic through libwseg (no device): built here if it is not yet (a no-op otherwise)."""
    from whisperseg_amd import build
    build.build(verbose=False)


def test_definition_by_hand():
    """Four points on a line and one off it: distances 1, 4, 9, ... by hand."""
    x = np.array([[0, 0], [1, 0], [3, 0], [6, 0], [1, 2]], np.float32)
    index, distance = NB.neighbors_host(x, k=2)
    assert index.dtype == np.int32 and distance.dtype == np.float32 and index.shape == distance.shape == (5, 2)
    assert index.tolist() == [[1, 4], [0, 2], [1, 4], [2, 1], [1, 0]]
    assert distance.tolist() == [[1, 5], [1, 4], [4, 8], [9, 25], [4, 5]]
    # queries against a corpus: a row's own index is a candidate like any other
    q = np.array([[1, 0], [5, 0]], np.float32)
    index, distance = NB.neighbors_host(q, x, k=3)
    assert index.tolist() == [[1, 0, 2], [3, 2, 1]] and distance.tolist() == [[0, 1, 4], [1, 4, 16]]
    # float64 inside: 1e-4 apart at 1e4 is invisible to a float32 |q|^2 + |x|^2 - 2 q.x, not to the direct form
    far = np.array([[1e4], [1e4 + 1e-3 * 8], [1e4 - 1e-3 * 16]], np.float32)
    index, distance = NB.neighbors_host(far, k=2)
    gap = np.float64(far[1, 0]) - np.float64(far[0, 0])
    assert index[0].tolist() == [1, 2] and distance[0, 0] == np.float32(gap * gap) and distance[0, 0] > 0
    assert np.array_equal(NB.distances_host(q, x), [[1, 0, 4, 25, 4], [25, 16, 4, 1, 20]])


def test_tie_rule_and_exclusion_by_index():
    """Among equal distances the lower index; a row is left out by its index, not by its value."""
    x = np.array([[0], [1], [-1], [1], [0], [2]], np.float32)
    index, distance = NB.neighbors_host(x, k=4)
    assert index[0].tolist() == [4, 1, 2, 3] and distance[0].tolist() == [0, 1, 1, 1]            # its twin at 0, then three ties by index
    assert index[4].tolist() == [0, 1, 2, 3] and distance[4].tolist() == [0, 1, 1, 1]
    assert index[1].tolist() == [3, 0, 4, 5] and index[3].tolist() == [1, 0, 4, 5]              # identical rows: each other's neighbour
    assert distance[1, 0] == 0 and distance[3, 0] == 0
    # as a corpus the same rows do contain the query's own index
    index, _ = NB.neighbors_host(x, x, k=2)
    assert index[:, 0].tolist() == [0, 1, 2, 1, 0, 5] and index[4].tolist() == [0, 4]
    # the ties at the k-th boundary of an integer case are many: the rule decides them
    ref = KC.reference("integer", 333, 3, 64)
    assert (ref.sorted[:, 63] == ref.sorted[:, 64]).mean() > 0.5


def test_fewer_than_k_candidates_and_empty_inputs():
    x = KC.integer_rows(5, 7)
    index, distance = NB.neighbors_host(x, k=8)
    assert (index[:, 4:] == -1).all() and np.isposinf(distance[:, 4:]).all() and (index[:, :4] >= 0).all() and np.isfinite(distance[:, :4]).all()
    assert all(sorted(index[i, :4].tolist()) == [j for j in range(5) if j != i] for i in range(5))
    index, distance = NB.neighbors_host(x, x, k=8)
    assert (index[:, 5:] == -1).all() and (index[:, :5] >= 0).all() and np.isposinf(distance[:, 5:]).all()
    index, distance = NB.neighbors_host(x[:1], k=3)                                  # one row: no candidate at all
    assert index.tolist() == [[-1, -1, -1]] and np.isposinf(distance).all()
    index, distance = NB.neighbors_host(x, np.zeros((0, 7), np.float32), k=2)        # an empty corpus
    assert index.shape == (5, 2) and (index == -1).all() and np.isposinf(distance).all()
    index, distance = NB.neighbors_host(np.zeros((0, 7), np.float32), x, k=2)        # no queries
    assert index.shape == distance.shape == (0, 2) and index.dtype == np.int32 and distance.dtype == np.float32


def test_invalid_input_is_refused():
    x = KC.integer_rows(5, 7)
    for k in (0, 65, -1, 2.5, None, "3", True):
        with pytest.raises(ValueError, match="k must"):
            NB.check_k(k)
        with pytest.raises(ValueError, match="k must"):
            NB.neighbors_host(x, k=k)
    assert NB.check_k(1) == 1 and NB.check_k(np.int64(64)) == 64 and isinstance(NB.check_k(np.int32(7)), int)
    with pytest.raises(ValueError, match="same D"):
        NB.neighbors_host(x, x[:, :6], k=2)
    with pytest.raises(ValueError, match="2-D"):
        NB.neighbors_host(x[0], k=2)
    with pytest.raises(ValueError, match="2-D"):
        NB.neighbors_host(x, x[None], k=2)
    with pytest.raises(ValueError, match="D must"):
        NB.neighbors_host(np.zeros((3, 0), np.float32), k=2)
    with pytest.raises(ValueError, match="D must"):
        NB.neighbors_host(np.zeros((2, 20481), np.float32), k=2)


@pytest.mark.parametrize("shape", KC.CLUSTERED_SHAPES)
def test_the_float_cases_prove_something(shape):
    """At least 90 % of a clustered case's rows are decided by the definition alone, even at twice the contract's margin."""
    ref = KC.reference("clustered", *shape)
    share, wide = ref.decided().mean(), ref.decided(4.0).mean()
    print(f"(D, N, k) = {shape}: {100 * share:.1f} % of the rows decided, {100 * wide:.1f} % at twice the margin; median tau {np.median(ref.tau):.3g}, "
          f"median k-th distance {np.median(ref.sorted[:, ref.k - 1]):.3g}")
    assert share >= wide >= KC.MIN_DECIDED
    # and the definition satisfies its own contract
    assert KC.check_contract(ref, ref.index, ref.distance, "the definition") == share


def test_the_cases_hold_what_they_promise():
    for n, d, k in KC.INTEGER_SHAPES:
        x = KC.integer_rows(n, d)
        assert x.shape == (n, d) and x.dtype == np.float32 and np.array_equal(x, np.round(x)) and x.min() >= -3 and x.max() <= 3
        assert 1 <= k <= 64 and 9 * d * 4 < 2 ** 24
    assert {k for _, _, k in KC.INTEGER_SHAPES} >= {1, 64} and any(n <= k for n, _, k in KC.INTEGER_SHAPES)
    assert any(d % 4 and d % 16 for _, d, _ in KC.INTEGER_SHAPES) and max(d for _, d, _ in KC.INTEGER_SHAPES) == NB.MAX_D
    q, x, which = KC.cross_case()
    assert q.shape == (37, 81) and x.shape == (500, 81) and len(which) == 10 and all(np.array_equal(q[i], x[j]) for i, j in which.items())
    ref = KC.reference("cross")
    assert all(ref.distance[i, 0] == 0 for i in which)
    rows = KC.picture_rows()
    assert rows.shape[1] == 2560 and np.array_equal(rows[-5:], rows[:5]) and np.isfinite(rows).all()
    u = KC.uniform_rows()
    assert u.shape == (96, 2560) and -1.5 <= u.min() and u.max() <= 0.5


def test_plan_through_the_library():
    """wseg_knn_scratch_bytes is host arithmetic (no device), monotone in each argument, 0 / WsegError for invalid input; the launch
    entry point validates on the host, before it touches a device, and names the argument."""
    from whisperseg_amd import _lib
    lib = _lib.load()
    pad = lambda b: max(256, -(-b // 256) * 256)
    # two norm arrays, then min(m_tiles * n_tiles, m_tiles + 2048) items of 128 rows x (k + 8) keys of 8 bytes
    for m, n, k in ((1, 1, 1), (64, 64, 15), (65, 1000, 15), (1000, 100000, 64), (100000, 100000, 15), (2 ** 31 - 1, 2 ** 31 - 1, 64)):
        mt, nt = -(-m // 128), -(-n // 128)
        assert NB.scratch_bytes(m, n, 2560, k) == pad(4 * m) + pad(4 * n) + pad(min(mt * nt, mt + 2048) * 128 * (k + 8) * 8), (m, n, k)
    assert NB.scratch_bytes(0, 0, 1, 1) == 3 * 256 and NB.scratch_bytes(10, 10, 1, 15) == NB.scratch_bytes(10, 10, 20480, 15)
    sizes = (0, 1, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 4097, 100000, 131072, 131073, 10 ** 7, 2 ** 31 - 1)
    for other in (1, 64, 65, 5000, 2 ** 31 - 1):
        for k in (1, 15, 64):
            by_m = [NB.scratch_bytes(s, other, 80, k) for s in sizes]
            by_n = [NB.scratch_bytes(other, s, 80, k) for s in sizes]
            assert by_m == sorted(by_m) and by_n == sorted(by_n), (other, k)
        by_k = [NB.scratch_bytes(other, 70000, 80, k) for k in range(1, 65)]
        assert by_k == sorted(by_k) and by_k[0] < by_k[-1]
    by_d = [NB.scratch_bytes(100, 100, d, 5) for d in (1, 2, 2560, 20480)]
    assert by_d == sorted(by_d)
    for args, word in (((-1, 5, 8, 3), "m must"), ((5, -1, 8, 3), "n must"), ((2 ** 31, 5, 8, 3), "m must"), ((5, 2 ** 31, 8, 3), "n must"),
                       ((5, 5, 0, 3), "d must"), ((5, 5, 20481, 3), "d must"), ((5, 5, 8, 0), "k must"), ((5, 5, 8, 65), "k must")):
        assert lib.wseg_knn_scratch_bytes(*args) == 0 and word.encode() in lib.wseg_last_error(), args
        with pytest.raises(_lib.WsegError, match=word):
            NB.scratch_bytes(*args)

    def call(m=5, n=5, d=8, k=3, exclude=0, q=64, x=64, scratch=None, nbytes=0, index=64, distance=64):      # (pointers never dereferenced: every call is refused)
        return lib.wseg_knn_f32(q, m, x, n, d, k, exclude, scratch, nbytes, index, distance, None)

    for kw, word in ((dict(k=0), b"k must"), (dict(k=65), b"k must"), (dict(d=0), b"d must"), (dict(d=20481), b"d must"), (dict(m=-1), b"m must"),
                     (dict(n=-1), b"n must"), (dict(m=2 ** 31), b"m must"), (dict(exclude=2), b"exclude_same_index"), (dict(q=None), b"queries"),
                     (dict(q=66), b"queries"), (dict(x=None), b"corpus"), (dict(x=65), b"corpus"), (dict(index=None), b"index_out"),
                     (dict(distance=None), b"distance_out"), (dict(), b"scratch"), (dict(scratch=260, nbytes=1 << 30), b"scratch"),
                     (dict(scratch=256, nbytes=8), b"scratch")):
        assert call(**kw) != 0 and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())
    assert call(m=0, q=None, x=None, index=None, distance=None) == 0                 # m == 0: nothing to do, nothing looked at


def test_patch_neighbors_input_errors():
    good = {"onset": [0.1, 0.2], "offset": [0.15, 0.3], "cluster": ["a", "b"], "patch": np.zeros((2, 80, 4), np.float32)}
    plain = {k: v for k, v in good.items() if k != "patch"}
    other = dict(good, patch=np.zeros((2, 80, 5), np.float32))
    for bad in ([plain], [good, plain], [[good, plain]], [[good], plain]):
        with pytest.raises(ValueError, match="patch"):
            NB.patch_neighbors(bad, 3)
    with pytest.raises(ValueError, match="different sizes"):
        NB.patch_neighbors([good, other], 3)
    with pytest.raises(ValueError, match="n_mels"):
        NB.patch_neighbors([dict(good, patch=np.zeros((2, 320), np.float32))], 3)
    for k in (0, 65, 2.5):
        with pytest.raises(ValueError, match="k must"):
            NB.patch_neighbors([good], k)
    # the flattened order is the archive's: file, channel, row
    a = dict(good, patch=np.arange(2 * 80 * 4, dtype=np.float32).reshape(2, 80, 4))
    c = {"onset": [0.5], "offset": [0.6], "cluster": ["c"], "patch": -np.ones((1, 80, 4), np.float32)}
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    for results, all_channels in (([[a, c], [c, a]], True), ([a, c, a], False)):
        arch = segment.patch_archive(results, None, all_channels)
        assert np.array_equal(NB.patch_rows_of(results), arch["patch"].reshape(len(arch["patch"]), -1))
    # no rows: empty arrays, no device needed
    none = NB.patch_neighbors([], 3)
    assert none["neighbor_index"].shape == none["neighbor_distance"].shape == (0, 3) and none["neighbor_index"].dtype == np.int32
    empty = dict(plain, onset=[], offset=[], cluster=[], patch=np.zeros((0, 80, 4), np.float32))
    assert NB.patch_neighbors([empty, [empty]], 64)["neighbor_distance"].shape == (0, 64)


def test_cli_flag(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    base = ["--model_path", "m", "--csv_save_path", "o.csv"]
    assert segment.parse_args(base).neighbors is None
    assert segment.parse_args(base + ["--patches", "8", "--patches_save_path", "p.npz"]).neighbors is None
    assert segment.parse_args(base + ["--patches", "8", "--patches_save_path", "p.npz", "--neighbors", "64"]).neighbors == 64
    for extra in (["--neighbors", "3"], ["--patches", "8", "--patches_save_path", "p.npz", "--neighbors", "0"],
                  ["--patches", "8", "--patches_save_path", "p.npz", "--neighbors", "65"]):
        with pytest.raises(SystemExit) as e:
            segment.main(base + extra)                       # refused by argparse, before a model is looked for
        assert e.value.code == 2 and "neighbors" in capsys.readouterr().err
