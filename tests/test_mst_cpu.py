"""whisperseg_amd/linkage.py on the host: the definition mst_host (a spanning tree in the order (w, a, b), scipy's total weight), the
rounds' rules in numpy giving the identical edge list, cut against sklearn's DBSCAN, hdbscan_labels against the blobs and sklearn's
HDBSCAN, the conventions, the host plan of the device path through the library and under the UB sanitizer, patch_clusters' input
errors and the CLI's --clusters flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mst_cases as MC
from conftest import ROOT
from whisperseg_amd import linkage as LK
from whisperseg_amd import neighbors as NB

HOST_TREES = tuple(c for c in MC.EXACT_TREES if c[2] <= 64)        # (the long rows are the device tests')


def test_definition_on_a_hand_computed_example():
    # five points on a line at 0, 1, 3, 7, 8 (squared distances); s = 1: core = the nearest other row
    x = np.array([[0.0], [1.0], [3.0], [7.0], [8.0]], np.float32)
    core, w = LK.weights_host(x, 1)
    assert core.tolist() == [1, 1, 4, 1, 1] and w.dtype == np.float32 and np.array_equal(w, w.T)
    assert w[0, 1] == 1 and w[1, 2] == 4 and w[0, 2] == 9 and w[2, 3] == 16 and w[3, 4] == 1
    edges, weight = LK.mst_host(x, 1)
    assert edges.tolist() == [[0, 1], [3, 4], [1, 2], [2, 3]] and weight.tolist() == [1, 1, 4, 16]
    assert edges.dtype == np.int32 and weight.dtype == np.float32
    # s = 2: core = the second nearest other row; every weight is at least both ends' cores
    core, w = LK.weights_host(x, 2)
    assert core.tolist() == [9, 4, 9, 16, 25]
    edges, weight = LK.mst_host(x, 2)
    # (9, 0, 1), (9, 0, 2), then (9, 1, 2) closes a ring; (16, 2, 3); (25, 2, 4) comes before (25, 3, 4)
    assert edges.tolist() == [[0, 1], [0, 2], [2, 3], [2, 4]] and weight.tolist() == [9, 9, 16, 25]


@pytest.mark.parametrize("case", HOST_TREES, ids=lambda c: "-".join(map(str, c)))
def test_definition_is_the_minimum_spanning_tree(case):
    from scipy.sparse.csgraph import minimum_spanning_tree
    ref = MC.reference(*case)
    MC.check_spanning(ref.edges, ref.weight, ref.n, case)
    assert np.array_equal(ref.core, NB.neighbors_host(ref.x, None, k=ref.s)[1][:, ref.s - 1])       # the issue's statement of core
    assert np.array_equal(ref.weight, ref.w[ref.edges[:, 0], ref.edges[:, 1]])
    if (np.triu(ref.w, 1)[np.triu_indices(ref.n, 1)] > 0).all():           # scipy reads 0 as "no edge"
        total = minimum_spanning_tree(np.triu(ref.w.astype(np.float64), 1)).sum()
        assert total == ref.weight.astype(np.float64).sum(), case
    else:
        assert case[0] in ("identical", "dyadic") or case[3] == 1, case


def test_float_definition_is_built_on_neighbors_distances():
    x = MC.rows_of("clustered", 300, 64)
    dist = NB.distances_host(x, x)
    assert np.array_equal(LK.distances_self_host(x), dist)                                 # the very bits, whatever the blocks
    core, w = LK.weights_host(x, 5)
    assert np.array_equal(core, NB.neighbors_host(x, None, k=5)[1][:, 4])
    assert np.array_equal(w, np.maximum(np.maximum(core[:, None], core[None, :]), dist.astype(np.float32))) and np.array_equal(w, w.T)
    assert MC.same_tree(LK.mst_host(x, 5), LK.mst_of_weights(w))


def test_some_case_is_compared_with_scipy():
    assert sum(bool((np.triu(MC.reference(*c).w, 1)[np.triu_indices(c[1], 1)] > 0).all()) for c in HOST_TREES) >= 5


@pytest.mark.parametrize("case", HOST_TREES, ids=lambda c: "-".join(map(str, c)))
def test_rounds_in_numpy_give_the_identical_tree(case):
    ref = MC.reference(*case)
    stats = {}
    assert MC.same_tree(MC.boruvka_host(ref, stats), (ref.edges, ref.weight)), case
    assert 1 <= stats["rounds"] <= int(np.ceil(np.log2(ref.n)))
    print(f"{case}: {stats['rounds']} rounds, {len(np.unique(ref.weight))} distinct weights among {ref.n - 1} edges")


def test_all_rows_identical():
    ref = MC.reference("identical", 130, 4, 5)
    assert ref.edges.tolist() == [[0, b] for b in range(1, 130)] and (ref.weight == 0).all() and not np.signbit(ref.weight).any()


def test_one_round_in_numpy():
    ref = MC.reference("integer", 257, 3, 5)
    for pattern in MC.PATTERNS:
        comp = MC.components_of(pattern, ref.n)
        index, weight = MC.round_host(ref.w, comp)
        assert index.dtype == np.int32 and weight.dtype == np.float32
        for i in range(ref.n):
            others = np.flatnonzero(comp != comp[i])
            if not len(others):
                assert index[i] == -1 and np.isposinf(weight[i])
                continue
            best = min((ref.w[i, j], j) for j in others)
            assert (weight[i], index[i]) == best, (pattern, i)
    assert (MC.round_host(ref.w, MC.components_of("one", ref.n))[0] == -1).all()


def test_conventions():
    x = MC.rows_of("integer", 257, 3)
    for n in (0, 1):
        edges, weight = LK.mst_host(x[:n], 5)
        assert edges.shape == (0, 2) and weight.shape == (0,) and edges.dtype == np.int32 and weight.dtype == np.float32
    edges, weight = LK.mst_host(x[:2], 1)
    assert edges.tolist() == [[0, 1]] and weight[0] == ((x[0] - x[1]) ** 2).sum()
    for n, s in ((2, 2), (2, 0), (10, 10), (257, 65), (257, 0), (257, -1), (257, 2.0), (257, True)):
        with pytest.raises(ValueError, match="min_samples"):
            LK.mst_host(x[:n], s)
    with pytest.raises(ValueError, match="2-D"):
        LK.mst_host(x[0], 1)
    with pytest.raises(ValueError, match="2-D"):
        LK.mst_host(x[None], 1)
    with pytest.raises(ValueError, match="D must"):
        LK.mst_host(np.zeros((3, 0), np.float32), 1)
    with pytest.raises(ValueError, match="D must"):
        LK.mst_host(np.zeros((3, 20481), np.float32), 1)
    with pytest.raises(ValueError, match="D must"):
        LK.mst(np.zeros((3, 20481), np.float32), 1)           # refused before a device is looked for
    with pytest.raises(ValueError, match="min_samples"):
        LK.mst(x, 65)
    edges, weight = LK.mst(x[:1], 5)                            # fewer than two rows: no tree, no device needed
    assert edges.shape == (0, 2) and weight.shape == (0,)


# ---- from the tree to labels ---------------------------------------------------------------------------------------------------------
def same_partition(a, b):
    """Equal up to renumbering, noise (-1) to noise."""
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len({p for p, _ in pairs}) == len({q for _, q in pairs}) and all((p == -1) == (q == -1) for p, q in pairs)


@pytest.mark.parametrize("case,threshold", [(("integer", 257, 3, 5), 1.0), (("integer", 257, 3, 5), 2.0), (("integer", 500, 17, 5), 60.0),
                                            (("integer", 500, 17, 5), 75.0), (("far", 200, 8, 5), 30.0), (("far", 200, 8, 5), 1e6)])
def test_cut_is_dbscan_star(case, threshold):
    from sklearn.cluster import DBSCAN
    ref = MC.reference(*case)
    labels = LK.cut(ref.edges, ref.weight, ref.n, threshold)
    assert labels.dtype == np.int32 and labels.shape == (ref.n,)
    is_core = ref.core <= threshold
    dist = np.sqrt(NB.distances_host(ref.x, ref.x))
    theirs = DBSCAN(eps=float(np.sqrt(threshold)), min_samples=ref.s + 1, metric="precomputed").fit(dist)
    assert np.array_equal(np.sort(theirs.core_sample_indices_), np.flatnonzero(is_core))
    assert same_partition(labels[is_core], theirs.labels_[is_core]) and (theirs.labels_[is_core] >= 0).all()
    # rows that are no core rows stand alone; with a minimum size they are noise, and clusters are numbered by their smallest row
    sizes = np.bincount(labels, minlength=ref.n)[labels]
    assert (sizes[~is_core] == 1).all()
    sized = LK.cut(ref.edges, ref.weight, ref.n, threshold, min_cluster_size=2)
    assert (sized[~is_core] == -1).all() and same_partition(sized[sizes > 1], labels[sizes > 1])
    kept = sized[sized >= 0]
    if len(kept):
        first = [int(np.flatnonzero(sized == c)[0]) for c in range(kept.max() + 1)]
        assert first == sorted(first)
    print(f"{case} at {threshold}: {int(is_core.sum())} core rows, {len(set(labels[is_core].tolist()))} clusters among them")


@pytest.fixture(scope="module")
def blobs():
    rng = np.random.default_rng(MC.SEED)
    centres = rng.uniform(-10, 10, size=(4, 32))
    truth = rng.permutation(np.repeat(np.arange(4), 60))
    return (centres[truth] + rng.standard_normal((240, 32))).astype(np.float32), truth


def test_hdbscan_labels_find_the_blobs(blobs):
    from sklearn.cluster import HDBSCAN
    x, truth = blobs
    s = 5
    edges, weight = LK.mst_host(x, s)
    labels = LK.hdbscan_labels(edges, weight, len(x), 15)
    assert labels.dtype == np.int32 and same_partition(labels, truth.astype(np.int32))
    first = [int(np.flatnonzero(labels == c)[0]) for c in range(4)]
    assert first == sorted(first) and labels[0] == 0
    theirs = HDBSCAN(min_cluster_size=15, min_samples=s + 1, metric="precomputed").fit(np.sqrt(NB.distances_host(x, x))).labels_
    assert same_partition(labels, theirs)
    # the order of the edges does not matter, and neither does the orientation of one
    flip = np.random.default_rng(1).permutation(len(edges))
    assert np.array_equal(LK.hdbscan_labels(edges[flip][:, ::-1], weight[flip], len(x), 15), labels)


def test_hdbscan_labels_noise_and_duplicates():
    rng = np.random.default_rng(MC.SEED + 1)
    blob = lambda c, n: c + 0.5 * rng.standard_normal((n, 4))
    x = np.concatenate([blob(0.0, 40), blob(20.0, 40), rng.uniform(-200, 200, size=(6, 4)) + 500.0]).astype(np.float32)
    edges, weight = LK.mst_host(x, 3)
    labels = LK.hdbscan_labels(edges, weight, len(x), 10)
    assert same_partition(labels[:80], np.repeat([0, 1], 40).astype(np.int32)) and (labels[80:] == -1).all()
    # duplicates in mass (weights 0, lambda infinite): labels without a NaN's trouble, every row labelled or noise
    ref = MC.reference("integer", 257, 3, 1)
    labels = LK.hdbscan_labels(ref.edges, ref.weight, ref.n, 5)
    assert labels.shape == (257,) and labels.min() >= -1
    assert (LK.hdbscan_labels(*LK.mst_host(x[:1], 1), 1, 5) == -1).all() and LK.hdbscan_labels(*LK.empty_tree(), 0, 5).shape == (0,)


def test_label_conventions():
    ref = MC.reference("far", 200, 8, 5)
    for bad in (dict(n=199), dict(n=-1), dict(n=2.5)):
        with pytest.raises(ValueError):
            LK.cut(ref.edges, ref.weight, bad["n"], 1.0)
    with pytest.raises(ValueError, match="edges"):
        LK.cut(ref.edges[:, :1], ref.weight, ref.n, 1.0)
    with pytest.raises(ValueError, match="outside"):
        LK.cut(ref.edges + 1, ref.weight, ref.n, 1.0)
    for size in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="min_cluster_size"):
            LK.cut(ref.edges, ref.weight, ref.n, 1.0, min_cluster_size=size)
    for size in (1, 0, 2.0):
        with pytest.raises(ValueError, match="min_cluster_size"):
            LK.hdbscan_labels(ref.edges, ref.weight, ref.n, size)
    with pytest.raises(ValueError, match="tree"):
        LK.hdbscan_labels(np.repeat(ref.edges[:1], ref.n - 1, axis=0), ref.weight, ref.n, 5)
    # the two far clusters: one heavy edge, cut below it gives the halves, above it one cluster
    assert ref.weight[-1] >= 94 ** 2 and ref.weight[-2] <= 8 * 36     # the gap is at least 100 - 6, a cluster at most 6 wide in 8 columns
    halves = LK.cut(ref.edges, ref.weight, ref.n, 1000.0, min_cluster_size=50)
    assert halves.tolist() == [0] * 100 + [1] * 100
    assert (LK.cut(ref.edges, ref.weight, ref.n, float(ref.weight[-1])) == 0).all()
    assert (LK.cut(ref.edges, ref.weight, ref.n, -1.0) == np.arange(200)).all()
    assert LK.hdbscan_labels(ref.edges, ref.weight, ref.n, 50).tolist() == [0] * 100 + [1] * 100


# ---- the host plan of the device path --------------------------------------------------------------------------------------------------
def test_plan_through_the_library():
    """wseg_mst_scratch_bytes is host arithmetic (no device), monotone in n and d, 0 / WsegError for invalid input; the launch entry
    point validates on the host, before it touches a device, and names the argument."""
    from whisperseg_amd import _lib
    lib = _lib.load()
    pad = lambda b: max(256, -(-b // 256) * 256)
    # the norms, then min(tiles * tiles, tiles + 2048) items of 128 rows x 9 keys of 8 bytes
    for n in (1, 64, 129, 1000, 100000, 2 ** 31 - 1):
        t = -(-n // 128)
        assert LK.scratch_bytes(n, 2560) == pad(4 * n) + pad(min(t * t, t + 2048) * 128 * 9 * 8), n
    assert LK.scratch_bytes(0, 1) == 2 * 256 and LK.scratch_bytes(10, 1) == LK.scratch_bytes(10, 20480)
    sizes = (0, 1, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 4097, 100000, 131072, 131073, 10 ** 7, 2 ** 31 - 1)
    by_n = [LK.scratch_bytes(s, 80) for s in sizes]
    assert by_n == sorted(by_n) and by_n[0] < by_n[-1]
    for args, word in (((-1, 8), "n must"), ((2 ** 31, 8), "n must"), ((5, 0), "d must"), ((5, 20481), "d must")):
        assert lib.wseg_mst_scratch_bytes(*args) == 0 and word.encode() in lib.wseg_last_error(), args
        with pytest.raises(_lib.WsegError, match=word):
            LK.scratch_bytes(*args)

    def call(n=5, d=8, rows=64, core=64, comp=64, scratch=None, nbytes=0, index=64, weight=64):      # (pointers never dereferenced: every call is refused)
        return lib.wseg_mst_round_f32(rows, n, d, core, comp, scratch, nbytes, index, weight, None)

    for kw, word in ((dict(d=0), b"d must"), (dict(d=20481), b"d must"), (dict(n=-1), b"n must"), (dict(n=2 ** 31), b"n must"),
                     (dict(rows=None), b"rows"), (dict(rows=66), b"rows"), (dict(core=None), b"core"), (dict(core=65), b"core"),
                     (dict(comp=None), b"component"), (dict(comp=67), b"component"), (dict(index=None), b"index_out"),
                     (dict(weight=None), b"weight_out"), (dict(), b"scratch"), (dict(scratch=260, nbytes=1 << 30), b"scratch"),
                     (dict(scratch=256, nbytes=8), b"scratch")):
        assert call(**kw) != 0 and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())
    assert call(n=0, rows=None, core=None, comp=None, index=None, weight=None) == 0          # n == 0: nothing to do, nothing looked at


def test_plan_check_program_is_clean_under_ubsan(tmp_path):
    exe = tmp_path / "mst_plan_check"
    subprocess.check_call(["c++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "mst_plan_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])


# ---- patch_clusters and the CLI ------------------------------------------------------------------------------------------------------
def test_patch_clusters_input_errors():
    good = {"onset": [0.1, 0.2], "offset": [0.15, 0.3], "cluster": ["a", "b"], "patch": np.zeros((2, 80, 4), np.float32)}
    plain = {k: v for k, v in good.items() if k != "patch"}
    for bad in ([plain], [good, plain], [[good], plain]):
        with pytest.raises(ValueError, match="patch"):
            LK.patch_clusters(bad, 5)
    with pytest.raises(ValueError, match="different sizes"):
        LK.patch_clusters([good, dict(good, patch=np.zeros((2, 80, 5), np.float32))], 5)
    for size in (1, 0, 2.5):
        with pytest.raises(ValueError, match="min_cluster_size"):
            LK.patch_clusters([good], size)
    for s in (0, 65, 1.5):
        with pytest.raises(ValueError, match="min_samples"):
            LK.patch_clusters([good], 5, min_samples=s)
    # fewer than two rows: no tree, every row noise, no device needed
    one = {"onset": [0.1], "offset": [0.2], "cluster": ["a"], "patch": np.zeros((1, 80, 4), np.float32)}
    empty = dict(plain, onset=[], offset=[], cluster=[], patch=np.zeros((0, 80, 4), np.float32))
    for preds, rows in (([], 0), ([empty, [empty]], 0), ([one, empty], 1)):
        got = LK.patch_clusters(preds, 5)
        assert list(got) == ["cluster", "mst_edges", "mst_weight"]
        assert got["cluster"].tolist() == [-1] * rows and got["cluster"].dtype == np.int32
        assert got["mst_edges"].shape == (0, 2) and got["mst_edges"].dtype == np.int32 and got["mst_weight"].shape == (0,) and got["mst_weight"].dtype == np.float32


def test_cli_flag(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    base = ["--model_path", "m", "--csv_save_path", "o.csv"]
    patches = ["--patches", "8", "--patches_save_path", "p.npz"]
    assert segment.parse_args(base).clusters is None and segment.parse_args(base + patches).clusters is None
    args = segment.parse_args(base + patches + ["--clusters", "10"])
    assert args.clusters == 10 and args.cluster_min_samples == 5
    assert segment.parse_args(base + patches + ["--clusters", "2", "--cluster_min_samples", "64"]).cluster_min_samples == 64
    for extra in (["--clusters", "3"], patches + ["--clusters", "1"], patches + ["--clusters", "0"],
                  patches + ["--clusters", "5", "--cluster_min_samples", "0"], patches + ["--clusters", "5", "--cluster_min_samples", "65"],
                  patches + ["--cluster_min_samples", "5"]):
        with pytest.raises(SystemExit) as e:
            segment.main(base + extra)                       # refused by argparse, before a model is looked for
        assert e.value.code == 2 and "cluster" in capsys.readouterr().err
