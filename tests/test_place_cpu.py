"""Placing new calls on an existing library, on the host: whisperseg_amd.embed's membership_host, row_keys, start_host and place_host
against a second, plainly written statement bit for bit (tests/place_cases.py), the conventions of the lists, a continued run, that a
row's result does not depend on its batch, linkage's reach_of and assign_host against a brute-force restatement, that it IS a
placement (held-out blobs land among their own), argument errors, the CLI's --onto flags and the host plan of the device path
(the validation of wseg_embed_place_f64: no device needed)."""
import os
import sys

import numpy as np
import pytest

import embed_cases as EC
import place_cases as PL
from conftest import ROOT
from whisperseg_amd import embed as EM
from whisperseg_amd import linkage as LK
from whisperseg_amd import neighbors as NB


@pytest.fixture(scope="module", autouse=True)
def library():
    """The plan tests reach the host arithmetic through libwseg (no device): built here if it is not yet (a no-op otherwise)."""
    from whisperseg_amd import build
    build.build(verbose=False)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_graph(got, want):
    return (got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float64 and got[0].tolist() == list(want[0])
            and got[1].tolist() == list(want[1]) and got[2].tolist() == list(want[2]))


@pytest.mark.parametrize("n_neg", (0, 1, 5))
@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("name", PL.EXACT_CASES)
def test_definition_against_the_plain_statement(name, dim, n_neg):
    graph, y, keys, init = PL.exact_args(name, dim)
    assert same_bits(EM.start_host(graph, y), PL.plain_start(graph, y))
    want = PL.plain_place(graph, y, keys, 0, PL.EXACT_EPOCHS, PL.EXACT_EPOCHS, n_neg, 1.0, 1.0, 1.0, 1.0, init)
    got = PL.exact_reference(name, dim, n_neg)
    assert got.shape == (len(graph[0]) - 1, dim) and np.isfinite(got).all()
    assert same_bits(got, want), (int((got != want).sum()), float(np.abs(got - want).max()))


@pytest.mark.parametrize("dim", (2, 3))
def test_definition_with_a_general_b_and_other_parameters(dim):
    a, b = EM.curve_ab(0.1)
    for name, n_neg, gamma, lr in (("m65", 5, 1.0, 1.0), ("row64", 16, 2.0, 0.9), ("on_top", 1, 0.7, 1.0)):
        graph, y, keys, init = PL.exact_args(name, dim)
        want = PL.plain_place(graph, y, keys, 0, 20, 20, n_neg, gamma, lr, a, b, init)
        assert same_bits(EM.place_host(graph, y, keys, 20, n_neg=n_neg, gamma=gamma, lr=lr, a=a, b=b, init=init), want), name
    assert same_bits(EM.place_host(graph, y, keys, 20, init=init), PL.plain_place(graph, y, keys, 0, 20, 20, 5, 1.0, 1.0, a, b, init))      # the defaults


def test_lists_to_memberships_keys_and_start():
    """membership_host, row_keys and start_host on real lists (the blobs' hold-out against their library, and random rows at several
    k) equal the plain statement bit for bit; a row's nearest entry has p = 1 and the entries stand in list order."""
    lib = PL.blob_library()
    cases = [(lib["lists"], 240)]
    rows = np.random.default_rng(0).normal(size=(90, 6)).astype(np.float32)
    cases += [(NB.neighbors_host(rows[50:], rows[:50], k), 50) for k in (1, 2, 15, 64)]
    for (index, distance), n in cases:
        graph = EM.membership_host(index, distance, n)
        assert same_graph(graph, PL.plain_membership(index, distance, n))
        indptr, indices, weight = graph
        assert (weight > 0).all() and (weight <= 1).all() and (weight[indptr[:-1]] == 1).all() and len(indptr) == len(index) + 1
        assert all(indices[a:b].tolist() == index[i, :b - a].tolist() for i, (a, b) in enumerate(zip(indptr[:-1], indptr[1:])) if b - a == index.shape[1])
        keys = EM.row_keys(index, distance, 5)
        assert keys.dtype == np.uint64 and keys.tolist() == PL.plain_keys(index, distance, 5) and keys.tolist() != EM.row_keys(index, distance, 6).tolist()
        positions = np.random.default_rng(n).normal(size=(n, 3)) * 5
        assert same_bits(EM.start_host(graph, positions), PL.plain_start(graph, positions))
    # the key: by hand for one row — (j0 << 32) | the bits of the float32 distance
    assert int(EM.row_keys(np.array([[3, 1]], np.int32), np.array([[1.0, 2.0]], np.float32), 9)[0]) == EC.draw(9, (3 << 32) | 0x3F800000)


def test_membership_conventions():
    # -1 tails are ignored: what stands behind a -1 is not looked at, and the row's own arithmetic uses the WIDTH of the list (log2 k)
    rows = np.random.default_rng(1).normal(size=(9, 5)).astype(np.float32)
    index, distance = NB.neighbors_host(rows[4:], rows[:4], 6)
    assert (index[:, 4:] == -1).all() and np.isposinf(distance[:, 4:]).all()
    graph = EM.membership_host(index, distance, 4)
    assert same_graph(graph, PL.plain_membership(index, distance, 4)) and np.diff(graph[0]).tolist() == [4] * 5
    padded = EM.membership_host(index, np.where(index < 0, np.nan, distance), 4)
    assert same_graph(padded, graph)
    assert not same_graph(EM.membership_host(index[:, :4], distance[:, :4], 4), graph)
    # a corpus row listed twice counts once, at its first entry; the bisection still sees both
    index = np.array([[2, 0, 2, 1], [1, 1, 1, 1]], np.int32)
    distance = np.array([[0.5, 1.0, 1.5, 4.0], [0.25, 0.5, 1.0, 2.0]], np.float32)
    graph = EM.membership_host(index, distance, 3)
    assert same_graph(graph, PL.plain_membership(index, distance, 3))
    assert graph[0].tolist() == [0, 3, 4] and graph[1].tolist() == [2, 0, 1, 1] and graph[2][0] == 1.0 and graph[2][3] == 1.0
    # all-zero distances: every weight 1 (sigma's floor is 0 only where the bisection ran to 0, which 64 steps do not reach)
    graph = EM.membership_host(np.array([[0, 1, 2]], np.int32), np.zeros((1, 3), np.float32), 3)
    assert same_graph(graph, PL.plain_membership(np.array([[0, 1, 2]]), np.zeros((1, 3), np.float32), 3)) and graph[2].tolist() == [1.0, 1.0, 1.0]
    # k = 1: the nearest row alone, p = 1
    index, distance = NB.neighbors_host(rows[4:], rows[:4], 1)
    graph = EM.membership_host(index, distance, 4)
    assert graph[0].tolist() == list(range(6)) and graph[1].tolist() == index[:, 0].tolist() and graph[2].tolist() == [1.0] * 5
    # an entry whose p underflowed to 0 is left out
    graph = EM.membership_host(np.array([[0, 1, 2]], np.int32), np.array([[1e-12, 1e-12, 1e30]], np.float32), 3)
    assert same_graph(graph, PL.plain_membership(np.array([[0, 1, 2]]), np.array([[1e-12, 1e-12, 1e30]], np.float32), 3)) and graph[1].tolist() == [0, 1]
    # no new rows, and rows without a valid entry
    assert [len(v) for v in EM.membership_host(np.zeros((0, 5), np.int32), np.zeros((0, 5), np.float32), 3)] == [1, 0, 0]
    graph = EM.membership_host(np.full((2, 3), -1, np.int32), np.full((2, 3), np.inf, np.float32), 3)
    assert graph[0].tolist() == [0, 0, 0] and EM.row_keys(np.zeros((0, 5), np.int32), np.zeros((0, 5), np.float32), 0).shape == (0,)


def test_the_cases_hold_what_they_promise():
    assert [len(PL.exact_case(n)[0][0]) - 1 for n in ("m1", "m2", "m65")] == [1, 2, 65]
    graph, y, keys, init = PL.exact_case("n1")
    assert len(y) == 1 and set(graph[1].tolist()) == {0} and all(PL.place_negative(int(k), t, 0, s, 1) == 0 for k in keys for t in (0, 7) for s in range(5))
    assert np.diff(PL.exact_case("row64")[0][0]).tolist() == [1, 1, 64, 1, 1]
    graph, y, keys, init = PL.exact_case("empty_row")
    assert np.diff(graph[0]).tolist() == [2, 3, 1, 0, 4, 0]
    for dim in (2, 3):
        got = PL.exact_reference("empty_row", dim, 5)
        start = EM.start_host(graph, y[:, :dim])
        assert np.array_equal(got[[3, 5]], start[[3, 5]]) and not start[[3, 5]].any() and not np.array_equal(got[0], start[0])
    rate = EM.scheduled_onto(PL.exact_case("rate1")[0], 50)[2]
    assert 0.2 < (rate == 1).mean() < 0.5 and not EM.active(rate[rate == 1], np.arange(PL.EXACT_EPOCHS)[:, None]).any()
    graph, y, keys, init = PL.exact_case("on_top")
    assert np.array_equal(init[0], y[graph[1][0]]) and np.array_equal(init[1], y[PL.place_negative(int(keys[1]), 0, 0, 0, 12)])
    mass = {}
    for name in ("close", "far"):                        # the clip: most repulsion terms of "close" clip, none of "far" reaches 0.01
        graph, y, keys, init = PL.exact_args(name, 2)
        stats = {}
        PL.plain_place(graph, y, keys, 0, 1, PL.EXACT_EPOCHS, 5, 1.0, 1.0, 1.0, 1.0, init, stats)
        mass[name] = stats["sum_abs"].sum() / (2 * stats["terms"].sum())
    print("mean |g| of the first epoch:", mass)
    assert mass["close"] > 2.0 and mass["far"] < 0.01


@pytest.mark.parametrize("general", (False, True), ids=("b1", "b"))
def test_a_continued_run_gives_the_whole_runs_bits(general):
    a, b = EM.curve_ab(0.1) if general else (1.0, 1.0)
    for name, dim in (("m65", 2), ("row64", 3)):
        graph, y, keys, init = PL.exact_args(name, dim)
        whole = EM.place_host(graph, y, keys, 50, a=a, b=b, init=init)
        part = EM.place_host(graph, y, keys, (0, 20), 50, a=a, b=b, init=init)
        rest = EM.place_host(graph, y, keys, (20, 50), 50, a=a, b=b, init=part)
        assert same_bits(rest, whole) and not same_bits(part, whole), name


def blob_assignment():
    """(core, labels, reach) of the blob library at min_samples 5, min_cluster_size 15."""
    lib = PL.blob_library()
    edges, weight = LK.mst_host(lib["rows"], 5)
    labels = LK.hdbscan_labels(edges, weight, 240, 15)
    return NB.neighbors_host(lib["rows"], None, 5)[1][:, 4], labels, LK.reach_of(edges, weight, labels)


@pytest.mark.parametrize("general", (False, True), ids=("b1", "b"))
def test_a_rows_result_does_not_depend_on_its_batch(general):
    """place_host of rows A u B in shuffled order equals, row by row and bit for bit, place_host of A alone and of B alone — every
    step from the lists on; and so does assign_host."""
    a, b = EM.curve_ab(0.1) if general else (1.0, 1.0)
    lib = PL.blob_library()
    index, distance = lib["lists"]

    def placed(rows):
        i, d = index[rows], distance[rows]
        return EM.place_host(EM.membership_host(i, d, 240), lib["positions"], EM.row_keys(i, d, 4), 60, a=a, b=b)

    order = np.random.default_rng(7).permutation(60)
    both = placed(order)
    first, second = np.sort(order[:23]), np.sort(order[23:])
    where = np.argsort(order)                            # the place of row r in the shuffled batch
    assert same_bits(both[where[first]], placed(first)) and same_bits(both[where[second]], placed(second))
    assert same_bits(both[where[[17]]], placed(np.array([17]))) and not same_bits(both[:23], placed(first))
    core, labels, reach = blob_assignment()
    whole = LK.assign_host(index[order], distance[order], core, labels, reach, 5)
    assert np.array_equal(whole[where[first]], LK.assign_host(index[first], distance[first], core, labels, reach, 5))
    assert np.array_equal(whole[where[second]], LK.assign_host(index[second], distance[second], core, labels, reach, 5))


def test_reach_and_assign_against_brute_force():
    """60 random rows against a library of 80 (two loose groups and scattered rows, so that there is noise, and anchors of every
    kind): reach_of and assign_host against loops over Python floats."""
    rng = np.random.default_rng(11)
    lib = np.concatenate([rng.normal(0, 1, (35, 3)), rng.normal(6, 1, (35, 3)), rng.uniform(-6, 12, (10, 3))]).astype(np.float32)
    new = np.concatenate([rng.normal(0, 1.5, (25, 3)), rng.normal(6, 1.5, (25, 3)), rng.uniform(-8, 14, (10, 3))]).astype(np.float32)
    s, k = 4, 9
    edges, weight = LK.mst_host(lib, s)
    labels = LK.hdbscan_labels(edges, weight, 80, 8)
    assert labels.max() >= 1 and (labels == -1).any()
    reach = LK.reach_of(edges, weight, labels)
    want = [-np.inf] * (labels.max() + 1)
    for (a, b), w in zip(edges.tolist(), weight.tolist()):
        if labels[a] == labels[b] and labels[a] >= 0:
            want[labels[a]] = max(want[labels[a]], w)
    assert reach.dtype == np.float32 and reach.tolist() == want
    core = NB.neighbors_host(lib, None, s)[1][:, s - 1]
    index, distance = NB.neighbors_host(new, lib, k)
    got = LK.assign_host(index, distance, core, labels, reach, s)
    brute = []
    for q in range(60):
        ranked = sorted((max(float(distance[q, s - 1]), float(core[j]), float(distance[q, c])), int(j)) for c, j in enumerate(index[q]))
        w, anchor = ranked[0]
        brute.append(int(labels[anchor]) if labels[anchor] >= 0 and w <= want[labels[anchor]] else -1)
    assert got.dtype == np.int32 and got.tolist() == brute
    assert len(set(brute)) >= 3 and -1 in brute                         # both clusters and noise occur
    # a cluster without an inner edge: -inf, and nothing is ever assigned to it
    assert LK.reach_of(np.array([[0, 1], [1, 2]]), np.array([1.0, 2.0], np.float32), np.array([0, 0, 1])).tolist() == [1.0, -np.inf]
    assert LK.reach_of(*LK.empty_tree(), np.zeros(0, np.int32)).shape == (0,)
    assert LK.assign_host(np.array([[2, 0]], np.int32), np.array([[0.0, 1.0]], np.float32), np.zeros(3, np.float32), np.array([0, 0, 1]), np.array([1.0, -np.inf], np.float32), 1).tolist() == [-1]
    assert LK.assign_host(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), core, labels, reach, 4).shape == (0,)


def test_it_is_a_placement():
    """Three Gaussian blobs of 100 rows (embed_cases.blobs); 60 are held out, the other 240 are the library, whose map is layout_host
    of its k = 10 graph after 200 epochs.  The hold-out is placed with k = 10, 100 epochs: the 10 nearest library points on the map of
    every placed row carry its label (the reference gives 1.0).  HDBSCAN on the library (min_samples 5, min_cluster_size 15) finds
    the three blobs, every held-out row gets the cluster of its blob, and rows from far away get -1."""
    lib = PL.blob_library()
    hold = np.sort(np.random.default_rng(1).choice(300, 60, replace=False))
    assert np.array_equal(lib["new_rows"], EC.blobs()[0][hold]) and len(lib["rows"]) == 240
    index, distance = lib["lists"]
    placed = EM.place_host(EM.membership_host(index, distance, 240), lib["positions"], EM.row_keys(index, distance, 0), 100)
    purity = PL.placed_purity(placed, lib["new_labels"], lib["positions"], lib["labels"])
    print(f"purity of the placed rows among the library's points: {purity:.4f}")
    assert placed.shape == (60, 2) and np.isfinite(placed).all() and purity >= 0.99
    core, labels, reach = blob_assignment()
    assert np.bincount(labels + 1).tolist() == [0, 79, 85, 76]                                  # no noise
    blob_of = np.array([np.bincount(lib["labels"][labels == c]).argmax() for c in range(3)])
    assert sorted(blob_of.tolist()) == [0, 1, 2] and all((lib["labels"][labels == c] == blob_of[c]).all() for c in range(3))
    got = LK.assign_host(index, distance, core, labels, reach, 5)
    assert (got >= 0).all() and np.array_equal(blob_of[got], lib["new_labels"])
    # the library's own rows, presented as new ones, keep their call types (each is its own nearest library row, at distance 0)
    own_index, own_distance = NB.neighbors_host(lib["rows"], lib["rows"], 10)
    assert (own_distance[:, 0] == 0).all() and np.array_equal(LK.assign_host(own_index, own_distance, core, labels, reach, 5), labels)
    far = np.random.default_rng(5).normal(40.0, 1.0, (5, 16)).astype(np.float32)
    far_index, far_distance = NB.neighbors_host(far, lib["rows"], 10)
    print(f"reach {reach.tolist()}; the far rows' core distances {far_distance[:, 4].tolist()}")
    assert reach.max() <= 33 and far_distance[:, 4].min() > 2e4
    assert LK.assign_host(far_index, far_distance, core, labels, reach, 5).tolist() == [-1] * 5


def test_argument_errors():
    graph, y, keys, init = PL.exact_args("m65", 2)
    index, distance = np.array([[0, 1], [2, -1]], np.int32), np.array([[0.5, 1.0], [0.25, np.inf]], np.float32)
    # the conventions of the lists
    for bad in ((index, distance, 0), (index, distance, 2), (np.array([[0, -2]], np.int32), distance[:1], 3), (index, np.array([[0.5, np.nan], [0.25, np.inf]], np.float32), 3),
                (index, np.array([[0.5, np.inf], [0.25, np.inf]], np.float32), 3), (index, -distance, 3), (index.astype(np.float32), distance, 3),
                (index[0], distance[0], 3), (index, distance[:, :1], 3), (np.zeros((2, 65), np.int32), np.zeros((2, 65), np.float32), 3)):
        with pytest.raises(ValueError):
            EM.membership_host(*bad)
    for bad in ((index[0], distance[0], 0), (index, distance[:, :1], 0), (index, distance, -1), (index, distance, 2 ** 64)):
        with pytest.raises(ValueError):
            EM.row_keys(*bad)
    # the graph, the positions, the keys and the start
    wide = (np.array([0, 65]), np.arange(65, dtype=np.int32), np.ones(65))
    for fn in (EM.place_host, EM.place):                 # refused before a device is looked for
        for g, pos, k, kw in ((graph, y[:0], keys, {}), (graph, y[:30], keys, {}), (graph, np.where(y > 9, np.nan, y), keys, {}), (graph, y * np.inf, keys, {}),
                              (graph, y[:, :1], keys, {}), (graph, np.zeros((40, 4)), keys, {}), (graph, y.ravel(), keys, {}), (wide, np.zeros((70, 2)), keys[:1], {}),
                              (graph, y, keys[:-1], {}), (graph, y, keys.astype(np.int64), {}), (None, y, keys, {}), ((graph[0], graph[1], graph[2] * 2), y, keys, {}),
                              ((graph[0], graph[1], -graph[2]), y, keys, {}), ((graph[0][:-1], graph[1], graph[2]), y, keys, {}), ((graph[0], graph[1] - 1, graph[2]), y, keys, {}),
                              (graph, y, keys, dict(epochs=0)), (graph, y, keys, dict(epochs=2.5)), (graph, y, keys, dict(epochs=(3, 3))), (graph, y, keys, dict(epochs=(0, 3), total=2)),
                              (graph, y, keys, dict(n_neg=-1)), (graph, y, keys, dict(n_neg=17)), (graph, y, keys, dict(a=1.0)), (graph, y, keys, dict(a=1.0, b=0.0)),
                              (graph, y, keys, dict(gamma=np.inf)), (graph, y, keys, dict(lr=np.nan)), (graph, y, keys, dict(init=np.zeros((65, 3)))),
                              (graph, y, keys, dict(init=np.zeros((64, 2)))), (graph, y, keys, dict(init=np.full((65, 2), np.nan)))):
            with pytest.raises(ValueError):
                fn(g, pos, k, **kw)
    with pytest.raises(ValueError):
        EM.start_host(graph, y[:30])
    # transform: every argument is checked before the search looks for a device
    rows, corpus, positions = np.zeros((5, 4), np.float32), np.zeros((7, 4), np.float32), np.zeros((7, 2))
    for r, c, p, kw in ((rows, corpus, positions, dict(k=0)), (rows, corpus, positions, dict(k=65)), (rows, corpus, positions, dict(min_dist=1.0)),
                        (rows, corpus, positions, dict(spread=0.0)), (rows, corpus, positions, dict(epochs=0)), (rows, corpus, positions, dict(epochs=1.5)),
                        (rows, corpus, positions, dict(seed=-1)), (rows, corpus, positions, dict(n_neg=17)), (rows, corpus, positions[:6], {}),
                        (rows, corpus, np.zeros((7, 4)), {}), (rows, corpus, np.full((7, 2), np.inf), {}), (rows, corpus[:, :3], positions, {}),
                        (rows, corpus[:0], positions[:0], {}), (rows[:0], corpus[:0], positions[:0], {}),
                        (rows, corpus, positions, dict(lists=NB.neighbors_host(rows, corpus, 3)))):
        with pytest.raises(ValueError):
            EM.transform(r, c, p, **kw)
    none = EM.transform(rows[:0], corpus, np.zeros((7, 3)))                      # no new rows: an empty result, no device needed
    assert none.shape == (0, 3) and none.dtype == np.float32
    # assign_host and assign
    core, labels, reach = np.zeros(7, np.float32), np.zeros(7, np.int32), np.zeros(1, np.float32)
    lists = NB.neighbors_host(rows, corpus, 4)
    for i, d, c, l, r, s in ((lists[0], lists[1], core, labels, reach, 5), (lists[0], lists[1], core, labels, reach, 0), (lists[0], lists[1], core[:6], labels, reach, 2),
                             (lists[0], lists[1], core, labels + 1, reach, 2), (lists[0] + 4, lists[1], core, labels, reach, 2),
                             (np.where(np.arange(4) >= 2, -1, lists[0]), lists[1], core, labels, reach, 3), (lists[0][0], lists[1][0], core, labels, reach, 2)):
        with pytest.raises(ValueError):
            LK.assign_host(i, d, c, l, r, s)
    tree = (np.stack([np.arange(6), np.arange(1, 7)], 1).astype(np.int32), np.ones(6, np.float32))
    for kw in (dict(min_samples=0), dict(k=0), dict(k=3, min_samples=4), dict(lists=NB.neighbors_host(rows, corpus, 3))):
        with pytest.raises(ValueError):
            LK.assign(rows, corpus, labels, *tree, **kw)
    with pytest.raises(ValueError):
        LK.assign(rows, corpus, labels[:6], *tree)
    with pytest.raises(ValueError):
        LK.assign(rows, corpus, labels, tree[0][:5], tree[1][:5])
    assert LK.assign(rows[:0], corpus, labels, *tree).shape == (0,)


def test_library_and_patch_onto_arguments(tmp_path):
    from whisperseg_amd import library as LB
    patch = np.random.default_rng(3).normal(size=(6, 80, 4)).astype(np.float32)
    arch = {"patch": patch, "onset": np.arange(6.0), "patch_cluster": np.zeros(6, np.int32), "mst_edges": np.stack([np.arange(5), np.arange(1, 6)], 1).astype(np.int32),
            "mst_weight": np.ones(5, np.float32), "embedding": np.zeros((6, 3), np.float32), "pca_mean": np.zeros(320), "pca_components": np.zeros((2, 320))}
    np.savez(tmp_path / "lib.npz", **arch)
    for source in (arch, str(tmp_path / "lib.npz")):
        lib = LB.patch_library(source)
        assert set(lib) == set(LB.KEYS) and all(np.array_equal(lib[key], arch[key]) for key in lib) and lib["patch"].dtype == np.float32
    assert set(LB.patch_library({"patch": patch, "cluster": np.zeros(6)})) == {"patch"}
    for bad in ({}, {"patch": patch[0]}, dict(arch, patch_cluster=np.zeros(5, np.int32)), dict(arch, mst_edges=arch["mst_edges"][:4]),
                dict(arch, embedding=np.zeros((6, 4))), dict(arch, embedding=np.zeros((5, 2))), dict(arch, pca_mean=np.zeros(319))):
        with pytest.raises(ValueError):
            LB.patch_library(bad)
    # refused before a device is looked for: another picture shape, an empty library, arguments out of range, k below min_samples
    for new, source, kw in ((patch[:, :, :3], arch, {}), (patch[:, :40], arch, {}), (patch, {"patch": patch[:0]}, {}), (patch, arch, dict(k=0)), (patch, arch, dict(k=65)),
                            (patch, arch, dict(min_dist=1.0)), (patch, arch, dict(seed=-1)), (patch, arch, dict(min_samples=0)), (patch, arch, dict(epochs=0)),
                            (patch, arch, dict(k=3, min_samples=5)), ([{"onset": []}], arch, {})):
        with pytest.raises(ValueError):
            LB.patch_onto(new, source, **kw)
    none = LB.patch_onto(patch[:0], arch, k=4, min_samples=4)                                 # no new call: empty arrays, no device needed
    assert list(none) == ["library_index", "library_distance", "patch_cluster", "embedding", "pca_scores"]
    assert [none[key].shape for key in none] == [(0, 4), (0, 4), (0,), (0, 3), (0, 2)]
    assert [str(none[key].dtype) for key in none] == ["int32", "float32", "int32", "float32", "float32"]
    assert list(LB.patch_onto([], {"patch": patch})) == ["library_index", "library_distance"]


def test_cli_flags(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    base = ["--model_path", "m", "--csv_save_path", "o.csv"]
    patches = ["--patches", "8", "--patches_save_path", "p.npz"]
    onto = patches + ["--onto", "lib.npz"]
    assert segment.parse_args(base).onto is None and segment.parse_args(base + patches).onto is None
    args = segment.parse_args(base + onto)
    assert (args.onto, args.embed_neighbors, args.embed_min_dist, args.embed_seed, args.cluster_min_samples) == ("lib.npz", 15, 0.1, 0, 5)
    args = segment.parse_args(base + onto + ["--embed_neighbors", "7", "--embed_min_dist", "0.3", "--embed_seed", "9", "--cluster_min_samples", "3", "--neighbors", "4"])
    assert (args.embed_neighbors, args.embed_min_dist, args.embed_seed, args.cluster_min_samples, args.neighbors) == (7, 0.3, 9, 3, 4)
    for extra, word in ((["--onto", "lib.npz"], "onto"), (onto + ["--clusters", "5"], "onto"), (onto + ["--embed", "2"], "onto"), (onto + ["--pca", "2"], "onto"),
                        (patches + ["--onto", "lib.npy"], "onto"), (onto + ["--embed_neighbors", "0"], "embed_neighbors"), (onto + ["--embed_neighbors", "65"], "embed_neighbors"),
                        (onto + ["--embed_min_dist", "1"], "embed_min_dist"), (onto + ["--embed_seed", "-1"], "embed_seed"),
                        (onto + ["--cluster_min_samples", "0"], "cluster_min_samples"), (onto + ["--embed_init", "pca"], "embed_init"),
                        # without the flag, what was an error is one still
                        (patches + ["--embed_neighbors", "5"], "embed_neighbors"), (patches + ["--cluster_min_samples", "3"], "cluster_min_samples")):
        with pytest.raises(SystemExit) as e:
            segment.main(base + extra)                       # refused by argparse, before a library or a model is looked for
        assert e.value.code == 2 and word in capsys.readouterr().err, extra


def test_a_library_of_another_width_is_refused_before_the_model(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    np.savez(tmp_path / "lib.npz", patch=np.zeros((3, 80, 4), np.float32))
    with pytest.raises(SystemExit) as e:
        segment.main(["--model_path", str(tmp_path / "no_model"), "--csv_save_path", "o.csv", "--patches", "8", "--patches_save_path", "p.npz", "--onto", str(tmp_path / "lib.npz")])
    assert e.value.code == 2 and "--patches must be the library's 4" in capsys.readouterr().err


def test_plan_through_the_library():
    """wseg_embed_place_f64 validates on the host, before it touches a device, and names the argument."""
    from whisperseg_amd import _lib
    lib = _lib.load()

    def call(indptr=64, indices=64, rate=64, key=64, m=5, nnz=8, corpus=4096, n=7, dim=2, y_in=1024, y_out=2048, t0=0, t1=3, total=3, lr=1.0, a=1.0, b=1.0,
             gamma=1.0, n_neg=5):                                    # (pointers never dereferenced: every call is refused)
        return lib.wseg_embed_place_f64(indptr, indices, rate, key, m, nnz, corpus, n, dim, y_in, y_out, t0, t1, total, lr, a, b, gamma, n_neg, None)

    for kw, word in ((dict(m=-1), b"m must"), (dict(m=2 ** 31), b"m must"), (dict(n=0), b"n must"), (dict(n=-1), b"n must"), (dict(n=2 ** 31), b"n must"),
                     (dict(m=0, n=-1), b"n must"), (dict(nnz=-1), b"nnz must"), (dict(nnz=2 ** 38 + 1), b"nnz must"), (dict(dim=1), b"dim must"), (dict(dim=4), b"dim must"),
                     (dict(total=0), b"total_epochs"), (dict(total=2 ** 31), b"total_epochs"), (dict(t0=-1), b"t0"), (dict(t0=3), b"t0"), (dict(t1=4), b"t0"),
                     (dict(n_neg=-1), b"n_neg"), (dict(n_neg=17), b"n_neg"), (dict(lr=float("nan")), b"lr must"), (dict(a=-1.0), b"a must"), (dict(b=0.0), b"b must"),
                     (dict(gamma=float("inf")), b"gamma must"), (dict(indptr=None), b"indptr"), (dict(indptr=68), b"indptr"), (dict(indices=None), b"indices"),
                     (dict(indices=66), b"indices"), (dict(rate=None), b"rate"), (dict(rate=65), b"rate"), (dict(key=None), b"key"), (dict(key=68), b"key"),
                     (dict(corpus=None), b"corpus"), (dict(corpus=4100), b"corpus"), (dict(y_in=None), b"y_in"), (dict(y_in=1028), b"y_in"), (dict(y_out=None), b"y_out"),
                     (dict(y_out=2052), b"y_out"), (dict(y_out=1024), b"overlap"), (dict(y_out=1024 + 72), b"overlap"), (dict(y_out=4096 + 104), b"overlap"),
                     (dict(y_out=4096 - 8), b"overlap"), (dict(y_out=64 + 40), b"overlap"), (dict(y_out=64, indptr=8192, indices=8192, rate=8192), b"overlap"),
                     (dict(y_out=64 + 24, indptr=8192, key=8192, rate=8192), b"overlap"), (dict(y_out=64 + 24, indptr=8192, key=8192, indices=8192), b"overlap")):
        assert call(**kw) != 0 and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())
    assert call(m=0, nnz=0, n=0, indptr=None, indices=None, rate=None, key=None, corpus=None, y_in=None, y_out=None) == 0      # no new row: nothing to do, nothing looked at
