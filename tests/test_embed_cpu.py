"""whisperseg_amd/embed.py on the host: the fuzzy graph and its conventions, the curve fit against scipy's values, the hash and the
schedule on hand-computed values, the definition of the layout against a second, plainly written one bit for bit, that the cases of
the device tests hold what they promise, argument errors, the CLI's --embed flags and the host plan of the device path
(wseg_embed_scratch_bytes and the validation of wseg_embed_epochs_f64: no device needed)."""
import os
import sys

import numpy as np
import pytest

import embed_cases as EC
from conftest import ROOT
from whisperseg_amd import embed as EM
from whisperseg_amd import neighbors as NB


@pytest.fixture(scope="module", autouse=True)
def library():
    """The plan tests reach the host arithmetic through libwseg (no device): built here if it is not yet (a no-op otherwise)."""
    from whisperseg_amd import build
    build.build(verbose=False)


def dense(graph):
    indptr, indices, weight = graph
    out = np.zeros((len(indptr) - 1,) * 2)
    out[np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)), indices] = weight
    return out


def directed_weights(index, distance):
    """p(i→j) as a dense [N, N] matrix and sum_j p(i→j) per row, restated with Python floats from the docstring of fuzzy_graph_host."""
    import math
    n = len(index)
    p, sums = np.zeros((n, n)), []
    for i, (row_i, row_d) in enumerate(zip(index.tolist(), distance.astype(np.float64).tolist())):
        d = [math.sqrt(v) for j, v in zip(row_i, row_d) if j >= 0]
        rho = min([v for v in d if v > 0], default=0.0)
        psum = lambda s: sum(math.exp(-max(0.0, v - rho) / s) for v in d)
        lo, hi, mid = 0.0, math.inf, 1.0
        for _ in range(64):
            if psum(mid) > math.log2(len(row_i)):
                hi = mid
                mid = (lo + hi) / 2
            else:
                lo = mid
                mid = mid * 2 if hi == math.inf else (lo + hi) / 2
        sigma = max(mid, 1e-3 * sum(d) / len(d))
        for j, v in zip([j for j in row_i if j >= 0], d):
            p[i, j] = math.exp(-max(0.0, v - rho) / sigma)
        sums.append(psum(sigma))
    return p, np.array(sums)


def test_fuzzy_graph_of_generic_rows():
    """The module's weights against p + q - p q of an independent bisection (Python floats), entry for entry: the target log2(k), the 64
    steps and the floor of sigma all show in a weight.  At k = 2 the nearest neighbour alone meets the target, the bisection runs to
    2^-64 and the floor 1e-3 * mean d IS sigma."""
    rows = np.random.default_rng(0).normal(size=(200, 8)).astype(np.float32)
    for k in (5, 15, 2):
        index, distance = NB.neighbors_host(rows, None, k)
        indptr, indices, weight = graph = EM.fuzzy_graph_host(index, distance)
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and weight.dtype == np.float64
        assert indptr.shape == (201,) and indptr[0] == 0 and indptr[-1] == len(indices) == len(weight)
        w = dense(graph)
        assert np.array_equal(w, w.T) and not np.diag(w).any() and (weight > 0).all() and (weight <= 1).all()
        assert all((np.diff(indices[a:b]) > 0).all() for a, b in zip(indptr[:-1], indptr[1:]))
        p, sums = directed_weights(index, distance)
        want = np.minimum(1.0, p + p.T - p * p.T)
        print(f"k {k}: largest difference of a weight from the restated p + q - p q {np.abs(w - want).max():.3g}; weights {weight.min():.3g} .. {weight.max():.3g}")
        # (the two bisections sum exp() of two libraries: a last-bit difference of sigma moves a weight by a few 1e-16)
        assert np.abs(w - want).max() <= 1e-14 and np.array_equal(w > 0, want > 0)
        if k == 2:                                                       # the floor decides every sigma: the weights are far from 0 / 1 patterns
            assert ((weight > 1e-300) & (weight < 0.5)).sum() > 50
            continue
        listed = np.zeros((200, 200), bool)
        listed[np.repeat(np.arange(200), k), index.ravel()] = True
        assert np.array_equal(w > 0, listed | listed.T)
        # the bisection met its target: sum_j p(i→j) = log2(k), for the p that the module's weights were just compared with
        assert np.abs(sums - np.log2(k)).max() <= 1e-5
        assert (w[np.arange(200), index[:, 0]] >= 1 - 4e-16).all()      # the nearest neighbour: d == rho, p == 1, w == 1 to the rounding of 1 + q - q


def test_fuzzy_graph_conventions():
    # all neighbours duplicates of the row: every weight 1
    rows = np.zeros((6, 3), np.float32)
    rows[3:] = 5
    index, distance = NB.neighbors_host(rows, None, 2)
    assert (distance == 0).all()
    graph = EM.fuzzy_graph_host(index, distance)
    assert (graph[2] == 1).all() and np.array_equal(dense(graph) > 0, np.kron(np.eye(2), np.ones((3, 3))) - np.eye(6) > 0)
    # -1 tails are ignored: the lists of 4 rows at k = 6 give the graph of k = 3 (log2 of ANOTHER k: other weights, the same pairs)
    rows = np.random.default_rng(1).normal(size=(4, 5)).astype(np.float32)
    index, distance = NB.neighbors_host(rows, None, 6)
    assert (index[:, 3:] == -1).all() and np.isposinf(distance[:, 3:]).all()
    graph = EM.fuzzy_graph_host(index, distance)
    assert np.array_equal(dense(graph) > 0, ~np.eye(4, dtype=bool)) and np.isfinite(graph[2]).all()
    padded = EM.fuzzy_graph_host(np.concatenate([index[:, :3], np.full((4, 3), -1, np.int32)], 1), np.concatenate([distance[:, :3], np.full((4, 3), np.nan, np.float32)], 1))
    assert all(np.array_equal(a, b) for a, b in zip(graph, padded))             # what stands behind a -1 is not looked at
    # N = 2: one edge of weight 1, whatever the distance
    index, distance = NB.neighbors_host(np.array([[0.0], [3.0]], np.float32), None, 15)
    indptr, indices, weight = EM.fuzzy_graph_host(index, distance)
    assert indptr.tolist() == [0, 1, 2] and indices.tolist() == [1, 0] and weight.tolist() == [1.0, 1.0]
    # no rows, one row, a row's own index
    assert [len(v) for v in EM.fuzzy_graph_host(np.zeros((0, 5), np.int32), np.zeros((0, 5), np.float32))] == [1, 0, 0]
    indptr, indices, _ = EM.fuzzy_graph_host(np.full((1, 5), -1, np.int32), np.full((1, 5), np.inf, np.float32))
    assert indptr.tolist() == [0, 0] and len(indices) == 0
    assert not dense(EM.fuzzy_graph_host(np.array([[0, 1], [1, 0]], np.int32), np.array([[0, 1], [0, 1]], np.float32))).diagonal().any()
    for bad in ((np.zeros((3, 2), np.int32), np.zeros((3, 3), np.float32)), (np.zeros(3, np.int32), np.zeros(3, np.float32)),
                (np.full((3, 2), 3, np.int32), np.zeros((3, 2), np.float32)), (np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float32)),
                (np.ones((3, 2), np.int32), np.full((3, 2), np.nan, np.float32)), (np.ones((3, 2), np.int32), np.full((3, 2), -1, np.float32))):
        with pytest.raises(ValueError):
            EM.fuzzy_graph_host(*bad)


@pytest.mark.parametrize("min_dist, a, b", [(0.0, 1.9328, 0.7905), (0.1, 1.5769, 0.8951), (0.25, 1.1214, 1.0575), (0.5, 0.5830, 1.3342), (0.8, 0.2321, 1.6812)])
def test_curve_ab_meets_scipys_fit(min_dist, a, b):
    got = EM.curve_ab(min_dist)
    print(f"min_dist {min_dist}: a {got[0]:.6f}, b {got[1]:.6f}")
    assert abs(got[0] - a) <= 1e-3 and abs(got[1] - b) <= 1e-3
    assert got == EM.curve_ab(min_dist, 1.0) and all(isinstance(v, float) for v in got)


def test_hash_and_schedule_by_hand():
    # SplitMix64 seeded with 0 gives 0xE220A8397B1DCDAF first: the finaliser of the golden-ratio increment
    assert EC.draw(1, 0) == 0xE220A8397B1DCDAF and EC.mix(0) == 0 and EC.mix(1) == 0x5692161D100B05E5
    assert int(EM.draw(1, [0])[0]) == 0xE220A8397B1DCDAF and int(EM.mix64([1])[0]) == 0x5692161D100B05E5
    # (seed, t, nnz, e, n_neg, s, n) -> the draw and the vertex, computed with Python integers
    for args, h, m in (((0, 0, 10, 0, 5, 0, 7), 0x0, 0), ((1, 3, 10, 4, 5, 2, 7), 0x57C4944FBF781144, 2),
                       ((12345, 49, 4510, 4509, 5, 4, 300), 0xDDF4AE7A429AB99C, 260),
                       ((2 ** 64 - 1, 199, 2 ** 38, 2 ** 38 - 1, 16, 15, 2 ** 31 - 1), 0x52EE6324D514B7DD, 695677329)):
        seed, t, nnz, e, n_neg, s, n = args
        counter = ((t * nnz + e) * n_neg + s) % 2 ** 64
        assert EC.draw(seed, counter) == h and ((h >> 32) * n) >> 32 == m == EC.negative(*args)
        assert int(EM.draw(seed, [counter])[0]) == h and EM.negatives(seed, t, nnz, [e], n_neg, n)[0, s] == m
    many = EM.negatives(9, 17, 1000, np.arange(1000), 5, 300)
    assert many.shape == (1000, 5) and many.min() == 0 and many.max() == 299 and abs(many.mean() - 149.5) < 5
    assert many[123, 3] == EC.negative(9, 17, 1000, 123, 5, 3, 300)
    # the start: [-10, 10), the same hash on the counters 2^63 + i dim + c
    assert EC.draw(0, 1 << 63) == 0x25C26EA579CEA98A and EC.draw(7, (1 << 63) + 5) == 0x819986666E011292
    y0 = EM.init_positions(2, 2, 0)
    assert y0.tolist() == EC.plain_init(2, 2, 0) == [[-7.0500389976622095, -7.281791342148216], [8.241737271429802, -7.652770238455073]]
    assert EM.init_positions(3, 3, 7)[1, 2] == -10 + 20 * ((0x819986666E011292 >> 11) * 2.0 ** -53)
    big = EM.init_positions(5000, 3, 1)
    assert big.min() >= -10 and big.max() < 10 and abs(big.mean()) < 0.2 and not np.array_equal(big, EM.init_positions(5000, 3, 2))
    # the rates and the schedule
    assert EM.rates([1.0, 0.5, 0.25, 1 / 65536, 0.4 / 65536, 0.6 / 65536, 0.0]).tolist() == [65536, 32768, 16384, 1, 0, 1, 0]
    assert EM.rates([0.2, 0.1]).tolist() == [65536, 32768] and EM.rates([]).dtype == np.uint32
    on = np.array([EM.active([65536, 32768, 1, 3, 0], t) for t in range(65536)])
    assert on[:, 0].all() and np.array_equal(np.flatnonzero(on[:, 1]), np.arange(1, 65536, 2))
    assert np.flatnonzero(on[:, 2]).tolist() == [65535] and on[:, 3].sum() == 3 and not on[:, 4].any()
    assert all(bool(on[t, c]) == EC.is_active(r, t) for c, r in enumerate((65536, 32768, 1, 3, 0)) for t in (0, 1, 2, 21845, 21846, 65535))
    assert EM.active([65536, 40000], 2 ** 31 - 2).tolist() == [True, EC.is_active(40000, 2 ** 31 - 2)]
    # entries of rate 0 leave the CSR before anything runs
    indptr, indices, rate = EM.scheduled((np.array([0, 2, 3, 5]), np.array([1, 2, 0, 0, 1]), np.array([1.0, 1e-6, 1.0, 1e-6, 0.5])))
    assert indptr.tolist() == [0, 1, 2, 3] and indices.tolist() == [1, 0, 1] and rate.tolist() == [65536, 65536, 32768]


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("general", (False, True), ids=("b1", "b"))
def test_definition_against_a_plain_double_loop(dim, general):
    """Bit for bit at N = 7: hashed start and a given one, every n_neg class, a continued run."""
    a, b = EM.curve_ab(0.1) if general else (1.0, 1.0)
    indptr, indices, weight = EC.ring_with_chords(7, 3)
    j = int(indices[0])                                             # the first edge, 0 - j, gets a weight whose rate is 0: it leaves the CSR
    weight = weight.copy()                                          # on both sides and every later entry moves up by one or two
    weight[0] = weight[indptr[j] + indices[indptr[j]:indptr[j + 1]].tolist().index(0)] = 1e-6
    graph = (indptr, indices, weight)
    plain = EC.plain_schedule(graph)
    assert len(indptr) == 8 and len(plain[1]) == len(indices) - 2 and min(plain[2]) > 0 and min(plain[2]) < 65536 == max(plain[2])
    assert [v.tolist() for v in EM.scheduled(graph)] == list(plain)
    for n_neg, init, gamma, lr in ((5, None, 1.0, 1.0), (0, None, 1.0, 1.0), (1, np.random.default_rng(2).normal(size=(7, dim)) * 30, 0.7, 0.9), (16, None, 2.0, 1.0)):
        want = EC.plain_layout(graph, dim, 0, 20, 20, n_neg, gamma, lr, a, b, init, 5)
        got = EM.layout_host(graph, dim, 20, n_neg=n_neg, gamma=gamma, lr=lr, a=a, b=b, init=init, seed=5)
        assert got.dtype == np.float64 and got.shape == (7, dim) and np.isfinite(got).all()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n_neg, np.abs(got - want).max())
        part = EM.layout_host(graph, dim, (0, 8), 20, n_neg=n_neg, gamma=gamma, lr=lr, a=a, b=b, init=init, seed=5)
        rest = EM.layout_host(graph, dim, (8, 20), 20, n_neg=n_neg, gamma=gamma, lr=lr, a=a, b=b, init=part, seed=5)
        assert np.array_equal(rest.view(np.uint64), want.view(np.uint64)) and not np.array_equal(part, want)
    assert not np.array_equal(got, EM.layout_host(graph, dim, 20, n_neg=16, gamma=2.0, a=a, b=b, seed=6))        # the seed matters


def test_the_cases_hold_what_they_promise():
    """The graphs of the device tests: symmetric CSRs that take the paths their names say, with a definition that stays finite."""
    for name in EC.EXACT_CASES:
        graph, init = EC.exact_case(name)
        w = dense(graph)
        assert np.array_equal(w, w.T) and not np.diag(w).any(), name
        for dim in (2, 3):
            y = EC.exact_reference(name, dim, 5)
            assert y.shape == (len(w), dim) and np.isfinite(y).all(), name
    assert [len(EC.exact_case(n)[0][0]) - 1 for n in ("n1", "n2", "n3", "n65")] == [1, 2, 3, 65]
    share = np.mean([EC.negative(3, t, 2, e, 5, s, 2) == e for t in range(50) for e in (0, 1) for s in range(5)])
    assert 0.3 < share < 0.7                                                      # N = 2: about half of the negatives are the vertex itself
    degree = np.diff(EC.exact_case("star257")[0][0])
    assert degree[0] == 256 and (degree[1:] == 1).all()
    degree = np.diff(EC.exact_case("isolated")[0][0])
    assert degree[7] == 0 and degree[39] == 0 and (np.delete(degree, [7, 39]) > 0).all()
    for dim in (2, 3):
        assert np.array_equal(EC.exact_reference("isolated", dim, 5)[[7, 39]], EM.init_positions(40, dim, 3)[[7, 39]])
    rate = EM.scheduled(EC.exact_case("rate1")[0])[2]
    assert 0.2 < (rate == 1).mean() < 0.5 and not EM.active(rate[rate == 1], np.arange(EC.EXACT_EPOCHS)[:, None]).any()
    graph, init = EC.exact_case("twins")
    assert np.array_equal(init[0], init[1]) and 1 in graph[1][graph[0][0]:graph[0][1]] and np.array_equal(init[0], init[5])
    assert any(EC.negative(3, 0, len(graph[1]), e, 5, s, 12) == 5 for e in range(graph[0][0], graph[0][1]) for s in range(5))
    # the clip: with a = b = 1 an attraction term is 2 delta / (1 + d2), at most 1, so only repulsion terms clip, and only near by.
    # In the first epoch of "close" most of them do (a clipped term weighs 4); in "far" no term reaches 0.01
    mass = {}
    for name in ("close", "far"):
        graph, init = EC.exact_case(name)
        stats = {}
        EC.plain_layout(graph, 2, 0, 1, EC.EXACT_EPOCHS, 5, 1.0, 1.0, 1.0, 1.0, init[:, :2], 3, stats)
        mass[name] = stats["sum_abs"].sum() / (2 * stats["terms"].sum())
    print("mean |g| of the first epoch:", mass)
    assert mass["close"] > 2.0 and mass["far"] < 0.01
    # the blobs: the definition itself draws a map (the device test repeats this next to the device's)
    rows, labels = EC.blobs()
    assert rows.shape == (300, 16) and rows.dtype == np.float32 and np.bincount(labels).tolist() == [100, 100, 100]
    assert EC.purity(rows, labels) == 1.0 and EC.purity(np.random.default_rng(0).normal(size=(300, 2)), labels) < 0.5
    assert EC.purity(EM.layout_host(EC.blob_graph(), 2, 200), labels) >= 0.99


def test_argument_errors():
    graph = EC.ring_with_chords(7, 3)
    for kw in (dict(dim=1), dict(dim=4), dict(dim=2.0), dict(dim=True), dict(epochs=0), dict(epochs=-3), dict(epochs=2.5), dict(epochs=(3, 3)),
               dict(epochs=(5, 3)), dict(epochs=(-1, 3)), dict(epochs=(0, 3), total=2), dict(epochs=(0, 1, 2)), dict(epochs=5, total=0), dict(n_neg=-1),
               dict(n_neg=17), dict(n_neg=1.5), dict(seed=-1), dict(seed=2 ** 64), dict(a=1.0), dict(b=1.0), dict(a=-1.0, b=1.0), dict(a=1.0, b=0.0),
               dict(a=np.nan, b=1.0), dict(gamma=np.inf), dict(lr=np.nan), dict(init=np.zeros((7, 3))), dict(init=np.zeros((6, 2))),
               dict(init=np.full((7, 2), np.nan)), dict(init=np.full((7, 2), np.inf)), dict(init=np.zeros(14))):
        for fn in (EM.layout_host, EM.layout):                       # refused before a device is looked for
            with pytest.raises(ValueError):
                fn(graph, **kw)
    for bad in (None, graph[:2], (graph[0][:-1], graph[1], graph[2]), (graph[0], graph[1] + 7, graph[2]), (graph[0], graph[1], -graph[2]),
                (graph[0], graph[1], graph[2][:-1]), (graph[0][::-1], graph[1], graph[2]), (graph[0], graph[1], np.where(graph[2] < 2, np.nan, 0))):
        with pytest.raises(ValueError):
            EM.layout_host(bad)
    rows = np.zeros((5, 4), np.float32)
    for kw in (dict(k=0), dict(k=65), dict(dim=1), dict(dim=4), dict(epochs=0), dict(epochs=1.5), dict(min_dist=-0.1), dict(min_dist=1.0),
               dict(min_dist=np.nan), dict(min_dist=0.5, spread=0.5), dict(spread=0.0), dict(n_neg=17), dict(seed=-1), dict(init=np.full((5, 2), np.inf))):
        with pytest.raises(ValueError):
            EM.embed(rows, **kw)                                     # refused before the search looks for a device
    lists = NB.neighbors_host(rows, None, 15)
    for kw in (dict(n_neg=17), dict(seed=-1), dict(init=np.full((5, 2), np.inf)), dict(init=np.zeros((5, 3)))):
        with pytest.raises(ValueError):
            EM.embed(rows, lists=lists, **kw)
    with pytest.raises(ValueError, match="lists"):
        EM.embed(rows, lists=NB.neighbors_host(rows, None, 3))
    for md in (-0.5, 1.0, 2.0):
        with pytest.raises(ValueError, match="min_dist"):
            EM.curve_ab(md)
    assert EM.curve_ab(1.5, 2.0)[1] > 0
    # no rows: an empty map, no device needed
    assert EM.embed(np.zeros((0, 4), np.float32), dim=3).shape == (0, 3) and EM.embed(np.zeros((0, 4), np.float32)).dtype == np.float32
    good = {"onset": [0.1, 0.2], "offset": [0.15, 0.3], "cluster": ["a", "b"], "patch": np.zeros((2, 80, 4), np.float32)}
    plain = {k: v for k, v in good.items() if k != "patch"}
    with pytest.raises(ValueError, match="patch"):
        EM.patch_embedding([good, plain])
    for kw in (dict(k=0), dict(dim=5), dict(epochs=0), dict(min_dist=1.0)):
        with pytest.raises(ValueError):
            EM.patch_embedding([good], **kw)
    none = EM.patch_embedding([], dim=3)
    assert list(none) == ["embedding"] and none["embedding"].shape == (0, 3) and none["embedding"].dtype == np.float32
    empty = dict(plain, onset=[], offset=[], cluster=[], patch=np.zeros((0, 80, 4), np.float32))
    assert EM.patch_embedding([empty, [empty]])["embedding"].shape == (0, 2)
    # a graph without an entry: the definition leaves the start where it is
    lone = (np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0))
    assert np.array_equal(EM.layout_host(lone, 3, 9, seed=4), EM.init_positions(3, 3, 4))
    assert np.array_equal(EM.layout_host(lone, 2, 9, init=np.ones((3, 2))), np.ones((3, 2)))


def test_cli_flags(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    base = ["--model_path", "m", "--csv_save_path", "o.csv"]
    patches = ["--patches", "8", "--patches_save_path", "p.npz"]
    assert segment.parse_args(base).embed is None and segment.parse_args(base + patches).embed is None
    args = segment.parse_args(base + patches + ["--embed", "2"])
    assert (args.embed, args.embed_neighbors, args.embed_min_dist, args.embed_seed) == (2, 15, 0.1, 0)
    args = segment.parse_args(base + patches + ["--embed", "3", "--embed_neighbors", "64", "--embed_min_dist", "0", "--embed_seed", "18446744073709551615"])
    assert (args.embed, args.embed_neighbors, args.embed_min_dist, args.embed_seed) == (3, 64, 0.0, 2 ** 64 - 1)
    for extra, word in ((["--embed", "2"], "embed"), (patches + ["--embed", "1"], "embed"), (patches + ["--embed", "4"], "embed"),
                        (patches + ["--embed", "2", "--embed_neighbors", "0"], "embed_neighbors"), (patches + ["--embed", "2", "--embed_neighbors", "65"], "embed_neighbors"),
                        (patches + ["--embed", "2", "--embed_min_dist", "1"], "embed_min_dist"), (patches + ["--embed", "2", "--embed_min_dist", "-0.1"], "embed_min_dist"),
                        (patches + ["--embed", "2", "--embed_min_dist", "nan"], "embed_min_dist"), (patches + ["--embed", "2", "--embed_seed", "-1"], "embed_seed"),
                        (patches + ["--embed_neighbors", "5"], "embed_neighbors"), (patches + ["--embed_min_dist", "0.2"], "embed_min_dist"),
                        (patches + ["--embed_seed", "1"], "embed_seed")):
        with pytest.raises(SystemExit) as e:
            segment.main(base + extra)                       # refused by argparse, before a model is looked for
        assert e.value.code == 2 and word in capsys.readouterr().err, extra


def test_plan_through_the_library():
    """wseg_embed_scratch_bytes is host arithmetic (no device); the launch entry point validates on the host, before it touches a
    device, and names the argument."""
    from whisperseg_amd import _lib
    lib = _lib.load()
    pad = lambda b: max(256, -(-b // 256) * 256)
    for n in (0, 1, 15, 16, 17, 64, 65, 1000, 100000, 2 ** 31 - 1):
        for dim in (2, 3):
            assert EM.scratch_bytes(n, dim) == pad(8 * n * dim), (n, dim)
    for args, word in (((-1, 2), "n must"), ((2 ** 31, 2), "n must"), ((5, 1), "dim must"), ((5, 4), "dim must")):
        assert lib.wseg_embed_scratch_bytes(*args) == 0 and word.encode() in lib.wseg_last_error(), args
        with pytest.raises(_lib.WsegError, match=word):
            EM.scratch_bytes(*args)

    def call(indptr=64, indices=64, rate=64, n=5, nnz=8, dim=2, y_in=1024, y_out=2048, scratch=None, nbytes=0, t0=0, t1=3, total=3, lr=1.0, a=1.0,
             b=1.0, gamma=1.0, n_neg=5, seed=0):                     # (pointers never dereferenced: every call is refused)
        return lib.wseg_embed_epochs_f64(indptr, indices, rate, n, nnz, dim, y_in, y_out, scratch, nbytes, t0, t1, total, lr, a, b, gamma, n_neg, seed, None)

    for kw, word in ((dict(n=-1), b"n must"), (dict(n=2 ** 31), b"n must"), (dict(nnz=-1), b"nnz must"), (dict(nnz=2 ** 38 + 1), b"nnz must"),
                     (dict(dim=1), b"dim must"), (dict(dim=4), b"dim must"), (dict(total=0), b"total_epochs"), (dict(total=2 ** 31), b"total_epochs"),
                     (dict(t0=-1), b"t0"), (dict(t0=3), b"t0"), (dict(t1=4), b"t0"), (dict(n_neg=-1), b"n_neg"), (dict(n_neg=17), b"n_neg"),
                     (dict(lr=float("nan")), b"lr must"), (dict(a=-1.0), b"a must"), (dict(a=float("inf")), b"a must"), (dict(b=0.0), b"b must"),
                     (dict(b=float("nan")), b"b must"), (dict(gamma=float("inf")), b"gamma must"), (dict(indptr=None), b"indptr"),
                     (dict(indptr=68), b"indptr"), (dict(indices=None), b"indices"), (dict(indices=66), b"indices"), (dict(rate=None), b"rate"),
                     (dict(rate=65), b"rate"), (dict(y_in=None), b"y_in"), (dict(y_in=1028), b"y_in"), (dict(y_out=None), b"y_out"),
                     (dict(y_out=2052), b"y_out"), (dict(), b"scratch"), (dict(scratch=4100, nbytes=1 << 20), b"scratch"),
                     (dict(scratch=4096, nbytes=255), b"scratch"), (dict(scratch=4096, nbytes=256, y_out=1024), b"overlap"),
                     (dict(scratch=4096, nbytes=256, y_out=1024 + 72), b"overlap"), (dict(scratch=2048 + 8, nbytes=256), b"overlap"),
                     (dict(scratch=1024 - 8, nbytes=256), b"overlap")):
        assert call(**kw) != 0 and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())
    assert call(n=0, nnz=0, indptr=None, indices=None, rate=None, y_in=None, y_out=None) == 0      # n == 0: nothing to do, nothing looked at
