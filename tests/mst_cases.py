"""Inputs of the minimum-spanning-tree tests (tests/test_mst_cpu.py, tests/test_mst_gpu.py), the numpy statement of one Boruvka
round, what the device may differ from the definition whisperseg_amd.linkage.mst_host by, and the checks of that contract.

EXACT CASES.  Integer rows in -3 .. 3 (every product, norm and d^ an integer below 9 * 20 480 * 4 < 2^24), rows that are multiples of
2^-6 in [-2, 2] with D <= 64 (every product a multiple of 2^-12 of at most 4, every sum of 64 of them and every d^ <= 4 * 256 a
multiple of 2^-12 below 2^10 = 2^22 * 2^-12: exact in float32) and two integer clusters 100 apart in one column with D = 8 (sums
below 8 * 2 * 103^2 < 2^18): there the selection's w^ IS w, so a round must reproduce its numpy statement entry for entry and
linkage.mst the tree of mst_host edge for edge, weight bits included, the mass ties with it.

THE SLACK on inexact float rows (derived, not measured).  With u = 2^-24, tests/knn_cases.py derives |d^(i, j) - d(i, j)| <=
2 (D + 4) u (|x_i|^2 + |x_j|^2) <= tau = 2 (D + 4) u * 2 max_i |x_i|^2 for the c-ordered fmaf chains both searches share.
  1. The core distances come from the nearest-neighbour search, whose s-th neighbour may be exchanged for one within 2 tau: the
     device's core' lies in [core, core + 2 tau], and so does w' = max(core'_i, core'_j, d32) in [w, w + 2 tau].
  2. A round ranks by w^' = max(core'_i, core'_j, d^), within tau of w', keeps the nine best and re-ranks them by w': the candidate a
     row reports is within 2 tau of the row's true minimum of w' (nine candidates ranked before the true one by w^' are each
     within 2 tau of it), and so is the edge a component takes.
  3. Lower w' by 2 tau on the edges the device took and call it w''.  Every edge of the device's tree is then a lightest edge
     leaving the component that took it, so the tree is a minimum spanning tree of w'', and w - 2 tau <= w'' <= w + 2 tau.
  4. The k-th smallest weight of a minimum spanning tree is monotone in the weight function, and it is the smallest k-th weight any
     spanning tree has.  With m_k, t_k the k-th sorted weights of the definition's tree (under w) and of the device's (as reported:
     w' = w'' + 2 tau on its edges):   t_k <= m_k + 2 tau + 2 tau = m_k + SLACK, SLACK = 4 tau,   and t_k >= m_k up to the
     one float32 ulp a reported weight may differ from the definition's w of its edge (the fp64 sum rounds once; see knn_cases).
"""
import functools

import numpy as np

import knn_cases as KC
from whisperseg_amd import linkage as LK
from whisperseg_amd import neighbors as NB

SEED = 20261021
U = 2.0 ** -24

ROUND_N = (2, 3, 127, 128, 129, 257, 1000)
ROUND_D = (1, 3, 4, 16, 17, 2562)
# (kind, N, D, s) of the whole trees on exact inputs: duplicates in mass at the three s classes; several tiles; all rows identical;
# the dyadic rows; two far clusters joined by one heavy edge; the scalar loads on long rows
EXACT_TREES = (("integer", 257, 3, 1), ("integer", 257, 3, 5), ("integer", 257, 3, 64), ("integer", 500, 17, 5), ("integer", 1000, 16, 15),
               ("identical", 130, 4, 5), ("dyadic", 300, 64, 5), ("dyadic", 129, 5, 15), ("far", 200, 8, 5), ("far", 200, 8, 64),
               ("integer", 130, 2562, 1))
FLOAT_TREES = ((64, 1000, 5), (2560, 1000, 5))           # (D, N, s): clustered Gaussian rows as in knn_cases


@functools.lru_cache(maxsize=None)
def rows_of(kind, n, d):
    rng = np.random.default_rng([SEED, n, d])
    if kind == "integer":
        rows = KC.integer_rows(n, d)
    elif kind == "identical":
        rows = np.tile(rng.integers(-3, 4, size=(1, d)).astype(np.float32), (n, 1))
    elif kind == "dyadic":
        rows = (rng.integers(-128, 129, size=(n, d)) / 64.0).astype(np.float32)
        rows[n // 2:n // 2 + 7] = rows[:7]                                  # and a few duplicates
    elif kind == "far":
        rows = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
        rows[n // 2:, 0] += 100.0
    elif kind == "clustered":
        rows = KC.clustered_rows(d, n)
    else:
        raise KeyError(kind)
    rows = np.ascontiguousarray(rows)
    rows.setflags(write=False)
    return rows


class Reference:
    """The definition on (rows, s), computed once: core, the dense w, the tree."""

    def __init__(self, rows, s):
        self.x, self.s = np.asarray(rows, np.float32), s
        self.n, self.d = self.x.shape
        self.core, self.w = LK.weights_host(self.x, s)
        self.edges, self.weight = LK.mst_of_weights(self.w)                 # (mst_host, without forming w a second time)
        for a in (self.core, self.w, self.edges, self.weight):
            a.setflags(write=False)
        self.tau = 2.0 * (self.d + 4) * U * 2.0 * float((self.x.astype(np.float64) ** 2).sum(axis=1).max())
        self.slack = 4.0 * self.tau


@functools.lru_cache(maxsize=None)
def reference(kind, n, d, s):
    return Reference(rows_of(kind, n, d), s)


def components_of(pattern, n):
    """int32 [n]: "mod3" i % 3; "one" all rows in one component; "alone" row n // 2 against the rest; "blocks" contiguous blocks cut
    at the tile boundaries (labels that are no row numbers: only equality counts)."""
    i = np.arange(n)
    return {"mod3": i % 3, "one": np.full(n, 7), "alone": np.where(i == n // 2, -5, 1 << 20), "blocks": 1000 - i // 128}[pattern].astype(np.int32)


PATTERNS = ("mod3", "one", "alone", "blocks")


def round_host(w, component):
    """One round in numpy on the dense w [N, N]: for every row the first j of another component in the order (w, j), and its weight;
    -1 / +inf where there is none."""
    masked = np.where(component[:, None] != component[None, :], w, np.float32(np.inf))
    index = np.argmin(masked, axis=1).astype(np.int32)                     # the first of equal values: the lower j
    weight = masked[np.arange(len(w)), index].astype(np.float32)
    index[np.isposinf(weight)] = -1
    return index, weight


def boruvka_host(ref, stats=None):
    """The tree by the rounds' rules, all in numpy: round_host feeding the host bookkeeping of linkage.mst."""
    return LK.boruvka(ref.n, lambda labels: round_host(ref.w, labels), stats)


def same_tree(a, b):
    return (a[0].dtype == b[0].dtype == np.int32 and a[1].dtype == b[1].dtype == np.float32 and np.array_equal(a[0], b[0])
            and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def check_spanning(edges, weight, n, what=""):
    """N - 1 edges a < b that join all rows, ascending in (w, a, b)."""
    assert edges.dtype == np.int32 and weight.dtype == np.float32 and edges.shape == (max(n - 1, 0), 2) and weight.shape == (max(n - 1, 0),), (what, edges.shape)
    if n < 2:
        return
    assert (edges[:, 0] >= 0).all() and (edges[:, 0] < edges[:, 1]).all() and (edges[:, 1] < n).all(), what
    assert np.array_equal(np.lexsort((edges[:, 1], edges[:, 0], weight)), np.arange(n - 1)), (what, "not ascending in (w, a, b)")
    parent = np.arange(n)
    for a, b in edges:
        ra, rb = LK.find(parent, a), LK.find(parent, b)
        assert ra != rb, (what, "a cycle", int(a), int(b))
        parent[rb] = ra
    assert len(np.unique(LK.roots_of(parent))) == 1, (what, "the edges do not span the rows")


def check_contract(ref, edges, weight, what=""):
    """Inexact float rows: a spanning tree; every weight the definition's w of that very edge to 1 float32 ulp; the sorted weights
    between the definition's - 1 ulp and + SLACK -> (largest share of the slack used, share of edges that are the definition's)."""
    check_spanning(edges, weight, ref.n, what)
    want = ref.w[edges[:, 0], edges[:, 1]]
    off = np.abs(weight.astype(np.float64) - want.astype(np.float64))
    assert (off <= np.spacing(want).astype(np.float64)).all(), (what, "a weight is not w of its edge", int(np.argmax(off)), float(off.max()))
    m, t = ref.weight.astype(np.float64), np.sort(weight).astype(np.float64)
    assert (t >= m - np.spacing(ref.weight).astype(np.float64)).all(), (what, "a sorted weight below the minimum spanning tree's")
    used = (t - m) / ref.slack
    assert (used <= 1.0).all(), (what, "a sorted weight beyond the slack", float(used.max()), ref.slack)
    mine = {(int(a), int(b)) for a, b in edges}
    same = sum((int(a), int(b)) in mine for a, b in ref.edges) / max(len(ref.edges), 1)
    return float(max(used.max(), 0.0)), same
