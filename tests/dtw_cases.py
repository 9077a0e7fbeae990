"""Inputs of the dynamic-time-warping tests (tests/test_dtw_cpu.py, tests/test_dtw_gpu.py), what the device may differ from the
definition whisperseg_amd.dtw.dtw_neighbors_host by, and the check of that contract.

THE SLACK (derived, not measured).  The device selects by G^, the recurrence in float32 over the costs c^(a, b) = |q_a|^2 + |x_b|^2 -
2 q_a.x_b, every term ONE fmaf chain over the C channels of a column.  With u = 2^-24:

  * a cell is within 2 (C + 4) u (|q_a|^2 + |x_b|^2) of c(a, b): the bound of tests/knn_cases.py on a pair of rows of dimension C;
    with E_i = max_a |q_i[:, a]|^2 + max_{j, b} |x_j[:, b]|^2 that is at most 2 (C + 4) u E_i, and c(a, b) itself is at most
    2 E_i ((q - x)^2 <= 2 q^2 + 2 x^2);
  * a warping path has at most 2 T - 1 cells, so the exact sum of its float32 costs is within (2 T - 1) 2 (C + 4) u E_i of the sum
    of the definition's;
  * the float32 running sum along a path rounds at most 2 T - 1 times, each time a partial sum of at most (2 T - 1) 2 E_i: another
    (2 T - 1)(2 T - 1) 2 u E_i <= 2 (2 T - 1) 2 T u E_i;
  * G^ and the definition are each the minimum over the same set of paths (the float32 recurrence is monotone: a smaller
    predecessor never gives a larger sum), and a minimum moves by no more than the worst of its terms.

Hence |G^(i, j) - dtw(i, j)| <= tau_i = 2 (2 T - 1)(C + 2 T + 4) u E_i, and two candidates can only be ranked against the
definition's order when their distances lie within 2 tau_i of each other.  The device keeps k + 8 candidates by G^ and recomputes
them by the definition's own float64 steps, so for every row, d_k being the definition's k-th distance:

  * every returned j has dtw(i, j) <= d_k + 2 tau_i, and every candidate with dtw(i, j) < d_k - 2 tau_i is returned;
  * distances are non-decreasing and among equal float32 distances the indices ascend;
  * a reported distance EQUALS float32(dtw(i, index)) bit for bit;
  * a row is DECIDED when d_(k+1) - d_k > 2 tau_i (or it has no more than k candidates): there the returned index SET equals the
    definition's.

Integer inputs in -3 .. 3: every product, norm, cost and path sum is an integer of at most 127 * 36 * 128 < 2^24 — exact in
float32 — so the device must reproduce the definition entry for entry, the exact ties at the k-th boundary with it.
"""
import functools

import numpy as np

import knn_cases as KC
from whisperseg_amd import dtw as DW

SEED = KC.SEED
U = 2.0 ** -24

# (N, C, T, band, k) of the integer self-searches: one row; fewer than k candidates; band 0 (the Euclidean lists); one row past a
# tile of four; C = T = 1; the full band at the largest k; the patch size with a ragged last tile; one step past a 32-block; the
# longest sequence at a narrow band; the largest C, T, band and k
INTEGER_SHAPES = ((1, 5, 4, 1, 1), (5, 7, 3, 2, 8), (64, 16, 8, 0, 4), (65, 17, 8, 2, 15), (200, 1, 1, 0, 15), (333, 3, 5, 4, 64),
                  (130, 80, 32, 4, 15), (70, 80, 33, 8, 1), (150, 2, 64, 1, 3), (70, 128, 64, 63, 64))
CROSS = dict(m=37, n=500, c=9, t=9, band=2, k=15, copies=10)        # queries != corpus; `copies` queries are corpus rows
TWINS = dict(n=40, c=6, t=12, k=3)
# (C, T, N, band, k) of the float cases and the definition's own decided share at 2 tau (computed on the CPU)
FLOAT_SHAPES = ((16, 8, 600, 2, 10), (1, 12, 500, 11, 15), (3, 33, 300, 32, 5), (80, 32, 150, 4, 5), (5, 64, 120, 8, 10))
FLOAT_LOOSE = (7, 20, 400, 3, 64)                                   # about 0.907 decided: the contract alone, no floor
MIN_DECIDED = 0.9                                                   # share of decided rows a float case must reach to prove anything


@functools.lru_cache(maxsize=None)
def integer_rows(n, d, seed=SEED):
    rows = np.random.default_rng([seed, n, d]).integers(-3, 4, size=(n, d)).astype(np.float32)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def cross_case():
    """(queries [37, 81], corpus [500, 81], {query row: corpus row it copies})."""
    c = CROSS
    d = c["c"] * c["t"]
    corpus = integer_rows(c["n"], d)
    queries = integer_rows(c["m"], d, SEED + 1).copy()
    rng = np.random.default_rng(SEED + 2)
    which = dict(zip(rng.choice(c["m"], c["copies"], replace=False).tolist(), rng.choice(c["n"], c["copies"], replace=False).tolist()))
    for i, j in which.items():
        queries[i] = corpus[j]
    queries.setflags(write=False)
    return queries, corpus, which


@functools.lru_cache(maxsize=None)
def twin_rows():
    """[2 n, C T]: n integer rows whose last two columns are equal, then the twin of each — [c0, c0, c1, ..., c_(T-2)]: the row one
    step late.  Warping with a band of at least 1 aligns the two at cost exactly 0."""
    w = TWINS
    cols = np.random.default_rng([SEED, w["n"], w["c"], w["t"]]).integers(-3, 4, size=(w["n"], w["c"], w["t"])).astype(np.float32)
    cols[:, :, -1] = cols[:, :, -2]
    late = np.concatenate([cols[:, :, :1], cols[:, :, :-1]], axis=2)
    rows = np.ascontiguousarray(np.concatenate([cols, late], axis=0).reshape(2 * w["n"], -1))
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def float_rows(c, t, n):
    """20 centres uniform in [-1.5, 0.5]^(C T) (the range of the patches' values) plus 0.3 * normal noise."""
    rng = np.random.default_rng([20261020, c, t, n])
    centres = rng.uniform(-1.5, 0.5, (20, c * t))
    rows = (centres[rng.integers(0, 20, n)] + 0.3 * rng.standard_normal((n, c * t))).astype(np.float32)
    rows.setflags(write=False)
    return rows


def column_energy(rows, channels):
    """max over the columns of a row of |column|^2 -> float64 [rows]."""
    r = np.asarray(rows, np.float64).reshape(len(rows), channels, -1)
    return (r * r).sum(axis=1).max(axis=1) if len(rows) else np.zeros(0)


class Reference:
    """The definition on (queries, corpus or None, k, channels, band), computed once: the float64 distances with a row's own column
    at +inf, the definition's lists, tau and which rows are decided at `margin` * tau.  The attributes check_contract and
    check_exact of knn_cases read, so that those checks are the ones used here."""

    def __init__(self, queries, corpus, k, channels, band):
        self.own = corpus is None
        self.q = np.asarray(queries, np.float32)
        self.x = self.q if self.own else np.asarray(corpus, np.float32)
        self.k, self.channels = k, channels
        self.m, self.n, self.d = self.q.shape[0], self.x.shape[0], self.q.shape[1]
        self.steps = self.d // channels
        self.band = DW.check_band(band, self.steps)
        self.dist = DW.dtw_host(self.q, self.x, channels, self.band)
        if self.own:
            self.dist[np.arange(self.m), np.arange(self.m)] = np.inf
        self.candidates = self.n - 1 if self.own else self.n
        take = max(0, min(k, self.candidates))
        order = np.argsort(self.dist, axis=1, kind="stable")[:, :take]
        self.index = np.full((self.m, k), -1, np.int32)
        self.distance = np.full((self.m, k), np.inf, np.float32)
        self.index[:, :take] = order
        self.distance[:, :take] = np.take_along_axis(self.dist, order, axis=1)
        e_x = column_energy(self.x, channels)
        energy = column_energy(self.q, channels) + (e_x.max() if self.n else 0.0)
        self.tau = 2.0 * (2 * self.steps - 1) * (channels + 2 * self.steps + 4) * U * energy
        self.sorted = np.sort(self.dist, axis=1)

    def decided(self, margin=2.0):
        if self.candidates <= self.k:
            return np.ones(self.m, dtype=bool)
        return self.sorted[:, self.k] - self.sorted[:, self.k - 1] > margin * self.tau


@functools.lru_cache(maxsize=None)
def reference(kind, *shape):
    """The shared, unchanged Reference of a case: ("integer", N, C, T, band, k), ("cross",), ("twins", band), ("float", C, T, N, band, k),
    ("pictures", band, k)."""
    if kind == "integer":
        n, c, t, band, k = shape
        return Reference(integer_rows(n, c * t), None, k, c, band)
    if kind == "cross":
        q, x, _ = cross_case()
        return Reference(q, x, CROSS["k"], CROSS["c"], CROSS["band"])
    if kind == "twins":
        return Reference(twin_rows(), None, TWINS["k"], TWINS["c"], shape[0])
    if kind == "float":
        c, t, n, band, k = shape
        return Reference(float_rows(c, t, n), None, k, c, band)
    if kind == "pictures":
        return Reference(KC.picture_rows(), None, shape[1], 80, shape[0])
    raise KeyError(kind)


check_exact = KC.check_exact


def check_contract(ref, index, distance, what=""):
    """knn_cases.check_contract with this module's tau, and the reported distances EQUAL to float32(dtw(i, index)) bit for bit ->
    the share of decided rows."""
    share = KC.check_contract(ref, index, distance, what)
    found = index >= 0
    rows = np.nonzero(found)[0]
    want = ref.dist[rows, index[found]].astype(np.float32)
    assert np.array_equal(distance[found].view(np.uint32), want.view(np.uint32)), (what, "a reported distance is not the definition's float32")
    return share
