"""Inputs of the nearest-neighbour tests (tests/test_knn_cpu.py, tests/test_knn_gpu.py), what the device may differ from the
definition whisperseg_amd.neighbors.neighbors_host by, and the check of that contract.

THE SLACK (derived, not measured).  The device selects by d^(i, j) = |q_i|^2 + |x_j|^2 - 2 q_i.x_j in float32, every term ONE
fmaf chain over the D columns.  With u = 2^-24 a chain of D terms is within gamma_D sum|terms| ~ D u sum|terms| of its exact value
(Higham, Accuracy and Stability, 3.1), so the two norms are within D u |q|^2 and D u |x|^2, the dot product within D u |q||x| and,
doubled, within D u (|q|^2 + |x|^2) (2 |q.x| <= 2 |q||x| <= |q|^2 + |x|^2); the addition of the norms rounds once (u (|q|^2 +
|x|^2)), the product by 2 is exact and the final fused subtraction rounds a value bounded by |q|^2 + |x|^2 + 2 |q.x| <= 2 (|q|^2 +
|x|^2) once: 3 u (|q|^2 + |x|^2) together, inside the 8 u the bound allows (second-order terms take the rest).  Hence

    |d^(i, j) - d(i, j)| <= 2 (D + 4) u (|q_i|^2 + |x_j|^2) <= tau_i = 2 (D + 4) u (|q_i|^2 + max_j |x_j|^2)

and two candidates can only be ranked against the definition's order when their distances lie within 2 tau_i of each other.  The
device keeps k + 8 candidates by d^ and re-ranks them by the direct form with fp64 accumulation, so for every row, d_k being the
definition's k-th distance:

  * every returned j has d(i, j) <= d_k + 2 tau_i, and every candidate with d(i, j) < d_k - 2 tau_i is returned;
  * distances are non-decreasing and among equal float32 distances the indices ascend;
  * a reported distance is within 1 float32 ulp of float32(d(i, index)): the fp64 sum of <= 20 480 non-negative terms is within
    20 480 * 2^-53 of the exact sum, far inside half a float32 ulp, which leaves the final rounding;
  * a row is DECIDED when d_(k+1) - d_k > 2 tau_i (or it has no more than k candidates): there the returned index SET equals the
    definition's.

Integer inputs in -3 .. 3: every product, norm and d^ is an integer below 9 * 20 480 * 4 < 2^24 — exact in float32 — so the device
must reproduce the definition entry for entry, distance bits included, the exact ties at the k-th boundary with it.
"""
import functools

import numpy as np

from whisperseg_amd import neighbors as NB

SEED = 20261020
U = 2.0 ** -24

# (N, D, k) of the integer self-searches: one row; fewer than k candidates; one full tile; one row and one column past a tile; D = 1;
# D = 3 at the largest k; several tiles; the patch size at W = 32; a D that is no multiple of 4 nor of the slab of 16, at k = 1; the
# longest row at the largest k
INTEGER_SHAPES = ((1, 5, 1), (5, 7, 8), (64, 16, 4), (65, 17, 15), (200, 1, 15), (333, 3, 64), (1000, 80, 15), (700, 2560, 15),
                  (300, 2562, 1), (130, 20480, 64))
CROSS = dict(m=37, n=500, d=81, k=15, copies=10)           # queries != corpus; `copies` queries are corpus rows
CLUSTERED_SHAPES = ((16, 1500, 10), (80, 1500, 15), (3, 700, 5))      # (D, N, k)
UNIFORM = dict(d=2560, n=96, k=3)
MIN_DECIDED = 0.9                                          # share of decided rows a clustered case must reach to prove anything


@functools.lru_cache(maxsize=None)
def integer_rows(n, d, seed=SEED):
    rows = np.random.default_rng([seed, n, d]).integers(-3, 4, size=(n, d)).astype(np.float32)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def cross_case():
    """(queries [37, 81], corpus [500, 81], {query row: corpus row it copies})."""
    c = CROSS
    corpus = integer_rows(c["n"], c["d"])
    queries = integer_rows(c["m"], c["d"], SEED + 1).copy()
    rng = np.random.default_rng(SEED + 2)
    which = dict(zip(rng.choice(c["m"], c["copies"], replace=False).tolist(), rng.choice(c["n"], c["copies"], replace=False).tolist()))
    for i, j in which.items():
        queries[i] = corpus[j]
    queries.setflags(write=False)
    return queries, corpus, which


@functools.lru_cache(maxsize=None)
def clustered_rows(d, n, seed=SEED):
    """20 centres uniform in [-1.5, 0.5]^D (the range of the patches' values) plus 0.3 * normal noise."""
    rng = np.random.default_rng([seed, d, n])
    centres = rng.uniform(-1.5, 0.5, size=(20, d))
    rows = (centres[rng.integers(0, 20, size=n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def uniform_rows(n=UNIFORM["n"], d=UNIFORM["d"], seed=SEED):
    rows = np.random.default_rng([seed, n, d, 7]).uniform(-1.5, 0.5, size=(n, d)).astype(np.float32)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def picture_rows():
    """The definition's pictures of the patch tests' 16 kHz rows at W = 32, flattened to D = 2 560, the first five appended again."""
    import measure_cases as MC
    import patch_cases as PC
    from whisperseg_amd import patches as P
    x, bounds = MC.recording(16000), PC.rows_for(16000, 32)
    pictures = P.patches_host(x, 16000, MC.prediction(bounds, 16000, len(x)), width=32).reshape(len(bounds), -1)
    rows = np.ascontiguousarray(np.concatenate([pictures, pictures[:5]], axis=0))
    rows.setflags(write=False)
    return rows


class Reference:
    """The definition on (queries, corpus or None, k), computed once: the float64 distances with a row's own column at +inf, the
    definition's lists, tau and which rows are decided at `margin` * tau (2: the contract; 4: twice the margin)."""

    def __init__(self, queries, corpus, k):
        self.own = corpus is None
        self.q = np.asarray(queries, np.float32)
        self.x = self.q if self.own else np.asarray(corpus, np.float32)
        self.k = k
        self.m, self.n, self.d = self.q.shape[0], self.x.shape[0], self.q.shape[1]
        self.index, self.distance = NB.neighbors_host(self.q, None if self.own else self.x, k)
        self.dist = NB.distances_host(self.q, self.x)
        if self.own:
            self.dist[np.arange(self.m), np.arange(self.m)] = np.inf
        self.candidates = self.n - 1 if self.own else self.n
        xn = (self.x.astype(np.float64) ** 2).sum(axis=1)
        qn = (self.q.astype(np.float64) ** 2).sum(axis=1)
        self.tau = 2.0 * (self.d + 4) * U * (qn + (xn.max() if self.n else 0.0))
        self.sorted = np.sort(self.dist, axis=1)

    def decided(self, margin=2.0):
        if self.candidates <= self.k:
            return np.ones(self.m, dtype=bool)
        return self.sorted[:, self.k] - self.sorted[:, self.k - 1] > margin * self.tau


@functools.lru_cache(maxsize=None)
def reference(kind, *shape):
    """The shared, unchanged Reference of a case: ("integer", N, D, k), ("cross",), ("clustered", D, N, k), ("uniform",), ("pictures", k)."""
    if kind == "integer":
        n, d, k = shape
        return Reference(integer_rows(n, d), None, k)
    if kind == "cross":
        q, x, _ = cross_case()
        return Reference(q, x, CROSS["k"])
    if kind == "clustered":
        d, n, k = shape
        return Reference(clustered_rows(d, n), None, k)
    if kind == "uniform":
        return Reference(uniform_rows(), None, UNIFORM["k"])
    if kind == "pictures":
        return Reference(picture_rows(), None, shape[0])
    raise KeyError(kind)


def check_exact(ref, index, distance, what=""):
    """Integer inputs: the definition entry for entry, distance bits included."""
    assert index.dtype == np.int32 and distance.dtype == np.float32 and index.shape == distance.shape == (ref.m, ref.k), (what, index.shape)
    wrong = np.flatnonzero((index != ref.index).any(axis=1) | (distance.view(np.uint32) != ref.distance.view(np.uint32)).any(axis=1))
    assert not len(wrong), (what, int(wrong[0]), index[wrong[0]].tolist(), ref.index[wrong[0]].tolist(), distance[wrong[0]].tolist(),
                            ref.distance[wrong[0]].tolist())


def check_contract(ref, index, distance, what=""):
    """The slack contract on every row, set equality on the decided rows -> the share of decided rows."""
    assert index.dtype == np.int32 and distance.dtype == np.float32 and index.shape == distance.shape == (ref.m, ref.k), (what, index.shape)
    have = min(ref.k, ref.candidates)
    decided = ref.decided()
    for i in range(ref.m):
        got, dist = index[i], distance[i]
        assert (got[have:] == -1).all() and np.isposinf(dist[have:]).all(), (what, i, "the tail of a row without k candidates")
        got, dist = got[:have], dist[:have]
        assert ((got >= 0) & (got < ref.n)).all() and len(set(got.tolist())) == have, (what, i, got.tolist())
        assert not (ref.own and (got == i).any()), (what, i, "a row is its own neighbour")
        true = ref.dist[i, got]
        # reported distances: the direct form to 1 float32 ulp, non-decreasing, indices ascending among equal ones
        want = true.astype(np.float32)
        assert (np.abs(dist.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want).astype(np.float64)).all(), (what, i, dist.tolist(), want.tolist())
        assert (np.diff(dist) >= 0).all(), (what, i, dist.tolist())
        assert (np.diff(got)[np.diff(dist) == 0] > 0).all(), (what, i, got.tolist(), dist.tolist())
        if have == 0:
            continue
        if ref.candidates <= ref.k:
            assert set(got.tolist()) == set(ref.index[i, :have].tolist()), (what, i)
            continue
        d_k, slack = ref.sorted[i, ref.k - 1], 2.0 * ref.tau[i]
        assert (true <= d_k + slack).all(), (what, i, "a neighbour beyond the k-th distance and its slack", float(true.max()), float(d_k), float(slack))
        must = np.flatnonzero(ref.dist[i] < d_k - slack)
        assert set(must.tolist()) <= set(got.tolist()), (what, i, "a candidate clearly inside the k-th distance is missing")
        if decided[i]:
            assert set(got.tolist()) == set(ref.index[i].tolist()), (what, i, sorted(got.tolist()), sorted(ref.index[i].tolist()))
    return float(decided.mean())
