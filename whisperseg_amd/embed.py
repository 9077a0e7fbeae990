"""A map of the calls: the 2-D (or 3-D) UMAP layout of the per-segment patches (whisperseg_amd.patches) or any float32 rows, on which
a folder's calls are looked at, coloured by their cluster (whisperseg_amd.linkage) and outliers picked.  Given the nearest-neighbour
lists (whisperseg_amd.neighbors) the expensive part is the layout — epochs x active edges x (1 + negatives) force evaluations — and
that is the part on the GPU (wseg_embed_epochs_f64: whisperseg_amd/csrc/wseg_embed.hip); the graph is O(N k) host work.

`fuzzy_graph_host` and `layout_host` are THE definition (numpy, float64) and the oracle of every device test; `layout` runs the same
epochs on the GPU; `embed` goes from rows to positions and `patch_embedding` takes what `segment*(..., patches=W)` returned.

The layout is a SYNCHRONOUS variant of UMAP's optimiser (McInnes, Healy, Melville 2018): every epoch reads only the positions the
epoch before it left, every vertex moves by the sum of its own terms, and the negative samples come from a counter-based hash — so a
result is one function of its input: no races, no atomics, nothing that depends on a grid, a thread count or a run.  With
(indptr, indices, weight) a symmetric CSR over N vertices, positions y float64 [N, dim], dim 2 or 3, and T epochs in all:

  schedule       rate_e = floor(w_e / w_max * 65536 + 0.5) (uint32); entries of rate 0 are dropped from the CSR before anything
                 runs and nnz counts the rest; entry e (its position in that CSR) is ACTIVE in epoch t iff
                 ((t + 1) * rate_e) >> 16 != (t * rate_e) >> 16: rate 65536 every epoch, 32768 every second one
  hash           mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31 (splitmix64's
                 finaliser; uint64, wrapping); draw(c) = mix(seed * 0x9E3779B97F4A7C15 + c)
  negatives      sample s = 0 .. n_neg - 1 of the active entry e of row i in epoch t is the vertex
                 m = ((draw((t * nnz + e) * n_neg + s) >> 32) * N) >> 32; m == i is skipped and contributes nothing
  init           None: y0[i][c] = -10 + 20 * ((draw(2^63 + i * dim + c) >> 11) * 2^-53); or an array [N, dim], used as given
                 (embed(init="pca") builds one from the first dim principal-component scores of the rows: pca_start)
  a term         delta = y_i - y_j per component; d2 = the left-to-right sum of delta_c * delta_c; P = d2 if b == 1.0 else
                 pow(d2, b) (numpy's float64 power)
                 attraction (j = indices[e]):   coef = ((-2 a) b P) / (d2 (1 + a P)), 0 where d2 == 0
                 repulsion (j = a negative m):  coef = ((2 gamma) b) / ((0.001 + d2) (1 + a P))
                 g_c = min(4, max(-4, coef * delta_c))
  an epoch       for vertex i: G = 0; for its entries in CSR order, if the entry is active: G += its attraction term, then G += the
                 repulsion term of each of its negatives in the order of s; y_out[i] = y_in[i] + alpha_t * G with
                 alpha_t = lr * (1 - t / T)
  conventions    positions must stay small enough that d2 and P are finite (a clipped term moves a coordinate by at most 4 lr);
                 a dim other than 2 or 3, fewer than 1 epoch, an n_neg outside 0 .. 16, a min_dist outside [0, spread) or an init
                 that is not finite [N, dim]: ValueError before anything runs

What the device may differ by: nothing where b == 1 — float64 + - * / are correctly rounded on both sides and nothing is contracted,
so every coordinate has the definition's bits after any number of epochs; with another b a term differs by what the device's pow and
numpy's differ by (tests/embed_cases.py derives the bound of one epoch).

NEW ROWS ON AN EXISTING MAP (the layout step of a UMAP transform): the map is a library, its points stay frozen, and M new rows are
placed among them.  `membership_host`, `row_keys`, `start_host` and `place_host` are THE definition; `place` runs the same epochs on
the GPU (wseg_embed_place_f64: all epochs in one launch, a lane per new row) and `transform` goes from new rows to positions.  With
the frozen corpus positions Y float64 [N, dim], N >= 1, and the new rows' lists `index` int [M, k], `distance` float32 [M, k] exactly
as neighbors(new, corpus, k) returns them (squared, ascending, a tail of -1 / +inf):

  membership     per new row, over its valid entries in list order: d_j, rho, the 64-step bisection for sigma, the 1e-3 * mean floor
                 and p(i→j) exactly as fuzzy_graph_host states them; no entry is left out as "own" and nothing is symmetrised.  A
                 CSR (indptr int64 [M + 1], indices int32, weight p) with the entries in list order, nearest first; an entry whose p
                 underflowed to 0 is left out, a corpus index listed twice counts once, at its first entry
  schedule       rate_e = floor(p_e * 65536 + 0.5): a row's nearest entry has p = 1, so w_max is 1 and a rate is the row's own;
                 entries of rate 0 are dropped; q is an entry's position within its row of what is left, q < 64; ACTIVE as above
  key            key_i = draw((uint64(j0) << 32) | bits32(d0)), (j0, d0) the row's first list entry and its float32 distance
  negatives      sample s of entry q of row i in epoch t is the corpus vertex m = ((mix(key_i + ((t * 64 + q) * 16 + s)) >> 32) * N) >> 32;
                 nothing is skipped: a corpus vertex is never the row itself
  start          y0_i[c] = (sum_e p_e * Y[j_e][c]) / (sum_e p_e), both sums left to right over the row's scheduled entries (a row
                 without one: the origin); or an array [M, dim], used as given
  a term         exactly the attraction and repulsion term and clip above, with y_j = Y[j]
  an epoch       for row i: G = 0; for its entries in order, if the entry is active: G += its attraction term, then G += the repulsion
                 term of each of its n_neg negatives in the order of s; then y_i += alpha_t * G.  The corpus never moves and new rows
                 never see each other
  conventions    N == 0, an index outside -1 .. N - 1, a non-finite or negative listed distance, more than 64 entries in a row or
                 a Y that is not finite [N, dim]: ValueError before anything runs

Every output for a new row is a function of that row's list and the library alone: not of the other rows of the batch, their order
or their number.  What the device may differ by is what it may differ by above: nothing where b == 1, the bound of one epoch otherwise.
"""
import numpy as np

from . import _lib, neighbors as NB, pca as PC, resident as RS

MAX_NEG = 16                           # negative samples of an active entry (csrc/wseg_embed_plan.h::kEmbedMaxNeg)
MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
INIT_COUNTER = 1 << 63
BISECTION_STEPS = 64
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


# ---- the graph (host) ----------------------------------------------------------------------------------------------------------------
def fuzzy_graph_host(index, distance):
    """The fuzzy graph of UMAP from the nearest-neighbour lists `index` int [N, k] and `distance` [N, k] exactly as
    neighbors.neighbors returns them (SQUARED float32 distances; entries of index -1 are ignored, and so is a row's own index)
    -> (indptr int64 [N + 1], indices int32 [nnz] ascending within a row, weight float64 [nnz]): a symmetric CSR without a diagonal.

    Per row i, over its entries j in list order, in float64:
      d_j    = sqrt(float64(distance[i, j]))
      rho    = the smallest d_j > 0, or 0 if there is none
      sigma  : lo = 0, hi = inf, mid = 1; exactly 64 times: psum = sum_j exp(-max(0, d_j - rho) / mid) (left to right);
               if psum > log2(k): hi = mid, mid = (lo + hi) / 2; else: lo = mid, mid = 2 mid while hi is inf, (lo + hi) / 2 after.
               sigma = mid — umap-learn's bisection without its early exit, so that the result is one function of the input
      floor  : sigma = max(sigma, 1e-3 * mean_j d_j); where that is 0 every weight of the row is 1
      p(i→j) = exp(-max(0, d_j - rho) / sigma)
    and w(i, j) = min(1, p + q - p q) with p = p(i→j), q = p(j→i), each 0 where the other row does not list this one (the min takes
    back a last-bit excess of the rounded sum).  Entries whose weight underflowed to 0 are left out, so every weight lies in (0, 1]."""
    index, distance = np.asarray(index), np.asarray(distance)
    if index.ndim != 2 or index.shape != distance.shape or not np.issubdtype(index.dtype, np.integer):
        raise ValueError(f"index (integer) and distance must both be [N, k] (got {index.shape} and {distance.shape})")
    n, k = index.shape
    if n and (index.max(initial=-1) >= n or index.min(initial=0) < -1):
        raise ValueError("an index names a row outside 0 .. N - 1")
    if n == 0 or k == 0:
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64)
    valid = (index >= 0) & (index != np.arange(n)[:, None])
    if not np.isfinite(np.asarray(distance, np.float64)[valid]).all() or (np.asarray(distance, np.float64)[valid] < 0).any():
        raise ValueError("the distances of the listed neighbours must be finite and not negative")
    p = directed_host(valid, distance)
    # symmetrise over the union of (i, j) and (j, i); a pair a row lists twice counts once (its first entry)
    i_of = np.repeat(np.arange(n, dtype=np.int64), k)[valid.ravel()]
    j_of = index.astype(np.int64).ravel()[valid.ravel()]
    key, first = np.unique(i_of * n + j_of, return_index=True)
    p_of = p.ravel()[valid.ravel()][first]
    back = (key % n) * n + key // n
    pairs = np.union1d(key, back)
    fwd, bwd = np.zeros(len(pairs)), np.zeros(len(pairs))
    fwd[np.searchsorted(pairs, key)] = p_of
    bwd[np.searchsorted(pairs, back)] = p_of
    weight = np.minimum(1.0, fwd + bwd - fwd * bwd)
    keep = weight > 0
    pairs, weight = pairs[keep], weight[keep]
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(pairs // n, minlength=n), out=indptr[1:])
    return indptr, (pairs % n).astype(np.int32), weight


def directed_host(valid, distance):
    """p(i→j) float64 [N, k] of fuzzy_graph_host's docstring — d_j, rho, the 64-step bisection for sigma, its floor — for the lists'
    SQUARED distances [N, k], k >= 1, over the entries `valid` says are there (their distances finite and not negative); what stands
    at the others is not looked at and their p means nothing.  Every row is computed from that row alone: fuzzy_graph_host and
    membership_host share this arithmetic."""
    n, k = valid.shape
    d = np.sqrt(np.where(valid, distance, 0).astype(np.float64))
    rho = np.where(valid & (d > 0), d, np.inf).min(axis=1)
    rho = np.where(np.isinf(rho), 0.0, rho)
    over = np.maximum(0.0, d - rho[:, None])

    def row_sum(terms):                                  # left to right over the list; an entry that is not there adds 0
        total = np.zeros(n)
        for c in range(k):
            total = total + np.where(valid[:, c], terms[:, c], 0.0)
        return total

    target = np.log2(float(k))
    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(BISECTION_STEPS):
            above = row_sum(np.exp(-over / mid[:, None])) > target
            hi = np.where(above, mid, hi)
            lo = np.where(above, lo, mid)
            mid = np.where(np.isinf(hi), mid * 2.0, (lo + hi) / 2.0)
    count = valid.sum(axis=1)
    mean = row_sum(d) / np.maximum(count, 1)
    sigma = np.maximum(mid, 1e-3 * mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(sigma[:, None] == 0, 1.0, np.exp(-over / sigma[:, None]))
    return p


def curve_ab(min_dist, spread=1.0):
    """(a, b) of the curve 1 / (1 + a x^(2 b)) that fits umap-learn's target in the least-squares sense: at x = linspace(0, 3 spread,
    300) the value 1 below min_dist and exp(-(x - min_dist) / spread) above it.  Levenberg-Marquardt from a = b = 1 in float64."""
    min_dist, spread = float(min_dist), float(spread)
    if not (np.isfinite(spread) and spread > 0):
        raise ValueError(f"spread must be positive (got {spread!r})")
    if not 0 <= min_dist < spread:
        raise ValueError(f"min_dist must lie in [0, spread = {spread}) (got {min_dist!r})")
    x = np.linspace(0.0, 3.0 * spread, 300)
    want = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    log_x = np.log(x[1:])

    def curve(a, b):                                     # the values and their derivatives by a and b (x = 0: 1, 0, 0)
        xb = np.concatenate(([0.0], np.exp(2.0 * b * log_x)))
        f = 1.0 / (1.0 + a * xb)
        return f, np.stack([-xb * f * f, np.concatenate(([0.0], -a * xb[1:] * 2.0 * log_x * f[1:] * f[1:]))], axis=1)

    ab, damp = np.array([1.0, 1.0]), 1e-3
    f, jac = curve(*ab)
    cost = float(((f - want) ** 2).sum())
    for _ in range(200):
        normal, grad = jac.T @ jac, jac.T @ (f - want)
        step = np.linalg.solve(normal + damp * np.diag(np.diag(normal)), -grad)
        trial = ab + step
        f_new, jac_new = curve(*trial) if trial[0] > 0 and trial[1] > 0 else (None, None)
        cost_new = np.inf if f_new is None else float(((f_new - want) ** 2).sum())
        if cost_new <= cost:
            small = np.abs(step).max() < 1e-12
            ab, f, jac, cost, damp = trial, f_new, jac_new, cost_new, max(damp / 10.0, 1e-12)
            if small:
                break
        else:
            damp *= 10.0
            if damp > 1e12:
                break
    return float(ab[0]), float(ab[1])


# ---- the hash, the schedule, the init -------------------------------------------------------------------------------------------------
def mix64(x):
    """splitmix64's finaliser of a uint64 array (wrapping)."""
    x = np.array(x, dtype=np.uint64, ndmin=1)
    x ^= x >> np.uint64(30)
    x *= _M1
    x ^= x >> np.uint64(27)
    x *= _M2
    x ^= x >> np.uint64(31)
    return x


def draw(seed, counter):
    """mix(seed * 0x9E3779B97F4A7C15 + counter) for a uint64 array of counters (wrapping) -> uint64 array."""
    return mix64(np.array(counter, dtype=np.uint64, ndmin=1) + np.uint64((int(seed) * GOLDEN) & MASK))


def negatives(seed, t, nnz, entries, n_neg, n):
    """int64 [len(entries), n_neg]: the negative samples of the entries (positions in the CSR) in epoch t among n vertices."""
    e = np.array(entries, dtype=np.uint64, ndmin=1)
    base = (np.uint64((int(t) * int(nnz)) & MASK) + e) * np.uint64(n_neg)
    h = draw(seed, base[:, None] + np.arange(n_neg, dtype=np.uint64)[None, :])
    return (((h >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def rates(weight):
    """uint32: floor(w / w_max * 65536 + 0.5) of a float64 array of weights (empty: empty)."""
    w = np.asarray(weight, dtype=np.float64)
    if not len(w):
        return np.zeros(0, np.uint32)
    return np.floor(w / w.max() * 65536.0 + 0.5).astype(np.uint32)


def active(rate, t):
    """bool: which entries of these rates are active in epoch t."""
    r = np.asarray(rate).astype(np.uint64)
    return ((np.uint64(t + 1) * r) >> np.uint64(16)) != ((np.uint64(t) * r) >> np.uint64(16))


def init_positions(n, dim, seed):
    """float64 [n, dim]: the hashed start in [-10, 10)."""
    h = draw(seed, np.uint64(INIT_COUNTER) + np.arange(n * dim, dtype=np.uint64))
    return (-10.0 + 20.0 * ((h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)).reshape(n, dim)


def scheduled(graph):
    """(indptr int64 [N + 1], indices int32 [nnz], rate uint32 [nnz]) of the CSR the epochs run on: the graph's entries whose rate is
    not 0.  ValueError unless the graph is a CSR over N vertices with finite weights that are not negative."""
    try:
        indptr, indices, weight = graph
    except (TypeError, ValueError):
        raise ValueError("a graph is (indptr [N + 1], indices [nnz], weight [nnz])") from None
    indptr, indices, weight = np.asarray(indptr), np.asarray(indices), np.asarray(weight, dtype=np.float64)
    if indptr.ndim != 1 or len(indptr) < 1 or indices.ndim != 1 or weight.shape != indices.shape:
        raise ValueError("a graph is (indptr [N + 1], indices [nnz], weight [nnz])")
    n = len(indptr) - 1
    if n > np.iinfo(np.int32).max:
        raise ValueError("a graph has at most 2^31 - 1 vertices")
    indptr = indptr.astype(np.int64)
    if indptr[0] != 0 or indptr[-1] != len(indices) or (np.diff(indptr) < 0).any():
        raise ValueError("indptr must ascend from 0 to nnz")
    if len(indices) and (not np.issubdtype(indices.dtype, np.integer) or indices.min() < 0 or indices.max() >= n):
        raise ValueError("an entry names a vertex outside 0 .. N - 1")
    if not np.isfinite(weight).all() or (weight < 0).any():
        raise ValueError("the weights must be finite and not negative")
    rate = rates(weight)
    keep = rate > 0
    row = np.repeat(np.arange(n), np.diff(indptr))[keep]
    out = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=out[1:])
    return out, np.ascontiguousarray(indices[keep], dtype=np.int32), np.ascontiguousarray(rate[keep])


def check_dim(dim):
    """`dim` as an int, ValueError unless it is the integer 2 or 3."""
    return RS.check_int(dim, "dim", 2, 3, "2 or 3")


def check_epochs(epochs, total):
    """(t0, t1, T) of `epochs` — T, or (t0, t1) of `total` (default t1) — as ints; ValueError unless 0 <= t0 < t1 <= T <= 2^31 - 1."""
    whole = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if isinstance(epochs, (tuple, list)):
        if len(epochs) != 2 or not all(whole(v) for v in epochs):
            raise ValueError(f"epochs must be an integer or (t0, t1) (got {epochs!r})")
        t0, t1 = int(epochs[0]), int(epochs[1])
        total = t1 if total is None else total
    elif whole(epochs):
        t0, t1 = 0, int(epochs)
        total = t1 if total is None else total
    else:
        raise ValueError(f"epochs must be an integer or (t0, t1) (got {epochs!r})")
    if not whole(total) or not 1 <= int(total) <= 2 ** 31 - 1 or not 0 <= t0 < t1 <= int(total):
        raise ValueError(f"epochs must be at least 1, and (t0, t1) must satisfy 0 <= t0 < t1 <= total (got {epochs!r} of {total!r})")
    return t0, t1, int(total)


def check_curve(a, b, gamma, lr):
    """(a, b, gamma, lr) as floats, a and b defaulting to curve_ab(0.1); ValueError unless a >= 0, b > 0 and all four are finite."""
    if (a is None) != (b is None):
        raise ValueError("give a and b together (curve_ab), or neither")
    if a is None:
        a, b = curve_ab(0.1)
    a, b, gamma, lr = float(a), float(b), float(gamma), float(lr)
    if not (np.isfinite(a) and a >= 0 and np.isfinite(b) and b > 0 and np.isfinite(gamma) and np.isfinite(lr)):
        raise ValueError(f"a >= 0, b > 0, gamma and lr must be finite (got {a!r}, {b!r}, {gamma!r}, {lr!r})")
    return a, b, gamma, lr


class Run:
    """The checked arguments of layout_host / layout: the scheduled CSR, the epochs (t0, t1) of T, the parameters and the start."""

    def __init__(self, graph, dim, epochs, total, n_neg, gamma, lr, a, b, init, seed):
        check_dim(dim)
        t0, t1, total = check_epochs(epochs, total)
        RS.check_int(n_neg, "n_neg", 0, MAX_NEG)
        RS.check_int(seed, "seed", 0, MASK, "in 0 .. 2^64 - 1")
        a, b, gamma, lr = check_curve(a, b, gamma, lr)
        self.indptr, self.indices, self.rate = scheduled(graph)
        self.n, self.nnz = len(self.indptr) - 1, len(self.indices)
        self.dim, self.t0, self.t1, self.total, self.n_neg, self.seed = int(dim), t0, t1, int(total), int(n_neg), int(seed)
        self.a, self.b, self.gamma, self.lr = a, b, gamma, lr
        if init is None:
            self.y0 = init_positions(self.n, self.dim, self.seed)
        else:
            y0 = np.array(init, dtype=np.float64, order="C")
            if y0.shape != (self.n, self.dim) or not np.isfinite(y0).all():
                raise ValueError(f"init must be finite [N, dim] = {(self.n, self.dim)} (got {y0.shape})")
            self.y0 = y0

    def alpha(self, t):
        return self.lr * (1.0 - t / self.total)


def _terms(run, delta, attraction):
    """g [M, dim] of the differences delta [M, dim]: the clipped attraction or repulsion terms of the definition."""
    d2 = delta[:, 0] * delta[:, 0]
    for c in range(1, run.dim):
        d2 = d2 + delta[:, c] * delta[:, c]
    power = d2 if run.b == 1.0 else np.power(d2, run.b)
    with np.errstate(divide="ignore", invalid="ignore"):
        if attraction:
            coef = np.where(d2 == 0, 0.0, ((-2.0 * run.a) * run.b * power) / (d2 * (1.0 + run.a * power)))
        else:
            coef = ((2.0 * run.gamma) * run.b) / ((0.001 + d2) * (1.0 + run.a * power))
    return np.minimum(4.0, np.maximum(-4.0, coef[:, None] * delta))


def layout_host(graph, dim=2, epochs=200, total=None, n_neg=5, gamma=1.0, lr=1.0, a=None, b=None, init=None, seed=0):
    """The definition -> positions float64 [N, dim] after the epochs.  `graph`: (indptr, indices, weight), as fuzzy_graph_host returns
    it; `epochs`: T, or (t0, t1) of `total` (default t1) epochs to continue a run from `init`; a, b: default curve_ab(0.1).
    All terms of an epoch are formed at once; the sums then run over the position of an entry within its row, which is the CSR order
    of every vertex's own chain."""
    return host_epochs(Run(graph, dim, epochs, total, n_neg, gamma, lr, a, b, init, seed))


def host_epochs(run):
    """The epochs of a checked Run in numpy -> positions float64 [N, dim]."""
    y = run.y0.copy()
    if run.nnz == 0:
        for t in range(run.t0, run.t1):
            y = y + run.alpha(t) * np.zeros_like(y)
        return y
    row = np.repeat(np.arange(run.n, dtype=np.int64), np.diff(run.indptr))
    place = np.arange(run.nnz, dtype=np.int64) - run.indptr[row]
    for t in range(run.t0, run.t1):
        e = np.flatnonzero(active(run.rate, t))
        i = row[e]
        pull = _terms(run, y[i] - y[run.indices[e]], True)
        if run.n_neg:
            m = negatives(run.seed, t, run.nnz, e, run.n_neg, run.n)
            push = _terms(run, np.repeat(y[i], run.n_neg, axis=0) - y[m.ravel()], False).reshape(len(e), run.n_neg, run.dim)
            hit = m != i[:, None]
        force = np.zeros_like(y)
        order = np.argsort(place[e], kind="stable")
        starts = np.searchsorted(place[e][order], np.arange(place[e].max(initial=-1) + 2))
        for q in range(len(starts) - 1):                 # the q-th entry of every row that has one: distinct rows
            sel = order[starts[q]:starts[q + 1]]
            if not len(sel):
                continue
            force[i[sel]] += pull[sel]
            for s in range(run.n_neg):
                part = sel[hit[sel, s]]
                force[i[part]] += push[part, s]
        y = y + run.alpha(t) * force
    return y


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(n, dim):
    """wseg_embed_scratch_bytes (host arithmetic, no device); WsegError for invalid input."""
    return _lib.size_or_raise(_lib.load().wseg_embed_scratch_bytes(int(n), int(dim)))


def layout_epochs(run, device="cuda"):
    """The launches of a checked Run -> the positions as a DEVICE tensor float64 [N, dim].  Stream-ordered, no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    dev = torch.device(device)
    indptr = torch.from_numpy(run.indptr).to(dev)
    indices = torch.from_numpy(run.indices).to(dev)
    rate = torch.from_numpy(run.rate.view(np.int32)).to(dev)
    y_in = torch.from_numpy(run.y0).to(dev)
    y_out = torch.empty_like(y_in)
    if run.n == 0:
        return y_out
    scratch = RS.new_scratch(scratch_bytes(run.n, run.dim), dev)
    with torch.cuda.device(dev):
        _lib.check(lib.wseg_embed_epochs_f64(indptr.data_ptr(), indices.data_ptr() if run.nnz else None, rate.data_ptr() if run.nnz else None,
                                             run.n, run.nnz, run.dim, y_in.data_ptr(), y_out.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                             run.t0, run.t1, run.total, run.lr, run.a, run.b, run.gamma, run.n_neg, run.seed, _lib.stream_ptr()))
    return y_out


def layout(graph, dim=2, epochs=200, total=None, n_neg=5, gamma=1.0, lr=1.0, a=None, b=None, init=None, seed=0, device="cuda"):
    """layout_host's positions, with the epochs on the GPU -> float64 [N, dim] as numpy.  The arguments are layout_host's; the CSR and
    the start are uploaded once and only the positions travel back.  epochs=(t0, t1) with init= the positions a run to t0 returned
    continues that run: (0, s) then (s, T), both with total=T, give the bits of (0, T)."""
    run = Run(graph, dim, epochs, total, n_neg, gamma, lr, a, b, init, seed)
    return layout_epochs(run, device).cpu().numpy()


def check_embed(k, dim, min_dist, spread, epochs):
    """The checked arguments of embed / patch_embedding -> (k, a, b)."""
    k = NB.check_k(k)
    check_dim(dim)
    RS.check_int(epochs, "epochs", 1, 2 ** 31 - 1, "of at least 1")
    return (k,) + curve_ab(min_dist, spread)


def pca_start(scores, seed):
    """float64 [N, dim]: the start of the layout from the first dim principal-component scores Z [N, dim] of the rows —
    y0 = Z * (10 / max|Z|) + 1e-5 * init_positions(N, dim, seed): the scores scaled into [-10, 10], as the hashed start is, plus a
    deterministic jitter, without which two identical rows would start at one point and, every term between them being 0 at
    d2 == 0, could never separate.  Where max|Z| == 0 or N < 3 it is init_positions alone."""
    z = np.array(scores, dtype=np.float64, ndmin=2)
    n, dim = z.shape
    top = float(np.abs(z).max(initial=0.0))
    if n < 3 or top == 0.0:
        return init_positions(n, dim, seed)
    return z * (10.0 / top) + 1e-5 * init_positions(n, dim, seed)


def check_init(init):
    """`init` of embed / patch_embedding: None, the string "pca" or an array; ValueError for another string."""
    if isinstance(init, str) and init != "pca":
        raise ValueError(f'init must be None, "pca" or an array [N, dim] (got {init!r})')
    return init


def embed(rows, k=15, dim=2, min_dist=0.1, epochs=200, seed=0, device="cuda", spread=1.0, n_neg=5, init=None, lists=None):
    """float32 [N, dim]: the map of the rows (float32 [N, D]: numpy, or a device tensor, searched where it lies) — the k nearest
    neighbours of every row (neighbors.neighbors), their fuzzy graph (fuzzy_graph_host), and `epochs` epochs of layout with
    a, b = curve_ab(min_dist, spread).  `lists`: (index, distance) [N, k] where the caller already has them.  `init`: None (the hashed
    start), an array [N, dim], or "pca": pca_start of the first dim principal-component scores of the rows (pca.pca, on the GPU).
    No rows: [0, dim]; one row: its start, for there is no edge."""
    k, a, b = check_embed(k, dim, min_dist, spread, epochs)
    from_pca = isinstance(check_init(init), str)
    if from_pca:
        init = None
    n = int(rows.shape[0]) if hasattr(rows, "shape") and len(rows.shape) == 2 else len(np.asarray(rows))
    nothing = (np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    Run(nothing, dim, int(epochs), None, n_neg, 1.0, 1.0, a, b, init, seed)          # every argument is checked before the search runs
    if from_pca and n > dim:                                 # (N - 1 < dim rows have no dim components: the hashed start, which init=None is)
        init = pca_start(PC.pca(rows, dim, device=device)["scores"], seed)
    if lists is not None:
        index, distance = np.asarray(lists[0]), np.asarray(lists[1])
        if index.shape != (n, k) or distance.shape != (n, k):
            raise ValueError(f"lists must be (index, distance) [N, k] = {(n, k)} (got {index.shape} and {distance.shape})")
    elif n < 2:
        index, distance = np.full((n, k), -1, np.int32), np.full((n, k), np.inf, np.float32)
    else:
        index, distance = NB.neighbors(rows, None, k, device=device)
    run = Run(fuzzy_graph_host(index, distance), dim, int(epochs), None, n_neg, 1.0, 1.0, a, b, init, seed)
    if n == 0:
        return np.zeros((0, dim), np.float32)
    return layout_epochs(run, device).cpu().numpy().astype(np.float32)


def patch_embedding(predictions, k=15, dim=2, min_dist=0.1, epochs=200, seed=0, device="cuda", lists=None, init=None):
    """{"embedding": float32 [rows, dim]} of all the calls of `predictions` — what segment*(..., patches=W) returned, or the
    pictures themselves (neighbors.patch_pictures_of): the rows of the CLI's CSV.  `lists`: the (neighbor_index, neighbor_distance) of patch_neighbors with
    this k, where the caller has them.  `init`: as embed's."""
    check_embed(k, dim, min_dist, 1.0, epochs)
    check_init(init)
    rows = NB.patch_rows_of(predictions)
    if not len(rows):
        return {"embedding": np.zeros((0, dim), np.float32)}
    return {"embedding": embed(rows, k, dim, min_dist, epochs, seed, device, init=init, lists=lists)}


# ---- new rows on an existing map (the definition, then the device path) -----------------------------------------------------------------
PLACE_ROW = 64                         # entries of a new row: the largest k of a list (csrc/wseg_embed_plan.h::kEmbedPlaceRow)
PLACE_EPOCHS = 100                     # umap-learn's epochs for a transform of a small set: a parameter, not a measured optimum


def check_lists(index, distance, n):
    """(index, distance, valid) of the lists of new rows among n corpus rows, as numpy; ValueError unless they are an integer and a
    float array [M, k], k <= 64, n >= 1, every index in -1 .. n - 1 and every listed distance finite and not negative."""
    index, distance = np.asarray(index), np.asarray(distance)
    if index.ndim != 2 or index.shape != distance.shape or not np.issubdtype(index.dtype, np.integer):
        raise ValueError(f"index (integer) and distance must both be [M, k] (got {index.shape} and {distance.shape})")
    n = RS.check_int(n, "the corpus size N", 1, 2 ** 31 - 1, "of at least 1 (new rows need a corpus)")
    if index.shape[1] > PLACE_ROW:
        raise ValueError(f"a new row lists at most {PLACE_ROW} neighbours (got k = {index.shape[1]})")
    if index.size and (index.max() >= n or index.min() < -1):
        raise ValueError("an index names a corpus row outside -1 .. N - 1")
    valid = index >= 0
    listed = np.asarray(distance, np.float64)[valid]
    if not np.isfinite(listed).all() or (listed < 0).any():
        raise ValueError("the distances of the listed neighbours must be finite and not negative")
    return index, distance, valid


def membership_host(index, distance, n):
    """The memberships of M NEW rows in a corpus of n rows from their lists `index` int [M, k] and `distance` [M, k] exactly as
    neighbors.neighbors(new, corpus, k) returns them -> (indptr int64 [M + 1], indices int32 [nnz], weight float64 [nnz]): row i
    holds p(i→j) of fuzzy_graph_host's docstring for its valid entries j (corpus rows) in LIST order, nearest first.  No entry is
    left out as the row's own, and there is no symmetrisation: a corpus row has no list that could name a new one.  An entry whose p
    underflowed to 0 is left out, and a corpus row listed twice counts once, at its first entry.  A row's nearest entry has p = 1."""
    index, distance, valid = check_lists(index, distance, n)
    m, k = index.shape
    if m == 0 or k == 0:
        return np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64)
    p = directed_host(valid, distance)
    again = np.zeros_like(valid)                         # an entry that repeats an index standing earlier in its list
    for c in range(1, k):
        again[:, c] = (valid[:, :c] & (index[:, :c] == index[:, c:c + 1])).any(axis=1)
    keep = valid & ~again & (p > 0)
    indptr = np.zeros(m + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    return indptr, np.ascontiguousarray(index[keep], dtype=np.int32), np.ascontiguousarray(p[keep])


def row_keys(index, distance, seed):
    """uint64 [M]: the key of every new row, from which its negative samples are drawn — draw(seed, (uint64(j0) << 32) | bits32(d0))
    with (j0, d0) the row's FIRST list entry and its float32 distance (j0 as its 32-bit pattern: a row without an entry has no use
    for its key).  A function of the row's own list: two batches that hold the same call give it the same key."""
    index, distance = np.asarray(index), np.asarray(distance)
    if index.ndim != 2 or index.shape != distance.shape or not np.issubdtype(index.dtype, np.integer):
        raise ValueError(f"index (integer) and distance must both be [M, k] (got {index.shape} and {distance.shape})")
    RS.check_int(seed, "seed", 0, MASK, "in 0 .. 2^64 - 1")
    if index.shape[0] == 0 or index.shape[1] == 0:
        return np.zeros(index.shape[0], np.uint64)
    j0 = index[:, 0].astype(np.int32).view(np.uint32).astype(np.uint64)
    d0 = np.ascontiguousarray(distance[:, 0], dtype=np.float32).view(np.uint32).astype(np.uint64)
    return draw(seed, (j0 << np.uint64(32)) | d0)


def scheduled_onto(graph, n):
    """(indptr int64 [M + 1], indices int32 [nnz], rate uint32 [nnz], weight float64 [nnz]) of the CSR the placement runs on: the
    entries of `graph` (membership_host's: rows are new rows, indices corpus rows 0 .. n - 1, weights in [0, 1]) whose rate
    floor(p * 65536 + 0.5) is not 0.  A row's nearest entry has p = 1, so w_max is 1 and a rate is the row's own, whatever else is in
    the batch.  ValueError unless it is such a CSR and no row keeps more than 64 entries."""
    try:
        indptr, indices, weight = graph
    except (TypeError, ValueError):
        raise ValueError("a graph is (indptr [M + 1], indices [nnz], weight [nnz])") from None
    indptr, indices, weight = np.asarray(indptr), np.asarray(indices), np.asarray(weight, dtype=np.float64)
    if indptr.ndim != 1 or len(indptr) < 1 or indices.ndim != 1 or weight.shape != indices.shape:
        raise ValueError("a graph is (indptr [M + 1], indices [nnz], weight [nnz])")
    m = len(indptr) - 1
    if m > np.iinfo(np.int32).max:
        raise ValueError("at most 2^31 - 1 new rows")
    indptr = indptr.astype(np.int64)
    if indptr[0] != 0 or indptr[-1] != len(indices) or (np.diff(indptr) < 0).any():
        raise ValueError("indptr must ascend from 0 to nnz")
    if len(indices) and (not np.issubdtype(indices.dtype, np.integer) or indices.min() < 0 or indices.max() >= n):
        raise ValueError("an entry names a corpus row outside 0 .. N - 1")
    if not np.isfinite(weight).all() or (weight < 0).any() or (weight > 1).any():
        raise ValueError("the weights must lie in [0, 1]")
    rate = np.floor(weight * 65536.0 + 0.5).astype(np.uint32)
    keep = rate > 0
    out = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(np.repeat(np.arange(m), np.diff(indptr))[keep], minlength=m), out=out[1:])
    if m and np.diff(out).max() > PLACE_ROW:
        raise ValueError(f"a new row has at most {PLACE_ROW} entries (got {int(np.diff(out).max())})")
    return out, np.ascontiguousarray(indices[keep], dtype=np.int32), np.ascontiguousarray(rate[keep]), np.ascontiguousarray(weight[keep])


def check_positions(positions):
    """The frozen corpus positions as float64 [N, dim]; ValueError unless N >= 1, dim is 2 or 3 and every coordinate is finite."""
    y = np.array(positions, dtype=np.float64, order="C")
    if y.ndim != 2 or y.shape[1] not in (2, 3) or y.shape[0] < 1 or not np.isfinite(y).all():
        raise ValueError(f"the corpus positions must be finite [N, dim], N >= 1, dim 2 or 3 (got {y.shape})")
    return y


def _weighted_start(indptr, indices, weight, y):
    """start_host on a scheduled CSR."""
    m, dim = len(indptr) - 1, y.shape[1]
    top, mass = np.zeros((m, dim)), np.zeros(m)
    begin, count = indptr[:-1], np.diff(indptr)
    for q in range(int(count.max(initial=0))):           # the q-th entry of every row that has one: left to right within a row
        rows = np.flatnonzero(count > q)
        e = begin[rows] + q
        top[rows] = top[rows] + weight[e][:, None] * y[indices[e]]
        mass[rows] = mass[rows] + weight[e]
    out = np.zeros((m, dim))
    has = mass > 0
    out[has] = top[has] / mass[has][:, None]
    return out


def start_host(graph, positions):
    """float64 [M, dim]: where a new row starts — y0_i[c] = (sum_e p_e Y[j_e][c]) / (sum_e p_e), both sums left to right over the
    row's SCHEDULED entries (scheduled_onto): the membership-weighted mean of its neighbours on the map, as umap-learn's transform
    starts.  A row without an entry starts at the origin."""
    y = check_positions(positions)
    indptr, indices, _, weight = scheduled_onto(graph, len(y))
    return _weighted_start(indptr, indices, weight, y)


class Place:
    """The checked arguments of place_host / place: the scheduled CSR of the new rows, the frozen corpus positions, the keys, the
    epochs (t0, t1) of T, the parameters and the start."""

    def __init__(self, graph, positions, keys, epochs, total, n_neg, gamma, lr, a, b, init):
        self.y = check_positions(positions)
        self.n, self.dim = self.y.shape
        self.t0, self.t1, self.total = check_epochs(epochs, total)
        self.n_neg = RS.check_int(n_neg, "n_neg", 0, MAX_NEG)
        self.a, self.b, self.gamma, self.lr = check_curve(a, b, gamma, lr)
        self.indptr, self.indices, self.rate, weight = scheduled_onto(graph, self.n)
        self.m, self.nnz = len(self.indptr) - 1, len(self.indices)
        keys = np.asarray(keys)
        if keys.shape != (self.m,) or keys.dtype != np.uint64:
            raise ValueError(f"keys must be uint64 [M] = {(self.m,)} (row_keys; got {keys.dtype} {keys.shape})")
        self.key = np.ascontiguousarray(keys)
        if init is None:
            self.y0 = _weighted_start(self.indptr, self.indices, weight, self.y)
        else:
            y0 = np.array(init, dtype=np.float64, order="C")
            if y0.shape != (self.m, self.dim) or not np.isfinite(y0).all():
                raise ValueError(f"init must be finite [M, dim] = {(self.m, self.dim)} (got {y0.shape})")
            self.y0 = y0

    def alpha(self, t):
        return self.lr * (1.0 - t / self.total)


def place_negatives(key, t, q, n_neg, n):
    """int64 [len(key), n_neg]: the negative samples among n corpus vertices of the entries at the positions q of the rows with
    these keys in epoch t — ((mix64(key + ((t * 64 + q) * 16 + s)) >> 32) * n) >> 32."""
    base = np.asarray(key, np.uint64) + (np.uint64(int(t) * PLACE_ROW) + np.asarray(q).astype(np.uint64)) * np.uint64(MAX_NEG)
    h = mix64(base[:, None] + np.arange(n_neg, dtype=np.uint64)[None, :])
    return (((h >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def place_host(graph, positions, keys, epochs=PLACE_EPOCHS, total=None, n_neg=5, gamma=1.0, lr=1.0, a=None, b=None, init=None):
    """The definition of placing new rows on a frozen map -> their positions float64 [M, dim] after the epochs.  `graph`: what
    membership_host returned; `positions`: the corpus positions Y float64 [N, dim]; `keys`: row_keys; `epochs`, `total`, a, b: as
    layout_host's; `init`: None for start_host, or the positions a run to t0 returned.  The module docstring states an epoch."""
    return place_epochs_host(Place(graph, positions, keys, epochs, total, n_neg, gamma, lr, a, b, init))


def place_epochs_host(run):
    """The epochs of a checked Place in numpy -> positions float64 [M, dim].  All terms of an epoch are formed at once and summed
    over the position of an entry within its row, which is every row's own chain."""
    y = run.y0.copy()
    row = np.repeat(np.arange(run.m, dtype=np.int64), np.diff(run.indptr))
    place = np.arange(run.nnz, dtype=np.int64) - run.indptr[row]
    for t in range(run.t0, run.t1):
        e = np.flatnonzero(active(run.rate, t))
        i = row[e]
        force = np.zeros_like(y)
        if len(e):
            pull = _terms(run, y[i] - run.y[run.indices[e]], True)
            if run.n_neg:
                v = place_negatives(run.key[i], t, place[e], run.n_neg, run.n)
                push = _terms(run, np.repeat(y[i], run.n_neg, axis=0) - run.y[v.ravel()], False).reshape(len(e), run.n_neg, run.dim)
            order = np.argsort(place[e], kind="stable")
            starts = np.searchsorted(place[e][order], np.arange(place[e].max() + 2))
            for q in range(len(starts) - 1):             # the q-th entry of every row that has one: distinct rows
                sel = order[starts[q]:starts[q + 1]]
                force[i[sel]] += pull[sel]
                for s in range(run.n_neg):
                    force[i[sel]] += push[sel, s]
        y = y + run.alpha(t) * force
    return y


def place_rows(run, device="cuda"):
    """The launch of a checked Place -> the positions as a DEVICE tensor float64 [M, dim]: one launch of wseg_embed_place_f64 for all
    its epochs.  Stream-ordered, no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    dev = torch.device(device)
    y_in = torch.from_numpy(run.y0).to(dev)
    y_out = torch.empty_like(y_in)
    if run.m == 0:
        return y_out
    indptr = torch.from_numpy(run.indptr).to(dev)
    indices = torch.from_numpy(run.indices).to(dev)
    rate = torch.from_numpy(run.rate.view(np.int32)).to(dev)
    key = torch.from_numpy(run.key.view(np.int64)).to(dev)
    corpus = torch.from_numpy(run.y).to(dev)
    with torch.cuda.device(dev):
        _lib.check(lib.wseg_embed_place_f64(indptr.data_ptr(), indices.data_ptr() if run.nnz else None, rate.data_ptr() if run.nnz else None,
                                            key.data_ptr(), run.m, run.nnz, corpus.data_ptr(), run.n, run.dim, y_in.data_ptr(), y_out.data_ptr(),
                                            run.t0, run.t1, run.total, run.lr, run.a, run.b, run.gamma, run.n_neg, _lib.stream_ptr()))
    return y_out


def place(graph, positions, keys, epochs=PLACE_EPOCHS, total=None, n_neg=5, gamma=1.0, lr=1.0, a=None, b=None, init=None, device="cuda"):
    """place_host's positions, with the epochs on the GPU -> float64 [M, dim] as numpy.  The arguments are place_host's.
    epochs=(t0, t1) with init= the positions a run to t0 returned continues that run, as layout's."""
    run = Place(graph, positions, keys, epochs, total, n_neg, gamma, lr, a, b, init)
    return place_rows(run, device).cpu().numpy()


def transform(rows, corpus_rows, corpus_positions, k=15, min_dist=0.1, spread=1.0, epochs=PLACE_EPOCHS, seed=0, n_neg=5, lists=None,
              device="cuda"):
    """float32 [M, dim]: the new `rows` (float32 [M, D]) on the map `corpus_positions` [N, dim] of `corpus_rows` [N, D] — the k nearest
    corpus rows of every new row (neighbors.neighbors, or the caller's `lists` (index, distance) [M, k]), their memberships
    (membership_host), keys (row_keys), start (start_host) and `epochs` epochs of place with a, b = curve_ab(min_dist, spread): the
    values the map itself was made with.  The map does not move, and a row's position does not depend on the other new rows.
    Rows and positions: numpy or device tensors (searched where they lie).  No new rows: [0, dim]; no corpus: ValueError.  Every
    argument is checked before the search runs."""
    k = NB.check_k(k)
    a, b = curve_ab(min_dist, spread)
    RS.check_int(epochs, "epochs", 1, 2 ** 31 - 1, "of at least 1")
    RS.check_int(seed, "seed", 0, MASK, "in 0 .. 2^64 - 1")
    RS.check_int(n_neg, "n_neg", 0, MAX_NEG)
    y = check_positions(corpus_positions.cpu().numpy() if hasattr(corpus_positions, "cpu") else corpus_positions)
    m, n, _ = NB.check_shapes(RS.shape_of(rows), RS.shape_of(corpus_rows))
    if n != len(y):
        raise ValueError(f"the corpus has {n} rows and {len(y)} positions")
    if lists is not None:
        index, distance = np.asarray(lists[0]), np.asarray(lists[1])
        if index.shape != (m, k) or distance.shape != (m, k):
            raise ValueError(f"lists must be (index, distance) [M, k] = {(m, k)} (got {index.shape} and {distance.shape})")
    if m == 0:
        return np.zeros((0, y.shape[1]), np.float32)
    if lists is None:
        index, distance = NB.neighbors(rows, corpus_rows, k, device=device)
    run = Place(membership_host(index, distance, n), y, row_keys(index, distance, seed), int(epochs), None, n_neg, 1.0, 1.0, a, b, None)
    return place_rows(run, device).cpu().numpy().astype(np.float32)
