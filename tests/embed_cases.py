"""Shared cases of the embedding tests (tests/test_embed_cpu.py, tests/test_embed_gpu.py): a second, plainly written statement of
whisperseg_amd.embed.layout_host (Python integers and floats, a double loop), the small graphs on which the device must give the
definition's bits, the bound of one epoch with a general b, and the blobs of the "it is a map" test.

THE BOUND of one epoch with b != 1.  Both sides start from the same float64 y_in and run the same operations in the same order; they
differ only where pow(d2, b) does.  The OpenCL profile the device's pow is built to allows it 16 ulp, numpy's is within 1 ulp: at most
2 * 16 u relative between the two P, u = 2^-53.  A term runs at most 12 further roundings after its delta (d2: up to 5, coef: 5, the
product with delta_c, and min / max none), each u relative, and 1 / (1 + a P) and P / (d2 (1 + a P)) amplify a relative error of P
by at most 1: a term g differs by at most (12 + 32) u |g| <= 64 u |g| (a clipped term is exactly +-4 on both sides unless coef * delta
sits within that error of the clip, where the difference is smaller still).  The sequential sum of n_terms terms adds at most
n_terms u sum|g| on either side, the product with alpha_t and the final sum one rounding each:
    |y_dev - y_def| <= alpha_t * u * sum_terms |g| * (64 + n_terms) + 1 ulp(y)
per coordinate.  Which terms exist (the schedule, the m == i skip, d2 == 0) is decided in integers or on identical inputs."""
import functools

import numpy as np

from whisperseg_amd import embed as EM

MASK = (1 << 64) - 1
U = 2.0 ** -53


def mix(x):
    """splitmix64's finaliser on a Python integer."""
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return x


def draw(seed, counter):
    return mix((seed * 0x9E3779B97F4A7C15 + counter) & MASK)


def negative(seed, t, nnz, e, n_neg, s, n):
    return ((draw(seed, ((t * nnz + e) * n_neg + s) & MASK) >> 32) * n) >> 32


def is_active(rate, t):
    return ((t + 1) * rate) >> 16 != (t * rate) >> 16


def plain_init(n, dim, seed):
    return [[-10.0 + 20.0 * ((draw(seed, (1 << 63) + i * dim + c) >> 11) * 2.0 ** -53) for c in range(dim)] for i in range(n)]


def plain_schedule(graph):
    """(indptr, indices, rate) as Python lists: rate = floor(w / w_max * 65536 + 0.5) entry by entry, the entries of rate 0 dropped —
    the CSR whose positions number the entries e.  It does not go through embed.scheduled."""
    import math
    old_ptr, old_idx, weight = (np.asarray(v).tolist() for v in graph)
    top = max(weight, default=1.0)
    indptr, indices, rate = [0], [], []
    for i in range(len(old_ptr) - 1):
        for e in range(old_ptr[i], old_ptr[i + 1]):
            r = int(math.floor(weight[e] / top * 65536.0 + 0.5))
            if r:
                indices.append(int(old_idx[e]))
                rate.append(r)
        indptr.append(len(indices))
    return indptr, indices, rate


def plain_layout(graph, dim, t0, t1, total, n_neg, gamma, lr, a, b, init, seed, stats=None):
    """layout_host once more: per epoch, per vertex, per entry, Python floats (pow is numpy's float64 power, as the definition says).
    `stats`: a dict that receives, for the LAST epoch run, "sum_abs" [N, dim] (sum of |g| per coordinate) and "terms" [N]."""
    indptr, indices, rate = plain_schedule(graph)
    n, nnz = len(indptr) - 1, len(indices)
    y = [list(map(float, r)) for r in (plain_init(n, dim, seed) if init is None else np.asarray(init, np.float64).tolist())]

    def term(yi, yj, attraction):
        delta = [yi[c] - yj[c] for c in range(dim)]
        d2 = delta[0] * delta[0]
        for c in range(1, dim):
            d2 = d2 + delta[c] * delta[c]
        power = d2 if b == 1.0 else float(np.power(np.float64(d2), np.float64(b)))
        if attraction:
            coef = 0.0 if d2 == 0 else ((-2.0 * a) * b * power) / (d2 * (1.0 + a * power))
        else:
            coef = ((2.0 * gamma) * b) / ((0.001 + d2) * (1.0 + a * power))
        return [min(4.0, max(-4.0, coef * delta[c])) for c in range(dim)]

    for t in range(t0, t1):
        alpha = lr * (1.0 - t / total)
        out, sum_abs, terms = [], [], []
        for i in range(n):
            force, mass, count = [0.0] * dim, [0.0] * dim, 0
            for e in range(indptr[i], indptr[i + 1]):
                if not is_active(rate[e], t):
                    continue
                pulls = [term(y[i], y[indices[e]], True)]
                for s in range(n_neg):
                    m = negative(seed, t, nnz, e, n_neg, s, n)
                    if m != i:
                        pulls.append(term(y[i], y[m], False))
                for g in pulls:
                    count += 1
                    for c in range(dim):
                        force[c] = force[c] + g[c]
                        mass[c] += abs(g[c])
            out.append([y[i][c] + alpha * force[c] for c in range(dim)])
            sum_abs.append(mass)
            terms.append(count)
        y = out
        if stats is not None:
            stats["sum_abs"], stats["terms"] = np.array(sum_abs).reshape(n, dim), np.array(terms)
    return np.array(y, dtype=np.float64).reshape(n, dim)


def one_epoch_bound(y_def, alpha, stats):
    """float64 [N, dim]: what a device coordinate may differ by from the definition's after one epoch (the module docstring)."""
    return abs(alpha) * U * stats["sum_abs"] * (64 + stats["terms"])[:, None] + np.spacing(np.abs(y_def))


# ---- graphs ------------------------------------------------------------------------------------------------------------------------
def graph_of(n, edges):
    """The symmetric CSR of the undirected edges {(i, j): weight}, indices ascending within a row."""
    both = sorted({(i, j): w for (a, b), w in edges.items() for i, j in ((a, b), (b, a))}.items())
    indptr = np.zeros(n + 1, np.int64)
    for (i, _), _ in both:
        indptr[i + 1] += 1
    return np.cumsum(indptr), np.array([j for (_, j), _ in both], np.int32), np.array([w for _, w in both], np.float64)


def ring_with_chords(n, seed, chords=2):
    """A ring of n vertices and a few random chords a vertex, random weights in (0, 1] with one of them 1."""
    rng = np.random.default_rng(seed)
    edges = {(i, (i + 1) % n): 1.0 for i in range(n) if i != (i + 1) % n}
    for i in range(n):
        for j in rng.integers(0, n, chords):
            if i != j:
                edges[(min(i, int(j)), max(i, int(j)))] = 1.0
    edges = {k: float(w) for k, w in zip(sorted(edges), rng.uniform(0.05, 1.0, len(edges)))}
    edges[sorted(edges)[0]] = 1.0
    return graph_of(n, edges)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(graph, init or None) of a case of the b == 1 bit-equality tests; init is [N, 3] and a 2-D run takes its first two columns."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("n1", "n2", "n3"):                       # most negatives hit m == i
        n = int(name[1])
        return graph_of(n, {(i, j): 1.0 / (1 + i + j) for i in range(n) for j in range(i + 1, n)}), None
    if name == "n65":                                    # one lane past a wave
        return ring_with_chords(65, 5), None
    if name == "star257":                                # one row of 256 entries, 256 rows of one
        return graph_of(257, {(0, j): float(w) for j, w in zip(range(1, 257), rng.uniform(0.3, 1.0, 256))}), None
    if name == "isolated":                               # vertex 7 of 40 has no entry (and the last one neither)
        ring = ring_with_chords(38, 9)
        indptr = np.concatenate([ring[0][:8], ring[0][7:], ring[0][-1:]])
        return (indptr, np.where(ring[1] >= 7, ring[1] + 1, ring[1]).astype(np.int32), ring[2]), None
    if name == "rate1":                                  # a third of the edges has rate 1: never active within 50 epochs
        g = ring_with_chords(70, 11)
        lo, hi = np.minimum(np.repeat(np.arange(70), np.diff(g[0])), g[1]), np.maximum(np.repeat(np.arange(70), np.diff(g[0])), g[1])
        return (g[0], g[1], np.where((lo + hi) % 3 == 0, g[2].max() / 65536.0, g[2])), None
    if name == "twins":                                  # two linked vertices at one position, and a negative sample's twin: d2 == 0
        g = ring_with_chords(12, 13)
        y = rng.uniform(-10, 10, (12, 3))
        y[1] = y[0]
        y[5] = y[0]
        return g, y
    if name == "far":                                    # a start scaled by 1e3: every term is tiny next to the coordinate it moves
        return ring_with_chords(66, 17), rng.uniform(-10, 10, (66, 3)) * 1e3
    if name == "close":                                  # a start scaled by 1e-3: the repulsion terms clip (an attraction term with
        return ring_with_chords(66, 17), rng.uniform(-10, 10, (66, 3)) * 1e-3       # a = b = 1 is 2 delta / (1 + d2): never above 1)
    raise KeyError(name)


EXACT_CASES = ("n1", "n2", "n3", "n65", "star257", "isolated", "rate1", "twins", "far", "close")
EXACT_EPOCHS = 50


def exact_init(name, dim):
    init = exact_case(name)[1]
    return None if init is None else np.ascontiguousarray(init[:, :dim])


@functools.lru_cache(maxsize=None)
def exact_reference(name, dim, n_neg):
    """layout_host of a case with a = b = 1 after EXACT_EPOCHS epochs: computed once, shared, never modified."""
    y = EM.layout_host(exact_case(name)[0], dim, EXACT_EPOCHS, n_neg=n_neg, a=1.0, b=1.0, init=exact_init(name, dim), seed=3)
    y.setflags(write=False)
    return y


# ---- blobs --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blobs(seed=0, groups=3, per=100, d=16):
    """(rows float32 [groups * per, d], labels): Gaussian blobs of unit spread around centres drawn from N(0, 4^2)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (groups, d))
    rows = (np.repeat(centres, per, axis=0) + rng.normal(0.0, 1.0, (groups * per, d))).astype(np.float32)
    return rows, np.repeat(np.arange(groups), per)


@functools.lru_cache(maxsize=None)
def blob_graph(seed=0, k=10, **kw):
    from whisperseg_amd import neighbors as NB
    return EM.fuzzy_graph_host(*NB.neighbors_host(blobs(seed, **kw)[0], None, k))


def purity(y, labels, k=10):
    """The mean share of a point's k nearest neighbours on the map (ties: the lower index) that carry its own label."""
    y = np.asarray(y, np.float64)
    dist = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(dist, np.inf)
    near = np.argsort(dist, axis=1, kind="stable")[:, :k]
    return float((labels[near] == labels[:, None]).mean())
