"""Shared cases of the placement tests (tests/test_place_cpu.py, tests/test_place_gpu.py): a second, plainly written statement of
whisperseg_amd.embed's membership_host, row_keys, start_host and place_host (Python integers and floats, a triple loop: row, epoch,
entry; it goes through none of embed.py's helpers), the small cases on which the device must give the definition's bits, and the
blobs of the "it is a placement" test.

The bound of one epoch with b != 1 is tests/embed_cases.py::one_epoch_bound, unchanged: a new row's epoch is the same chain of the
same terms (an attraction term, then n_neg repulsion terms, per active entry), only its partners are corpus positions; plain_place
returns the `sum_abs` and `terms` of the last epoch that bound is made of."""
import functools
import math
import struct

import numpy as np

import embed_cases as EC
from whisperseg_amd import embed as EM

MASK = EC.MASK
ROW, NEG = 64, 16                      # the strides of the counter: entries of a row, negatives of an entry


# ---- the plain statement ------------------------------------------------------------------------------------------------------------
def exp(x):
    return float(np.exp(np.float64(x)))                 # numpy's float64 exp, as the definition says


def plain_membership(index, distance, n):
    """membership_host once more: per row, Python floats -> (indptr, indices, weight) as lists."""
    index, distance = np.asarray(index), np.asarray(distance)
    k = index.shape[1]
    indptr, indices, weight = [0], [], []
    for row_j, row_d in zip(index.tolist(), distance.astype(np.float64).tolist()):
        listed = [(j, math.sqrt(v)) for j, v in zip(row_j, row_d) if j >= 0]
        d = [v for _, v in listed]
        rho = min([v for v in d if v > 0], default=0.0)
        over = [max(0.0, v - rho) for v in d]

        def psum(sigma):
            total = 0.0
            for v in over:
                total = total + exp(-v / sigma)
            return total

        lo, hi, mid = 0.0, math.inf, 1.0
        for _ in range(64):
            if psum(mid) > float(np.log2(float(k))):
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == math.inf else (lo + hi) / 2.0
        total = 0.0
        for v in d:
            total = total + v
        sigma = max(mid, 1e-3 * (total / max(len(d), 1)))
        seen = set()
        for (j, _), v in zip(listed, over):
            p = 1.0 if sigma == 0 else exp(-v / sigma)
            if j not in seen and p > 0:
                indices.append(j)
                weight.append(p)
            seen.add(j)
        indptr.append(len(indices))
    return indptr, indices, weight


def plain_keys(index, distance, seed):
    """row_keys once more, as Python integers."""
    out = []
    for row_j, row_d in zip(np.asarray(index).tolist(), np.asarray(distance, np.float32).tolist()):
        bits = struct.unpack("<I", struct.pack("<f", row_d[0]))[0]
        out.append(EC.draw(seed, (((row_j[0] & 0xFFFFFFFF) << 32) | bits) & MASK))
    return out


def plain_schedule(graph):
    """(indptr, indices, rate, weight) as lists: rate = floor(p * 65536 + 0.5) entry by entry, the entries of rate 0 dropped."""
    old_ptr, old_idx, weight = (np.asarray(v).tolist() for v in graph)
    indptr, indices, rate, kept = [0], [], [], []
    for i in range(len(old_ptr) - 1):
        for e in range(old_ptr[i], old_ptr[i + 1]):
            r = int(math.floor(weight[e] * 65536.0 + 0.5))
            if r:
                indices.append(int(old_idx[e]))
                rate.append(r)
                kept.append(float(weight[e]))
        indptr.append(len(indices))
    return indptr, indices, rate, kept


def plain_start(graph, positions):
    """start_host once more."""
    indptr, indices, _, weight = plain_schedule(graph)
    y = np.asarray(positions, np.float64).tolist()
    dim = len(y[0])
    out = []
    for i in range(len(indptr) - 1):
        top, mass = [0.0] * dim, 0.0
        for e in range(indptr[i], indptr[i + 1]):
            for c in range(dim):
                top[c] = top[c] + weight[e] * y[indices[e]][c]
            mass = mass + weight[e]
        out.append([top[c] / mass for c in range(dim)] if mass > 0 else [0.0] * dim)
    return np.array(out, dtype=np.float64).reshape(len(indptr) - 1, dim)


def place_negative(key, t, q, s, n):
    return ((EC.mix((key + ((t * ROW + q) * NEG + s)) & MASK) >> 32) * n) >> 32


def plain_place(graph, positions, keys, t0, t1, total, n_neg, gamma, lr, a, b, init=None, stats=None, rate=None):
    """place_host once more: per new row, per epoch, per entry, Python floats (pow is numpy's float64 power, as the definition says).
    `stats`: a dict that receives, for the LAST epoch run, "sum_abs" [M, dim] (sum of |g| per coordinate) and "terms" [M].
    `rate`: rates to use instead of the schedule's own, entry for entry of the scheduled CSR (a 0 switches an entry off and leaves
    the numbering of the others as it is)."""
    indptr, indices, own_rate, _ = plain_schedule(graph)
    rate = own_rate if rate is None else [int(r) for r in rate]
    corpus = np.asarray(positions, np.float64).tolist()
    n, dim, m = len(corpus), len(corpus[0]), len(indptr) - 1
    start = (plain_start(graph, positions) if init is None else np.asarray(init, np.float64)).tolist()
    keys = [int(v) for v in keys]

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

    out, sum_abs, terms = [], [], []
    for i in range(m):
        y = list(map(float, start[i]))
        for t in range(t0, t1):
            force, mass, count = [0.0] * dim, [0.0] * dim, 0
            for q, e in enumerate(range(indptr[i], indptr[i + 1])):
                if not EC.is_active(rate[e], t):
                    continue
                pulls = [term(y, corpus[indices[e]], True)]
                pulls += [term(y, corpus[place_negative(keys[i], t, q, s, n)], False) for s in range(n_neg)]
                for g in pulls:
                    count += 1
                    for c in range(dim):
                        force[c] = force[c] + g[c]
                        mass[c] += abs(g[c])
            alpha = lr * (1.0 - t / total)
            y = [y[c] + alpha * force[c] for c in range(dim)]
        out.append(y)
        sum_abs.append(mass)
        terms.append(count)
    if stats is not None:
        stats["sum_abs"], stats["terms"] = np.array(sum_abs).reshape(m, dim), np.array(terms)
    return np.array(out, dtype=np.float64).reshape(m, dim)


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def bipartite(rng, degrees, n):
    """A CSR of len(degrees) new rows over n corpus vertices: distinct random vertices per row, weights in (0.05, 1], a row's first 1."""
    indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    indices = np.concatenate([rng.choice(n, int(d), replace=False) for d in degrees] + [np.zeros(0, np.int64)]).astype(np.int32)
    weight = rng.uniform(0.05, 1.0, len(indices))
    weight[indptr[:-1][np.asarray(degrees) > 0]] = 1.0
    return indptr, indices, weight


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(graph, Y [N, 3], keys uint64 [M], init [M, 3] or None) of a case of the b == 1 bit-equality tests; a 2-D run takes the first
    two columns of Y and init."""
    rng = np.random.default_rng(sum(map(ord, name)) + 1000)
    keys_of = lambda m: EM.draw(77, np.arange(m, dtype=np.uint64))
    if name in ("m1", "m2", "m65"):                      # m65: one lane past a wave
        m = int(name[1:])
        return bipartite(rng, rng.integers(1, 9, m), 40), rng.uniform(-10, 10, (40, 3)), keys_of(m), None
    if name == "n1":                                     # a one-vertex corpus: every negative is the attraction target
        return bipartite(rng, [1, 1, 1], 1), rng.uniform(-10, 10, (1, 3)), keys_of(3), rng.uniform(-10, 10, (3, 3))
    if name == "row64":                                  # one row of 64 entries among rows of one
        return bipartite(rng, [1, 1, 64, 1, 1], 80), rng.uniform(-10, 10, (80, 3)), keys_of(5), None
    if name == "empty_row":                              # rows 3 and 5 (the last) of 6 have no entry
        return bipartite(rng, [2, 3, 1, 0, 4, 0], 30), rng.uniform(-10, 10, (30, 3)), keys_of(6), None
    if name == "rate1":                                  # a third of the entries has rate 1: never active within 50 epochs
        graph = bipartite(rng, rng.integers(1, 9, 70), 50)
        return (graph[0], graph[1], np.where(np.arange(len(graph[1])) % 3 == 1, 1.0 / 65536.0, graph[2])), rng.uniform(-10, 10, (50, 3)), keys_of(70), None
    if name == "on_top":                                 # a start exactly on a linked corpus vertex, and on one drawn as a negative: d2 == 0
        graph, y, keys = bipartite(rng, [3, 3, 2], 12), rng.uniform(-10, 10, (12, 3)), keys_of(3)
        init = rng.uniform(-10, 10, (3, 3))
        init[0] = y[graph[1][0]]
        init[1] = y[place_negative(int(keys[1]), 0, 0, 0, 12)]
        return graph, y, keys, init
    if name in ("far", "close"):                         # Y and the start scaled by 1e3 / 1e-3, as in embed_cases
        scale = 1e3 if name == "far" else 1e-3
        return bipartite(rng, rng.integers(1, 9, 66), 66), rng.uniform(-10, 10, (66, 3)) * scale, keys_of(66), rng.uniform(-10, 10, (66, 3)) * scale
    raise KeyError(name)


EXACT_CASES = ("m1", "m2", "m65", "n1", "row64", "empty_row", "rate1", "on_top", "far", "close")
EXACT_EPOCHS = 50


def exact_args(name, dim):
    """(graph, Y [N, dim], keys, init [M, dim] or None) of a case in `dim` dimensions."""
    graph, y, keys, init = exact_case(name)
    return graph, np.ascontiguousarray(y[:, :dim]), keys, None if init is None else np.ascontiguousarray(init[:, :dim])


@functools.lru_cache(maxsize=None)
def exact_reference(name, dim, n_neg):
    """place_host of a case with a = b = 1 after EXACT_EPOCHS epochs: computed once, shared, never modified."""
    graph, y, keys, init = exact_args(name, dim)
    out = EM.place_host(graph, y, keys, EXACT_EPOCHS, n_neg=n_neg, a=1.0, b=1.0, init=init)
    out.setflags(write=False)
    return out


# ---- blobs: a library of 240 rows and 60 held out ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blob_library(k=10):
    """The rows of embed_cases.blobs() split into a library of 240 and 60 held-out rows; the library's map is the DEFINITION's
    (layout_host of its k = 10 graph, 200 epochs), and so are the hold-out's lists against it."""
    from whisperseg_amd import neighbors as NB
    rows, labels = EC.blobs()
    hold = np.sort(np.random.default_rng(1).choice(300, 60, replace=False))
    keep = np.setdiff1d(np.arange(300), hold)
    lib_rows, new_rows = np.ascontiguousarray(rows[keep]), np.ascontiguousarray(rows[hold])
    positions = EM.layout_host(EM.fuzzy_graph_host(*NB.neighbors_host(lib_rows, None, k)), 2, 200)
    positions.setflags(write=False)
    return {"rows": lib_rows, "labels": labels[keep], "positions": positions, "new_rows": new_rows, "new_labels": labels[hold],
            "lists": NB.neighbors_host(new_rows, lib_rows, k)}


def placed_purity(placed, placed_labels, positions, labels, k=10):
    """The mean share of the k nearest LIBRARY points on the map (ties: the lower index) of a placed row that carry its label."""
    y, z = np.asarray(placed, np.float64), np.asarray(positions, np.float64)
    dist = ((y[:, None, :] - z[None, :, :]) ** 2).sum(axis=2)
    near = np.argsort(dist, axis=1, kind="stable")[:, :k]
    return float((labels[near] == placed_labels[:, None]).mean())
