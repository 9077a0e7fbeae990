"""Which calls are the same call type: density-based clustering of the per-segment patches (whisperseg_amd.patches) or any float32
rows.  The expensive part of HDBSCAN, DBSCAN* and robust single linkage is one object — the minimum spanning tree (MST) of the rows
under the mutual-reachability distance; everything after it is O(N log N) host work on N - 1 edges.

`mst_host` is THE definition (numpy, float64) and the oracle of every device test; `mst` builds the same tree with Boruvka rounds
whose N^2 D part runs on the GPU (wseg_mst_round_f32: whisperseg_amd/csrc/wseg_mst.hip) without ever forming the N x N matrix; `cut`
and `hdbscan_labels` turn a tree into labels on the host; `patch_clusters` takes what `segment*(..., patches=W)` returned.

For rows X (float32 [N, D], finite), D in 1 .. 20 480, and min_samples s in 1 .. min(64, N - 1).  All distances are SQUARED, as in
whisperseg_amd.neighbors:

  core(i)        neighbors_host(X, None, k=s)[1][i, s - 1]: the float32 squared distance to the s-th nearest OTHER row.  The row
                 itself is not counted; sklearn's and hdbscan's `min_samples` count it, so their min_samples = s + 1
  d32(i, j)      float32(sum_c (float64(X[i, c]) - float64(X[j, c]))^2): the value `neighbors` reports
  w(i, j)        max(core(i), core(j), d32(i, j)): float32, exact, symmetric — the mutual-reachability distance
  order          edges carry the strict total order (w, a, b) with a = min(i, j) < b = max(i, j); under a strict total order the
                 minimum spanning tree is unique
  result         edges int32 [N - 1, 2] (a < b) and weight float32 [N - 1], ascending in that order; N < 2: empty arrays
  conventions    an s outside its range, an array that is not 2-D or a D outside 1 .. 20 480: ValueError before anything runs

What the device may differ by: a round's selection ranks candidates by max(core_i, core_j, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) in
float32, which is within tau = 2 (D + 4) 2^-24 * 2 max|x|^2 of w; it keeps 1 + 8 candidates per row and re-ranks them by the exact w
(direct form, fp64 accumulation).  On inputs whose products and sums are exact in float32 the tree is the definition's, edge for
edge and bit for bit; on other float rows it is a spanning tree whose every weight is the definition's w of that very edge to one
float32 ulp and whose sorted weights lie within a derived slack of the definition's (tests/mst_cases.py).
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib, neighbors as NB, resident as RS

MAX_SAMPLES = NB.MAX_K                 # min_samples: a core distance is a column of the nearest-neighbour search
MAX_D = NB.MAX_D
KRUSKAL_CHUNK = 8192                   # sorted edges mst_host looks at between two relabellings
HOST_BLOCK_BYTES = 16 << 20            # float64 differences a thread of distances_self_host holds at a time
HOST_THREADS = 8


def check_samples(min_samples, n):
    """`min_samples` as an int; ValueError unless it is an integer in 1 .. min(64, n - 1)."""
    top = min(MAX_SAMPLES, n - 1)
    return RS.check_int(min_samples, "min_samples", 1, top, f"in 1 .. min({MAX_SAMPLES}, N - 1) = {top}")


def check_rows(shape):
    """(N, D) of the shape; ValueError unless it is 2-D with D in 1 .. 20 480."""
    if len(shape) != 2:
        raise ValueError(f"rows must be 2-D [N, D] (got {tuple(shape)})")
    if not 1 <= shape[1] <= MAX_D:
        raise ValueError(f"D must be 1 .. {MAX_D} (got {shape[1]})")
    return int(shape[0]), int(shape[1])


def empty_tree():
    return np.zeros((0, 2), np.int32), np.zeros((0,), np.float32)


def roots_of(parent):
    """The root of every node of a union-find forest, by pointer jumping (numpy)."""
    parent = parent.copy()
    while True:
        up = parent[parent]
        if np.array_equal(up, parent):
            return parent
        parent = up


def find(parent, i):
    """The root of `i`, halving the path on the way."""
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def distances_self_host(rows):
    """float64 [N, N]: neighbors.distances_host(rows, rows) entry for entry — the same reduction over c per pair — but only the
    blocks on and above the diagonal are formed ((a - b)^2 is symmetric) and the blocks are shared among a few threads."""
    x = np.asarray(rows, dtype=np.float64)
    n = len(x)
    out = np.empty((n, n), dtype=np.float64)
    step = max(1, HOST_BLOCK_BYTES // max(1, 8 * n * x.shape[1]))

    def block(r0):
        diff = x[r0:r0 + step, None, :] - x[None, r0:, :]
        out[r0:r0 + step, r0:] = np.einsum("mnc,mnc->mn", diff, diff)

    with ThreadPoolExecutor(max_workers=HOST_THREADS) as pool:
        list(pool.map(block, range(0, n, step)))
    lower = np.tril_indices(n, -1)
    out[lower] = out.T[lower]
    return out


def weights_host(rows, min_samples):
    """(core float32 [N], w float32 [N, N]) of the definition, for SMALL inputs; the diagonal of w is core.  The float64 distances
    are formed once: core is their s-th smallest per row with the row's own column left out — the very value
    neighbors_host(rows, None, k=s)[1][:, s - 1] (tests/test_mst_cpu.py compares)."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    dist = distances_self_host(x)
    d32 = dist.astype(np.float32)
    np.fill_diagonal(dist, np.inf)
    core = np.partition(dist, min_samples - 1, axis=1)[:, min_samples - 1].astype(np.float32)
    return core, np.maximum(np.maximum(core[:, None], core[None, :]), d32)


def mst_host(rows, min_samples=5):
    """The definition -> (edges int32 [N - 1, 2], weight float32 [N - 1]): a dense Kruskal over the upper triangle in the order
    (w, a, b).  O(N^2 D) time and O(N^2) memory: meant for N up to a few thousand."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    n, _ = check_rows(x.shape)
    if n < 2:
        return empty_tree()
    s = check_samples(min_samples, n)
    return mst_of_weights(weights_host(x, s)[1])


def mst_of_weights(w):
    """mst_host's Kruskal on a dense symmetric float32 w [N, N], N >= 2 (the diagonal is not read)."""
    n = len(w)
    a, b = np.triu_indices(n, 1)
    wu = w[a, b]
    order = np.lexsort((b, a, wu))
    a, b, wu = a[order].astype(np.int64), b[order].astype(np.int64), wu[order]
    parent = np.arange(n, dtype=np.int64)
    label = parent.copy()
    edges, weight = np.empty((n - 1, 2), np.int32), np.empty((n - 1,), np.float32)
    got = 0
    for e0 in range(0, len(wu), KRUSKAL_CHUNK):
        sl = slice(e0, e0 + KRUSKAL_CHUNK)
        for e in e0 + np.flatnonzero(label[a[sl]] != label[b[sl]]):         # the others already lie inside one component
            ra, rb = find(parent, a[e]), find(parent, b[e])
            if ra == rb:
                continue
            parent[max(ra, rb)] = min(ra, rb)
            edges[got] = (a[e], b[e])
            weight[got] = wu[e]
            got += 1
        if got == n - 1:
            break
        label = roots_of(parent)
    assert got == n - 1
    return edges, weight


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(n, d):
    """wseg_mst_scratch_bytes (host arithmetic, no device); WsegError for invalid input."""
    return _lib.size_or_raise(_lib.load().wseg_mst_scratch_bytes(int(n), int(d)))


def mst_round(rows, core, component, out_index=None, out_weight=None, scratch=None):
    """The launches of one round: (index int32 [N], weight float32 [N]) as DEVICE tensors (`out_index` / `out_weight`, where given)
    for the contiguous device tensors `rows` float32 [N, D], `core` float32 [N] and `component` int32 [N]: for every row the
    candidate of another component that comes first in the order (w, j), and its weight; -1 / +inf where there is none.
    Stream-ordered, no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    RS.check_tensor(rows, "the rows of mst_round", "[N, D]")
    n, d = check_rows(rows.shape)
    RS.check_tensor(core, "core", "[N]", torch.float32, (n,), rows.device)
    RS.check_tensor(component, "component", "[N]", torch.int32, (n,), rows.device)
    out_index = RS.out_tensor(out_index, "out_index", "[N]", torch.int32, (n,), rows.device)
    out_weight = RS.out_tensor(out_weight, "out_weight", "[N]", torch.float32, (n,), rows.device)
    if n == 0:
        return out_index, out_weight
    nbytes = scratch_bytes(n, d)
    if scratch is None:
        scratch = RS.new_scratch(nbytes, rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(lib.wseg_mst_round_f32(rows.data_ptr(), n, d, core.data_ptr(), component.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                          out_index.data_ptr(), out_weight.data_ptr(), _lib.stream_ptr()))
    return out_index, out_weight


def round_edges(component, index, weight):
    """The host half of a round: for each component the smallest (w, min(i, j), max(i, j)) over its rows' choices -> (a, b, w) of the
    chosen edges, ascending in that order (an edge two components chose appears twice).  For a fixed i the row order (w, j) is that
    same order, so the two levels agree."""
    i = np.flatnonzero(index >= 0)
    j = index[i].astype(np.int64)
    a, b, w = np.minimum(i, j), np.maximum(i, j), weight[i]
    order = np.lexsort((b, a, w, component[i]))
    first = np.ones(len(order), dtype=bool)
    first[1:] = np.diff(component[i][order]) != 0
    pick = order[first]
    pick = pick[np.lexsort((b[pick], a[pick], w[pick]))]
    return a[pick], b[pick], w[pick]


def mst(rows, min_samples=5, device="cuda", stats=None):
    """mst_host's tree, built with Boruvka rounds on the GPU -> (edges int32 [N - 1, 2], weight float32 [N - 1]) as numpy, ascending
    in (w, a, b).  `rows`: numpy (uploaded to `device` once) or a device tensor, which is searched where it lies; per round only the
    two result vectors travel back and the new components up.  `stats`: a dict that receives {"rounds": the rounds taken}."""
    import torch
    n, d = check_rows(RS.shape_of(rows))
    if n < 2:
        if stats is not None:
            stats["rounds"] = 0
        return empty_tree()
    s = check_samples(min_samples, n)
    x = RS.resident(rows, device)
    core = NB.knn_rows(x, None, s)[1][:, s - 1].contiguous()
    scratch = RS.new_scratch(scratch_bytes(n, d), x.device)
    out_index = torch.empty((n,), dtype=torch.int32, device=x.device)
    out_weight = torch.empty((n,), dtype=torch.float32, device=x.device)

    def device_round(labels):
        component = torch.from_numpy(labels.astype(np.int32)).to(x.device)
        mst_round(x, core, component, out_index, out_weight, scratch)
        return out_index.cpu().numpy(), out_weight.cpu().numpy()

    return boruvka(n, device_round, stats)


def boruvka(n, round_of, stats=None):
    """The host bookkeeping of the rounds -> (edges, weight) ascending in (w, a, b).  round_of(component int64 [n]) gives one round's
    (index int32 [n], weight float32 [n]): mst_round on the device, or any restatement of it.  Per round the components' chosen
    edges go ascending through a union-find that skips an edge whose ends are already joined, then the rows are relabelled by their
    root; N - 1 edges stand after at most ceil(log2 N) rounds."""
    edges, weight = np.empty((max(n - 1, 0), 2), np.int32), np.empty((max(n - 1, 0),), np.float32)
    parent = np.arange(n, dtype=np.int64)
    labels = parent.copy()
    got = rounds = 0
    while got < n - 1:
        index, w_row = round_of(labels)
        rounds += 1
        before = got
        for a, b, w in zip(*round_edges(labels, index, w_row)):
            ra, rb = find(parent, a), find(parent, b)
            if ra == rb:           # the cycle guard: the other end chose this very edge, or inexact float rows closed a ring
                continue
            parent[max(ra, rb)] = min(ra, rb)
            edges[got] = (a, b)
            weight[got] = w
            got += 1
        if got == before:
            raise RuntimeError(f"a round joined no components ({got} of {n - 1} edges): are the rows finite?")
        labels = roots_of(parent)
    if stats is not None:
        stats["rounds"] = rounds
    order = np.lexsort((edges[:, 1], edges[:, 0], weight))
    return np.ascontiguousarray(edges[order]), np.ascontiguousarray(weight[order])


# ---- from the tree to labels (host) ------------------------------------------------------------------------------------------------
def check_tree(edges, weight, n):
    edges, weight = np.asarray(edges), np.asarray(weight)
    n = RS.check_int(n, "n", 0, math.inf, "of at least 0")
    if edges.ndim != 2 or edges.shape[1] != 2 or weight.shape != (len(edges),) or len(edges) != max(int(n) - 1, 0):
        raise ValueError(f"a tree of {n} rows has edges [N - 1, 2] and weight [N - 1] (got {edges.shape} and {weight.shape})")
    if len(edges) and (edges.min() < 0 or edges.max() >= n):
        raise ValueError("an edge names a row outside 0 .. N - 1")
    return edges.astype(np.int64), weight.astype(np.float64), int(n)


def check_size(min_cluster_size, least):
    return RS.check_int(min_cluster_size, "min_cluster_size", least, math.inf, f">= {least}")


def by_smallest_row(group, keep):
    """int32 labels: the groups `keep` says are clusters, numbered 0, 1, ... by their smallest row; every other row -1."""
    labels = np.full(len(group), -1, dtype=np.int32)
    rows = np.flatnonzero(keep)
    _, first, inverse = np.unique(group[rows], return_index=True, return_inverse=True)
    labels[rows] = np.argsort(np.argsort(first))[inverse]                # np.unique orders by group id; the rank of its first row
    return labels


def cut(edges, weight, n, threshold, min_cluster_size=1):
    """DBSCAN* at eps^2 = `threshold` (squared units) from the tree: the edges with weight > threshold are dropped; the components
    with at least `min_cluster_size` rows are the clusters, numbered by their smallest row; all other rows are -1."""
    edges, weight, n = check_tree(edges, weight, n)
    size = check_size(min_cluster_size, 1)
    parent = np.arange(n, dtype=np.int64)
    for a, b in edges[weight <= threshold]:
        ra, rb = find(parent, a), find(parent, b)
        parent[max(ra, rb)] = min(ra, rb)
    group = roots_of(parent)
    return by_smallest_row(group, np.bincount(group, minlength=n)[group] >= size)


def hdbscan_labels(edges, weight, n, min_cluster_size):
    """HDBSCAN (Campello, Moulavi, Sander 2013) from the tree: the single-linkage hierarchy of the edges, condensed at
    `min_cluster_size` with lambda = 1 / sqrt(weight) in float64 (weights are squared distances), cluster stability, selection by
    excess of mass — never the root alone: one cluster is not an answer — and noise -1.  Clusters are numbered by their smallest row.
    Edges of equal weight merge in the order (w, a, b): a row whose core distance ties its links to two clusters goes where that order
    puts it, which is the one place another implementation's labels may differ by such a row (sklearn's agree on separated blobs)."""
    edges, weight, n = check_tree(edges, weight, n)
    mcs = check_size(min_cluster_size, 2)
    if n < 2:
        return np.full(n, -1, dtype=np.int32)
    order = np.lexsort((edges[:, 1], edges[:, 0], weight))
    edges, weight = edges[order], weight[order]
    with np.errstate(divide="ignore"):
        lam = 1.0 / np.sqrt(weight)
    # the single-linkage hierarchy: merge k makes node n + k of the nodes its edge's ends are in
    parent = np.arange(n, dtype=np.int64)
    node_of = np.arange(n, dtype=np.int64)               # of a union-find root: the hierarchy's node it stands for
    left, right = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64)
    size = np.ones(2 * n - 1, dtype=np.int64)
    for k, (a, b) in enumerate(edges):
        ra, rb = find(parent, a), find(parent, b)
        if ra == rb:
            raise ValueError("the edges do not form a tree")
        left[k], right[k] = node_of[ra], node_of[rb]
        size[n + k] = size[left[k]] + size[right[k]]
        parent[rb] = ra
        node_of[ra] = n + k

    def leaves(node):                                    # the rows below a node of the hierarchy
        out, stack = [], [node]
        while stack:
            v = stack.pop()
            if v < n:
                out.append(v)
            else:
                stack += (left[v - n], right[v - n])
        return out

    # the condensed tree: clusters 0 (the root), 1, ...; a child is always younger than its parent
    c_parent, c_birth = [-1], [0.0]
    stability = [0.0]
    fell = []                                            # (row, cluster it fell out of)
    stack = [(2 * n - 2, 0)]
    while stack:
        node, c = stack.pop()
        while node >= n:                                 # follow the cluster down while only small parts split off
            l, r, at = left[node - n], right[node - n], lam[node - n]
            big_l, big_r = size[l] >= mcs, size[r] >= mcs
            if big_l and big_r:                          # a true split: two new clusters are born, c dies
                for child in (l, r):
                    c_parent.append(c)
                    c_birth.append(at)
                    stability.append(0.0)
                    stack.append((child, len(c_parent) - 1))
                stability[c] += size[node] * (at - c_birth[c]) if at != c_birth[c] else 0.0
                node = -1
                break
            for child, big in ((l, big_l), (r, big_r)):
                if not big:
                    rows = leaves(child)
                    fell += [(v, c) for v in rows]
                    stability[c] += len(rows) * (at - c_birth[c]) if at != c_birth[c] else 0.0
            node = l if big_l else r if big_r else -1
        if node >= 0:                                    # (a single row left: only with min_cluster_size 1, which is refused)
            fell.append((node, c))
    clusters = len(c_parent)
    # excess of mass, children before parents; the root is never chosen
    chosen = np.ones(clusters, dtype=bool)
    chosen[0] = False
    below = np.zeros(clusters)
    total = np.array(stability)
    kids = [[] for _ in range(clusters)]
    for c in range(1, clusters):
        kids[c_parent[c]].append(c)
    for c in range(clusters - 1, 0, -1):
        if kids[c] and total[c] < below[c]:
            chosen[c] = False
            total[c] = below[c]
        elif kids[c]:
            stack = list(kids[c])
            while stack:
                v = stack.pop()
                chosen[v] = False
                stack += kids[v]
        below[c_parent[c]] += total[c]
    home = np.full(clusters, -1, dtype=np.int64)         # the chosen cluster a cluster lies in (itself included)
    for c in range(1, clusters):
        home[c] = c if chosen[c] else home[c_parent[c]]
    group = np.full(n, -1, dtype=np.int64)
    for v, c in fell:
        group[v] = home[c]
    return by_smallest_row(group, group >= 0)


# ---- call types for new rows (host) -------------------------------------------------------------------------------------------------
def reach_of(edges, weight, labels):
    """float32 [clusters]: for every label 0, 1, ... of `labels` int [N] (the library's, -1: noise) the largest tree weight among the
    edges whose two ends both carry it.  A cluster of hdbscan_labels is the leaf set of one node of the hierarchy, so those edges span
    it and the value is the level at which the cluster is fully assembled: a new row that would join it above that level joins
    something larger than the cluster.  A cluster without such an edge (a single row) gets -inf."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"labels must be integers [N] (got {labels.dtype} {labels.shape})")
    edges, weight, _ = check_tree(edges, weight, len(labels))
    reach = np.full(int(labels.max(initial=-1)) + 1, -np.inf, dtype=np.float32)
    if len(edges):
        a, b = labels[edges[:, 0]], labels[edges[:, 1]]
        inside = (a == b) & (a >= 0)
        np.maximum.at(reach, a[inside], weight[inside].astype(np.float32))
    return reach


def assign_host(index, distance, core, labels, reach, s):
    """int32 [M]: the library's call type of every new row, or -1, from the row's lists among the library rows `index` int [M, k] and
    `distance` float32 [M, k] (neighbors.neighbors(new, library, k): squared, ascending), the library's core distances `core` float32
    [N] at min_samples = s, its `labels` [N] and their `reach` (reach_of).  Per new row q, in float32 and exact like the tree's weights:
      core(q)   = distance[q, s - 1]: the s-th nearest library row — every library row is an OTHER row
      w(q, j)   = max(core(q), core[j], distance[q, j]) over the listed j: the mutual-reachability distance
      anchor    = the listed j that comes first in the order (w, j): where q would hang in the tree
      label     = labels[anchor] if that is >= 0 and w <= reach[label], else -1
    A row is judged by its own list alone.  k < s, or a row with fewer than s valid entries: ValueError."""
    index, distance = np.asarray(index), np.asarray(distance, dtype=np.float32)
    core, labels, reach = np.asarray(core, dtype=np.float32), np.asarray(labels), np.asarray(reach, dtype=np.float32)
    if index.ndim != 2 or index.shape != distance.shape or not np.issubdtype(index.dtype, np.integer):
        raise ValueError(f"index (integer) and distance must both be [M, k] (got {index.shape} and {distance.shape})")
    n = len(labels)
    if labels.ndim != 1 or core.shape != (n,) or reach.ndim != 1 or (n and int(labels.max()) >= len(reach)):
        raise ValueError(f"core and labels must be [N] and reach hold every label (got {core.shape}, {labels.shape} and {reach.shape})")
    s = RS.check_int(s, "min_samples", 1, MAX_SAMPLES)
    m, k = index.shape
    if index.size and (index.max() >= n or index.min() < -1):
        raise ValueError("an index names a library row outside -1 .. N - 1")
    if k < s or (m and (index[:, s - 1] < 0).any()):
        raise ValueError(f"every new row needs its {s} nearest library rows (min_samples): k = {k}, or a list is shorter")
    if m == 0:
        return np.zeros(0, np.int32)
    valid = index >= 0
    j = np.where(valid, index, 0).astype(np.int64)
    w = np.maximum(np.maximum(distance[:, s - 1:s], core[j]), distance)
    w = np.where(valid, w, np.float32(np.inf))
    order = np.lexsort((np.where(valid, j, n), w), axis=1)[:, 0]         # per row: first by w, then by j
    rows = np.arange(m)
    anchor, at = j[rows, order], w[rows, order]
    label = labels[anchor].astype(np.int64)
    if not len(reach):                                   # a library without a cluster
        return np.full(m, -1, dtype=np.int32)
    ok = (label >= 0) & (at <= reach[np.maximum(label, 0)])
    return np.where(ok, label, -1).astype(np.int32)


def assign(rows, corpus_rows, labels, edges, weight, min_samples=5, k=15, lists=None, device="cuda"):
    """assign_host's labels int32 [M] for the new `rows` [M, D] against the library `corpus_rows` [N, D] with its `labels` and tree
    (`edges`, `weight`: mst / patch_clusters, built with this min_samples).  The lists of the new rows (or the caller's `lists`
    (index, distance) [M, k]) and the library's core distances, neighbors(corpus_rows, None, s)[1][:, s - 1], come from the GPU; the
    rule itself is O(M k) host work."""
    k = NB.check_k(k)
    s = RS.check_int(min_samples, "min_samples", 1, MAX_SAMPLES)
    if k < s:
        raise ValueError(f"k = {k} lists fewer library rows than min_samples = {s} needs")
    m, n, _ = NB.check_shapes(RS.shape_of(rows), RS.shape_of(corpus_rows))
    labels = np.asarray(labels)
    if labels.shape != (n,):
        raise ValueError(f"labels must be [N] = {(n,)} (got {labels.shape})")
    reach = reach_of(edges, weight, labels)
    if lists is not None:
        index, distance = np.asarray(lists[0]), np.asarray(lists[1])
        if index.shape != (m, k) or distance.shape != (m, k):
            raise ValueError(f"lists must be (index, distance) [M, k] = {(m, k)} (got {index.shape} and {distance.shape})")
    if m == 0:
        return np.zeros(0, np.int32)
    if n <= s:
        raise ValueError(f"a library of {n} rows has no core distances at min_samples = {s}")
    x = RS.resident(corpus_rows, device)
    if lists is None:
        index, distance = NB.neighbors(rows, x, k, device=device)
    core = NB.knn_rows(x, None, s)[1][:, s - 1].cpu().numpy()
    return assign_host(index, distance, core, labels, reach, s)


def patch_clusters(predictions, min_cluster_size, min_samples=5, device="cuda"):
    """{"cluster": int32 [rows] (hdbscan_labels; -1: noise), "mst_edges": int32 [rows - 1, 2], "mst_weight": float32 [rows - 1]} of
    all the calls of `predictions` — what segment*(..., patches=W) returned, or the pictures themselves
    (neighbors.patch_pictures_of): the rows of the CLI's CSV — with the tree built on the GPU.  min_samples is lowered to rows - 1 where there are fewer rows."""
    mcs = check_size(min_cluster_size, 2)
    min_samples = RS.check_int(min_samples, "min_samples", 1, MAX_SAMPLES)
    rows = NB.patch_rows_of(predictions)
    n = len(rows)
    if n < 2:
        edges, weight = empty_tree()
        return {"cluster": np.full(n, -1, dtype=np.int32), "mst_edges": edges, "mst_weight": weight}
    edges, weight = mst(rows, min(min_samples, n - 1), device=device)
    return {"cluster": hdbscan_labels(edges, weight, n, mcs), "mst_edges": edges, "mst_weight": weight}
