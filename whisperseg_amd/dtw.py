"""Nearest neighbours under dynamic time warping — the warping-tolerant counterpart of whisperseg_amd.neighbors.  Two renditions of
one syllable rarely differ by a uniform stretch: an element starts a little late, a trill has one pulse more, the segmenter's
onset is a column off.  Column-by-column Euclidean distance counts that as a different sound; banded dynamic time warping (DTW) over
the spectrogram columns does not.

`dtw_host` / `dtw_neighbors_host` are THE definition (numpy, float64) and the oracle of every device test, `dtw_plain` states it a
second time as a plain loop over Python floats; `dtw_neighbors` computes the same lists on the GPU (wseg_dtw_knn_f32:
whisperseg_amd/csrc/wseg_dtw.hip) without ever forming the M x N matrix of distances, `dtw_pairs` the distances of a list of pairs
(wseg_dtw_pairs_f64); `patch_dtw_neighbors` takes what `segment*(..., patches=W)` returned.

A row is a sequence of T columns of C channels in the patch layout, row[ch * T + t] (time fastest), so D = C T.  For queries Q
(float32 [M, C T]) and a corpus X (float32 [N, C T]), channels = C in 1 .. 128, T = D / C in 1 .. 64, k in 1 .. 64, band = r in
0 .. T - 1 (None: max(1, T // 8), clipped to T - 1):

  local cost     c(a, b) = sum_ch (float64(q[ch, a]) - float64(x[ch, b]))^2 — ONE sequential chain in ch = 0 .. C - 1; the
                 difference, the square and the addition are each rounded separately
  recurrence     over the cells with |a - b| <= r: G(0, 0) = c(0, 0); G(a, b) = c(a, b) + the least of those of G(a-1, b-1),
                 G(a-1, b), G(a, b-1) that exist and lie inside the band; dtw(q, x) = G(T-1, T-1).  No step weights, no
                 normalisation by the path length
  consequences   r = 0 is the squared Euclidean distance of neighbors.neighbors_host; dtw(q, x) = dtw(x, q) bit for bit; the
                 distance does not grow when the band widens
  order, result, self-search, conventions
                 those of neighbors.neighbors_host: the total order (distance, index); index int32 [M, k] and distance float32
                 [M, k], ascending, the tail -1 / +inf where candidates run out; corpus=None: a row is left out as its own
                 neighbour BY INDEX, not by value; inputs must be finite (with non-finite input the order is unspecified; the
                 device call still writes nothing outside its outputs); an argument outside its range, a D that C does not divide,
                 mismatched shapes or an array that is not 2-D: ValueError before anything runs

What the device may differ by: its selection runs the recurrence in float32 over costs |q_a|^2 + |x_b|^2 - 2 q_a.x_b from the
fp32 matrix cores, which is within tau_i = 2 (2 T - 1)(C + 2 T + 4) 2^-24 (max_a |q_i[:, a]|^2 + max_{j, b} |x_j[:, b]|^2) of
dtw(i, j); it keeps k + 8 candidates and recomputes them by the definition's own float64 steps, so a reported distance is the
definition's to the last float32 bit and only candidates within 2 tau_i of the k-th distance can be exchanged
(tests/dtw_cases.py).
"""
import numpy as np

from . import _lib, neighbors as NB, resident as RS

MAX_CHANNELS = 128                     # C (csrc/wseg_dtw_plan.h::kDtwMaxChannels)
MAX_STEPS = 64                         # T (kDtwMaxSteps)
HOST_BLOCK_BYTES = 128 << 20           # float64 costs the host definition holds at a time
COST_BLOCK_BYTES = 2 << 20             # of those, the ones a chain over the channels runs on at a time (they stay in the cache)


def check_channels(channels):
    """`channels` as an int, ValueError unless it is an integer in 1 .. 128."""
    return RS.check_int(channels, "channels", 1, MAX_CHANNELS)


def check_band(band, steps):
    """`band` as an int (None: max(1, T // 8) clipped to T - 1), ValueError unless it is an integer in 0 .. T - 1."""
    if band is None:
        return min(max(1, steps // 8), steps - 1)
    return RS.check_int(band, "band", 0, steps - 1, f"in 0 .. T - 1 = {steps - 1}")


def check_shapes(q_shape, x_shape, channels):
    """(M, N, C, T) of the two shapes; ValueError unless both are 2-D with one D = C T, C in 1 .. 128, T in 1 .. 64."""
    channels = check_channels(channels)
    if len(q_shape) != 2 or len(x_shape) != 2:
        raise ValueError(f"queries and corpus must be 2-D [rows, D] (got {tuple(q_shape)} and {tuple(x_shape)})")
    if q_shape[1] != x_shape[1]:
        raise ValueError(f"queries and corpus must have the same D (got {q_shape[1]} and {x_shape[1]})")
    d = int(q_shape[1])
    if d < 1 or d % channels:
        raise ValueError(f"D must be a positive multiple of channels = {channels} (got {d})")
    if d // channels > MAX_STEPS:
        raise ValueError(f"T = D / channels must be 1 .. {MAX_STEPS} (got {d // channels})")
    return int(q_shape[0]), int(x_shape[0]), channels, d // channels


def band_cells(steps, band):
    """(a, b) int arrays of the cells |a - b| <= band of the T x T square, row by row."""
    a, b = np.indices((steps, steps))
    keep = np.abs(a - b) <= band
    return a[keep], b[keep]


def cost_host(q_rows, x_rows, channels, band=None):
    """float64 [M, N, T, T]: c(a, b) of every pair inside the band, +inf outside — for SMALL inputs."""
    q = np.ascontiguousarray(q_rows, dtype=np.float32)
    x = np.ascontiguousarray(x_rows, dtype=np.float32)
    m, n, c, t = check_shapes(q.shape, x.shape, channels)
    band = check_band(band, t)
    a, b = band_cells(t, band)
    q64 = q.astype(np.float64).reshape(m, c, t)
    x64 = x.astype(np.float64).reshape(n, c, t)
    out = np.full((m, n, t, t), np.inf, dtype=np.float64)
    full = 2 * len(a) > t * t                                      # most of the square: all of it, without a gather
    rows = max(1, COST_BLOCK_BYTES // max(1, 8 * n * (t * t if full else len(a))))
    for r0 in range(0, m, rows):
        qb = q64[r0:r0 + rows]
        acc = np.zeros((len(qb), n, t, t) if full else (len(qb), n, len(a)), dtype=np.float64)
        diff = np.empty_like(acc)
        for ch in range(c):                                        # the chain: sequential in ch, every step rounded
            if full:
                np.subtract(qb[:, None, ch, :, None], x64[None, :, ch, None, :], out=diff)
            else:
                np.subtract(qb[:, ch, :][:, None, a], x64[:, ch, :][None, :, b], out=diff)
            np.multiply(diff, diff, out=diff)
            acc += diff
        out[r0:r0 + rows, :, a, b] = acc[:, :, a, b] if full else acc
    return out


def recurrence_host(cost, band):
    """float64 [M, N]: G(T-1, T-1) of the costs [M, N, T, T] over the band."""
    t = cost.shape[-1]
    g = np.full(cost.shape, np.inf, dtype=np.float64)
    for a in range(t):
        for b in range(max(0, a - band), min(t, a + band + 1)):
            if a == 0 and b == 0:
                g[..., 0, 0] = cost[..., 0, 0]
                continue
            best = np.full(cost.shape[:-2], np.inf, dtype=np.float64)          # (a cell outside the band holds +inf)
            if a > 0 and b > 0:
                best = np.minimum(best, g[..., a - 1, b - 1])
            if a > 0:
                best = np.minimum(best, g[..., a - 1, b])
            if b > 0:
                best = np.minimum(best, g[..., a, b - 1])
            g[..., a, b] = cost[..., a, b] + best
    return g[..., t - 1, t - 1]


def dtw_host(q_rows, x_rows, channels, band=None):
    """float64 [M, N]: the definition, for SMALL inputs (tests, the definition's blocks)."""
    q = np.ascontiguousarray(q_rows, dtype=np.float32)
    x = np.ascontiguousarray(x_rows, dtype=np.float32)
    m, n, c, t = check_shapes(q.shape, x.shape, channels)
    band = check_band(band, t)
    out = np.empty((m, n), dtype=np.float64)
    rows = max(1, HOST_BLOCK_BYTES // max(1, 8 * n * t * t))
    for r0 in range(0, m, rows):
        out[r0:r0 + rows] = recurrence_host(cost_host(q[r0:r0 + rows], x, c, band), band)
    return out


def dtw_plain(q_row, x_row, channels, band=None):
    """The definition a second time, on ONE pair of rows, as a plain loop over Python floats -> float (float64)."""
    q = [float(v) for v in np.asarray(q_row, dtype=np.float32).ravel()]
    x = [float(v) for v in np.asarray(x_row, dtype=np.float32).ravel()]
    _, _, c, t = check_shapes((1, len(q)), (1, len(x)), channels)
    band = check_band(band, t)
    inf = float("inf")
    g = [[inf] * t for _ in range(t)]
    for a in range(t):
        for b in range(t):
            if abs(a - b) > band:
                continue
            cost = 0.0
            for ch in range(c):
                diff = q[ch * t + a] - x[ch * t + b]
                cost = cost + diff * diff
            if a == 0 and b == 0:
                g[a][b] = cost
                continue
            before = []
            if a > 0 and b > 0 and abs((a - 1) - (b - 1)) <= band:
                before.append(g[a - 1][b - 1])
            if a > 0 and abs((a - 1) - b) <= band:
                before.append(g[a - 1][b])
            if b > 0 and abs(a - (b - 1)) <= band:
                before.append(g[a][b - 1])
            g[a][b] = cost + min(before)
    return g[t - 1][t - 1]


def dtw_pairs_host(q, x, pairs, channels, band=None):
    """float32 [P]: float32(dtw(q[pairs[p, 0]], x[pairs[p, 1]])) by the definition; `pairs` int [P, 2]."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    m, n, c, t = check_shapes(q.shape, x.shape, channels)
    band = check_band(band, t)
    pairs = check_pairs(np.asarray(pairs), m, n)
    out = np.empty(len(pairs), dtype=np.float32)
    step = max(1, HOST_BLOCK_BYTES // (8 * t * t))
    for p0 in range(0, len(pairs), step):
        i, j = pairs[p0:p0 + step, 0], pairs[p0:p0 + step, 1]
        a, b = band_cells(t, band)
        q64 = q[i].astype(np.float64).reshape(len(i), c, t)
        x64 = x[j].astype(np.float64).reshape(len(j), c, t)
        acc = np.zeros((len(i), len(a)), dtype=np.float64)
        for ch in range(c):
            diff = q64[:, ch, :][:, a] - x64[:, ch, :][:, b]
            acc += diff * diff
        cost = np.full((len(i), t, t), np.inf, dtype=np.float64)
        cost[:, a, b] = acc
        out[p0:p0 + step] = recurrence_host(cost, band)
    return out


def check_pairs(pairs, m, n):
    """`pairs` as int64 [P, 2]; ValueError unless it is an integer array [P, 2] of rows of the two sides."""
    if pairs.ndim != 2 or pairs.shape[1] != 2 or not (np.issubdtype(pairs.dtype, np.integer) or pairs.size == 0):
        raise ValueError(f"pairs must be an integer array [P, 2] (got {pairs.dtype} {pairs.shape})")
    pairs = pairs.astype(np.int64)
    if len(pairs) and (pairs.min() < 0 or pairs[:, 0].max() >= m or pairs[:, 1].max() >= n):
        raise ValueError(f"pairs must index rows 0 .. {m - 1} of the queries and 0 .. {n - 1} of the corpus")
    return pairs


def dtw_neighbors_host(queries, corpus=None, k=15, channels=80, band=None):
    """The definition -> (index int32 [M, k], distance float32 [M, k]).  corpus=None: the queries, a row not its own neighbour."""
    k = NB.check_k(k)
    q = np.ascontiguousarray(queries, dtype=np.float32)
    own = corpus is None
    x = q if own else np.ascontiguousarray(corpus, dtype=np.float32)
    m, n, c, t = check_shapes(q.shape, x.shape, channels)
    band = check_band(band, t)
    index = np.full((m, k), -1, dtype=np.int32)
    distance = np.full((m, k), np.inf, dtype=np.float32)
    take = min(k, n - 1 if own else n)
    if m == 0 or take <= 0:
        return index, distance
    dist = dtw_host(q, x, c, band)
    if own:                                                  # by index: the row's own column goes behind every candidate
        dist[np.arange(m), np.arange(m)] = np.inf
    order = np.argsort(dist, axis=1, kind="stable")[:, :take]            # stable: among equal distances the lower index
    index[:, :take] = order
    distance[:, :take] = np.take_along_axis(dist, order, axis=1)
    return index, distance


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(m, n, channels, steps, k):
    """wseg_dtw_scratch_bytes (host arithmetic, no device); WsegError for invalid input."""
    return _lib.size_or_raise(_lib.load().wseg_dtw_scratch_bytes(int(m), int(n), int(channels), int(steps), int(k)))


def dtw_knn_rows(queries, corpus=None, k=15, channels=80, band=None, out_index=None, out_distance=None):
    """The launches: (index int32 [M, k], distance float32 [M, k]) as DEVICE tensors (`out_index` / `out_distance`, where given) for
    the contiguous float32 device tensors `queries` [M, C T] and `corpus` [N, C T] (None: the queries, a row not its own neighbour).
    Stream-ordered, no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    k = NB.check_k(k)
    x, own = NB.device_sides(queries, corpus, "dtw_knn_rows")
    m, n, c, t = check_shapes(queries.shape, x.shape, channels)
    band = check_band(band, t)
    out_index, out_distance = NB.list_outputs(out_index, out_distance, m, k, queries.device)
    if m == 0:
        return out_index, out_distance
    scratch = RS.new_scratch(scratch_bytes(m, n, c, t, k), queries.device)
    with torch.cuda.device(queries.device):
        _lib.check(lib.wseg_dtw_knn_f32(queries.data_ptr(), m, x.data_ptr() if n else None, n, c, t, band, k, 1 if own else 0,
                                        scratch.data_ptr(), scratch.numel(), out_index.data_ptr(), out_distance.data_ptr(), _lib.stream_ptr()))
    return out_index, out_distance


def dtw_pairs(queries, corpus, pairs, channels, band=None, device="cuda"):
    """dtw_pairs_host's distances, computed on the GPU -> float32 [P] as numpy.  `queries`, `corpus` (None: the queries): numpy
    (uploaded to `device`) or device tensors; `pairs`: an integer array or tensor [P, 2] of (query row, corpus row).  ValueError
    for a pair outside the rows, before a launch."""
    import torch
    lib = _lib.load(require_device=True)
    m, n, c, t = check_shapes(RS.shape_of(queries), RS.shape_of(queries if corpus is None else corpus), channels)
    band = check_band(band, t)
    pairs = check_pairs(pairs.cpu().numpy() if torch.is_tensor(pairs) else np.asarray(pairs), m, n)
    if not len(pairs):
        return np.zeros(0, np.float32)
    q = RS.resident(queries, device)
    x = q if corpus is None else RS.resident(corpus, q.device)
    held = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(q.device)
    out = torch.empty(len(pairs), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        _lib.check(lib.wseg_dtw_pairs_f64(q.data_ptr(), m, x.data_ptr(), n, c, t, band, held.data_ptr(), len(pairs), out.data_ptr(),
                                          _lib.stream_ptr()))
    return out.cpu().numpy()


def dtw_neighbors(queries, corpus=None, k=15, channels=80, band=None, device="cuda"):
    """dtw_neighbors_host's lists, computed on the GPU -> (index int32 [M, k], distance float32 [M, k]) as numpy.  `queries`,
    `corpus`: numpy (uploaded to `device`) or device tensors, which are searched where they lie; only the two result arrays travel
    back."""
    k = NB.check_k(k)
    _, _, _, t = check_shapes(RS.shape_of(queries), RS.shape_of(queries if corpus is None else corpus), channels)
    check_band(band, t)
    q = RS.resident(queries, device)
    x = None if corpus is None else RS.resident(corpus, q.device)
    index, distance = dtw_knn_rows(q, x, k, channels, band)
    return index.cpu().numpy(), distance.cpu().numpy()


def patch_dtw_neighbors(predictions, k, band=None, device="cuda"):
    """{"neighbor_index": int32 [rows, k], "neighbor_distance": float32 [rows, k]} of every call among all the calls of
    `predictions` (see neighbors.patch_pictures_of: what segment* returned, or the pictures themselves) under DTW over the
    pictures' columns, on the GPU; channels is the pictures' mel count.  ValueError for pictures wider than 64 columns."""
    k = NB.check_k(k)
    pictures = NB.patch_pictures_of(predictions)
    rows, mels, width = (int(v) for v in pictures.shape)
    if not rows:
        return {"neighbor_index": np.zeros((0, k), np.int32), "neighbor_distance": np.zeros((0, k), np.float32)}
    if width > MAX_STEPS:
        raise ValueError(f"DTW takes pictures of up to {MAX_STEPS} columns (got W = {width})")
    index, distance = dtw_neighbors(pictures.reshape(rows, mels * width), None, k, mels, band, device=device)
    return {"neighbor_index": index, "neighbor_distance": distance}
