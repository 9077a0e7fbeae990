"""Nearest neighbours of every row among a set of rows — the k-nearest-neighbour graph that clustering (HDBSCAN), embedding (UMAP),
"show me calls like this one" and duplicate finding over the per-segment patches (whisperseg_amd.patches) all begin with.

`neighbors_host` is THE definition (numpy, float64) and the oracle of every device test; `neighbors` computes the same lists on the
GPU (wseg_knn_f32: whisperseg_amd/csrc/wseg_knn.hip) without ever forming the M x N matrix of distances; `patch_neighbors` takes
what `segment*(..., patches=W)` returned.

For queries Q (float32 [M, D]) and a corpus X (float32 [N, D]), k in 1 .. 64, D in 1 .. 20 480:

  distance       d(i, j) = sum_c (float64(Q[i, c]) - float64(X[j, c]))^2 — the squared Euclidean distance in its direct form
  order          the neighbours of row i are the k candidates that come first in the total order (d(i, j), j): the smaller
                 distance first, among equal distances the lower index
  result         index int32 [M, k] and distance float32 [M, k], both ascending; where a row has fewer than k candidates the tail
                 is index -1, distance +inf
  self-search    corpus=None: the corpus is the queries and a row is not its own neighbour — j == i is left out BY INDEX, not by
                 value: two identical rows are each other's neighbour at distance 0
  cosine         is not a second metric: normalise the rows to unit length first; then d = 2 - 2 cos and the order is the cosine's
  conventions    inputs must be finite (with non-finite input the order is unspecified; the device call still writes nothing
                 outside its outputs); a k or D outside its range, a mismatched D or an array that is not 2-D: ValueError before
                 anything runs

What the device may differ by: its selection ranks candidates by |q|^2 + |x|^2 - 2 q.x in float32, which is within
tau_i = 2 (D + 4) 2^-24 (|q_i|^2 + max_j |x_j|^2) of d(i, j); it keeps k + 8 candidates and re-ranks them by the direct form with
fp64 accumulation, so a reported distance is the definition's to the last float32 bit or the next and only candidates within
2 tau_i of the k-th distance can be exchanged (tests/knn_cases.py).
"""
import numpy as np

from . import _lib, resident as RS

MAX_K = 64                             # neighbours per row (csrc/wseg_knn_plan.h::kKnnMaxK)
MAX_D = 20480                          # columns: 80 x 256, the widest patch (kKnnMaxD)
HOST_BLOCK_BYTES = 128 << 20           # float64 differences neighbors_host holds at a time


def check_k(k):
    """`k` as an int, ValueError unless it is an integer in 1 .. 64."""
    return RS.check_int(k, "k", 1, MAX_K)


def check_shapes(q_shape, x_shape):
    """(M, N, D) of the two shapes; ValueError unless both are 2-D with one D in 1 .. 20 480."""
    if len(q_shape) != 2 or len(x_shape) != 2:
        raise ValueError(f"queries and corpus must be 2-D [rows, D] (got {tuple(q_shape)} and {tuple(x_shape)})")
    if q_shape[1] != x_shape[1]:
        raise ValueError(f"queries and corpus must have the same D (got {q_shape[1]} and {x_shape[1]})")
    if not 1 <= q_shape[1] <= MAX_D:
        raise ValueError(f"D must be 1 .. {MAX_D} (got {q_shape[1]})")
    return int(q_shape[0]), int(x_shape[0]), int(q_shape[1])


def distances_host(queries, corpus):
    """float64 [M, N]: the direct form, for SMALL inputs (tests, the definition's blocks)."""
    q = np.asarray(queries, dtype=np.float64)
    x = np.asarray(corpus, dtype=np.float64)
    out = np.empty((len(q), len(x)), dtype=np.float64)
    rows = max(1, HOST_BLOCK_BYTES // max(1, 8 * x.shape[0] * x.shape[1]))
    for r0 in range(0, len(q), rows):
        diff = q[r0:r0 + rows, None, :] - x[None, :, :]
        out[r0:r0 + rows] = np.einsum("mnc,mnc->mn", diff, diff)
    return out


def neighbors_host(queries, corpus=None, k=15):
    """The definition -> (index int32 [M, k], distance float32 [M, k]).  corpus=None: the queries, a row not its own neighbour."""
    k = check_k(k)
    q = np.ascontiguousarray(queries, dtype=np.float32)
    own = corpus is None
    x = q if own else np.ascontiguousarray(corpus, dtype=np.float32)
    m, n, d = check_shapes(q.shape, x.shape)
    index = np.full((m, k), -1, dtype=np.int32)
    distance = np.full((m, k), np.inf, dtype=np.float32)
    take = min(k, n - 1 if own else n)
    if m == 0 or take <= 0:
        return index, distance
    x64 = x.astype(np.float64)
    rows = max(1, HOST_BLOCK_BYTES // (8 * n * d))
    for r0 in range(0, m, rows):
        dist = distances_host(q[r0:r0 + rows], x64)
        if own:                                              # by index: the row's own column goes behind every candidate
            r = np.arange(dist.shape[0])
            dist[r, r0 + r] = np.inf
        order = np.argsort(dist, axis=1, kind="stable")[:, :take]        # stable: among equal distances the lower index
        index[r0:r0 + rows, :take] = order
        distance[r0:r0 + rows, :take] = np.take_along_axis(dist, order, axis=1)
    return index, distance


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(m, n, d, k):
    """wseg_knn_scratch_bytes (host arithmetic, no device); WsegError for invalid input."""
    return _lib.size_or_raise(_lib.load().wseg_knn_scratch_bytes(int(m), int(n), int(d), int(k)))


def device_sides(queries, corpus, who):
    """(x, own) of the launch function `who`: the corpus, and whether it is the queries themselves (None).  WsegError unless both
    sides are contiguous float32 device tensors on one device."""
    RS.check_tensor(queries, f"the queries of {who}", "[M, D]")
    if corpus is None:
        return queries, True
    RS.check_tensor(corpus, f"the corpus of {who}", "[N, D]")
    if corpus.device != queries.device:
        raise _lib.WsegError(f"the corpus is on {corpus.device}, the queries on {queries.device}")
    return corpus, False


def list_outputs(out_index, out_distance, m, k, device):
    """(index int32 [M, k], distance float32 [M, k]) on `device`: the arguments where given (checked), new tensors where None."""
    import torch
    return (RS.out_tensor(out_index, "out_index", "[M, k]", torch.int32, (m, k), device),
            RS.out_tensor(out_distance, "out_distance", "[M, k]", torch.float32, (m, k), device))


def knn_rows(queries, corpus=None, k=15, out_index=None, out_distance=None):
    """The launches: (index int32 [M, k], distance float32 [M, k]) as DEVICE tensors (`out_index` / `out_distance`, where given) for
    the contiguous float32 device tensors `queries` [M, D] and `corpus` [N, D] (None: the queries, a row not its own neighbour).
    Stream-ordered, no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    k = check_k(k)
    x, own = device_sides(queries, corpus, "knn_rows")
    m, n, d = check_shapes(queries.shape, x.shape)
    out_index, out_distance = list_outputs(out_index, out_distance, m, k, queries.device)
    if m == 0:
        return out_index, out_distance
    scratch = RS.new_scratch(scratch_bytes(m, n, d, k), queries.device)
    with torch.cuda.device(queries.device):
        _lib.check(lib.wseg_knn_f32(queries.data_ptr(), m, x.data_ptr() if n else None, n, d, k, 1 if own else 0, scratch.data_ptr(),
                                    scratch.numel(), out_index.data_ptr(), out_distance.data_ptr(), _lib.stream_ptr()))
    return out_index, out_distance


def neighbors(queries, corpus=None, k=15, device="cuda"):
    """neighbors_host's lists, computed on the GPU -> (index int32 [M, k], distance float32 [M, k]) as numpy.  `queries`, `corpus`:
    numpy (uploaded to `device`) or device tensors, which are searched where they lie; only the two result arrays travel back."""
    k = check_k(k)
    check_shapes(RS.shape_of(queries), RS.shape_of(queries if corpus is None else corpus))
    q = RS.resident(queries, device)
    x = None if corpus is None else RS.resident(corpus, q.device)
    index, distance = knn_rows(q, x, k)
    return index.cpu().numpy(), distance.cpu().numpy()


def patch_pictures_of(predictions, none=(0, 0)):
    """[rows, n_mels, W]: the pictures of `predictions`, in THE row order of everything that is computed from them and of the CLI's
    archive and CSV: file, channel, row.  `predictions` is what segment*(..., patches=W) returned — a list of prediction dicts
    carrying "patch", or of per-channel lists of them as segment_files(channel_id="all") returns: float32 numpy, concatenated once —
    or the pictures themselves, a numpy array (as float32) or a tensor [rows, n_mels, W], which is returned as it is: a device
    tensor stays where it lies.  `none`: (n_mels, W) of the result where there is no prediction to read them from.  ValueError for a
    dict without "patch" or pictures of different sizes."""
    if hasattr(predictions, "shape"):
        pictures = predictions if not isinstance(predictions, np.ndarray) else np.ascontiguousarray(predictions, dtype=np.float32)
        if len(pictures.shape) != 3:
            raise ValueError(f'the pictures must be [rows, n_mels, W] (got {tuple(pictures.shape)})')
        return pictures
    flat = [r for res in predictions for r in (res if isinstance(res, (list, tuple)) else [res])]
    pictures = []
    for r in flat:
        if not isinstance(r, dict) or "patch" not in r:
            raise ValueError('every prediction must carry "patch": call segment*(..., patches=W)')
        p = np.asarray(r["patch"], dtype=np.float32)
        if p.ndim != 3:
            raise ValueError(f'"patch" must be [rows, n_mels, W] (got {p.shape})')
        pictures.append(p)
    if len({p.shape[1:] for p in pictures}) > 1:
        raise ValueError("the predictions carry patches of different sizes")
    if not pictures:
        return np.zeros((0,) + tuple(none), np.float32)
    return np.ascontiguousarray(np.concatenate(pictures, axis=0))


def patch_rows_of(predictions):
    """[rows, n_mels * W]: patch_pictures_of, every picture as one row — the 2-D view of it."""
    pictures = patch_pictures_of(predictions)
    return pictures.reshape(pictures.shape[0], pictures.shape[1] * pictures.shape[2])


def patch_neighbors(predictions, k, device="cuda"):
    """{"neighbor_index": int32 [rows, k], "neighbor_distance": float32 [rows, k]} of every call among all the calls of
    `predictions` (see patch_pictures_of: what segment* returned, or the pictures themselves), on the GPU; indices count rows of that
    order — the rows of the CLI's CSV."""
    k = check_k(k)
    rows = patch_rows_of(predictions)
    if not len(rows):
        return {"neighbor_index": np.zeros((0, k), np.int32), "neighbor_distance": np.zeros((0, k), np.float32)}
    index, distance = neighbors(rows, None, k, device=device)
    return {"neighbor_index": index, "neighbor_distance": distance}
