"""Principal components of the calls: the linear step between the per-segment pictures (whisperseg_amd.patches) and what works on
them as rows of D = 80 W numbers — neighbours, clusters, the map.  The first r components are the classic input of those, the
explained variances and the scores belong next to the measurements in a per-call feature table, and the first `dim` scores are the
start of the map (embed.embed(init="pca")).  The heavy parts are the second moments S = X^T X (N D^2 multiply-adds) and the scores
Z = (X - mean) V (N D r): those run on the GPU, in float64 on the matrix cores (wseg_pca_moments_f64 / wseg_pca_project_f64:
whisperseg_amd/csrc/wseg_pca.hip), without an N x D float64 copy; the D x D eigen-decomposition is host work.

`moments_host`, `pca_from_moments` and `project_host` are THE definition (numpy, float64) and the oracle of every device test;
`moments` and `project` are the device steps, `pca` goes from rows to components and scores and `patch_pca` takes what
`segment*(..., patches=W)` returned.

For rows X float32 [N, D], finite, 2 <= N <= 2^31 - 1, 1 <= D <= 8192 (the float64 Gram matrix is then 512 MiB; 80 x 64, the widest
DTW patch, fits), and r in 1 .. min(64, D, N - 1):

  moments        s[c] = sum_n x[n, c] and S[i, j] = sum_n x[n, i] x[n, j]: every product is the exact float64 product of the two
                 float32 values (48 significant bits at most), and a sum is DEFINED as its correctly rounded value — the order of
                 the additions is not part of the definition.  S is symmetric bit for bit.  moments_exact computes exactly that
                 (math.fsum; small inputs), moments_host is numpy for larger ones
  covariance     on the host, float64, in this order: mean = s / N; C = (S - outer(s, s) / N) / (N - 1).  The subtraction cancels
                 about log2(mean^2 / variance) of the 53 bits of a column — harmless for log-mel pictures, whose offset and spread are
                 of one order (2 to 6 bits), but rows riding on a huge offset (mean^2 / variance towards 2^40 and beyond) should have
                 it subtracted BEFORE the call: the result for x - c is the same and keeps its bits
  decomposition  numpy.linalg.eigh(C); the r largest eigenvalues in descending order; variance = those, values below 0 clamped to 0;
                 variance_ratio = variance / trace(C), 0 where the trace is not positive; every component's sign is fixed so that its
                 entry of largest magnitude (the first one on a tie) is positive.  pca_from_moments is this step (and the covariance)
                 alone: the host and the device path both call it
  scores         Z[n, j] = sum_c (float64(x[n, c]) - mean[c]) basis[c, j] in float64, basis = components^T [D, r]; the entry points
                 round them once to float32
  conventions    an r outside its range, an X that is not 2-D, a D outside 1 .. 8192 or N < 2: ValueError before anything runs

What the device may differ by: nothing in the moments where every partial sum is exact (integer-valued rows, say); elsewhere a sum
of N terms is within (N - 1) 2^-53 sum|terms| of its exact value — the products are exact, only the additions round — and a score
within (D + 2) 2^-53 sum_c |x - mean| |basis| (tests/pca_cases.py).  The device result is the same on every run: the rows are split
as a function of (N, D) alone and the partial sums added in ascending split order.
"""
import math

import numpy as np

from . import _lib, neighbors as NB, resident as RS

MAX_D = 8192                           # columns (csrc/wseg_pca_plan.h::kPcaMaxD)
MAX_R = 64                             # components (kPcaMaxR)
MAX_ROWS = 2 ** 31 - 1
HOST_BLOCK_BYTES = 128 << 20           # float64 rows moments_host / project_host hold at a time


def check_shape(shape):
    """(N, D) of a shape; ValueError unless it is 2-D with N >= 2 and D in 1 .. 8192."""
    if len(shape) != 2:
        raise ValueError(f"the rows must be 2-D [N, D] (got {tuple(shape)})")
    n, d = int(shape[0]), int(shape[1])
    if not 1 <= d <= MAX_D:
        raise ValueError(f"D must be 1 .. {MAX_D} (got {d})")
    if not 2 <= n <= MAX_ROWS:
        raise ValueError(f"N must be 2 .. 2^31 - 1 rows (got {n})")
    return n, d


def check_r(r, n, d):
    """`r` as an int, ValueError unless it is an integer in 1 .. min(64, D, N - 1)."""
    top = min(MAX_R, d, n - 1)
    return RS.check_int(r, "r", 1, top, f"in 1 .. min({MAX_R}, D, N - 1) = {top}")


# ---- the definition (host) -----------------------------------------------------------------------------------------------------------
def moments_exact(rows):
    """(s float64 [D], S float64 [D, D]): the moments with every sum correctly rounded (math.fsum over exact products), for SMALL
    inputs: D^2 N / 2 Python operations."""
    x = np.ascontiguousarray(rows, dtype=np.float32).astype(np.float64)
    n, d = check_shape(x.shape)
    s = np.array([math.fsum(x[:, c]) for c in range(d)], dtype=np.float64)
    gram = np.empty((d, d), np.float64)
    for i in range(d):
        prod = x[:, i:i + 1] * x[:, i:]                    # exact: two float32 values
        for j in range(i, d):
            gram[i, j] = gram[j, i] = math.fsum(prod[:, j - i])
    return s, gram


def moments_host(rows):
    """(s float64 [D], S float64 [D, D]) in numpy, block of rows by block of rows; the upper triangle is mirrored, so S is symmetric
    bit for bit."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    n, d = check_shape(x.shape)
    s, gram = np.zeros(d, np.float64), np.zeros((d, d), np.float64)
    step = max(1, HOST_BLOCK_BYTES // (8 * d))
    for r0 in range(0, n, step):
        block = x[r0:r0 + step].astype(np.float64)
        s += block.sum(axis=0)
        gram += block.T @ block
    upper = np.triu(gram)
    return s, upper + np.triu(gram, 1).T


def pca_from_moments(s, gram, n, r):
    """The covariance, the decomposition and the conventions of the definition -> {"mean" [D], "components" [r, D], "variance" [r],
    "variance_ratio" [r]}, all float64."""
    s, gram = np.asarray(s, dtype=np.float64), np.asarray(gram, dtype=np.float64)
    if s.ndim != 1 or gram.shape != (len(s), len(s)):
        raise ValueError(f"the moments must be s [D] and S [D, D] (got {s.shape} and {gram.shape})")
    n = int(n)
    check_shape((n, len(s)))
    r = check_r(r, n, len(s))
    mean = s / n
    cov = (gram - np.outer(s, s) / n) / (n - 1)
    values, vectors = np.linalg.eigh(cov)
    order = np.argsort(-values, kind="stable")[:r]
    components = np.ascontiguousarray(vectors[:, order].T)
    for v in components:
        if v[np.argmax(np.abs(v))] < 0:
            v *= -1.0
    variance = np.maximum(values[order], 0.0)
    trace = float(np.trace(cov))
    ratio = variance / trace if trace > 0 else np.zeros(r, np.float64)
    return {"mean": mean, "components": components, "variance": variance, "variance_ratio": ratio}


def project_host(rows, mean, basis):
    """The scores float64 [N, r] of the float32 rows [N, D] on the float64 basis [D, r] about the float64 mean [D]."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    mean, basis = np.asarray(mean, dtype=np.float64), np.asarray(basis, dtype=np.float64)
    check_project(x.shape, mean.shape, basis.shape)
    out = np.empty((len(x), basis.shape[1]), np.float64)
    step = max(1, HOST_BLOCK_BYTES // (8 * x.shape[1]))
    for r0 in range(0, len(x), step):
        out[r0:r0 + step] = (x[r0:r0 + step].astype(np.float64) - mean) @ basis
    return out


def check_project(x_shape, mean_shape, basis_shape):
    """(N, D, r) of a projection; ValueError unless rows [N, D], mean [D] and basis [D, r] fit, D in 1 .. 8192, r in 1 .. 64."""
    if len(x_shape) != 2:
        raise ValueError(f"the rows must be 2-D [N, D] (got {tuple(x_shape)})")
    n, d = int(x_shape[0]), int(x_shape[1])
    if not 1 <= d <= MAX_D:
        raise ValueError(f"D must be 1 .. {MAX_D} (got {d})")
    if n > MAX_ROWS:
        raise ValueError(f"N must be at most 2^31 - 1 rows (got {n})")
    if tuple(mean_shape) != (d,) or len(basis_shape) != 2 or basis_shape[0] != d:
        raise ValueError(f"mean must be [D] and basis [D, r] with D = {d} (got {tuple(mean_shape)} and {tuple(basis_shape)})")
    if not 1 <= basis_shape[1] <= MAX_R:
        raise ValueError(f"r must be 1 .. {MAX_R} columns of the basis (got {basis_shape[1]})")
    return n, d, int(basis_shape[1])


def pca_host(rows, r, scores=True):
    """The definition -> {"mean" float64 [D], "components" float64 [r, D], "variance" float64 [r], "variance_ratio" float64 [r],
    "scores" float32 [N, r]} (`scores=False`: without the last)."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    n, d = check_shape(x.shape)
    r = check_r(r, n, d)
    out = pca_from_moments(*moments_host(x), n, r)
    if scores:
        out["scores"] = project_host(x, out["mean"], out["components"].T).astype(np.float32)
    return out


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(n, d):
    """wseg_pca_scratch_bytes (host arithmetic, no device); WsegError for invalid input."""
    return _lib.size_or_raise(_lib.load().wseg_pca_scratch_bytes(int(n), int(d)))


def moments_rows(x):
    """The launches: (s float64 [D], S float64 [D, D]) as DEVICE tensors for the contiguous float32 device tensor `x` [N, D].
    Stream-ordered, no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    RS.check_tensor(x, "the rows of moments_rows", "[N, D]")
    n, d = check_shape(x.shape)
    s = torch.empty(d, dtype=torch.float64, device=x.device)
    gram = torch.empty((d, d), dtype=torch.float64, device=x.device)
    scratch = RS.new_scratch(scratch_bytes(n, d), x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.wseg_pca_moments_f64(x.data_ptr(), n, d, s.data_ptr(), gram.data_ptr(), scratch.data_ptr(), scratch.numel(), _lib.stream_ptr()))
    return s, gram


def project_rows(x, mean, basis):
    """The launch: the scores float64 [N, r] as a DEVICE tensor for the contiguous float32 device tensor `x` [N, D] and the float64
    mean [D] and basis [D, r] (numpy, uploaded).  Stream-ordered, no host synchronisation."""
    import torch
    lib = _lib.load(require_device=True)
    RS.check_tensor(x, "the rows of project_rows", "[N, D]")
    mean, basis = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(basis, dtype=np.float64)
    n, d, r = check_project(x.shape, mean.shape, basis.shape)
    out = torch.empty((n, r), dtype=torch.float64, device=x.device)
    if n == 0:
        return out
    mean_d, basis_d = torch.from_numpy(mean).to(x.device), torch.from_numpy(basis).to(x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.wseg_pca_project_f64(x.data_ptr(), n, d, mean_d.data_ptr(), basis_d.data_ptr(), r, out.data_ptr(), _lib.stream_ptr()))
    return out


def moments(rows, device="cuda"):
    """moments_host's (s, S), computed on the GPU, as numpy.  `rows`: numpy (uploaded to `device`) or a device tensor."""
    check_shape(RS.shape_of(rows))
    s, gram = moments_rows(RS.resident(rows, device))
    return s.cpu().numpy(), gram.cpu().numpy()


def project(rows, mean, basis, device="cuda"):
    """project_host's scores float64 [N, r], computed on the GPU, as numpy."""
    check_project(RS.shape_of(rows), np.shape(mean), np.shape(basis))
    return project_rows(RS.resident(rows, device), mean, basis).cpu().numpy()


def pca(rows, r, device="cuda", scores=True):
    """pca_host's dict with the moments and the scores computed on the GPU: the rows go up once (or are used where they lie), the
    D x D moments come back for the host decomposition, the basis goes up and the scores come back."""
    n, d = check_shape(RS.shape_of(rows))
    r = check_r(r, n, d)
    x = RS.resident(rows, device)
    s, gram = moments_rows(x)
    out = pca_from_moments(s.cpu().numpy(), gram.cpu().numpy(), n, r)
    if scores:
        out["scores"] = project_rows(x, out["mean"], out["components"].T).cpu().numpy().astype(np.float32)
    return out


def empty_result(d, r, prefix=""):
    """The arrays of no decomposition (no rows, or a single one): empty, with the trailing shapes of a real one."""
    return {prefix + "mean": np.zeros(0, np.float64), prefix + "components": np.zeros((0, d), np.float64),
            prefix + "variance": np.zeros(0, np.float64), prefix + "variance_ratio": np.zeros(0, np.float64),
            prefix + "scores": np.zeros((0, r), np.float32)}


def patch_pca(predictions, r, device="cuda"):
    """{"pca_mean", "pca_components", "pca_variance", "pca_variance_ratio", "pca_scores"} of all the calls of `predictions` — what
    segment*(..., patches=W) returned, or the pictures themselves (neighbors.patch_pictures_of): the rows of the CLI's CSV.  No rows
    or a single one: empty arrays with the right trailing shapes, and nothing runs."""
    r = RS.check_int(r, "r", 1, MAX_R)
    rows = NB.patch_rows_of(predictions)
    if len(rows) < 2:
        return empty_result(int(rows.shape[1]), r, "pca_")
    return {"pca_" + key: value for key, value in pca(rows, r, device=device).items()}
