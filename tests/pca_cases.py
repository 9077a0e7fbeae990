"""Inputs, references and DERIVED bounds of the principal-component tests (whisperseg_amd/pca.py, csrc/wseg_pca.hip).  Nothing here is
taken from what the device returns; every reference is computed once (functools.lru_cache) and handed out read-only.

u = 2^-53 is the unit roundoff of float64.

Exact cases     integer-valued float32 rows in [-8, 8]: every product (|.| <= 64) and every partial sum (|.| <= 64 * 1027 < 2^17) is
                exact in float64 whatever the order, so the device must return moments_exact's bits.  The rows are deliberately not
                symmetric in any way — another distribution per column, a ramp over the rows added to every third column — so that a
                transposed, mirrored or misplaced fragment changes the result (the C/D map of the f64 MFMA is not the f32 one).
                N covers non-multiples of the k-step 4 and of the row chunk 32, D one partial tile, a tile edge, several 16-column
                tiles with off-diagonal ones, a second 64-column block and a ragged last tile.
                Row splits under the plan (splits_of mirrors csrc/wseg_pca_plan.h): ceil(N / 256) of them while the tiles are few,
                so (257, *) has 2 splits and (1027, *) has 5; every other N here has 1.  test_pca_cpu.py checks the mirror against
                the library's scratch size, test_pca_gpu.py runs both kinds.
Float cases     seeded normal rows plus a per-column offset.  The products are exact; a sum of N terms takes N - 1 additions, each
                with a relative error of at most u on a partial sum bounded by T = sum_n |x_ni x_nj|:
                    |S_dev - S_exact|[i, j] <= (N - 1) u T[i, j] / (1 - (N - 1) u)        (moments_bound; the same with |x| for s)
                whatever the order of the additions and the number of splits.
Projection      reference in numpy.longdouble (64 significant bits here).  One rounding of x - mean, one of the product (or none,
                fused), D - 1 additions:
                    |Z_dev - Z_ref| <= (D + 2) u A / (1 - (D + 2) u) + D 2^-64 A,  A = sum_c |x - mean| |basis|   (project_bound)
                the second term being the reference's own error.  With integer rows, mean and basis everything is exact.
Host constant   LAPACK's backward-error constant is not documented, so how far pca_host may be from a KNOWN answer is measured, on
                the CPU, against a construction — never against the device: X = U diag(sigma) W^T with U 16 zero-mean orthonormal
                columns of the 64 x 64 Sylvester-Hadamard matrix / 8 and W the 16 x 16 one / 4, sigma = 96, 64, 48, 36, 27, 20, 15,
                11, 8, 6, 5, 4, 3, 2, 1, 0.5.  X is exact in float32 (multiples of 1 / 64), its covariance is W diag(sigma^2 / 63) W^T,
                so the components are the columns of W — up to their sign: all 16 entries of a column have one magnitude, so
                the sign rule's choice hangs on the last bit and the comparison aligns the signs first — and
                variance = sigma^2 / 63.  Measured with numpy / OpenBLAS on x86-64 over the first 8 components, with 1, 4 and 16
                BLAS threads alike: the eigenvalue error is 2.92e-16 of the largest eigenvalue and the largest component entry
                error 2.23e-15 (known_answer_errors returns them).  HOST_EIG_REL and HOST_VEC_ABS are those with a 16x margin: another BLAS
                thread count reorders the reductions.
"""
import functools

import numpy as np

from whisperseg_amd import pca as PC

U = 2.0 ** -53

# (N, D): each N and each D at least once, plus the corners; about 14 pairs
EXACT_PAIRS = ((2, 1), (2, 130), (3, 17), (5, 15), (5, 16), (63, 65), (65, 16), (65, 130), (257, 1), (257, 17), (257, 65), (1027, 15), (1027, 130),
               (63, 1))
FLOAT_PAIRS = ((3, 17), (5, 130), (63, 16), (65, 65), (257, 15), (1027, 130))
MULTI_SPLIT = {(257, 1): 2, (257, 17): 2, (257, 65): 2, (257, 15): 2, (1027, 15): 5, (1027, 130): 5}

HOST_EIG_REL = 16 * 2.92e-16           # |variance - truth| / largest variance of pca_host on the known-answer construction, x 16
HOST_VEC_ABS = 16 * 2.23e-15           # largest |component entry - truth| there, x 16


def splits_of(n, d):
    """The row splits of wseg_pca_moments_f64 for (n, d): csrc/wseg_pca_plan.h::pca_plan in Python."""
    nb = -(-d // 64)
    tiles = nb * (nb + 1) // 2
    s = min(-(-1024 // tiles), -(-n // 256))
    rows_per_split = -(-(-(-n // s)) // 32) * 32
    return -(-n // rows_per_split)


def scratch_bytes_of(n, d):
    """wseg_pca_scratch_bytes(n, d) in Python: the same header."""
    nb = -(-d // 64)
    tiles = nb * (nb + 1) // 2
    bound = min(tiles * -(-n // 256), tiles + 1024, 2048)
    pad = lambda b: max(256, -(-b // 256) * 256)
    return pad(bound * 64 * 64 * 8) + pad(bound * 64 * 8)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def exact_rows(n, d):
    """Integer-valued float32 [n, d] in [-8, 8], no symmetry: column c draws from its own range [lo_c, hi_c], every third column
    carries a ramp over the rows."""
    rng = np.random.default_rng([20240, n, d])
    lo = -(np.arange(d) % 5) - 1                       # -1 .. -5
    hi = (np.arange(d) * 3) % 4 + 1                    # 1 .. 4
    x = rng.integers(lo, hi + 1, size=(n, d)).astype(np.int64)
    ramp = (np.arange(n) * 7 // max(n, 2)) % 4         # 0 .. 3, ascending in blocks
    x[:, ::3] += ramp[:, None]
    assert x.min() >= -8 and x.max() <= 8
    return _frozen(x.astype(np.float32))


@functools.lru_cache(maxsize=None)
def exact_moments(n, d):
    return _frozen(*PC.moments_exact(exact_rows(n, d)))


@functools.lru_cache(maxsize=None)
def float_rows(n, d):
    """Seeded normal float32 [n, d] with a per-column offset and scale (log-mel like: offset and spread of one order)."""
    rng = np.random.default_rng([20241, n, d])
    offset = rng.uniform(-3.0, 3.0, d)
    scale = rng.uniform(0.25, 2.0, d)
    return _frozen((rng.normal(0.0, 1.0, (n, d)) * scale + offset).astype(np.float32))


@functools.lru_cache(maxsize=None)
def float_moments(n, d):
    return _frozen(*PC.moments_exact(float_rows(n, d)))


def moments_bound(rows):
    """(bound of s [D], bound of S [D, D]) for the rows: (N - 1) u T / (1 - (N - 1) u), T the sum of the magnitudes (itself rounded
    up by its own (N + 1) u)."""
    x = np.abs(np.asarray(rows, dtype=np.float32).astype(np.float64))
    n = len(x)
    factor = (n - 1) * U / (1.0 - (n - 1) * U) * (1.0 + (n + 1) * 2 * U)
    return factor * x.sum(axis=0), factor * (x.T @ x)


def integer_projection(n, d, r):
    """(rows, mean, basis): integer-valued rows [n, d] (exact_rows), mean [d] in -4 .. 4 and basis [d, r] in -3 .. 3, no symmetry."""
    rng = np.random.default_rng([20242, n, d, r])
    mean = rng.integers(-4, 5, size=d).astype(np.float64)
    basis = rng.integers(-3, 4, size=(d, r)).astype(np.float64)
    basis[:, 0] += (np.arange(d) % 2)                  # column 0 differs from every other in distribution
    return exact_rows(n, d), mean, basis


def float_projection(n, d, r):
    """(rows, mean, basis) of a float case: the float rows, their float64 column means and a seeded orthonormal basis [d, r]."""
    rng = np.random.default_rng([20243, n, d, r])
    rows = float_rows(n, d)
    basis = np.linalg.qr(rng.normal(0.0, 1.0, (d, max(r, 1))))[0][:, :r]
    return rows, rows.astype(np.float64).mean(axis=0), np.ascontiguousarray(basis)


def project_reference(rows, mean, basis):
    """(Z float64 [n, r] rounded from numpy.longdouble, the bound [n, r] of a float64 evaluation against it)."""
    ld = np.longdouble
    diff = np.asarray(rows, dtype=np.float32).astype(ld) - np.asarray(mean, dtype=np.float64).astype(ld)
    b = np.asarray(basis, dtype=np.float64).astype(ld)
    z = diff @ b
    a = (np.abs(diff) @ np.abs(b)).astype(np.float64)
    d = diff.shape[1]
    eps_ref = float(np.finfo(ld).eps) / 2                # 2^-64 where longdouble is the x87 format
    bound = ((d + 2) * U / (1.0 - (d + 2) * U) + d * eps_ref) * a * (1.0 + 4 * d * U)
    return z.astype(np.float64), bound


def sylvester(n):
    h = np.array([[1.0]])
    while len(h) < n:
        h = np.block([[h, h], [h, -h]])
    return h


SIGMA = np.array([96, 64, 48, 36, 27, 20, 15, 11, 8, 6, 5, 4, 3, 2, 1, 0.5])
KNOWN_R = 8


@functools.lru_cache(maxsize=None)
def known_answer():
    """(rows float32 [64, 16], components [16, 16] (rows: W's columns), variance [16]) of the construction."""
    u = sylvester(64)[:, 1:17] / 8.0                   # zero-mean orthonormal columns
    w = sylvester(16) / 4.0
    x = (u * SIGMA) @ w.T
    rows = x.astype(np.float32)
    assert np.array_equal(rows.astype(np.float64), x) and np.array_equal(x * 64, np.round(x * 64))
    return _frozen(rows, np.ascontiguousarray(w.T), SIGMA ** 2 / 63.0)


def known_answer_errors(result, r=KNOWN_R):
    """(eigenvalue error / largest eigenvalue, largest component entry error) of a pca result on the construction."""
    _, components, variance = known_answer()
    eig = float(np.abs(result["variance"][:r] - variance[:r]).max() / variance[0])
    got = result["components"][:r]
    got = got * np.sign(np.einsum("ij,ij->i", got, components[:r]))[:, None]          # (the sign rule has no stable choice here)
    vec = float(np.abs(got - components[:r]).max())
    return eig, vec


@functools.lru_cache(maxsize=None)
def diagonal_case():
    """Rows float32 [64, 12] whose covariance is exactly diagonal with distinct entries and whose column sums are multiples of 64:
    column c = a_c * (column c + 1 of the 64 x 64 Hadamard matrix) + m_c, a = 12, 11 .. 1 (integers), m_c integers.  Every moment is
    exact, the mean is integer, and a decomposition of a diagonal matrix has unit vectors as components: every score is a single
    exact product, so a device run and the definition agree in every bit of every array."""
    a = np.arange(12, 0, -1).astype(np.float64)
    m = (np.arange(12) % 5 - 2).astype(np.float64)
    return _frozen((sylvester(64)[:, 1:13] * a + m).astype(np.float32))
