#!/usr/bin/env python3
"""What the nearest-neighbour search costs on one MI355X (whisperseg_amd.neighbors: wseg_knn_f32 on rows that are resident in HBM),
against what a user would write today on the same GPU and, at the small size, on the host.  Not on the product path.

    python tools/knn_bench.py [--sizes 10000 100000] [--k 15] [--device_only] [--out profiles/knn_ab.txt]

Self-search over N random rows of D = 2 560 (a patch at W = 32) with values uniform in the patches' range [-1.5, 0.5], k = 15
(--k 64 times the selection kernel with the long lists).
Reported per N:
  * the kernels: HIP-event time around the one call that enqueues the norms, the selection and the finish kernel, rows resident and
    the outputs allocated — ms per call, and 2 N^2 D / time against the 157.3 TFLOP/s fp32 matrix peak (the norms and the exact
    re-rank are not counted as work: the figure is the rate of the N x N products a search needs);
  * blocked torch on the same GPU: per block of queries sized to 1 GiB of scores, |q|^2 + |x|^2 - 2 q @ x.T, the block's own diagonal
    set to +inf, torch.topk(k, largest=False) — the same HIP-event clock, the two device paths alternating;
  * at N <= 10 000 only, blocked numpy float32 on the host's threads (sgemm, argpartition, a sort of the k kept), wall time;
  * how many rows of the torch result carry the same index set as the kernels' (float32 |q|^2 + |x|^2 - 2 q.x against the exact
    re-rank: they may differ at the k-th boundary).
One warm-up of each, then five repetitions; all five are printed, the median is the figure.  Per N one more line: the SHA-256 of the
kernels' index and distance arrays, so that two builds of the library (WSEG_LIB) can be held together bit for bit.  --device_only
skips the torch and numpy baselines: the kernels' times and the digest alone."""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, REPS = 2560, 5
PEAK_TFLOPS = 157.3                    # fp32 matrix (= vector) peak of an MI355X
SCORE_BLOCK_BYTES = 1 << 30
HOST_MAX_N = 10000


def rows_of(n, seed=11):
    return np.random.default_rng([seed, n]).uniform(-1.5, 0.5, size=(n, D)).astype(np.float32)


def digest(*tensors):
    """SHA-256 over the bytes of device tensors, in order"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def torch_blocked(x, k):
    import torch
    n = x.shape[0]
    xn = (x * x).sum(dim=1)
    block = max(1, SCORE_BLOCK_BYTES // (4 * n))
    index = torch.empty((n, k), dtype=torch.int64, device=x.device)
    distance = torch.empty((n, k), dtype=torch.float32, device=x.device)
    for r0 in range(0, n, block):
        q = x[r0:r0 + block]
        scores = torch.addmm(xn[r0:r0 + block, None] + xn[None, :], q, x.t(), alpha=-2.0)
        r = torch.arange(q.shape[0], device=x.device)
        scores[r, r0 + r] = float("inf")
        distance[r0:r0 + block], index[r0:r0 + block] = torch.topk(scores, k, dim=1, largest=False)
    return index, distance


def numpy_blocked(x, k):
    n = x.shape[0]
    xn = np.einsum("nc,nc->n", x, x)
    block = max(1, SCORE_BLOCK_BYTES // (4 * n))
    index = np.empty((n, k), dtype=np.int64)
    for r0 in range(0, n, block):
        q = x[r0:r0 + block]
        scores = xn[r0:r0 + block, None] + xn[None, :] - 2.0 * (q @ x.T)
        r = np.arange(len(q))
        scores[r, r0 + r] = np.inf
        part = np.argpartition(scores, k, axis=1)[:, :k]
        order = np.argsort(np.take_along_axis(scores, part, axis=1), axis=1, kind="stable")
        index[r0:r0 + block] = np.take_along_axis(part, order, axis=1)
    return index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--device_only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_ab.txt"))
    args = ap.parse_args()
    K = args.k
    import torch
    from whisperseg_amd import _lib, neighbors as NB
    _lib.load(require_device=True)
    lines = [f"k nearest neighbours, self-search, D = {D}, k = {K}, uniform [-1.5, 0.5] rows ({torch.cuda.get_device_name(0)}; warm-up, then {REPS} "
             f"repetitions; times in ms; TFLOP/s = 2 N^2 D / time, peak {PEAK_TFLOPS})"]
    for n in args.sizes:
        print(f"N {n} ...", flush=True)
        host = rows_of(n)
        x = torch.from_numpy(host).cuda()
        out_i = torch.empty((n, K), dtype=torch.int32, device=x.device)
        out_d = torch.empty((n, K), dtype=torch.float32, device=x.device)

        def timed(fn):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            got = fn()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop), got

        kernels = lambda: timed(lambda: NB.knn_rows(x, None, K, out_index=out_i, out_distance=out_d))
        baseline = lambda: timed(lambda: torch_blocked(x, K))
        kernels()                                        # warm-up: code objects, the allocator, the BLAS library's choice
        if not args.device_only:
            baseline()
        t_kernel, t_torch = [], []
        for _ in range(REPS):
            ms, _ = kernels()
            t_kernel.append(ms)
            if not args.device_only:
                ms, (base_i, _) = baseline()
                t_torch.append(ms)
        med = statistics.median
        fmt = lambda v: " ".join(f"{t:.3f}" for t in v)
        rate = lambda ms: 2.0 * n * n * D / (ms * 1e-3) / 1e12
        lines.append(f"N {n}: {2.0 * n * n * D / 1e12:.2f} TFLOP of products, scratch {NB.scratch_bytes(n, n, D, K) / 2 ** 20:.1f} MiB")
        lines.append(f"  wseg_knn_f32 (HIP events)       median {med(t_kernel):9.1f}   [{fmt(t_kernel)}]   {rate(med(t_kernel)):6.1f} TFLOP/s, "
                     f"{100 * rate(med(t_kernel)) / PEAK_TFLOPS:.0f} % of the fp32 matrix peak")
        lines.append(f"  sha256(index, distance) {digest(out_i, out_d)}")
        if not args.device_only:
            same = (torch.sort(out_i.long(), dim=1).values == torch.sort(base_i, dim=1).values).all(dim=1).float().mean().item()
            lines.append(f"  blocked torch (addmm + topk)    median {med(t_torch):9.1f}   [{fmt(t_torch)}]   {rate(med(t_torch)):6.1f} TFLOP/s")
            lines.append(f"  torch / kernels: {med(t_torch) / med(t_kernel):.2f}x;  rows with the same index set: {100 * same:.2f} %")
        if n <= HOST_MAX_N and not args.device_only:
            numpy_blocked(host, K)
            t_host = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                host_i = numpy_blocked(host, K)
                t_host.append((time.perf_counter() - t0) * 1e3)
            same_host = (np.sort(host_i, axis=1) == np.sort(out_i.cpu().numpy().astype(np.int64), axis=1)).all(axis=1).mean()
            lines.append(f"  blocked numpy float32, {os.environ.get('OMP_NUM_THREADS', '?')} threads  median {med(t_host):9.1f}   [{fmt(t_host)}]   "
                         f"{rate(med(t_host)):6.2f} TFLOP/s;  host / kernels: {med(t_host) / med(t_kernel):.0f}x;  same index set: {100 * same_host:.2f} %")
        del x, out_i, out_d
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
