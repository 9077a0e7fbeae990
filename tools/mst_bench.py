#!/usr/bin/env python3
"""What the mutual-reachability minimum spanning tree costs on one MI355X (whisperseg_amd.linkage: Boruvka rounds of
wseg_mst_round_f32 on rows that are resident in HBM), against the one nearest-neighbour pass it starts from and, at the small size,
against HDBSCAN on the host.  Not on the product path.

    python tools/mst_bench.py [--sizes 10000 100000] [--device_only] [--out profiles/mst_ab.txt]

Self-search rows as in tools/knn_bench.py: N random rows of D = 2 560 (a patch at W = 32) with values uniform in the patches' range
[-1.5, 0.5], min_samples s = 5.  Reported per N:
  * the one wseg_knn_f32 call (k = s) that gives the core distances: HIP-event time, ms;
  * the rounds: how many, and the HIP-event time of each wseg_mst_round_f32 call (norms, selection, finish) — a round is expected to
    cost about one nearest-neighbour pass; 2 N^2 D / time against the 157.3 TFLOP/s fp32 matrix peak;
  * linkage.mst() as a user calls it on resident rows: wall time with the device drained, host bookkeeping and copies included;
  * the round count for CLUSTERED rows of the same size (20 centres, 0.3 * normal noise, as tests/knn_cases.py) — one run;
  * at N <= 10 000 only, sklearn.cluster.HDBSCAN(min_samples = s + 1: it counts the row itself) on the host's threads, wall time,
    and hdbscan_labels on the device's tree for the same rows (the host part that follows the tree).
One warm-up, then five repetitions; all five are printed, the median is the figure.  Per N one more line: the SHA-256 of the first
round's index and weight arrays and of the tree's edges and weights, so that two builds of the library (WSEG_LIB) can be held
together bit for bit.  --device_only skips the sklearn baseline and the host's labels."""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, S, REPS = 2560, 5, 5
MIN_CLUSTER = 15
PEAK_TFLOPS = 157.3                    # fp32 matrix (= vector) peak of an MI355X
HOST_MAX_N = 10000


def rows_of(n, seed=11):
    return np.random.default_rng([seed, n]).uniform(-1.5, 0.5, size=(n, D)).astype(np.float32)


def clustered_rows_of(n, seed=12):
    rng = np.random.default_rng([seed, n])
    centres = rng.uniform(-1.5, 0.5, size=(20, D)).astype(np.float32)
    rows = centres[rng.integers(0, 20, size=n)]
    rows += 0.3 * rng.standard_normal((n, D), dtype=np.float32)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--device_only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mst_ab.txt"))
    args = ap.parse_args()
    import torch
    from whisperseg_amd import _lib, linkage as LK, neighbors as NB
    _lib.load(require_device=True)
    lines = [f"mutual-reachability minimum spanning tree, D = {D}, min_samples = {S}, uniform [-1.5, 0.5] rows ({torch.cuda.get_device_name(0)}; warm-up, "
             f"then {REPS} repetitions; times in ms; TFLOP/s = 2 N^2 D / time, peak {PEAK_TFLOPS})"]
    med = statistics.median
    fmt = lambda v: " ".join(f"{t:.3f}" for t in v)
    for n in args.sizes:
        print(f"N {n} ...", flush=True)
        host = rows_of(n)
        x = torch.from_numpy(host).cuda()
        rate = lambda ms: 2.0 * n * n * D / (ms * 1e-3) / 1e12

        def timed(fn):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            got = fn()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop), got

        def one_tree(rows):
            """-> (ms of the knn call, [ms of every round], wall ms of the same work through LK.boruvka, edges, weight)"""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            knn_ms, (_, dist) = timed(lambda: NB.knn_rows(rows, None, S))
            core = dist[:, S - 1].contiguous()
            scratch = torch.empty(LK.scratch_bytes(n, D), dtype=torch.uint8, device=rows.device)
            out_i = torch.empty((n,), dtype=torch.int32, device=rows.device)
            out_w = torch.empty((n,), dtype=torch.float32, device=rows.device)
            round_ms, sha = [], hashlib.sha256()

            def device_round(labels):
                component = torch.from_numpy(labels.astype(np.int32)).to(rows.device)
                ms, _ = timed(lambda: LK.mst_round(rows, core, component, out_i, out_w, scratch))
                round_ms.append(ms)
                got = out_i.cpu().numpy(), out_w.cpu().numpy()
                if len(round_ms) == 1:
                    sha.update(got[0].tobytes() + got[1].tobytes())
                return got

            edges, weight = LK.boruvka(n, device_round)
            sha.update(edges.tobytes() + weight.tobytes())
            return knn_ms, round_ms, (time.perf_counter() - t0) * 1e3, edges, weight, sha.hexdigest()

        def public_call():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = LK.mst(x, S)
            return (time.perf_counter() - t0) * 1e3, got

        one_tree(x), public_call()                       # warm-up: code objects, the allocator
        t_knn, t_round, t_rounds_all, t_wall, t_public = [], [], [], [], []
        for _ in range(REPS):
            knn_ms, round_ms, wall, edges, weight, sha = one_tree(x)
            t_knn.append(knn_ms)
            t_round.append(med(round_ms))
            t_rounds_all.append(round_ms)
            t_wall.append(wall)
            ms, got = public_call()
            t_public.append(ms)
            assert np.array_equal(got[0], edges) and np.array_equal(got[1], weight)
        rounds = len(t_rounds_all[0])
        assert all(len(r) == rounds for r in t_rounds_all)
        per_round = [med([r[i] for r in t_rounds_all]) for i in range(rounds)]
        lines.append(f"N {n}: {2.0 * n * n * D / 1e12:.2f} TFLOP of products a pass, scratch {LK.scratch_bytes(n, D) / 2 ** 20:.1f} MiB; {rounds} rounds")
        lines.append(f"  wseg_knn_f32, k = {S} (HIP events)          median {med(t_knn):9.1f}   [{fmt(t_knn)}]   {rate(med(t_knn)):6.1f} TFLOP/s")
        lines.append(f"  wseg_mst_round_f32, a round (HIP events)   median {med(t_round):9.1f}   [{fmt(t_round)}]   {rate(med(t_round)):6.1f} TFLOP/s, "
                     f"{100 * rate(med(t_round)) / PEAK_TFLOPS:.0f} % of the fp32 matrix peak; round / knn pass: {med(t_round) / med(t_knn):.2f}x")
        lines.append(f"  the rounds one by one (medians)            [{fmt(per_round)}]")
        lines.append(f"  sha256(first round's index, weight; edges, weight) {sha}")
        lines.append(f"  linkage.mst(), resident rows (wall)        median {med(t_public):9.1f}   [{fmt(t_public)}]   of which knn + rounds on the device "
                     f"{med(t_knn) + sum(per_round):.1f}")
        del x
        torch.cuda.empty_cache()
        c = torch.from_numpy(clustered_rows_of(n)).cuda()
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c_edges, c_weight = LK.mst(c, S, stats=stats)
        c_ms = (time.perf_counter() - t0) * 1e3
        lines.append(f"  clustered rows (20 centres + 0.3 noise)    {stats['rounds']} rounds, linkage.mst() {c_ms:.1f} (one run)")
        if n <= HOST_MAX_N and not args.device_only:
            from sklearn.cluster import HDBSCAN
            t0 = time.perf_counter()
            labels = LK.hdbscan_labels(edges, weight, n, MIN_CLUSTER)
            t_labels = (time.perf_counter() - t0) * 1e3
            t_host = []
            for _ in range(3):
                t0 = time.perf_counter()
                theirs = HDBSCAN(min_cluster_size=MIN_CLUSTER, min_samples=S + 1, n_jobs=-1).fit(host).labels_
                t_host.append((time.perf_counter() - t0) * 1e3)
                if t_host[-1] > 20e3:                # (minutes at this size: once is the figure)
                    break
            lines.append(f"  hdbscan_labels on the tree (host, numpy)   {t_labels:9.1f}   ({int(labels.max()) + 1} clusters, {int((labels < 0).sum())} rows noise: uniform rows have none to find)")
            lines.append(f"  sklearn HDBSCAN, {os.environ.get('OMP_NUM_THREADS', '?')} threads (wall)          median {med(t_host):9.1f}   [{fmt(t_host)}]   ({int(theirs.max()) + 1} clusters); "
                         f"host / (linkage.mst() + hdbscan_labels): {med(t_host) / (med(t_public) + t_labels):.1f}x")
        del c
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
