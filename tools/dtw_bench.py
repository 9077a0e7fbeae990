#!/usr/bin/env python3
"""What the nearest-neighbour search under dynamic time warping costs on one MI355X (whisperseg_amd.dtw: wseg_dtw_knn_f32 on rows
that are resident in HBM), against the Euclidean search on the same rows — the price of warping — and against the host definition.
Not on the product path.

    python tools/dtw_bench.py [--sizes 2000 20000] [--host_rows 800] [--out profiles/dtw_ab.txt]

Self-search over N patch-like rows (C = 80 channels x T = 32 steps: 20 centres uniform in [-1.5, 0.5] plus 0.3 * normal noise),
band = 4, k = 15.  Reported per N:
  * wseg_dtw_knn_f32: HIP-event time around the one call that enqueues the norms, the selection and the finish kernel, rows
    resident and the outputs allocated — ms per call, and the matrix work 2 N^2 T^2 C / time against the 157.3 TFLOP/s fp32 matrix
    peak (the sweep, the norms and the exact re-rank are not counted as work);
  * wseg_knn_f32 (Euclidean) on the same rows, the same clock, the two alternating;
  * the time of each of the three kernels of one more call, from torch.profiler's kernel trace where it is available: the selection
    kernel holds the matrix-core loop AND the float32 sweep (a trace does not split a kernel), the finish kernel the float64 re-rank;
  * how many rows carry the same index set under the two distances.
Once, on the first --host_rows rows: dtw_neighbors_host (numpy, one thread), wall time, and that the device's lists are its lists.
One warm-up of each, then five repetitions; all five are printed, the median is the figure.  Per N one more line: the SHA-256 of the
index and distance arrays, so that two builds of the library (WSEG_LIB) can be held together bit for bit."""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, T, BAND, K, REPS = 80, 32, 4, 15, 5
PEAK_TFLOPS = 157.3                    # fp32 matrix (= vector) peak of an MI355X


def rows_of(n, seed=11):
    rng = np.random.default_rng([seed, n])
    centres = rng.uniform(-1.5, 0.5, size=(20, C * T))
    return (centres[rng.integers(0, 20, n)] + 0.3 * rng.standard_normal((n, C * T))).astype(np.float32)


def kernel_trace(fn):
    """{kernel name: ms} of the dtw kernels of one call of fn, or None where the profiler gives no kernel trace."""
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        found = {}
        for ev in prof.key_averages():
            if "dtw_" in ev.key:
                us = getattr(ev, "device_time_total", None)
                if us is None:
                    us = getattr(ev, "cuda_time_total", 0.0)
                found[ev.key.split("(")[0]] = found.get(ev.key.split("(")[0], 0.0) + us / 1e3
        return found or None
    except Exception as e:                               # (a measurement aid: the figures above do not depend on it)
        print(f"no kernel trace: {e!r}")
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--host_rows", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_ab.txt"))
    args = ap.parse_args()
    import torch
    from whisperseg_amd import _lib, dtw as DW, neighbors as NB
    _lib.load(require_device=True)
    lines = [f"k nearest neighbours under DTW, self-search, C = {C}, T = {T}, band = {BAND}, k = {K}, patch-like rows ({torch.cuda.get_device_name(0)}; "
             f"warm-up, then {REPS} repetitions; times in ms; TFLOP/s = 2 N^2 T^2 C / time, peak {PEAK_TFLOPS})"]
    med = statistics.median
    fmt = lambda v: " ".join(f"{t:.3f}" for t in v)
    for n in args.sizes:
        print(f"N {n} ...", flush=True)
        host = rows_of(n)
        x = torch.from_numpy(host).cuda()
        out_i = torch.empty((n, K), dtype=torch.int32, device=x.device)
        out_d = torch.empty((n, K), dtype=torch.float32, device=x.device)
        euc_i = torch.empty((n, K), dtype=torch.int32, device=x.device)
        euc_d = torch.empty((n, K), dtype=torch.float32, device=x.device)

        def timed(fn):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)

        warped = lambda: DW.dtw_knn_rows(x, None, K, C, BAND, out_index=out_i, out_distance=out_d)
        euclid = lambda: NB.knn_rows(x, None, K, out_index=euc_i, out_distance=euc_d)
        timed(warped), timed(euclid)                     # warm-up: code objects, the allocator
        t_dtw, t_knn = [], []
        for _ in range(REPS):
            t_dtw.append(timed(warped))
            t_knn.append(timed(euclid))
        work = 2.0 * n * n * T * T * C
        rate = lambda ms: work / (ms * 1e-3) / 1e12
        same = (torch.sort(out_i, dim=1).values == torch.sort(euc_i, dim=1).values).all(dim=1).float().mean().item()
        lines.append(f"N {n}: {work / 1e12:.2f} TFLOP of column products, scratch {DW.scratch_bytes(n, n, C, T, K) / 2 ** 20:.1f} MiB")
        lines.append(f"  wseg_dtw_knn_f32 (HIP events)   median {med(t_dtw):9.1f}   [{fmt(t_dtw)}]   {rate(med(t_dtw)):6.1f} TFLOP/s, "
                     f"{100 * rate(med(t_dtw)) / PEAK_TFLOPS:.0f} % of the fp32 matrix peak")
        lines.append(f"  sha256(index, distance) {hashlib.sha256(out_i.cpu().numpy().tobytes() + out_d.cpu().numpy().tobytes()).hexdigest()}")
        lines.append(f"  wseg_knn_f32, Euclidean         median {med(t_knn):9.1f}   [{fmt(t_knn)}]")
        lines.append(f"  the price of warping: {med(t_dtw) / med(t_knn):.1f}x;  rows with the same index set under both distances: {100 * same:.2f} %")
        trace = kernel_trace(warped)
        if trace:
            total = sum(trace.values())
            lines.append("  one call's kernels (torch.profiler): " + ";  ".join(f"{name} {ms:.1f} ms ({100 * ms / total:.0f} %)" for name, ms in sorted(trace.items())))
        else:
            lines.append("  one call's kernels: no kernel trace available")
        if n == args.sizes[0] and args.host_rows > 1:
            sub = host[:min(n, args.host_rows)]
            t0 = time.perf_counter()
            want_i, want_d = DW.dtw_neighbors_host(sub, None, K, C, BAND)
            t_host = time.perf_counter() - t0
            got_i, got_d = DW.dtw_neighbors(sub, None, K, C, BAND)
            t_sub = [timed(lambda: DW.dtw_knn_rows(x[:len(sub)], None, K, C, BAND)) for _ in range(3)]
            same_rows = (np.sort(got_i, axis=1) == np.sort(want_i, axis=1)).all(axis=1).mean()
            same_bits = (got_d.view(np.uint32) == want_d.view(np.uint32))[got_i == want_i].mean()
            lines.append(f"  dtw_neighbors_host on the first {len(sub)} rows (numpy, one thread): {t_host:.1f} s wall; the kernels on the same rows "
                         f"{med(t_sub):.1f} ms ({1e3 * t_host / med(t_sub):.0f}x);  rows with the definition's index set {100 * same_rows:.2f} %, "
                         f"distances with its bits where the index agrees {100 * same_bits:.2f} %")
        del x, out_i, out_d, euc_i, euc_d
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
