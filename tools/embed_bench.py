#!/usr/bin/env python3
"""What the map of the calls costs on one MI355X (whisperseg_amd.embed: the epochs of wseg_embed_epochs_f64 over the fuzzy graph of the
nearest-neighbour lists), against the definition on the host.  Not on the product path.

    python tools/embed_bench.py [--sizes 10000 100000] [--out profiles/embed_ab.txt]

Rows: N points of D = 16 around 20 centres drawn from N(0, 4^2), unit spread; k = 15, T = 200 epochs, dim 2, n_neg 5.  Reported per N:
  * the nearest-neighbour search (neighbors.neighbors, wall) and the graph step on the host (fuzzy_graph_host, wall; numpy);
  * the entries of the scheduled CSR, and how many terms (attraction + repulsion) the 200 epochs evaluate;
  * embed.layout's epochs for both kernel instances — b == 1 (a = 1: no pow) and the general b of curve_ab(0.1) — HIP events around
    the one wseg_embed_epochs_f64 call (200 launches), resident CSR and start: ms, ms an epoch, terms a second;
  * embed.layout() as a user calls it from numpy, upload and download included (wall);
  * at N <= 10 000 only, layout_host on the host (numpy, wall; one run), and whether the b == 1 result has its bits.
One warm-up, then five repetitions; all five are printed, the median is the figure.

Every size is a CHILD process under its own time limit (timeout -k 10), one after the other; after a child that did not end with
status 0 no further one is started, and what the finished ones printed is still written."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, K, T, DIM, NEG, REPS = 16, 15, 200, 2, 5, 5
HOST_MAX_N = 10000
STEP_SECONDS = 420


def rows_of(n, seed=21):
    rng = np.random.default_rng([seed, n])
    centres = rng.normal(0.0, 4.0, (20, D))
    return (centres[rng.integers(0, 20, size=n)] + rng.normal(0.0, 1.0, (n, D))).astype(np.float32)


def step(n):
    """The measurements of one size -> printed lines (this is the child)."""
    import torch
    from whisperseg_amd import _lib, embed as EM, neighbors as NB
    lib = _lib.load(require_device=True)
    med = statistics.median
    fmt = lambda v: " ".join(f"{t:.1f}" for t in v)
    rows = rows_of(n)
    NB.neighbors(rows[:256], None, K)                    # warm-up: code objects, the allocator
    t0 = time.perf_counter()
    index, distance = NB.neighbors(rows, None, K)
    t_knn = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    graph = EM.fuzzy_graph_host(index, distance)
    t_graph = (time.perf_counter() - t0) * 1e3
    print(f"N {n}: neighbors(k = {K}) {t_knn:.1f} ms (wall), fuzzy_graph_host {t_graph:.1f} ms (host, wall); {len(graph[1])} entries, "
          f"{len(graph[1]) / n:.1f} a vertex, the longest row {int(np.diff(graph[0]).max())}")
    for label, (a, b) in (("b == 1 (a = 1)", (1.0, 1.0)), ("b = curve_ab(0.1)", EM.curve_ab(0.1))):
        run = EM.Run(graph, DIM, T, None, NEG, 1.0, 1.0, a, b, None, 0)
        on = sum(int(EM.active(run.rate, t).sum()) for t in range(T))
        # the m == i skip takes 1 / N of the negatives: not counted
        terms = on * (1 + NEG)
        dev = torch.device("cuda")
        indptr, indices = torch.from_numpy(run.indptr).to(dev), torch.from_numpy(run.indices).to(dev)
        rate = torch.from_numpy(run.rate.view(np.int32)).to(dev)
        y_in = torch.from_numpy(run.y0).to(dev)
        y_out = torch.empty_like(y_in)
        scratch = torch.empty(EM.scratch_bytes(n, DIM), dtype=torch.uint8, device=dev)

        def epochs():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            _lib.check(lib.wseg_embed_epochs_f64(indptr.data_ptr(), indices.data_ptr(), rate.data_ptr(), n, run.nnz, DIM, y_in.data_ptr(), y_out.data_ptr(),
                                                 scratch.data_ptr(), scratch.numel(), 0, T, T, 1.0, a, b, 1.0, NEG, 0, _lib.stream_ptr()))
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)

        def public_call():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = EM.layout(graph, DIM, T, a=a, b=b)
            return (time.perf_counter() - t0) * 1e3, got

        epochs(), public_call()                          # warm-up
        t_dev, t_wall = [], []
        for _ in range(REPS):
            t_dev.append(epochs())
            ms, got = public_call()
            t_wall.append(ms)
            assert np.array_equal(got, y_out.cpu().numpy())
        print(f"  {label}: {run.nnz} scheduled entries, {on} active over {T} epochs, {terms / 1e6:.1f} M terms")
        print(f"    wseg_embed_epochs_f64, {T} epochs (HIP events)  median {med(t_dev):9.1f}   [{fmt(t_dev)}]   {med(t_dev) / T * 1e3:.1f} us an epoch, "
              f"{terms / med(t_dev) / 1e6:.2f} G terms/s")
        print(f"    embed.layout() from numpy (wall)               median {med(t_wall):9.1f}   [{fmt(t_wall)}]")
        if n <= HOST_MAX_N:
            t0 = time.perf_counter()
            want = EM.layout_host(graph, DIM, T, a=a, b=b)
            t_host = (time.perf_counter() - t0) * 1e3
            same = np.array_equal(want.view(np.uint64), got.view(np.uint64))
            print(f"    layout_host (host, numpy, wall; one run)       {t_host:9.1f}   host / device epochs: {t_host / med(t_dev):.0f}x; "
                  f"{'the same bits' if same else f'largest difference {np.abs(want - got).max():.3g}'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed_ab.txt"))
    ap.add_argument("--step", type=int, default=None, help="(the child of one size)")
    args = ap.parse_args()
    if args.step is not None:
        step(args.step)
        return 0
    lines = [f"layout epochs of the embedding: D = {D} rows around 20 centres, k = {K}, T = {T} epochs, dim {DIM}, n_neg {NEG} (one MI355X; warm-up, then "
             f"{REPS} repetitions; times in ms)"]
    status = 0
    for n in args.sizes:
        print(f"N {n} ...", flush=True)
        done = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", str(n)],
                              stdout=subprocess.PIPE, text=True)
        lines += done.stdout.splitlines()
        if done.returncode != 0:                         # a fault, an abort, a time limit: nothing more is started
            lines.append(f"N {n}: the step ended with status {done.returncode}; nothing was started after it")
            status = 1
            break
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return status


if __name__ == "__main__":
    sys.exit(main())
