#!/usr/bin/env python3
"""What placing new rows on a frozen map costs on one MI355X (whisperseg_amd.embed.place: the one launch of wseg_embed_place_f64),
against the definition on the host and against the same epochs run as one launch per epoch.  Not on the product path.

    python tools/place_bench.py [--sizes 64 1000 10000] [--out profiles/place_ab.txt]

The corpus: N = 20 000 points of D = 16 around 20 centres drawn from N(0, 4^2), unit spread, on a random 2-D cloud in [-10, 10)^2 (the
cost of an epoch does not depend on where the frozen points lie); M new rows of the same family, k = 15, T = 100 epochs, n_neg 5,
a, b = curve_ab(0.1) (the kernel instance with pow).  Reported per M:
  * the search for the lists (neighbors.neighbors of the new rows among the corpus, wall) and the host steps membership_host,
    row_keys and start_host (wall; numpy);
  * embed.place_rows with resident inputs — ONE launch for the 100 epochs — HIP events around the call: ms;
  * the same epochs as 100 calls (t, t + 1), each continuing from the one before (ping-pong between two buffers): HIP events
    around all of them: ms, and whether the result has the single launch's bits;
  * embed.place() as a user calls it from numpy, upload and download included (wall);
  * place_host on the host (numpy, wall; one run), and the largest difference from the device's result.
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

N, D, K, T, DIM, NEG, REPS = 20000, 16, 15, 100, 2, 5, 5
STEP_SECONDS = 300


def rows_of(n, seed):
    rng = np.random.default_rng([seed, n])
    centres = np.random.default_rng(21).normal(0.0, 4.0, (20, D))
    return (centres[rng.integers(0, 20, size=n)] + rng.normal(0.0, 1.0, (n, D))).astype(np.float32)


def step(m):
    """The measurements of one size -> printed lines (this is the child)."""
    import torch
    from whisperseg_amd import _lib, embed as EM, neighbors as NB
    lib = _lib.load(require_device=True)
    med = statistics.median
    fmt = lambda v: " ".join(f"{t:.2f}" for t in v)
    corpus_rows, new_rows = rows_of(N, 1), rows_of(m, 2)
    positions = np.random.default_rng(3).uniform(-10.0, 10.0, (N, DIM))
    NB.neighbors(new_rows[:64], corpus_rows, K)          # warm-up: code objects, the allocator
    t0 = time.perf_counter()
    index, distance = NB.neighbors(new_rows, corpus_rows, K)
    t_knn = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    graph, keys = EM.membership_host(index, distance, N), EM.row_keys(index, distance, 0)
    a, b = EM.curve_ab(0.1)
    run = EM.Place(graph, positions, keys, T, None, NEG, 1.0, 1.0, a, b, None)
    t_host_steps = (time.perf_counter() - t0) * 1e3
    on = sum(int(EM.active(run.rate, t).sum()) for t in range(T))
    print(f"M {m} new rows, N {N}: neighbors(k = {K}) {t_knn:.1f} ms (wall), membership / keys / start {t_host_steps:.1f} ms (host, wall); "
          f"{run.nnz} scheduled entries, {on} active over {T} epochs, {on * (1 + NEG) / 1e6:.2f} M terms")
    dev = torch.device("cuda")
    indptr, indices = torch.from_numpy(run.indptr).to(dev), torch.from_numpy(run.indices).to(dev)
    rate, key = torch.from_numpy(run.rate.view(np.int32)).to(dev), torch.from_numpy(run.key.view(np.int64)).to(dev)
    corpus, y_in = torch.from_numpy(run.y).to(dev), torch.from_numpy(run.y0).to(dev)
    ping, pong = torch.empty_like(y_in), torch.empty_like(y_in)

    def launch(src, dst, t_from, t_to):
        _lib.check(lib.wseg_embed_place_f64(indptr.data_ptr(), indices.data_ptr(), rate.data_ptr(), key.data_ptr(), m, run.nnz, corpus.data_ptr(), N, DIM,
                                            src.data_ptr(), dst.data_ptr(), t_from, t_to, T, 1.0, a, b, 1.0, NEG, _lib.stream_ptr()))

    def timed(work):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = work()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop), out

    def one_launch():
        launch(y_in, ping, 0, T)
        return ping

    def per_epoch():
        src, dst = y_in, pong
        for t in range(T):
            launch(src, dst, t, t + 1)
            src, dst = dst, (ping if dst is pong else pong)
        return src

    def public_call():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = EM.place(graph, positions, keys, T, n_neg=NEG, a=a, b=b)
        return (time.perf_counter() - t0) * 1e3, got

    timed(one_launch), timed(per_epoch), public_call()   # warm-up
    t_one, t_each, t_wall = [], [], []
    for _ in range(REPS):
        ms, out = timed(one_launch)
        t_one.append(ms)
        single = out.cpu().numpy()
        ms, out = timed(per_epoch)
        t_each.append(ms)
        same = np.array_equal(single.view(np.uint64), out.cpu().numpy().view(np.uint64))
        ms, got = public_call()
        t_wall.append(ms)
        assert np.array_equal(got.view(np.uint64), single.view(np.uint64))
    print(f"    wseg_embed_place_f64, one launch for {T} epochs (HIP events)   median {med(t_one):9.2f}   [{fmt(t_one)}]")
    print(f"    the same epochs as {T} launches (t, t + 1) (HIP events)        median {med(t_each):9.2f}   [{fmt(t_each)}]   "
          f"{med(t_each) / med(t_one):.1f}x the one launch; {'the same bits' if same else 'OTHER bits'}")
    print(f"    embed.place() from numpy (wall)                              median {med(t_wall):9.2f}   [{fmt(t_wall)}]")
    t0 = time.perf_counter()
    want = EM.place_epochs_host(run)
    t_host = (time.perf_counter() - t0) * 1e3
    print(f"    place_host (host, numpy, wall; one run)                      {t_host:9.1f}   host / one launch: {t_host / med(t_one):.0f}x; "
          f"largest difference from the device {np.abs(want - single).max():.3g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1000, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_ab.txt"))
    ap.add_argument("--step", type=int, default=None, help="(the child of one size)")
    args = ap.parse_args()
    if args.step is not None:
        step(args.step)
        return 0
    lines = [f"placing M new rows on a frozen map of N = {N}: D = {D} rows around 20 centres, k = {K}, T = {T} epochs, dim {DIM}, n_neg {NEG}, "
             f"a, b = curve_ab(0.1) (one MI355X; warm-up, then {REPS} repetitions; times in ms)"]
    status = 0
    for m in args.sizes:
        print(f"M {m} ...", flush=True)
        done = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", str(m)],
                              stdout=subprocess.PIPE, text=True)
        lines += done.stdout.splitlines()
        if done.returncode != 0:                         # a fault, an abort, a time limit: nothing more is started
            lines.append(f"M {m}: the step ended with status {done.returncode}; nothing was started after it")
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
