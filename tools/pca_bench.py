#!/usr/bin/env python3
"""What the principal components cost on one MI355X (whisperseg_amd.pca: wseg_pca_moments_f64 and wseg_pca_project_f64, float64 on the
matrix cores), against torch's float64 products on the same GPU and the definition on the host.  Not on the product path.

    python tools/pca_bench.py [--shapes 100000x2560 1000000x2560 100000x80 1000000x80] [--out profiles/pca_ab.txt]

Rows: N x D normal float32 with a per-column offset, drawn on the device; r = 32.  Reported per shape:
  * wseg_pca_moments_f64 — HIP events around the call (the moments kernel and, with row splits, the finish kernel), resident rows:
    ms, and the multiply-add rate in two conventions: N D^2 (the full matrix a caller gets) and the tiles actually computed (the
    upper triangle of 64-column blocks), beside the data sheet's fp64 matrix figure (78.6 TFLOPS = 39.3 T multiply-adds a second);
  * torch on the same rows: X.double().T @ X.double() — the float64 copy of the rows that the kernel avoids is part of the line;
  * wseg_pca_project_f64 against (X.double() - mean) @ V, the same way;
  * at N <= 100 000 only, pca.moments_host on the host (numpy, wall; one run) and the largest difference relative to |S|.
One warm-up, then five repetitions, the two sides alternating; all five are printed, the median is the figure.
A last step times numpy.linalg.eigh of a D x D covariance at D = 2560 and 5120 on the host (wall; one run each): the part of pca()
that stays on the host.

Every shape is a CHILD process under its own time limit (timeout -k 10), one after the other; after a child that did not end with
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

R, REPS = 32, 5
HOST_MAX_N = 100000
STEP_SECONDS = 170
PEAK_TMAC = 39.3                        # data sheet: 78.6 TFLOPS fp64 on the matrix cores (and as much on the vector units)


def step(n, d):
    """The measurements of one shape -> printed lines (this is the child)."""
    import torch
    from whisperseg_amd import _lib, pca as PC
    lib = _lib.load(require_device=True)
    med = statistics.median
    fmt = lambda v: " ".join(f"{t:.2f}" for t in v)
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1000 * d + n % 1000)
    x = torch.randn((n, d), generator=gen, device=dev, dtype=torch.float32)
    x += torch.linspace(-3.0, 3.0, d, device=dev)
    r = min(R, d)
    s = torch.empty(d, dtype=torch.float64, device=dev)
    gram = torch.empty((d, d), dtype=torch.float64, device=dev)
    nbytes = PC.scratch_bytes(n, d)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    basis = torch.linalg.qr(torch.randn((d, r), generator=gen, device=dev, dtype=torch.float64))[0].contiguous()
    mean = x.double().mean(dim=0) if n * d <= 1 << 28 else torch.linspace(-3.0, 3.0, d, device=dev, dtype=torch.float64)
    out = torch.empty((n, r), dtype=torch.float64, device=dev)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        result = fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop), result

    def moments():
        _lib.check(lib.wseg_pca_moments_f64(x.data_ptr(), n, d, s.data_ptr(), gram.data_ptr(), scratch.data_ptr(), nbytes, _lib.stream_ptr()))

    def project():
        _lib.check(lib.wseg_pca_project_f64(x.data_ptr(), n, d, mean.data_ptr(), basis.data_ptr(), r, out.data_ptr(), _lib.stream_ptr()))

    def torch_moments():
        x64 = x.double()
        return x64.T @ x64

    def torch_project():
        return (x.double() - mean) @ basis

    kernel_ms = {}
    nb = -(-d // 64)
    tiles = nb * (nb + 1) // 2
    splits = -(-n // (-(-(-(-n // min(-(-1024 // tiles), -(-n // 256)))) // 32) * 32))
    print(f"N {n}, D {d}: {tiles} tiles of 64 x 64 columns, {splits} row splits, scratch {nbytes / 2 ** 20:.1f} MiB")
    for label, ours, theirs, macs, issued in (
            ("moments", moments, torch_moments, n * d * d, n * tiles * 64 * 64),
            ("project", project, torch_project, n * d * r, n * d * 16 * -(-r // 16))):
        timed(ours), timed(theirs)                       # warm-up: code objects, the allocator, the BLAS plan
        t_ours, t_theirs = [], []
        for _ in range(REPS):
            t_ours.append(timed(ours)[0])
            ms, ref = timed(theirs)
            t_theirs.append(ms)
        got = gram if label == "moments" else out
        kernel_ms[label] = med(t_ours)
        scale = float(ref.abs().max())
        worst = float((got - ref).abs().max()) / scale
        del ref
        name = "wseg_pca_moments_f64" if label == "moments" else f"wseg_pca_project_f64 (r = {r})"
        other = "X.double().T @ X.double()" if label == "moments" else "(X.double() - mean) @ V"
        print(f"  {name} (HIP events)  median {med(t_ours):10.2f}   [{fmt(t_ours)}]   {macs / med(t_ours) / 1e9:.2f} T multiply-adds/s "
              f"({macs / med(t_ours) / 1e9 / PEAK_TMAC * 100:.0f} % of the data sheet's {PEAK_TMAC}); computed tiles: {issued / med(t_ours) / 1e9:.2f} T/s")
        print(f"  torch {other} (HIP events)  median {med(t_theirs):10.2f}   [{fmt(t_theirs)}]   torch / kernel: {med(t_theirs) / med(t_ours):.2f}x; "
              f"largest difference {worst:.2e} of the largest entry")
    if n <= HOST_MAX_N:
        rows = x.cpu().numpy()
        t0 = time.perf_counter()
        _, want = PC.moments_host(rows)
        t_host = (time.perf_counter() - t0) * 1e3
        worst = float(np.abs(gram.cpu().numpy() - want).max() / np.abs(want).max())
        print(f"  pca.moments_host (host, numpy, wall; one run)  {t_host:10.1f}   host / kernel: {t_host / kernel_ms['moments']:.0f}x; "
              f"largest difference {worst:.2e} of the largest entry")


def eigh_step():
    """numpy.linalg.eigh of a covariance-like D x D matrix on the host."""
    rng = np.random.default_rng(5)
    for d in (2560, 5120):
        a = rng.normal(0.0, 1.0, (d + 64, d))
        cov = a.T @ a / (d + 63)
        t0 = time.perf_counter()
        values, _ = np.linalg.eigh(cov)
        print(f"numpy.linalg.eigh at D = {d} (host, wall; one run)  {(time.perf_counter() - t0) * 1e3:10.1f} ms   (largest eigenvalue {values[-1]:.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["100000x2560", "1000000x2560", "100000x80", "1000000x80"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_ab.txt"))
    ap.add_argument("--step", default=None, help="(the child of one shape, NxD, or `eigh`)")
    args = ap.parse_args()
    if args.step == "eigh":
        eigh_step()
        return 0
    if args.step is not None:
        step(*(int(v) for v in args.step.split("x")))
        return 0
    lines = [f"principal components: wseg_pca_moments_f64 / wseg_pca_project_f64 (r = {R}) against torch float64 on the same GPU (one MI355X; warm-up, "
             f"then {REPS} repetitions, alternating; times in ms)"]
    status = 0
    for shape in args.shapes + ["eigh"]:
        print(f"{shape} ...", flush=True)
        done = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", shape],
                              stdout=subprocess.PIPE, text=True)
        lines += done.stdout.splitlines()
        if done.returncode != 0:                         # a fault, an abort, a time limit: nothing more is started
            lines.append(f"{shape}: the step ended with status {done.returncode}; nothing was started after it")
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
