"""SHA-256 digests of a fixed list of seeded GEMMs through wseg_debug_gemm / wseg_debug_gemm_resid_ln in every 16-bit, split and mixed
mode (the cases of tests/gemm_handover_cases.py, all served by the 256x256 ping-pong kernel): run it on two builds of the library on
one GPU box and compare the lines — a schedule change that keeps the summation order leaves every digest where it was.
    python tools/gemm_digest.py [--record tests/gemm_handover_digests.json]
(WSEG_LIB selects a variant build.)  --record writes the digests the test file compares against."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from whisperseg_amd import _lib
from gemm_handover_cases import CASES, digest, reaches_pingpong, run_case

ap = argparse.ArgumentParser()
ap.add_argument("--record", default="")
a = ap.parse_args()
lib = _lib.load(require_device=True)
ws = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
n_cu = torch.cuda.get_device_properties(0).multi_processor_count
digests, ok = {}, True
for case in CASES:
    pp, S = reaches_pingpong(case, n_cu)
    first, second, errs, bounds = run_case(lib, case, ws)
    stable = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(first, second))
    within = all(e <= b for e, b in zip(errs, bounds))
    digests[case[0]] = digest(first)
    ok = ok and pp and stable and within
    print(f"{case[0]:22s} M={case[3]:6d} N={case[4]:5d} K={case[5]:5d} epi={case[6]} pingpong={int(pp)} S={S:2d} stable={int(stable)} "
          f"err/scale={' '.join('%.2e' % e for e in errs)} (bound {' '.join('%.0e' % b for b in bounds)})  sha256 {digests[case[0]]}", flush=True)
if a.record:
    if not ok:
        sys.exit("not recorded: a case missed the kernel, differed between two runs or left its bound")
    with open(a.record, "w") as f:
        json.dump({"device_cus": n_cu, "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
sys.exit(0 if ok else 1)
