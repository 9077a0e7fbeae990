"""The 256x256 ping-pong GEMM's hand-over schedule leaves every output bit where it was: the cases of tests/gemm_handover_cases.py
(every stretch of the peeled K loop, both forms of the barrier that closes a K tile, the stream across an epilogue, ragged rows,
uneven split-K shares, odd and even (hi, MX) pair counts; five modes, three epilogues) against the exact-mode GEMM of the same
library within the bounds of tests/test_gemm_gpu.py, twice for bit-stability, and against SHA-256 digests of the outputs recorded
from the build BEFORE the hand-over was touched (tests/gemm_handover_digests.json, written by tools/gemm_digest.py --record)."""
import json
import os

import pytest
import torch

from gemm_handover_cases import CASES, digest, reaches_pingpong, run_case

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_handover_digests.json")) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def workspace():
    return torch.empty(256 << 20, dtype=torch.uint8, device="cuda")


def test_every_case_has_a_recorded_digest():
    assert sorted(RECORDED["digests"]) == sorted(c[0] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_handover_case(gpu_lib, workspace, case):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    pp, S = reaches_pingpong(case, n_cu)
    assert pp, "the shape does not reach gemm_h16_pp_kernel on %d CUs" % n_cu
    if case[2] == "resid_ln":      # uneven shares
        k_tiles = case[5] * (1 if case[1] in ("bf16", "f16") else 2) // 64
        units = k_tiles // 2 if case[1] == "f16m6" else k_tiles
        assert S >= 2 and units % S != 0
    first, second, errs, bounds = run_case(gpu_lib, case, workspace)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    print(case[0], "error / scale against the exact mode:", errs, "bounds:", bounds)
    for e, b in zip(errs, bounds):
        assert e <= b, (errs, bounds)
    assert digest(first) == RECORDED["digests"][case[0]]
