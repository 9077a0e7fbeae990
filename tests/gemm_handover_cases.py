"""Cases of tests/test_gemm_handover_gpu.py and tools/gemm_digest.py: seeded GEMMs that plan_h16 sends to the 256x256 ping-pong kernel
(gemm_h16_pp_kernel), chosen to walk every stretch of its peeled K loop and both forms of the barrier that closes a K tile.

A case is (name, mode, kind, M, N, K, epi): kind "gemm" goes through wseg_debug_gemm (epi 0 bias, 1 bias + GELU, 2 bias + fp32 residual),
kind "resid_ln" through wseg_debug_gemm_resid_ln (the split-K copies of the kernel + the fused reduction).  K is the LOGICAL K: the
split / mixed modes see rows of 2K 16-bit words, i.e. K / 32 K tiles, the plain 16-bit modes K / 64.

Which family a shape gets is not visible from outside the library; tests/test_gemm_gpu.py knows it by the rule of plan_large_tiles /
pp_splitk_plan written next to its PP_SHAPES, and so does reaches_pingpong() below (the test asserts it for the device's CU count).
K = one K tile (64 words) never reaches the kernel (plan_large_tiles: "one K tile, 128x128 kernel"), so first = final occurs only as
the one (hi, MX) tile pair of f16m6 and inside split-K shares."""
import hashlib

import torch

MODES = ("bf16", "f16", "bf16x3", "f16x3", "f16m6")
TOL = {"bf16": 2e-2, "f16": 3e-3, "bf16x3": 6e-5, "f16x3": 6e-6, "f16m6": 1e-4}      # tests/test_gemm_gpu.py, per mode, x max(1, |ref|)
RESID_LN_X_TOL = {"bf16": 2e-5, "f16": 2e-5, "bf16x3": 2e-5, "f16x3": 2e-5, "f16m6": 1e-4}      # test_gemm_resid_layernorm_step: the fp32 residual stream
RESID_LN_Y_TOL = {"bf16": 2e-2, "f16": 3e-3, "bf16x3": 2e-5, "f16x3": 2e-5, "f16m6": 1e-4}


def words(mode, K):
    return K * (1 if mode in ("bf16", "f16") else 2)


def _cases():
    out = []
    for mi, mode in enumerate(MODES):
        wide = mode not in ("bf16", "f16")
        # 26 x 8 = 208 tiles (one round of a 256-CU chip, the last row tile ragged: 6 500 rows); K tiles per output tile 2..5 =
        # edge-edge, edge-edge-edge, edge-middle-edge-edge, two middle tiles; f16m6: 1, 2, 3 (hi, MX) pairs = first-is-final, edge-edge,
        # edge-middle-edge, an odd and an even number of pairs.  Every mode meets every epilogue.
        tiles = (2, 4, 6) if mode == "f16m6" else (2, 3, 4, 5)
        for i, nkt in enumerate(tiles):
            out.append(("%s_k%d" % (mode, nkt), mode, "gemm", 6500, 2048, nkt * (32 if wide else 64), (i + mi) % 3))
        # 52 x 8 = 416 tiles at 2 K tiles: every workgroup owns one or two output tiles, the K-tile stream runs across an epilogue
        out.append(("%s_two_tiles" % mode, mode, "gemm", 13200, 2048, 64 if wide else 128, (mi + 2) % 3))
        # split-K copies: 40 K tiles in 6 shares (6 / 7 tiles) for the plain modes at 2 048 rows; 50 K tiles (f16m6: 25 pairs) in 12 shares at 500 rows
        out.append(("%s_splitk" % mode, mode, "resid_ln") + ((500, 1280, 1600) if wide else (2048, 1280, 2560)) + (2,))
    return out


CASES = _cases()


def reaches_pingpong(case, n_cu):
    """plan_large_tiles / pp_splitk_plan of csrc/wseg_gemm.hip for the cases above: (family is ping-pong, split-K copies S)."""
    _, mode, kind, M, N, K, epi = case
    split = mode not in ("bf16", "f16")
    kw = words(mode, K)
    mt = (M + 255) // 256
    if kind == "resid_ln":
        nt, nk = mt * (N // 256), kw // 64
        if M < (448 if split else 2048) or N % 256 or nk < 40:
            return False, 0
        S = min(n_cu // nt, 64)
        while S >= 2 and ((nt * S) % 8 or nk // S < 4):
            S -= 1
        return S >= 2 and nt * S >= 96, S
    big = M > 128 and N % 128 == 0 and ((M + 127) // 128) * (N // 128) >= 340
    nt = mt * (N // 256)
    rounds = (nt + n_cu - 1) // n_cu
    ragged = rounds < 4 and nt * 5 < rounds * n_cu * (3 if split else 4)
    need = 160 if (split and epi == 1) else 192
    return big and N % 256 == 0 and nt >= need and not ragged and kw >= 128, 1


_operands, _outer = {}, {}


def operands(M, N, K):
    """fp32 operands of a shape, from a CPU generator (the same values on every box), made once and kept on the device (under 300 MB
    for all cases); shared by all modes."""
    Mp = (M + 255) // 256 * 256
    if (M, N) not in _outer:      # bias, LayerNorm gain and shift, residual
        g = torch.Generator().manual_seed(M * 31 + N * 7)
        vec = [torch.rand(N, generator=g) - 0.5 for _ in range(3)]
        vec[1] += 1.0
        _outer[(M, N)] = tuple(t.cuda() for t in vec + [torch.rand(Mp, N, generator=g) - 0.5])
    if (M, N, K) not in _operands:
        g = torch.Generator().manual_seed(M * 31 + N * 7 + K)
        A = torch.rand(Mp, K, generator=g) * 2 - 1
        A[:, : K // 2] *= 0.02          # blocks of very different magnitude inside a row (the MX block scales matter)
        W = (torch.rand(N, K, generator=g) * 2 - 1) * K ** -0.5
        _operands[(M, N, K)] = (A.cuda(), W.cuda())
    return _operands[(M, N, K)] + _outer[(M, N)]


def run_case(lib, case, ws):
    """Runs the case twice and its fp32 exact-mode twin once.  Returns (out bytes tensors of run 1, of run 2, worst error / scale per
    output against the exact mode, the bounds for them)."""
    from whisperseg_amd import _lib
    from whisperseg_amd.engine import DTYPES, SPLIT_BASE, split_operand, unsplit_m6, unsplit_operand
    _, mode, kind, M, N, K, epi = case
    DT = DTYPES[mode][0]
    split, m6 = mode in SPLIT_BASE, mode == "f16m6"
    A, W, bias, gam, bet, res = operands(M, N, K)
    Mp = A.shape[0]
    st = _lib.stream_ptr()
    if split:
        base = SPLIT_BASE[mode]
        Ao, Wo = split_operand(A, base), split_operand(W, base)
        if m6:
            As, Ws = Ao, Wo
            Ao, Wo = torch.empty_like(As), torch.empty_like(Ws)
            _lib.check(lib.wseg_convert_operand(As.data_ptr(), Ao.data_ptr(), Mp, K, 0, st))
            _lib.check(lib.wseg_convert_operand(Ws.data_ptr(), Wo.data_ptr(), N, K, 1, st))
        Ar, Wr, vr, pd = A, W, (bias, gam, bet), torch.float32
    else:
        pd = DTYPES[mode][1]
        Ao, Wo = A.to(pd), W.to(pd)
        vr = tuple(v.to(pd).float() for v in (bias, gam, bet))
        Ar, Wr = Ao.float(), Wo.float()          # the exact mode multiplies the same (rounded) operands
    vo = tuple(v.to(pd) for v in (bias, gam, bet))

    def as_values(rows, is_mx):
        if not split:
            return rows.float()
        return unsplit_m6(rows) if is_mx else unsplit_operand(rows, SPLIT_BASE[mode])

    if kind == "resid_ln":
        runs = []
        for rep in range(2):
            x = res.clone()
            y = torch.full((Mp, 2 * N), 0x7e00, device="cuda", dtype=torch.int16) if split else torch.full((Mp, N), float("nan"), device="cuda", dtype=pd)
            _lib.check(lib.wseg_debug_gemm_resid_ln(DT, M, N, K, Ao.data_ptr(), Wo.data_ptr(), vo[0].data_ptr(), x.data_ptr(), vo[1].data_ptr(),
                                                    vo[2].data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), st))
            runs.append((x[:M], y[:M]))
        xr, yr = res.clone(), torch.empty(Mp, N, device="cuda")
        _lib.check(lib.wseg_debug_gemm_resid_ln(0, M, N, K, Ar.data_ptr(), Wr.data_ptr(), vr[0].data_ptr(), xr.data_ptr(), vr[1].data_ptr(),
                                                vr[2].data_ptr(), yr.data_ptr(), ws.data_ptr(), ws.numel(), st))
        xr, yr = xr[:M], yr[:M]
        ex = (runs[0][0] - xr).abs().max().item() / max(1.0, xr.abs().max().item())
        ey = (as_values(runs[0][1], m6) - yr).abs().max().item() / max(1.0, yr.abs().max().item())
        return runs[0], runs[1], (ex, ey), (RESID_LN_X_TOL[mode], RESID_LN_Y_TOL[mode])
    od = torch.float32 if epi == 2 else pd
    reso = res.to(od)
    runs = []
    for rep in range(2):
        if split and epi != 2:
            out = torch.full((Mp, 2 * N), -1, device="cuda", dtype=torch.int16)      # 0xffff words: NaN in both 16-bit types
        else:
            out = torch.full((Mp, N), float("nan"), device="cuda", dtype=od)
        _lib.check(lib.wseg_debug_gemm(DT, epi, M, N, K, Ao.data_ptr(), Wo.data_ptr(), vo[0].data_ptr(), reso.data_ptr(), out.data_ptr(),
                                       ws.data_ptr(), ws.numel(), st))
        runs.append(out)
    ref = torch.empty(Mp, N, device="cuda")
    _lib.check(lib.wseg_debug_gemm(0, epi, M, N, K, Ar.data_ptr(), Wr.data_ptr(), vr[0].data_ptr(), reso.float().data_ptr(), ref.data_ptr(),
                                   ws.data_ptr(), ws.numel(), st))
    is_mx = m6 and epi != 2 and bool(lib.wseg_debug_gemm_out_is_mx(DT, M, N, K))
    got = runs[0][:M] if epi == 2 else as_values(runs[0][:M], is_mx)
    assert torch.isfinite(got).all()
    err = (got - ref[:M]).abs().max().item() / max(1.0, ref[:M].abs().max().item())
    return (runs[0][:M],), (runs[1][:M],), (err,), (TOL[mode],)


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy())
    return h.hexdigest()
