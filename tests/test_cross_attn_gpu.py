"""Cross-attention of the decode step and the K / V rows it reads, alone against float64: the writer (launch_gemm with the K / V
epilogue, st_bfp_row) through wseg_debug_cross_kv and the four reader kernels (dec_cross_attn_k24_kernel, _bfp_, _pk_ and the general
dec_cross_attn_kernel; beam tiles 1 / 2 / 4 / 8; 512-key and long-key forms) through wseg_debug_cross_attention, on the cases of
cross_attn_cases.py and the row definition of oracle/cross_kv.py.

Writer.  Exact inputs through an identity weight: the planes equal the definition's bit for bit, and the decoded rows lie within
2^(ceil(log2 rowmax) - MANT - 1) of the values (a whole unit where |v| = 2^k = rowmax, 0 in zero rows) — that bound is taken from the row
maximum here, not through the restated rounding.  Random inputs: the same plus the GEMM bound of test_gemm_gpu.py.

Readers.  Two float64 references: (a) softmax attention over the rows AS STORED (decoded by oracle.cross_kv), which isolates the
reader, and (b) over the rows as given, writer + reader.  The bound is cross_attn_cases.derived_bound — fp32 scores, their error carried
through the softmax, the normaliser, the P V sum, the output format's rounding; for (b) the stored rows' error through scores and sum —
plus the one term that cannot be derived from the project, the error of the device expf: EXP_REL * sum_t p_t |v_te - o_e|.

EXP_REL: profiles/cross_attn_error.txt holds, per (mode, beams, t_len) and family (one line of five cells), the largest error against
(a) over both query forms, the derived bound where it occurred, the largest error / derived bound and the largest
(error - derived bound) / sum_t p_t |v_te - o_e| ("excess").
Allowed is 3 x the largest excess of a mode — the factor of the late-step logits test, for other seeds and accumulation orders.  The
derived part is a worst-case bound and covered every measured error: the largest error / derived bound is 0.02 (f32), 0.45 (bf16x3),
0.65 (f16x3), 0.92 (f16m6), 0.99 (bf16) and 0.97 (f16) — the last three are the output's own rounding, which a correctly rounded
store reaches —, the excess is negative in every line, so the allowance is 0 in every mode: the device expf is inside the derived part.
WSEG_CROSS_ATTN_PROFILE=<file> appends these lines.

bf16 / f16 rows: the output term is half a unit in the last place, 2^-9 / 2^-12 of the power of two above |o|.  Read as 2^-9 / 2^-12 of
|o| itself the term cannot be met by any store that rounds to nearest (that reaches 2^-8 / 2^-11 of |o| just above a power of two):
measured 1.90 x such a bound in both modes, with the error equal to the rounding of the float64 result."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cross_attn_cases as X
from oracle import cross_kv as CK

pytestmark = pytest.mark.gpu

# 3 x the largest excess of profiles/cross_attn_error.txt per mode (see above): none is positive
EXP_REL = {"f32": 0.0, "bf16": 0.0, "f16": 0.0, "bf16x3": 0.0, "f16x3": 0.0, "f16m6": 0.0}
GUARD, FILL = 256, 0x5A
WS_BYTES = 64 << 20
PERM = (3, 0, 4, 1, 2)      # window w of the permuted buffers lives in slot PERM[w]


def enc_chunk_rows(t_len):
    """Rows the encode pass plans its K / V projection for: a whole encoder chunk (enc_chunk, wseg_model.hip)."""
    return (256 if t_len <= 512 else max(16, (256 * 512 // t_len) & ~15)) * t_len


class Dev:
    """Device bytes between guard words."""

    def __init__(self, nbytes, body=FILL, host=None):
        self.n = nbytes
        buf = np.full(GUARD + nbytes + (-nbytes) % 256 + GUARD, FILL, np.uint8)
        buf[GUARD:GUARD + nbytes] = body if host is None else np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        self.dev = torch.from_numpy(buf).cuda()
        self.ptr = self.dev.data_ptr() + GUARD
        assert self.ptr % 256 == 0

    def bytes(self):
        raw = self.dev.cpu().numpy()
        assert (raw[:GUARD] == FILL).all() and (raw[GUARD + self.n:] == FILL).all(), "a guard byte changed"
        return raw[GUARD:GUARD + self.n].copy()


def torch_type(mode):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}.get(mode, torch.float32)


def operand(lib, x, mode, weight=False):
    """float64 / float32 [M][K] -> the mode's GEMM operand rows on the device, M padded to whole 256-row tiles with zeros."""
    from whisperseg_amd import _lib
    from whisperseg_amd.engine import SPLIT_BASE, split_operand
    x = (x if torch.is_tensor(x) else torch.from_numpy(np.array(x))).float()
    m, k = x.shape
    xp = torch.zeros((m + 255) // 256 * 256, k)
    xp[:m] = x
    xp = xp.cuda()
    if mode not in X.SPLIT_MODES:
        return xp.to(torch_type(mode)).contiguous()
    op = split_operand(xp, SPLIT_BASE[mode])
    if mode == "f16m6":
        m6 = torch.empty_like(op)
        _lib.check(lib.wseg_convert_operand(op.data_ptr(), m6.data_ptr(), op.shape[0], k, 1 if weight else 0, _lib.stream_ptr()))
        torch.cuda.synchronize()
        return m6
    return op


_WS = {}


def workspace():
    if "ws" not in _WS:
        _WS["ws"] = torch.empty(WS_BYTES, dtype=torch.uint8, device="cuda")
    return _WS["ws"]


def identity_weight():
    return np.concatenate([np.eye(X.D), np.eye(X.D)])      # k | v = the input twice


def kv_bytes(lib, mode, nb, n_slots, t_len):
    fmt = C.c_int32(-1)
    n = lib.wseg_debug_cross_kv_bytes(X.DTYPE_ID[mode], nb, n_slots, X.HEADS, t_len, C.byref(fmt))
    assert n > 0 and fmt.value == X.kv_format(mode, nb)
    return n, fmt.value


def project(lib, mode, nb, a_op, w_op, bias, slot_map, n_windows, n_slots, t_len, plan_m, k, v):
    """One call of the writer tap into the guarded buffers k and v."""
    from whisperseg_amd import _lib
    sm = torch.tensor(slot_map, dtype=torch.int32, device="cuda") if slot_map is not None else None
    ws = workspace()
    torch.cuda.synchronize()
    rc = lib.wseg_debug_cross_kv(X.DTYPE_ID[mode], nb, n_windows, n_slots, t_len, X.HEADS, plan_m, a_op.data_ptr(), a_op.numel() * a_op.element_size(),
                                 w_op.data_ptr(), bias.data_ptr() if bias is not None else None, sm.data_ptr() if sm is not None else None,
                                 k.ptr, v.ptr, k.n, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    assert rc == 0, lib.wseg_last_error().decode()
    torch.cuda.synchronize()


def write_kv(lib, mode, nb, xk, xv, slot_map, n_slots, plan_m=None):
    """K from xk and V from xv ([n_windows][t_len][HEADS][64], exact in the operand) through the identity weight: two launches, the
    unwanted half of each goes to a spare buffer.  Returns (k, v, fmt)."""
    n_windows, t_len = xk.shape[:2]
    n, fmt = kv_bytes(lib, mode, nb, n_slots, t_len)
    k, v, spare = Dev(n), Dev(n), Dev(n)
    w_op = operand(lib, identity_weight(), mode, weight=True)
    plan_m = plan_m or enc_chunk_rows(t_len)
    project(lib, mode, nb, operand(lib, xk.reshape(-1, X.D), mode), w_op, None, slot_map, n_windows, n_slots, t_len, plan_m, k, spare)
    project(lib, mode, nb, operand(lib, xv.reshape(-1, X.D), mode), w_op, None, slot_map, n_windows, n_slots, t_len, plan_m, spare, v)
    return k, v, fmt


def stored_rows(raw, mode, fmt, n_slots, t_len):
    """The buffer's bytes -> float64 [n_slots][HEADS][t_len][64]."""
    if fmt:
        return CK.decode(raw, fmt, n_slots, X.HEADS, t_len)
    t = torch.from_numpy(raw).view(torch_type(mode))
    return t.double().numpy().reshape(n_slots, X.HEADS, t_len, 64)


def to_slots(x, slot_map, n_slots):
    """[n_windows][t_len][HEADS][64] -> [n_slots][HEADS][t_len][64] (NaN in the slots no window goes to)."""
    out = np.full((n_slots, X.HEADS, x.shape[1], 64), np.nan)
    for i, s in enumerate(slot_map if slot_map is not None else range(x.shape[0])):
        out[s] = x[i].transpose(1, 0, 2)
    return out


def plain_bytes(rows, mode):
    """float64 rows -> the bytes of plain K / V rows of the mode."""
    return torch.from_numpy(np.ascontiguousarray(rows)).to(torch_type(mode)).contiguous().view(torch.uint8).numpy().reshape(-1)


def check_slots(raw, want_rows, mode, fmt, t_len, what):
    """The touched slots hold exactly the definition's bytes of want_rows [n_slots][HEADS][t_len][64]; every other slot keeps the fill."""
    n_slots = want_rows.shape[0]
    per = raw.size // n_slots
    assert per * n_slots == raw.size
    for s in range(n_slots):
        got = raw[s * per:(s + 1) * per]
        if np.isnan(want_rows[s]).any():
            assert (got == FILL).all(), (what, "untouched slot", s)
            continue
        if fmt:
            q, e = CK.encode(want_rows[s:s + 1], fmt)
            want = CK.pack(q, e, fmt)
            if not np.array_equal(got, want):
                gq, gs = CK.unpack(got, fmt, 1, X.HEADS, t_len)
                bad = np.argwhere((gq != q) | (gs != CK.stored_scale(e, fmt))[..., None])
                raise AssertionError((what, "slot", s, "first differences (slot, head, position, element)", bad[:5].tolist(),
                                      gq[tuple(bad[0])], q[tuple(bad[0])]))
        else:
            assert np.array_equal(got, plain_bytes(want_rows[s], mode)), (what, "slot", s)


def independent_row_bound(v, fmt):
    """2^(ceil(log2 rowmax) - MANT - 1); a whole unit at |v| = 2^k = rowmax; 0 in zero rows.  Spelled out with log2: no code shared with
    the definition under test."""
    am = np.abs(v).max(-1, keepdims=True)
    lg = np.log2(np.where(am > 0, am, 1.0))
    half = np.where(am > 0, np.exp2(np.ceil(lg) - CK.MANT[fmt] - 1), 0.0)
    return np.where((np.abs(v) == am) & (lg == np.round(lg)), 2 * half, half)


# ---- writer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_len", X.T_LENS)
@pytest.mark.parametrize("mode", X.SPLIT_MODES)
def test_writer_stores_the_definitions_bits(gpu_lib, mode, t_len):
    """Planted rows, exact through the identity weight, 3 windows into slots (4, 0, 2) of 5 (and 2 windows where a wave tile spans two):
    planes and scales bit for bit, the independent bound on the decoded rows, untouched slots and guards — on the encode pass's plan
    (large tiles, 8 columns per lane) and on a plan for the rows launched (weight-stream family, the 4-column writer of the reduction)."""
    cases = [(3, (4, 0, 2))] + ([(2, (3, 1))] if t_len in (128, 251) else [])
    nb = 4      # (the format follows the mode up to 4 beams; more beams: test_writer_plain_rows)
    for n_windows, slot_map in cases:
        fmt = X.kv_format(mode, nb)
        x, places = X.writer_input(mode, fmt, t_len, n_windows)
        want = to_slots(x, slot_map, X.SLOTS)
        for plan_m in (enc_chunk_rows(t_len), n_windows * t_len):
            k, v, got_fmt = write_kv(gpu_lib, mode, nb, x, x, slot_map, X.SLOTS, plan_m)
            assert got_fmt == fmt in (2, 3)
            for name, buf in (("k", k), ("v", v)):
                raw = buf.bytes()
                check_slots(raw, want, mode, fmt, t_len, (name, n_windows, plan_m))
                rows = stored_rows(raw, mode, fmt, X.SLOTS, t_len)
                for s in slot_map:
                    err = np.abs(rows[s] - want[s])
                    assert (err <= independent_row_bound(want[s], fmt)).all(), (name, s, plan_m)
                for kind, (w, t, h) in places.items():      # the planted rows, by name
                    got, val = rows[slot_map[w], h, t], x[w, t, h]
                    if kind == "zero":
                        assert not got.any()
                    elif kind in ("pow2_max", "neg_pow2_max"):
                        i = np.abs(val).argmax()
                        assert got[i] == val[i] * (1 - 2.0 ** -CK.MANT[fmt]), (kind, got[i], val[i])      # +-QMAX units: one unit short
                    elif kind == "clamp_below":
                        assert np.array_equal(got, val)


@pytest.mark.parametrize("mode", X.SPLIT_MODES)
def test_writer_exponent_clamp_in_every_split_mode(gpu_lib, mode):
    """A row maximum of 2^-90 (format 3) / 2^-100 (format 2) stops at the exponent clamp.  The IEEE-half operands cannot hold such a
    value; the fp32 bias can: zero input rows, the planted row as bias — every stored row is that row's definition."""
    t_len, nb = 128, 4
    n, fmt = kv_bytes(gpu_lib, mode, nb, 1, t_len)
    rng = np.random.default_rng(5)
    row = np.stack([X.planted_row("clamp_below", fmt, "bf16x3", rng) for _ in range(2 * X.HEADS)])      # [k heads | v heads][64]
    bias = torch.from_numpy(row.reshape(-1)).float().cuda()
    assert np.array_equal(bias.double().cpu().numpy(), row.reshape(-1))
    a = operand(gpu_lib, np.zeros((t_len, X.D)), mode)
    for plan_m in (enc_chunk_rows(t_len), t_len):
        k, v = Dev(n), Dev(n)
        project(gpu_lib, mode, nb, a, operand(gpu_lib, identity_weight(), mode, weight=True), bias, None, 1, 1, t_len, plan_m, k, v)
        for i, buf in enumerate((k, v)):
            want = np.broadcast_to(row[i * X.HEADS:(i + 1) * X.HEADS][None, :, None, :], (1, X.HEADS, t_len, 64))
            check_slots(buf.bytes(), want, mode, fmt, t_len, ("kv"[i], plan_m))
            q, s = CK.unpack(buf.bytes(), fmt, 1, X.HEADS, t_len)
            assert (s == np.float32(2.0 ** (-CK.CLAMP[fmt] - (8 if fmt == 3 else 0)))).all() and q.max() == 1 << 10


@pytest.mark.parametrize("mode,nb", [(m, 4) for m in ("f32", "bf16", "f16")] + [(m, nb) for m in X.SPLIT_MODES for nb in (5, 8)])
def test_writer_plain_rows(gpu_lib, mode, nb):
    """Plain rows (the 16-bit and exact modes; the split modes at more than 4 beams: fp32 rows): exact inputs come back exactly, in
    the mapped slots, at every length."""
    for t_len in X.T_LENS:
        x, _ = X.writer_input(mode, 0, t_len, 3)
        k, v, fmt = write_kv(gpu_lib, mode, nb, x, x, (4, 0, 2), X.SLOTS)
        assert fmt == 0
        want = to_slots(x, (4, 0, 2), X.SLOTS)
        check_slots(k.bytes(), want, mode, 0, t_len, ("k", t_len))
        check_slots(v.bytes(), want, mode, 0, t_len, ("v", t_len))


GEMM_TOL = {"bf16x3": 6e-5, "f16x3": 6e-6, "f16m6": 1e-4,      # test_split_precision_gemm_matches_fp64 / test_mixed_precision_gemm_matches_fp64
            "bf16": 2e-2, "f16": 3e-3, "f32": 2e-5}            # test_gemm_matches_torch


@pytest.mark.parametrize("mode,nb", [(m, 4) for m in X.MODES] + [(m, 8) for m in X.SPLIT_MODES])
def test_writer_random_inputs_and_weight(gpu_lib, mode, nb):
    """Uniform random fp32 rows, a random weight and bias (K = 128) against the float64 product of the same operands: plain rows
    within the GEMM tolerance of test_gemm_gpu.py; packed rows within that plus the row bound (taken at the row maximum + the tolerance:
    the stored row is the definition of the GEMM's output, not of the reference).  And a window's bytes do not depend on how many
    windows are projected with it on one plan (the claim of the encode pass)."""
    for t_len in (128, 251, 500):
        g = torch.Generator().manual_seed(17 + t_len)
        A = torch.rand(5 * t_len, X.D, generator=g) * 2 - 1
        W = (torch.rand(2 * X.D, X.D, generator=g) * 2 - 1) * X.D ** -0.5
        bias = torch.rand(2 * X.D, generator=g) - 0.5
        td = torch_type(mode)
        if mode in ("bf16", "f16"):
            A, W, bias = A.to(td).float(), W.to(td).float(), bias.to(td).float()
        ref = (A.double() @ W.double().T + bias.double()).numpy().reshape(5, t_len, 2, X.HEADS, 64)      # [w][t][k | v][h][64]
        tol = GEMM_TOL[mode] * max(1.0, np.abs(ref).max())
        n, fmt = kv_bytes(gpu_lib, mode, nb, X.SLOTS, t_len)
        plan_m = enc_chunk_rows(t_len)
        w_op, b_dev = operand(gpu_lib, W, mode, weight=True), bias.to(td).cuda()
        k, v = Dev(n), Dev(n)
        project(gpu_lib, mode, nb, operand(gpu_lib, A, mode), w_op, b_dev, PERM, 5, X.SLOTS, t_len, plan_m, k, v)
        raws = (k.bytes(), v.bytes())
        for sec, raw in enumerate(raws):
            rows = stored_rows(raw, mode, fmt, X.SLOTS, t_len)
            want = to_slots(ref[:, :, sec], PERM, X.SLOTS)
            err = np.abs(rows - want)
            bound = tol + (independent_row_bound(np.abs(want) + tol, fmt) if fmt else 0.0)
            print(f"{mode} nb {nb} t_len {t_len} {'kv'[sec]}: max err {err.max():.3e}, largest err / bound {(err / bound).max():.3f}")
            assert (err <= bound).all(), (t_len, sec, (err / bound).max())
        # window 2 alone, same plan, same slot: the same bytes
        k1, v1 = Dev(n), Dev(n)
        project(gpu_lib, mode, nb, operand(gpu_lib, A[2 * t_len:3 * t_len], mode), w_op, b_dev, (PERM[2],), 1, X.SLOTS, t_len, plan_m, k1, v1)
        per = n // X.SLOTS
        for full, one in zip(raws, (k1.bytes(), v1.bytes())):
            s = PERM[2]
            assert np.array_equal(full[s * per:(s + 1) * per], one[s * per:(s + 1) * per]), (t_len, "a window's rows follow the row count")
            assert (np.delete(one.reshape(X.SLOTS, per), s, 0) == FILL).all()


# ---- readers -----------------------------------------------------------------------------------------------------------------
_KV = {}


def reader_buffers(lib, mode, nb, t_len, permuted=False):
    """The cases' K / V written by the writer tap, once per (mode, format, t_len): (k, v, fmt, stored K, stored V as float64)."""
    fmt = X.kv_format(mode, nb)
    key = (mode, fmt, t_len, permuted)
    if key not in _KV:
        K, V = X.reader_kv(mode, t_len)
        xk, xv = K.transpose(0, 2, 1, 3), V.transpose(0, 2, 1, 3)      # [w][t][h][64]
        k, v, got = write_kv(lib, mode, nb, xk, xv, PERM if permuted else None, X.SLOTS)
        assert got == fmt
        rk, rv = k.bytes(), v.bytes()
        _KV[key] = (k, v, fmt, stored_rows(rk, mode, fmt, X.SLOTS, t_len), stored_rows(rv, mode, fmt, X.SLOTS, t_len))
    return _KV[key]


def out_rows(raw, mode, fmt, R):
    """The output's bytes -> float64 [R][D]."""
    from whisperseg_amd.engine import SPLIT_BASE, unsplit_m6, unsplit_operand
    if mode not in X.SPLIT_MODES:
        return torch.from_numpy(raw).view(torch_type(mode)).double().numpy().reshape(R, X.D)
    t = torch.from_numpy(raw).view(torch.int16).view(R, 2 * X.D)
    if mode == "f16m6" and fmt != 0:
        return unsplit_m6(t).double().numpy()
    return unsplit_operand(t, SPLIT_BASE[mode]).double().numpy()


def attend(lib, mode, nb, t_len, k, v, q=None, planes=None, bias=None, done=None, kv_slot=None, expect=0):
    """One call of the reader tap.  Returns the output's bytes [R][row bytes] (0xff where nothing was written)."""
    from whisperseg_amd import _lib
    R = X.SLOTS * nb
    es = 2 if mode in ("bf16", "f16") else 4
    out = Dev(R * X.D * es, body=0xFF)
    td = torch_type(mode)
    keep = []
    if q is not None:
        qd = torch.from_numpy(np.array(q)).to(td).cuda()
        assert np.array_equal(qd.double().cpu().numpy(), q)      # the finished rows are exact in the query's type
        args = (qd.data_ptr(), None, 0, 0, None)
        keep.append(qd)
    else:
        pd, bd = torch.from_numpy(planes).cuda(), torch.from_numpy(bias).to(td).cuda()
        assert np.array_equal(bd.double().cpu().numpy(), bias)
        args = (None, pd.data_ptr(), planes.shape[0], planes.shape[1], bd.data_ptr())
        keep += [pd, bd]
    dn = torch.tensor(done if done is not None else [0] * X.SLOTS, dtype=torch.int32, device="cuda")
    ks = torch.tensor(kv_slot, dtype=torch.int32, device="cuda") if kv_slot is not None else None
    torch.cuda.synchronize()
    rc = lib.wseg_debug_cross_attention(X.DTYPE_ID[mode], nb, X.SLOTS, X.SLOTS, t_len, X.HEADS, *args, X.SCALE, dn.data_ptr(),
                                        ks.data_ptr() if ks is not None else None, k.ptr, v.ptr, k.n, out.ptr, out.n, _lib.stream_ptr())
    assert rc == expect, lib.wseg_last_error().decode()
    torch.cuda.synchronize()
    return out.bytes().reshape(R, X.D * es)


def profile_line(mode, nb, t_len, err, bound, spread):
    """One line per (mode, beams, t_len) with the five families side by side in the order of X.FAMILIES, each as max_err / derived_there /
    ratio / excess: the
    largest error against (a), the derived bound at that element, the largest error / bound and the largest excess of the family
    (err: the larger of the two query forms per element)."""
    fam = X.pair_of_rows(nb)
    cells = []
    for i, name in enumerate(X.FAMILIES):
        m = fam == i
        at = np.argmax(np.where(m, err, -1))
        excess = np.where(m & (spread > 0), (err - bound) / np.where(spread > 0, spread, 1), -np.inf).max()
        cells.append(f"{err.flat[at]:.2e} {bound.flat[at]:.2e} {(err[m] / np.maximum(bound[m], 1e-300)).max():.3f} {excess:+.1e}")
    return f"{mode:6s} {nb} {t_len:4d} | " + " | ".join(cells)


@pytest.mark.parametrize("nb", X.BEAMS)
@pytest.mark.parametrize("mode", X.MODES)
def test_readers_match_float64_attention(gpu_lib, mode, nb):
    """Every length, both query forms, every beam row on its own (each beam has its own query: a kernel that read beam min(j, nb - 1)
    for beam j would miss), against (a) and (b); an idle window's rows stay untouched while the others repeat bit for bit; a
    non-identity kv_slot on permuted buffers gives the identity run's bits."""
    problems, lines = [], []
    R = X.SLOTS * nb
    for i, t_len in enumerate(X.T_LENS):
        k, v, fmt, Ks, Vs = reader_buffers(gpu_lib, mode, nb, t_len)
        K, V = X.reader_kv(mode, t_len)
        Q = X.reader_q(mode, t_len, nb)
        err_k, err_v = np.abs(Ks - K), np.abs(Vs - V)
        if fmt:      # what is stored obeys the row bound (the writer's own test says so bit for bit); plain rows are exact
            assert (err_k <= independent_row_bound(K, fmt)).all() and (err_v <= independent_row_bound(V, fmt)).all()
            assert err_k.max() > 0 and err_v.max() > 0
        else:
            assert not err_k.any() and not err_v.any()
        ref_a, info_a = X.attention(Q, Ks, Vs, nb)
        ref_b, info_b = X.attention(Q, K, V, nb, independent_row_bound(K, fmt) if fmt else 0 * K, independent_row_bound(V, fmt) if fmt else 0 * V)
        bound_a = X.derived_bound(ref_a, info_a, nb, t_len, mode, fmt)
        bound_b = X.derived_bound(ref_b, info_b, nb, t_len, mode, fmt, stored_error=True)
        spread_a, spread_b = X.spread_pv(ref_a, info_a, nb), X.spread_pv(ref_b, info_b, nb)
        raw = attend(gpu_lib, mode, nb, t_len, k, v, q=Q)
        forms = [("finished", raw)]
        if mode != "f32":
            splits = 2 + i % 2
            planes, bias = X.query_planes(X.reader_q_unrounded(mode, t_len, nb), splits, R + 3 + i, 31 * t_len + nb)
            forms.append((f"planes{splits}", attend(gpu_lib, mode, nb, t_len, k, v, planes=planes, bias=bias)))
        worst = None
        for form, bytes_ in forms:
            got = out_rows(bytes_, mode, fmt, R)
            if not np.isfinite(got).all():
                problems.append(f"t_len {t_len} {form}: not finite")
                continue
            ea, eb = np.abs(got - ref_a), np.abs(got - ref_b)
            worst = ea if worst is None else np.maximum(worst, ea)
            for name, e, b, sp in (("a", ea, bound_a, spread_a), ("b", eb, bound_b, spread_b)):
                allow = b + EXP_REL[mode] * sp
                if not (e <= allow).all():
                    at = np.unravel_index(np.argmax(e / allow), e.shape)
                    problems.append(f"t_len {t_len} {form} reference ({name}): {int((e > allow).sum())} elements, worst row {at[0]} column {at[1]} "
                                    f"({X.FAMILIES[X.pair_of_rows(nb)[at]]}) error {e[at]:.3e} allowed {allow[at]:.3e}")
        if worst is not None:
            lines.append(profile_line(mode, nb, t_len, worst, bound_a, spread_a))
        if len(forms) == 2 and not np.array_equal(forms[0][1], forms[1][1]):
            # the planes reduce exactly to the finished query (cross_attn_cases.query_planes): the two forms compute the same numbers
            problems.append(f"t_len {t_len}: the two query forms differ in {int((forms[0][1] != forms[1][1]).sum())} bytes")
        # idle window: its rows keep their 0xff, every other row repeats the first run bit for bit
        idle = i % X.SLOTS
        again = attend(gpu_lib, mode, nb, t_len, k, v, q=Q, done=[int(w == idle) for w in range(X.SLOTS)])
        rows_idle = slice(idle * nb, (idle + 1) * nb)
        if not (again[rows_idle] == 0xFF).all():
            problems.append(f"t_len {t_len}: idle window {idle} was written")
        if not np.array_equal(np.delete(again, np.r_[rows_idle], 0), np.delete(raw, np.r_[rows_idle], 0)):
            problems.append(f"t_len {t_len}: the second run differs")
        if fmt:      # window w reads slot PERM[w] of buffers written through slot_map = PERM
            kp, vp, _, Kp, _ = reader_buffers(gpu_lib, mode, nb, t_len, permuted=True)
            assert np.array_equal(Kp[list(PERM)], Ks)
            mapped = attend(gpu_lib, mode, nb, t_len, kp, vp, q=Q, kv_slot=list(PERM))
            if not np.array_equal(mapped, raw):
                problems.append(f"t_len {t_len}: kv_slot, {int((mapped != raw).any(1).sum())} rows differ from the identity run")
    path = os.environ.get("WSEG_CROSS_ATTN_PROFILE")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not problems, "\n".join([f"{len(problems)} problems"] + problems[:8])


def test_kv_slot_is_refused_for_plain_rows(gpu_lib):
    """The slot map exists for the packed rows only: a plain-row mode is refused before any launch (the output keeps its fill)."""
    for mode, nb in (("bf16", 4), ("f32", 1), ("f16x3", 5)):
        k, v, fmt, _, _ = reader_buffers(gpu_lib, mode, nb, 128)
        raw = attend(gpu_lib, mode, nb, 128, k, v, q=X.reader_q(mode, 128, nb), kv_slot=list(PERM), expect=-1)
        assert b"kv_slot" in gpu_lib.wseg_last_error() and (raw == 0xFF).all()
