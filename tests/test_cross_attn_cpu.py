"""The cross-attention cases (cross_attn_cases.py) and the host definition of the packed K / V rows (oracle/cross_kv.py), on float64
alone: every case has the property it is named for, decode(encode(v)) stays within the bound the GPU tests assert, the byte layout is
the documented one — and both model-free taps (wseg_debug_cross_kv, wseg_debug_cross_attention) refuse each bad argument on the host,
before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import cross_attn_cases as X
from oracle import cross_kv as CK


# ---- the row formats ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [2, 3])
def test_planted_rows_encode_as_their_names_say(fmt):
    rng = np.random.default_rng(3)
    mode = "bf16x3"      # (its operand holds every kind, the exponent-clamp row included)
    QM, M = CK.qmax(fmt), CK.MANT[fmt]
    rows = {k: X.planted_row(k, fmt, mode, rng) for k in X.PLANTED}
    enc = {k: CK.encode(v, fmt) for k, v in rows.items()}
    q, s = enc["zero"]
    assert not q.any() and s == -CK.CLAMP[fmt]
    q, s = enc["pow2_max"]
    assert s == 3 - M and q[17] == QM and rows["pow2_max"][17] * 2.0 ** -s == QM + 1      # scaled to 2^MANT, clamped: one unit off
    q, s = enc["pow2_max_plus"]
    assert s == 4 - M and q[5] == (1 << (M - 1)) + (1 << (M - 11))                       # the exponent steps up: the maximum takes half the range
    q, s = enc["neg_pow2_max"]
    assert s == 2 - M and q[63] == -QM and q.min() == -QM
    q, s = enc["outlier"]
    v = rows["outlier"]
    assert np.abs(v).max() >= 4096 * np.sort(np.abs(v))[-2] and s == 13 - M
    q, s = enc["ties"]
    assert s == 15 - M and q[8:18].tolist() == [2, 4, -2, -4, 6, 8, -6, -8, 0, 0]        # exact halves go to the even neighbour, both signs
    assert np.array_equal(rows["ties"][8:18] * 2.0 ** -s, np.array([2.5, 3.5, -2.5, -3.5, 6.5, 7.5, -6.5, -7.5, 0.5, -0.5]))
    q, s = enc["alternating"]
    assert (np.sign(q) == np.where(np.arange(64) % 2 == 0, 1, -1)).all()
    q, s = enc["clamp_below"]
    top = -90 if fmt == 3 else -100
    assert s == -CK.CLAMP[fmt] and top - M < -CK.CLAMP[fmt] and q[9] == 1 << (top + CK.CLAMP[fmt])
    assert np.array_equal(q * 2.0 ** s, rows["clamp_below"])                              # on the clamped grid: stored exactly
    assert np.isfinite(CK.stored_scale(s, fmt)) and CK.stored_scale(s, fmt) >= 2.0 ** -126   # a normal float32 even at the clamp


@pytest.mark.parametrize("fmt", [2, 3])
def test_decode_of_encode_stays_within_the_row_bound(fmt):
    """|decode(encode(v)) - v| <= 2^(ceil(log2 rowmax) - MANT - 1), one whole unit at an element |v| = 2^k = rowmax, 0 in zero rows —
    row_error_bound, which is taken from the row maximum alone."""
    rng = np.random.default_rng(11)
    v = rng.standard_normal((3, 2, 40, 64)) * np.exp2(rng.integers(-20, 20, (3, 2, 40, 1)))
    v = v.astype(np.float32).astype(np.float64)
    v[0, 0, 0] = 0.0
    v[0, 0, 1, 7] = 2.0 ** np.ceil(np.log2(np.abs(v[0, 0, 1]).max()))      # maximum exactly 2^k
    v[0, 1, 2, 3] = -2.0 ** np.ceil(np.log2(np.abs(v[0, 1, 2]).max()))
    for kind in X.PLANTED:
        v[1, 0, X.PLANTED.index(kind)] = X.planted_row(kind, fmt, "bf16x3", rng)
    q, s = CK.encode(v, fmt)
    buf = CK.pack(q, s, fmt)
    assert buf.nbytes == 3 * 2 * 40 * {2: 132, 3: 196}[fmt] == 3 * 2 * 40 * CK.ROW_BYTES[fmt]
    back = CK.decode(buf, fmt, 3, 2, 40)
    assert np.array_equal(back, q * np.exp2(s)[..., None].astype(np.float64))
    q2, sc2 = CK.unpack(buf, fmt, 3, 2, 40)
    assert np.array_equal(q2, q) and np.array_equal(sc2, CK.stored_scale(s, fmt))
    err, bound = np.abs(back - v), CK.row_error_bound(v, fmt)
    assert (err <= bound).all()
    am = np.abs(v).max(-1)
    half = np.where(am > 0, np.exp2(np.ceil(np.log2(np.where(am > 0, am, 1))) - CK.MANT[fmt] - 1), 0)      # the formula, spelled out once more
    not_clamped = (np.ceil(np.log2(np.where(am > 0, am, 1))) - CK.MANT[fmt] >= -CK.CLAMP[fmt]) | (am == 0)
    whole = (np.abs(v) == am[..., None]) & (np.exp2(np.round(np.log2(np.where(am > 0, am, 1)))) == am)[..., None] & (am > 0)[..., None]
    assert np.array_equal(bound[not_clamped], np.where(whole, 2 * half[..., None], half[..., None])[not_clamped])
    assert (bound[0, 0, 0] == 0).all() and err[0, 0, 1, 7] == 2 * half[0, 0, 1] and err[0, 1, 2, 3] == 2 * half[0, 1, 2]
    # the bound is up to twice 2^-24 / 2^-16 of the row maximum, and reached
    rel = (err / np.where(am > 0, am, 1)[..., None]).max()
    assert 2.0 ** -(CK.MANT[fmt] + 1) < rel <= 2.0 ** -CK.MANT[fmt]


def test_block_layout_is_the_documented_one():
    """Block per (slot, head); hi plane, low-byte plane (format 3), scale plane; value = q scale / 256 q scale."""
    t_len = 5
    q = np.arange(2 * 2 * t_len * 64, dtype=np.int32).reshape(2, 2, t_len, 64) * 1237 % (1 << 23) - (1 << 22)
    s = np.arange(2 * 2 * t_len).reshape(2, 2, t_len) - 7
    b3 = CK.pack(q, s, 3).reshape(2, 2, t_len * 196)
    blk = b3[1, 0]
    assert np.array_equal(blk[:t_len * 128].view(np.int16).reshape(t_len, 64), (q[1, 0] >> 8).astype(np.int16))
    assert np.array_equal(blk[t_len * 128:t_len * 192].reshape(t_len, 64), (q[1, 0] & 0xff).astype(np.uint8))
    assert np.array_equal(blk[t_len * 192:].view(np.float32), np.exp2(s[1, 0] - 8.0).astype(np.float32))
    q2 = np.clip(q, -32767, 32767)
    b2 = CK.pack(q2, s, 2).reshape(2, 2, t_len * 132)
    assert np.array_equal(b2[0, 1][:t_len * 128].view(np.int16).reshape(t_len, 64), q2[0, 1].astype(np.int16))
    assert np.array_equal(b2[0, 1][t_len * 128:].view(np.float32), np.exp2(s[0, 1].astype(np.float64)).astype(np.float32))
    assert np.array_equal(CK.decode(b3.reshape(-1), 3, 2, 2, t_len), q * np.exp2(s.astype(np.float64))[..., None])


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", X.MODES)
def test_writer_rows_are_planted_and_exact_in_the_operand(mode):
    for t_len in (128, 251):
        fmt = X.kv_format(mode, 4)
        x, places = X.writer_input(mode, fmt, t_len, 3)
        assert np.array_equal(X.operand_grid(x, mode), x)
        assert set(places) == {k for k in X.PLANTED if X.representable(k, mode)} and len(set(places.values())) == len(places)
        assert places["zero"] == (2, t_len - 1, 1) and not x[2, t_len - 1, 1].any()
        if mode in X.HALF_FAMILY:
            nz = np.abs(x[x != 0])
            assert nz.min() >= 2.0 ** -14 and nz.max() <= 2.0 ** 15 and np.array_equal(x, np.rint(x * 2.0 ** 24) / 2.0 ** 24)
        if mode in ("bf16", "f16"):
            import torch
            td = torch.bfloat16 if mode == "bf16" else torch.float16
            assert np.array_equal(torch.from_numpy(x.copy()).to(td).double().numpy(), x)
        if mode in X.SPLIT_MODES:
            import torch
            from whisperseg_amd.engine import SPLIT_BASE, split_operand, unsplit_operand
            rows = torch.from_numpy(x.reshape(-1, X.D).copy()).float()
            assert np.array_equal(rows.double().numpy(), x.reshape(-1, X.D))
            op = split_operand(rows, SPLIT_BASE[mode])
            assert np.array_equal(unsplit_operand(op, SPLIT_BASE[mode]).double().numpy(), x.reshape(-1, X.D))      # hi + lo holds it exactly
            if mode == "f16m6":      # ... in the hi words alone
                assert not op.view(torch.float16).view(-1, X.D // 32, 2, 32)[:, :, 1].any()


@pytest.mark.parametrize("t_len", X.T_LENS)
def test_reader_cases_have_the_properties_they_are_named_for(t_len):
    for mode in ("f16x3", "bf16"):
        K, V = X.reader_kv(mode, t_len)
        assert np.array_equal(X.operand_grid(K, mode), K) and np.array_equal(X.operand_grid(V, mode), V)
        for nb in X.BEAMS:
            Q = X.reader_q(mode, t_len, nb)
            out, info = X.attention(Q, K, V, nb)
            p, s = info["p"], info["s"]
            hit = set()
            for w in range(X.SLOTS):
                for h in range(X.HEADS):
                    pair, fam = w * X.HEADS + h, X.FAMILY_OF[w * X.HEADS + h]
                    sp, pp = s[w, :, h], p[w, :, h]
                    if fam == "spread1":
                        assert 2 < (sp.max(-1) - sp.min(-1)).min() and np.abs(sp).max() < 10
                    elif fam == "spread60":
                        assert (sp.max(-1) - sp.min(-1)).min() > 75 and 59 < np.abs(sp).max() < 61      # exp(s) unshifted: 1e26 beside 1e-26
                    elif fam == "ties":
                        t1, t2 = X.tie_positions(t_len)
                        assert (sp[:, t1] == sp[:, t2]).all() and (sp[:, t1] == sp.max(-1)).all() and t1 != t2
                        assert (np.sort(sp, -1)[:, -3] < sp[:, t1] - 1).all() and not np.array_equal(V[w, h, t1], V[w, h, t2])
                    elif fam == "scales":
                        rk, rv = np.abs(K[w, h]).max(-1), np.abs(V[w, h]).max(-1)
                        assert (CK.ceil_log2(rk) - CK.ceil_log2(rv) >= 18).all() and np.median(CK.ceil_log2(rk) - CK.ceil_log2(rv)) == 20
                        assert 2 < (sp.max(-1) - sp.min(-1)).min() and np.abs(sp).max() < 10
                    else:
                        for j in range(nb):
                            t = X.dominant_position(t_len, pair, j)
                            assert pp[j, t] > 0.99 and sp[j].argmax() == t
                            hit.add(t)
            assert hit == set(X.dominant_positions(t_len)), (nb, hit)      # every position is some beam's, at every beam count
            # every beam of a window has its own query
            q = Q.reshape(X.SLOTS, nb, X.D)
            assert all(not np.array_equal(q[w, i], q[w, j]) for w in range(X.SLOTS) for i in range(nb) for j in range(i))
    assert {0, t_len - 1} <= set(X.dominant_positions(t_len)) and all(t in X.dominant_positions(t_len) for t in (255, 256, 511, 512) if t < t_len)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x3"])
def test_query_planes_sum_exactly_to_the_query(mode):
    """The split-K planes of a query reduce — in float32, in the kernel's order — to exactly the un-rounded query; the 16-bit kernels
    then round it (El<T>::rnd) to the finished rows the other form is given."""
    for t_len, nb, splits in ((128, 3, 2), (500, 8, 3)):
        qu = X.reader_q_unrounded(mode, t_len, nb)
        planes, bias = X.query_planes(qu, splits, X.SLOTS * nb + 3, 9)
        assert np.isnan(planes[:, X.SLOTS * nb:]).all()
        assert np.array_equal(X.reduce_planes_f32(planes, bias, X.SLOTS * nb), qu)
        q = X.reader_q(mode, t_len, nb)
        assert np.array_equal(q, X.round_to(qu, mode)) and (mode == "f16x3") == np.array_equal(q, qu)


def test_bounds_are_small_against_a_dropped_low_byte():
    """The point of the tight bound: a reader that ignored the low-byte plane truncates every element by 127.5 units on average
    (always the same sign), a unit being 2^(2 - 23) in rows whose maximum lies between 2 and 4; where one key dominates that is the
    output's error.  In f16x3 the derived bound of those problems is several times smaller."""
    t_len, nb, mode = 128, 4, "f16x3"
    K, V = X.reader_kv(mode, t_len)
    Q = X.reader_q(mode, t_len, nb)
    out, info = X.attention(Q, K, V, nb)
    bound = X.derived_bound(out, info, nb, t_len, mode, 3)
    dom = X.pair_of_rows(nb) == X.FAMILIES.index("dominant")
    rowmax = np.abs(V[2:]).max(-1)
    assert ((rowmax > 2) & (rowmax < 4)).mean() > 0.8
    assert 4 * np.median(bound[dom]) < 127.5 * 2.0 ** -21 and 4 * np.median(bound[~dom]) < 127.5 * 2.0 ** -21 * 10


# ---- the taps' host-side validation (nothing is launched: every pointer here is a fake, never dereferenced) ----------------------
FAKE = 0x10000


def kv_call(lib, **over):
    a = dict(dtype=4, num_beams=4, n_windows=3, n_slots=5, t_len=128, n_heads=2, plan_m=384, a=FAKE, a_bytes=512 * 128 * 4, w=FAKE, bias=None,
             slot_map=None, k=FAKE, v=FAKE, kv_bytes=5 * 2 * 128 * 196, ws=FAKE, ws_bytes=1 << 20)
    a.update(over)
    rc = lib.wseg_debug_cross_kv(a["dtype"], a["num_beams"], a["n_windows"], a["n_slots"], a["t_len"], a["n_heads"], a["plan_m"], a["a"], a["a_bytes"],
                                 a["w"], a["bias"], a["slot_map"], a["k"], a["v"], a["kv_bytes"], a["ws"], a["ws_bytes"], None)
    return rc, lib.wseg_last_error().decode()


KV_BAD = {
    "null_a": (dict(a=None), "a is null"), "null_w": (dict(w=None), "w is null"), "null_k": (dict(k=None), "k is null"),
    "null_v": (dict(v=None), "v is null"), "t_len_0": (dict(t_len=0), "t_len"), "t_len_1505": (dict(t_len=1505), "t_len"),
    "t_len_127": (dict(t_len=127), "t_len"), "num_beams_0": (dict(num_beams=0), "num_beams"), "num_beams_9": (dict(num_beams=9), "num_beams"),
    "n_heads_0": (dict(n_heads=0), "n_heads"), "n_heads_odd": (dict(n_heads=3), "n_heads"), "dtype_6": (dict(dtype=6), "dtype"),
    "n_windows_0": (dict(n_windows=0), "n_windows"), "more_windows_than_slots": (dict(n_windows=6), "n_windows"),
    "plan_m_short": (dict(plan_m=383), "plan_m"), "short_a": (dict(a_bytes=512 * 128 * 4 - 1), "a_bytes"),
    "short_kv": (dict(kv_bytes=5 * 2 * 128 * 196 - 1), "kv_bytes"), "short_kv_plain": (dict(num_beams=5, kv_bytes=5 * 2 * 128 * 256 - 1), "kv_bytes"),
    "misaligned_k": (dict(k=FAKE + 4), "aligned"), "workspace_without_size": (dict(ws_bytes=0), "splitk_ws"),
}


@pytest.mark.parametrize("name", sorted(KV_BAD))
def test_cross_kv_tap_rejects_bad_argument_on_the_host(name):
    from whisperseg_amd import _lib
    lib = _lib.load()
    over, word = KV_BAD[name]
    rc, msg = kv_call(lib, **over)
    assert rc == -1 and msg.startswith("wseg_debug_cross_kv:") and word in msg, (rc, msg)


def attn_call(lib, **over):
    a = dict(dtype=4, num_beams=4, n_windows=3, n_slots=5, t_len=128, n_heads=2, q=FAKE, q_part=None, q_splits=0, m_pad=0, q_bias=None, scale=0.125,
             done=FAKE, kv_slot=None, k=FAKE, v=FAKE, kv_bytes=5 * 2 * 128 * 196, out=FAKE, out_bytes=12 * 128 * 4)
    a.update(over)
    rc = lib.wseg_debug_cross_attention(a["dtype"], a["num_beams"], a["n_windows"], a["n_slots"], a["t_len"], a["n_heads"], a["q"], a["q_part"],
                                        a["q_splits"], a["m_pad"], a["q_bias"], a["scale"], a["done"], a["kv_slot"], a["k"], a["v"], a["kv_bytes"],
                                        a["out"], a["out_bytes"], None)
    return rc, lib.wseg_last_error().decode()


PART = dict(q=None, q_part=FAKE, q_splits=2, m_pad=16, q_bias=FAKE)
ATTN_BAD = {
    "null_q_and_q_part": (dict(q=None), "q and q_part"), "both_q_and_q_part": (dict(q_part=FAKE, q_splits=2, m_pad=16), "q and q_part"),
    "null_done": (dict(done=None), "done"), "null_k": (dict(k=None), "k is null"), "null_v": (dict(v=None), "v is null"),
    "null_out": (dict(out=None), "out is null"), "t_len_0": (dict(t_len=0), "t_len"), "t_len_1505": (dict(t_len=1505), "t_len"),
    "num_beams_0": (dict(num_beams=0), "num_beams"), "num_beams_9": (dict(num_beams=9), "num_beams"), "n_heads_0": (dict(n_heads=0), "n_heads"),
    "dtype_minus_1": (dict(dtype=-1), "dtype"), "n_windows_0": (dict(n_windows=0), "n_windows"),
    "more_windows_than_slots": (dict(n_windows=6, out_bytes=24 * 128 * 4), "n_windows"),
    "short_kv": (dict(kv_bytes=5 * 2 * 128 * 196 - 1), "kv_bytes"), "short_kv_format_2": (dict(dtype=5, kv_bytes=5 * 2 * 128 * 132 - 1), "kv_bytes"),
    "short_out": (dict(out_bytes=12 * 128 * 4 - 1), "out_bytes"), "short_out_16_bit": (dict(dtype=1, kv_bytes=1 << 20, out_bytes=12 * 128 * 2 - 1), "out_bytes"),
    "kv_slot_with_plain_rows": (dict(dtype=1, kv_slot=FAKE, kv_bytes=1 << 20), "kv_slot"),
    "kv_slot_with_fp32_rows": (dict(num_beams=5, kv_slot=FAKE, kv_bytes=1 << 20, out_bytes=1 << 20), "kv_slot"),
    "q_splits_0": (dict(PART, q_splits=0), "q_splits"), "q_splits_17": (dict(PART, q_splits=17), "q_splits"),
    "m_pad_short": (dict(PART, m_pad=11), "m_pad"), "planes_in_the_exact_mode": (dict(PART, dtype=0, kv_bytes=1 << 20), "q_part"),
    "bias_without_planes": (dict(q_bias=FAKE), "q_bias"), "misaligned_q": (dict(q=FAKE + 8), "aligned"),
}


@pytest.mark.parametrize("name", sorted(ATTN_BAD))
def test_cross_attention_tap_rejects_bad_argument_on_the_host(name):
    from whisperseg_amd import _lib
    lib = _lib.load()
    over, word = ATTN_BAD[name]
    rc, msg = attn_call(lib, **over)
    assert rc == -1 and msg.startswith("wseg_debug_cross_attention:") and word in msg, (rc, msg)


def test_cross_kv_sizes_and_formats_come_from_the_library():
    """132 / 196 bytes per packed row, 64 elements per plain row; the format follows mode and beam count as cross_attn_cases.kv_format says."""
    from whisperseg_amd import _lib
    lib = _lib.load()
    fmt = C.c_int32(-1)
    for mode in X.MODES:
        for nb in X.BEAMS:
            n = lib.wseg_debug_cross_kv_bytes(X.DTYPE_ID[mode], nb, 5, 2, 251, C.byref(fmt))
            assert fmt.value == X.kv_format(mode, nb), (mode, nb)
            row = {0: 64 * (2 if mode in ("bf16", "f16") else 4), 2: 132, 3: 196}[fmt.value]
            assert n == 5 * 2 * 251 * row and row == (CK.ROW_BYTES.get(fmt.value) or row)
    assert lib.wseg_debug_cross_kv_bytes(4, 4, 5, 2, 251, None) == 5 * 2 * 251 * 196
    for bad in ((6, 4, 5, 2, 251), (4, 0, 5, 2, 251), (4, 9, 5, 2, 251), (4, 4, 0, 2, 251), (4, 4, 5, 0, 251), (4, 4, 5, 2, 0), (4, 4, 5, 2, 1505)):
        assert lib.wseg_debug_cross_kv_bytes(*bad, None) == 0 and b"wseg_debug_cross_kv_bytes" in lib.wseg_last_error(), bad
