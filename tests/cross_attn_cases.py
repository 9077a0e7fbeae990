"""Cases for the cross-attention tests (test_cross_attn_cpu.py / test_cross_attn_gpu.py), built on float64 alone: nothing here
comes from a kernel.  2 heads (d = 128), 5 window slots.

Writer rows (writer_input): ordinary random rows with one (position, head) row of each kind of PLANTED planted among them.  Every
value is exactly representable as the mode's GEMM operand (operand_grid), so that the projection with an identity weight and no
bias returns it exactly and the stored integers and scales are bit-determined.

Reader problems (reader_kv, reader_q): every (window, head) pair is one attention problem of a named family (FAMILY_OF):
    spread1    scores of spread ~1
    spread60   scores between -60 and +60
    ties       two exactly equal maxima (two identical K rows with different V rows)
    scales     K rows 2^20 times the V rows of the same positions, scores of spread ~1
    dominant   one key with probability > 0.99, for beam j at position dominant_positions(t_len)[(pair + j) % n] (six pairs:
               every position is some beam's, at every beam count)
Dimensions 0..7 of a head are ANCHORS in the ties and dominant families: beam j's query is 1 in anchor j (ties: anchor 0) and 0 in
the others, K is 0 there except in the planted rows — so a planted score is the random part plus an exact constant."""
import functools

import numpy as np

from oracle import cross_kv as CK

HEADS, D, SLOTS = 2, 128, 5
T_LENS = (128, 251, 256, 257, 500, 512, 513, 750, 1500)
BEAMS = (1, 2, 3, 4, 5, 8)
MODES = ("f32", "bf16", "f16", "bf16x3", "f16x3", "f16m6")
SPLIT_MODES = ("bf16x3", "f16x3", "f16m6")
DTYPE_ID = {"f32": 0, "bf16": 1, "f16": 2, "bf16x3": 3, "f16x3": 4, "f16m6": 5}
SCALE = 0.125
U = 2.0 ** -24
FAMILY_OF = ("spread1", "spread60", "ties", "scales") + ("dominant",) * 6      # pair = window * HEADS + head
FAMILIES = ("spread1", "spread60", "ties", "scales", "dominant")
DOMINANT_SCORE, TIE_SCORE = 40.0, 8.0


def kv_format(mode, nb):
    """What x3_cross_kv_format chooses (the GPU tests take it from the library and compare)."""
    return 0 if mode not in SPLIT_MODES or nb > 4 else (2 if mode == "f16m6" else 3)


def gamma(n):
    return n * U / (1 - n * U)


def sig_round(x, bits):
    """x rounded to `bits` significant bits (nearest even)."""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)


# significant bits that the mode's GEMM operand carries exactly: a 16-bit element; hi + lo of a split pair (one bit kept in hand);
# f16m6: the IEEE-half hi alone (its lo is re-coded as fp6 — with lo = 0 the operand is exact)
OPERAND_BITS = {"f32": 24, "bf16": 8, "f16": 11, "bf16x3": 15, "f16x3": 20, "f16m6": 11}
HALF_FAMILY = ("f16", "f16x3", "f16m6")


def operand_grid(x, mode):
    """x -> the nearest values the mode's operand rows hold exactly: OPERAND_BITS significant bits; IEEE-half modes: multiples of
    2^-24 (the half subnormal step: the lo word holds them) of magnitude 2^-14 (normal) .. 2^15, smaller values become 0."""
    y = sig_round(x, OPERAND_BITS[mode])
    if mode in HALF_FAMILY:
        y = np.clip(np.rint(np.ldexp(y, 24)) * 2.0 ** -24, -2.0 ** 15, 2.0 ** 15)
        y = np.where(np.abs(y) < 2.0 ** -14, 0.0, y)
        y = sig_round(y, OPERAND_BITS[mode])
    return y


def round_to(x, mode):
    """El<T>::rnd of the 16-bit modes (round to nearest even); the identity elsewhere."""
    if mode == "bf16":
        return sig_round(x, 8)
    if mode == "f16":
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)
    return np.asarray(x, np.float64)


# ---- writer ------------------------------------------------------------------------------------------------------------------
PLANTED = ("zero", "pow2_max", "pow2_max_plus", "outlier", "ties", "neg_pow2_max", "alternating", "clamp_below")


def planted_row(kind, fmt, mode, rng):
    """64 float64 values of one planted row, exact in the mode's operand.  fmt 0 (plain rows): the rows of format 3."""
    fmt = fmt or 3
    small = operand_grid(rng.uniform(-1, 1, 64), mode)
    if kind == "zero":
        return np.zeros(64)
    if kind == "pow2_max":          # the maximum 2^3 scales to 2^MANT and is clamped to QMAX
        v = small.copy(); v[17] = 8.0
        return v
    if kind == "pow2_max_plus":     # just above a power of two: the exponent steps up, half a unit is 2^-23 / 2^-15 of 16, not of the maximum
        v = small.copy(); v[5] = 8.0 * (1 + 2.0 ** -10) if mode != "bf16" else 8.0 * (1 + 2.0 ** -7)
        return v
    if kind == "outlier":           # one element 2^12 times the rest
        v = small.copy(); v[40] = -4096.0 * 1.25
        return v
    if kind == "ties":              # maximum 1.5 * 2^14: s = 15 - MANT; elements (n + 1/2) 2^s for even and odd n, both signs
        s = 15 - CK.MANT[fmt]
        v = np.zeros(64); v[0] = 1.5 * 2.0 ** 14
        for i, n in enumerate((2, 3, -3, -4, 6, 7, -7, -8, 0, -1)):
            v[8 + i] = (n + 0.5) * 2.0 ** s
        return v
    if kind == "neg_pow2_max":      # -2^k must become -QMAX, not wrap
        v = small.copy(); v[63] = -4.0
        return v
    if kind == "alternating":
        return operand_grid(np.where(np.arange(64) % 2 == 0, 1.0, -1.0) * rng.uniform(0.5, 1.0, 64), mode)
    if kind == "clamp_below":       # maximum 2^-90 (format 3) / 2^-100 (format 2): s stops at -CLAMP, elements are multiples of 2^-CLAMP
        top = -90 if fmt == 3 else -100
        v = np.ldexp(np.rint(rng.uniform(-1, 1, 64) * 2.0 ** 7) + 0.0, -CK.CLAMP[fmt]); v[9] = 2.0 ** top      # (+ 0.0: no -0, a sum of products has none)
        return v
    raise KeyError(kind)


def representable(kind, mode):
    """Can the mode's GEMM operand hold the planted row?  The IEEE-half operands end at 2^-24: clamp_below reaches their writers
    through the fp32 bias instead (test_cross_attn_gpu.py)."""
    return not (kind == "clamp_below" and mode in HALF_FAMILY)


@functools.lru_cache(maxsize=None)
def writer_input(mode, fmt, t_len, n_windows):
    """(x float64 [n_windows][t_len][HEADS][64], places {kind: (window, position, head)}): uniform rows with the planted rows at
    known places, the last position of the last window among them."""
    rng = np.random.default_rng(1000 * t_len + 10 * n_windows + fmt)
    x = operand_grid(rng.uniform(-1, 1, (n_windows, t_len, HEADS, 64)) * np.exp2(rng.integers(-3, 4, (n_windows, t_len, HEADS, 1))), mode)
    places = {}
    kinds = [k for k in PLANTED if representable(k, mode)]
    for i, kind in enumerate(kinds):
        w, t, h = (i % n_windows, (7 + 37 * i) % t_len, i % HEADS) if i else (n_windows - 1, t_len - 1, HEADS - 1)
        x[w, t, h] = planted_row(kind, fmt, mode, rng)
        places[kind] = (w, t, h)
    x.setflags(write=False)
    return x, places


# ---- readers -----------------------------------------------------------------------------------------------------------------
def dominant_positions(t_len):
    """First and last key and both sides of the 256-row and 512-row steps of the streaming loops, where t_len has them."""
    return sorted({t for t in (0, t_len - 1, 255, 256, 511, 512) if t < t_len})


def dominant_position(t_len, pair, beam):
    pos = dominant_positions(t_len)
    return pos[(pair + beam) % len(pos)]


def tie_positions(t_len):
    return t_len // 3, t_len - 2


@functools.lru_cache(maxsize=None)
def reader_kv(mode, t_len):
    """(K, V) float64 [SLOTS][HEADS][t_len][64], exact in the mode's operand; the same for every beam count."""
    rng = np.random.default_rng(77 + t_len)
    K = rng.standard_normal((SLOTS, HEADS, t_len, 64))
    V = rng.standard_normal((SLOTS, HEADS, t_len, 64))
    for w in range(SLOTS):
        for h in range(HEADS):
            pair, fam = w * HEADS + h, FAMILY_OF[w * HEADS + h]
            if fam == "scales":
                K[w, h] *= 2.0 ** 10
                V[w, h] *= 2.0 ** -10
            elif fam == "ties":
                t1, t2 = tie_positions(t_len)
                K[w, h, :, 0] = 0.0
                K[w, h, t2] = K[w, h, t1]
                K[w, h, (t1, t2), 0] = TIE_SCORE
            elif fam == "dominant":
                K[w, h, :, :8] = 0.0
                for j in range(8):
                    K[w, h, dominant_position(t_len, pair, j), j] = DOMINANT_SCORE
    K, V = operand_grid(K, mode), operand_grid(V, mode)
    K.setflags(write=False); V.setflags(write=False)
    return K, V


QUERY_STEP = {"scales": 2.0 ** -22}      # the query grid of a family (default 2^-12): coarse enough for exact split-K planes (query_planes)


@functools.lru_cache(maxsize=None)
def reader_q(mode, t_len, nb):
    """Q float64 [SLOTS * nb][D]: the finished, pre-scaled query rows (row = window * nb + beam), a different one for every beam.
    16-bit modes: Q is what the kernel's rounding makes of the un-rounded rows (query_planes sums to those)."""
    return round_to(reader_q_unrounded(mode, t_len, nb), mode)


@functools.lru_cache(maxsize=None)
def reader_q_unrounded(mode, t_len, nb):
    K, _ = reader_kv(mode, t_len)
    rng = np.random.default_rng(5000 + 10 * t_len + nb)
    Q = rng.standard_normal((SLOTS, nb, HEADS, 64)) / 8.0
    for w in range(SLOTS):
        for h in range(HEADS):
            fam = FAMILY_OF[w * HEADS + h]
            if fam == "spread60":
                s = Q[w, :, h] @ K[w, h].T
                Q[w, :, h] *= (60.0 / np.abs(s).max(-1))[:, None]
            elif fam == "scales":
                Q[w, :, h] *= 2.0 ** -10
            elif fam == "ties":
                Q[w, :, h, 0] = 1.0
            elif fam == "dominant":
                Q[w, :, h, :8] = 0.0
                for j in range(nb):
                    Q[w, j, h, j] = 1.0
            step = QUERY_STEP.get(fam, 2.0 ** -12)
            Q[w, :, h] = np.rint(Q[w, :, h] / step) * step
    Q = Q.reshape(SLOTS * nb, D)
    Q.setflags(write=False)
    return Q


def query_planes(q_unrounded, splits, m_pad, seed):
    """(planes float32 [splits][m_pad][D], bias float64 [D]) with (sum of the planes in order + bias) * SCALE == q_unrounded EXACTLY in
    float32 arithmetic: bias and all planes but the last are multiples of 2^-6 below 2, the last plane is what is missing — multiples
    of the query grid / SCALE of magnitude < 2^7, 22 bits at the most.  Rows beyond the queries hold NaN: they must not be read."""
    R = q_unrounded.shape[0]
    rng = np.random.default_rng(seed)
    bias = np.rint(rng.uniform(-1, 1, D) * 64) / 64
    planes = np.full((splits, m_pad, D), np.nan)
    planes[:-1, :R] = np.rint(rng.uniform(-2, 2, (splits - 1, R, D)) * 64) / 64
    planes[-1, :R] = q_unrounded / SCALE - bias - planes[:-1, :R].sum(0)
    p32 = planes.astype(np.float32)
    assert np.array_equal(p32[:, :R].astype(np.float64), planes[:, :R])
    return p32, bias


def reduce_planes_f32(planes, bias, R):
    """reduce1 of wseg_dec.hip in float32: planes summed in order from 0, + bias, * SCALE."""
    v = np.zeros((R, planes.shape[2]), np.float32)
    for z in range(planes.shape[0]):
        v = v + planes[z, :R]
    return ((v + bias.astype(np.float32)) * np.float32(SCALE)).astype(np.float64)


def attention(Q, K, V, nb, err_k=None, err_v=None):
    """float64 softmax attention of every (window, beam, head) and what the error bounds need.  Q [S * nb][D]; K, V [S][H][T][64].
    Returns out [S * nb][D] and a dict of arrays: p [S][nb][H][T], s (scores), sum_qk [S][nb][H][T] = sum_e |q_e k_te|,
    sum_pv [S * nb][D] = sum_t p_t |v_te|, and with err_k / err_v (per-element error of the rows, [S][H][T][64]):
    ds_rows [S][nb][H][T] = sum_e |q_e| err_k[t][e], dv [S * nb][D] = sum_t p_t err_v[t][e]."""
    S, H, T, _ = K.shape
    q = Q.reshape(S, nb, H, 64)
    qh, Kt = q.transpose(0, 2, 1, 3), K.transpose(0, 1, 3, 2)      # [S][H][nb][64], [S][H][64][T]
    s = (qh @ Kt).transpose(0, 2, 1, 3)                             # [S][nb][H][T]
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ph = p.transpose(0, 2, 1, 3)                                    # [S][H][nb][T]
    rows = lambda x: x.transpose(0, 2, 1, 3).reshape(S * nb, H * 64)
    out = rows(ph @ V)
    info = dict(p=p, s=s, V=V, sum_qk=(np.abs(qh) @ np.abs(Kt)).transpose(0, 2, 1, 3), sum_pv=rows(ph @ np.abs(V)))
    if err_k is not None:
        info["ds_rows"] = (np.abs(qh) @ err_k.transpose(0, 1, 3, 2)).transpose(0, 2, 1, 3)
        info["dv"] = rows(ph @ err_v)
    return out, info


def output_rounding(out, mode, fmt):
    """The output format's own rounding, per element of out [R][D]: f16x3 hi | lo rows 2^-22 relative, bf16x3 2^-17, fp32 2^-24; M6 rows
    (f16m6 from the block-floating-point kernel) 2^-14 of the 32-column block maximum; bf16 / f16 rows half a unit in the last place,
    2^-9 / 2^-12 of the power of two above |o| (up to 2^-8 / 2^-11 of |o| itself: what a correctly rounded store reaches)."""
    a = np.abs(out)
    if mode == "f16m6" and fmt != 0:
        bm = a.reshape(a.shape[0], -1, 32).max(-1, keepdims=True)
        return np.broadcast_to(2.0 ** -14 * bm, (a.shape[0], a.shape[1] // 32, 32)).reshape(a.shape)
    if mode in ("bf16", "f16"):
        _, e = np.frexp(a)      # |o| = m 2^e, 1/2 <= m < 1
        return np.where(a > 0, np.ldexp(2.0 ** -9 if mode == "bf16" else 2.0 ** -12, e), 0.0) + (2.0 ** -25 if mode == "f16" else 0.0)
    rel = {"f32": 2.0 ** -24, "bf16x3": 2.0 ** -17, "f16x3": 2.0 ** -22, "f16m6": 2.0 ** -22}[mode]
    return rel * a + (2.0 ** -25 if mode in HALF_FAMILY else 0.0)      # (IEEE-half words end at 2^-24: half a step, absolute)


def derived_bound(out, info, nb, t_len, mode, fmt, stored_error=False):
    """The derivable part of |device - reference| per output element [S * nb][D], device arithmetic in fp32 (u = 2^-24,
    gamma_n = n u / (1 - n u)):
      score      gamma_72 sum_e |q_e k_te| (64 products and their sum, with room for the order) + u |s_t - max s| (the subtraction in
                 front of exp); stored_error: + sum_e |q_e| err_K[t][e].  Call it D_t, and D its maximum over the keys;
      softmax    scores off by d_t, |d_t| <= D_t, turn p_t into p_t exp(d_t) / sum_u p_u exp(d_u).  Because sum_t p_t (v_te - o_e) = 0 the
                 output moves by sum_t p_t (exp(d_t) - 1) (v_te - o_e) / sum_u p_u exp(d_u), at most
                 exp(D) sum_t p_t (exp(D_t) - 1) |v_te - o_e| — a dominant key moves nothing, its v is the output;
      normaliser ceil(t_len / 64) sequential additions per lane, 6 wave levels, the reciprocal and its product: gamma_(ceil(t_len / 64) + 8);
      P V        gamma_(t_len + 8) sum_t p_t |v_te|; stored_error: + exp(2 D) sum_t p_t err_V[t][e];
      output     output_rounding.
    What is NOT here is the error of the device expf: a relative error of p_t like exp(d_t) - 1 above, so it is measured and allowed in
    units of spread_pv (EXP_REL in test_cross_attn_gpu.py)."""
    S = out.shape[0] // nb
    ds = gamma(72) * info["sum_qk"] + U * np.abs(info["s"] - info["s"].max(-1, keepdims=True))
    if stored_error:
        ds = ds + info["ds_rows"]
    dmax = np.repeat(ds.max(-1)[..., None], 64, -1).reshape(S * nb, D)      # [S][nb][H] -> per output element
    bound = (gamma(-(-t_len // 64) + 8) + gamma(t_len + 8)) * info["sum_pv"] + output_rounding(out, mode, fmt)
    bound = bound + np.exp(dmax) * spread_pv(out, info, nb, np.expm1(ds))
    if stored_error:
        bound = bound + info["dv"] * np.exp(2 * dmax)      # (p_t exp(d_t) / sum_u p_u exp(d_u) <= p_t exp(2 D))
    return bound


def spread_pv(out, info, nb, weight=None):
    """sum_t p_t weight_t |v_te - o_e| per output element [S * nb][D] (weight [S][nb][H][T], default 1): what a relative error of the
    probabilities moves the output by."""
    V, p = info["V"], info["p"]
    S, H = V.shape[:2]
    o = out.reshape(S, nb, H, 64)
    pw = p if weight is None else p * weight
    res = np.empty((S, nb, H, 64))
    for w in range(S):
        for j in range(nb):
            res[w, j] = np.einsum("ht,hte->he", pw[w, j], np.abs(V[w] - o[w, j][:, None, :]))
    return res.reshape(S * nb, H * 64)


def pair_of_rows(nb):
    """family index of every output element [S * nb][D] (position in FAMILIES)."""
    fam = np.array([[FAMILIES.index(FAMILY_OF[w * HEADS + h]) for h in range(HEADS)] for w in range(SLOTS)])      # [S][H]
    return np.repeat(np.repeat(fam[:, None, :], nb, 1)[..., None], 64, -1).reshape(SLOTS * nb, D)
