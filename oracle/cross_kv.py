"""Host definition (numpy, float64) of the packed cross-attention K / V rows of the split-precision modes: the formats CrossKv<2> and
CrossKv<3> of whisperseg_amd/csrc/wseg_kernels.h, written by st_bfp_row (wseg_gemm_epi.h) and read by dec_cross_attn_bfp_kernel /
dec_cross_attn_k24_kernel (wseg_dec.hip).  tests/test_cross_attn_*.py compare the kernels with it.

A ROW is the 64 elements of one (position, head).  Its integers q and its power-of-two exponent s:
    s = the smallest integer with max|v| <= 2^MANT * 2^s, clamped to [-CLAMP, +CLAMP]      MANT 15 / 23, CLAMP 110 / 100 (format 2 / 3)
    q = v / 2^s rounded to the nearest integer, ties to even, clamped to +-QMAX            QMAX = 2^MANT - 1
    value = q * 2^s
An all-zero row takes s = -CLAMP.  A row maximum of exactly 2^k scales to 2^MANT and is clamped to QMAX: a whole unit off.

BYTES: one block per (slot, head), blocks back to back, the planes of a block one after the other:
    hi plane     [t_len][64] int16    format 2: q; format 3: q >> 8 (arithmetic)
    low plane    [t_len][64] uint8    format 3 only: q & 0xff
    scale plane  [t_len] float32      format 2: 2^s; format 3: 2^(s - 8), the reader multiplies the word [hi | low | 0] = 256 q by it
132 / 196 bytes per row."""
import numpy as np

MANT = {2: 15, 3: 23}
CLAMP = {2: 110, 3: 100}
ROW_BYTES = {2: 128 + 4, 3: 128 + 64 + 4}


def qmax(fmt):
    return (1 << MANT[fmt]) - 1


def ceil_log2(x):
    """ceil(log2 x) of positive float64 values, exactly (frexp: x = m 2^e with 0.5 <= m < 1)."""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.where(m == 0.5, e - 1, e).astype(np.int64)


def row_exponent(v, fmt):
    """s of every row of v [..., 64]."""
    am = np.abs(np.asarray(v, np.float64)).max(-1)
    s = np.where(am > 0, ceil_log2(np.where(am > 0, am, 1.0)) - MANT[fmt], -CLAMP[fmt])
    return np.clip(s, -CLAMP[fmt], CLAMP[fmt]).astype(np.int64)


def encode(v, fmt):
    """v [..., 64] -> (q int32 [..., 64], s int64 [...])."""
    v = np.asarray(v, np.float64)
    s = row_exponent(v, fmt)
    q = np.rint(np.ldexp(v, -s[..., None]))      # exact scaling, then round to nearest even
    return np.clip(q, -qmax(fmt), qmax(fmt)).astype(np.int32), s


def stored_scale(s, fmt):
    """The float32 the scale plane holds for exponent s."""
    return np.ldexp(1.0, np.asarray(s) - (8 if fmt == 3 else 0)).astype(np.float32)


def pack(q, s, fmt):
    """q int32 [slots][heads][t_len][64], s [slots][heads][t_len] -> the buffer's bytes (uint8, one dimension)."""
    slots, heads, t_len, e = q.shape
    assert e == 64 and s.shape == (slots, heads, t_len)
    out = np.empty((slots, heads, t_len * ROW_BYTES[fmt]), np.uint8)
    hi = (q >> 8 if fmt == 3 else q).astype(np.int16)
    out[:, :, :t_len * 128] = hi.reshape(slots, heads, -1).view(np.uint8)
    at = t_len * 128
    if fmt == 3:
        out[:, :, at:at + t_len * 64] = (q & 0xff).astype(np.uint8).reshape(slots, heads, -1)
        at += t_len * 64
    out[:, :, at:] = np.ascontiguousarray(stored_scale(s, fmt)).reshape(slots, heads, -1).view(np.uint8)
    return out.reshape(-1)


def unpack(buf, fmt, slots, heads, t_len):
    """The buffer's bytes -> (q int32 [slots][heads][t_len][64], scale float32 [slots][heads][t_len]) as stored."""
    raw = np.ascontiguousarray(buf, np.uint8).reshape(-1)[:slots * heads * t_len * ROW_BYTES[fmt]].reshape(slots, heads, -1)
    q = np.ascontiguousarray(raw[:, :, :t_len * 128]).view(np.int16).reshape(slots, heads, t_len, 64).astype(np.int32)
    at = t_len * 128
    if fmt == 3:
        low = raw[:, :, at:at + t_len * 64].reshape(slots, heads, t_len, 64).astype(np.int32)
        q = q * 256 + low
        at += t_len * 64
    scale = np.ascontiguousarray(raw[:, :, at:]).view(np.float32).reshape(slots, heads, t_len)
    return q, scale


def decode(buf, fmt, slots, heads, t_len):
    """The buffer's bytes -> float64 [slots][heads][t_len][64]: q * scale (format 2), 256 q * scale (format 3)."""
    q, scale = unpack(buf, fmt, slots, heads, t_len)
    return q.astype(np.float64) * (256.0 if fmt == 3 else 1.0) * scale.astype(np.float64)[..., None]


def row_error_bound(v, fmt):
    """Per element of v [..., 64]: the largest |stored - v| the definition allows, from the row's maximum alone (NOT through the
    rounding above): half a unit 2^(s - 1); a whole unit 2^s where |v| is the row maximum and a power of two (the clamp to QMAX);
    0 in an all-zero row.  Valid below the upper exponent clamp (row maxima under 2^(CLAMP + MANT))."""
    v = np.asarray(v, np.float64)
    am = np.abs(v).max(-1, keepdims=True)
    assert (am < np.ldexp(1.0, CLAMP[fmt] + MANT[fmt])).all()
    s = row_exponent(v, fmt)[..., None]
    half = np.ldexp(1.0, s - 1)
    m, _ = np.frexp(am)
    unit_here = (np.abs(v) == am) & (m == 0.5)
    return np.where(am == 0, 0.0, np.where(unit_here, 2.0 * half, half))
