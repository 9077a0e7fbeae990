// Epilogues shared by the GEMM kernels of wseg_gemm.hip (16-bit / split / mixed MFMA kernels, split-K reductions) and wseg_gemm_f32.hip
// (exact-parity fp32 kernels): NC = 4 or 8 consecutive output columns of one row -> bias / GELU / residual / layout scatter.
#pragma once
#include <type_traits>
#include "wseg_kernels.h"

namespace wseg {

// NC consecutive elements of type PT (float or a 16-bit type) <-> NC floats: one 8-byte (4 x 16 bit) or 16-byte access, two at 8 floats
template <typename PT, int NC> struct VecN {
  static_assert(NC == 4 || NC == 8, "4 or 8 columns per lane");
  static __device__ __forceinline__ void ld(const PT* p, float v[NC]) {
    if constexpr (sizeof(PT) == 4) {
#pragma unroll
      for (int i = 0; i < NC; i += 4) { const float4 t = *(const float4*)(p + i); v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w; }
    } else if constexpr (NC == 8) {
      unpack8<PT>(*(const uint4*)p, v);
    } else {
      const uint2 t = *(const uint2*)p;
      v[0] = H16<PT>::lo(t.x); v[1] = H16<PT>::hi(t.x);
      v[2] = H16<PT>::lo(t.y); v[3] = H16<PT>::hi(t.y);
    }
  }
  static __device__ __forceinline__ void st(PT* p, const float v[NC]) {
    if constexpr (sizeof(PT) == 4) {
#pragma unroll
      for (int i = 0; i < NC; i += 4) *(float4*)(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
    } else if constexpr (NC == 8) {
      *(uint4*)p = pack8<PT>(v);
    } else {
      *(uint2*)p = make_uint2(H16<PT>::pack(v[0], v[1]), H16<PT>::pack(v[2], v[3]));
    }
  }
};

// Cross K / V as block floating point (EpiParams::kv24 = FMT; byte layout: CrossKv<FMT>, wseg_kernels.h): the NL lanes that hold the 64
// columns of one (position, head) row — 8 consecutive lanes with 8 columns each (LDS-staged epilogues) or 16 with 4 each (split-K
// reduction) — agree on the row's power-of-two scale 2^s by DPP (the smallest with max|v| <= 2^MANT * 2^s, so that |v / 2^s| < 2^MANT after
// the clamp), every lane stores its columns as integers q (round to nearest even) and the first lane the scale.
//   FMT 2 (r05): MANT = 15, q as int16, scale 2^s.
//   FMT 3 (r06): MANT = 23, q as two's-complement 24-bit integers in two planes (q >> 8 as int16, q & 0xff as bytes), scale 2^(s - 8): the
//   reader rebuilds the 32-bit word [q >> 8 | q & 0xff | 0] = 256 q with one v_perm, converts it with v_cvt_f32_i32 and multiplies the
//   finished score / the probability by the stored scale.  Error <= half a unit = 2^(ceil(log2 max) - MANT - 1) per element: 2^-24 of the
//   ROW maximum when that is a power of two, just under 2^-23 of it otherwise; a maximum of exactly 2^k scales to 2^MANT and is clamped to
//   QMAX, a whole unit (2^-23 of the maximum) off (tests/test_cross_attn_gpu.py asserts these).  The 24-bit floats stored until mid r06
//   had 2^-17 of EVERY element: those were the largest term of f16x3's logit error (2e-5 of 2.5e-5) and cost it one of 4 200 sweep
//   recordings.
// blk: the (slot, head) block.
template <int FMT, int NC>
__device__ __forceinline__ void st_bfp_row(unsigned char* blk, int t_len, int t, int e, const float (&v)[NC], bool first_lane) {
  static_assert(NC == 4 || NC == 8, "4 or 8 columns per lane");
  typedef CrossKv<FMT> KV;
  constexpr int MANT = FMT == 3 ? 23 : 15, CLAMP = FMT == 3 ? 100 : 110, QMAX = (1 << MANT) - 1;
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) am = fmaxf(am, fabsf(v[i]));
  am = fmaxf(am, lane_xor<1>(am));
  am = fmaxf(am, lane_xor<2>(am));
  am = fmaxf(am, lane_xor<4>(am));
  if constexpr (NC == 4) am = fmaxf(am, lane_xor<8>(am));
  const unsigned bits = __float_as_uint(am);
  int ex = (int)(bits >> 23) - 127 + ((bits & 0x7fffffu) ? 1 : 0) - MANT;      // ceil(log2 max) - MANT
  ex = max(-CLAMP, min(ex, CLAMP));
  const float inv = __uint_as_float((unsigned)(127 - ex) << 23), scl = __uint_as_float((unsigned)(127 + ex - (FMT == 3 ? 8 : 0)) << 23);
  int q[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) q[i] = max(-QMAX, min(QMAX, (int)__builtin_rintf(v[i] * inv)));
  if constexpr (FMT == 2) {
    unsigned w[NC / 2];
#pragma unroll
    for (int i = 0; i < NC / 2; ++i) w[i] = ((unsigned)q[2 * i] & 0xffffu) | ((unsigned)q[2 * i + 1] << 16);
    unsigned char* dh = blk + (size_t)t * KV::HI_STRIDE + e * 2;
    if constexpr (NC == 8) *(uint4*)dh = make_uint4(w[0], w[1], w[2], w[3]);
    else *(uint2*)dh = make_uint2(w[0], w[1]);
  } else {
    unsigned hw[NC / 2];
#pragma unroll
    for (int i = 0; i < NC / 2; ++i) hw[i] = (((unsigned)q[2 * i] >> 8) & 0xffffu) | ((((unsigned)q[2 * i + 1] >> 8) & 0xffffu) << 16);
    unsigned lw[NC / 4];
#pragma unroll
    for (int i = 0; i < NC / 4; ++i)
      lw[i] = ((unsigned)q[4 * i] & 0xffu) | (((unsigned)q[4 * i + 1] & 0xffu) << 8) | (((unsigned)q[4 * i + 2] & 0xffu) << 16) | (((unsigned)q[4 * i + 3] & 0xffu) << 24);
    unsigned char* dh = blk + (size_t)t * KV::HI_STRIDE + e * 2;
    unsigned char* dl = KV::low_plane(blk, t_len) + (size_t)t * KV::LOW_STRIDE + e;
    if constexpr (NC == 8) { *(uint4*)dh = make_uint4(hw[0], hw[1], hw[2], hw[3]); *(uint2*)dl = make_uint2(lw[0], lw[1]); }
    else { *(uint2*)dh = make_uint2(hw[0], hw[1]); *(unsigned*)dl = lw[0]; }
  }
  if (first_lane) *(float*)(KV::scale_plane(blk, t_len) + (size_t)t * KV::SCALE_STRIDE) = scl;
}

// Columns n0 .. n0 + NC - 1 of row m.  NC = 8: the MFMA paths' LDS-staged epilogues (16-byte loads / stores).
// T: element-type tag of the mode (float | bf16_t | f16_t | X3<HT> | M6); PT: its plain parameter type (bias, positional table,
// q / k / v storage: float in the split-precision modes).  Outputs that are the NEXT GEMM's operand (EPI_STORE, EPI_GELU) go
// through op_stn, i.e. as hi | lo pairs (M6 rows) in the split-precision modes.
template <int EPI, typename T, int NC>
__device__ __forceinline__ void epi_apply(const EpiParams& ep, int m, int n0, float v[NC]) {
  typedef typename IO<T>::P PT;
  if (ep.bias) {
    float b[NC];
    VecN<PT, NC>::ld((const PT*)ep.bias + n0, b);
#pragma unroll
    for (int i = 0; i < NC; ++i) v[i] += b[i];
  }
  if constexpr (NC == 8 && (EPI == EPI_QKV_DEC || EPI == EPI_SCALE)) {      // no 8-column form: two 4-column halves
    epi_apply<EPI, T, 4>(ep, m, n0, v);
    epi_apply<EPI, T, 4>(ep, m, n0 + 4, v + 4);
  } else if constexpr (EPI == EPI_STORE) {
    op_stn<T, NC>(ep.out, (size_t)m, ep.ldc, n0, v);
  } else if constexpr (EPI == EPI_GELU) {
    gelu_n<T, NC>(v);
    op_stn<T, NC>(ep.out, (size_t)m, ep.ldc, n0, v);
  } else if constexpr (EPI == EPI_RESID) {      // the residual stream is fp32 in every mode
    float r[NC];
    VecN<float, NC>::ld((const float*)ep.resid + (size_t)m * ep.ldc + n0, r);
#pragma unroll
    for (int i = 0; i < NC; ++i) v[i] = r[i] + v[i];
    VecN<float, NC>::st((float*)ep.out + (size_t)m * ep.ldc + n0, v);
  } else if constexpr (EPI == EPI_GELU_POS) {   // conv2 -> residual stream (fp32)
    float p[NC];
    VecN<PT, NC>::ld((const PT*)ep.pos + (size_t)(m % ep.pos_rows) * ep.ldc + n0, p);
    gelu_n<T, NC>(v, p);
    VecN<float, NC>::st((float*)ep.out + (size_t)m * ep.ldc + n0, v);
  } else if constexpr (EPI == EPI_QKV_ENC) {
    const int d = ep.d_model, sec = n0 / d, nn = n0 - sec * d, h = nn >> 6, e = nn & 63;
    const int b = m / ep.t_len, t = m - b * ep.t_len;
    const size_t bh = (size_t)b * ep.n_heads + h;
    if (sec == 0) {
#pragma unroll
      for (int i = 0; i < NC; ++i) v[i] *= ep.scale;
    }
    auto put = [&](auto* base, size_t plane, const float* x) {
      typedef std::remove_pointer_t<decltype(base)> QT;
      if (sec == 0) VecN<QT, NC>::st((QT*)ep.q + plane + enc_qk_index(bh, ep.t_pad, t) + e, x);
      else if (sec == 1) VecN<QT, NC>::st((QT*)ep.k + plane + enc_qk_index(bh, ep.t_pad, t) + e, x);
      else if (ep.vt_tiled) {      // (enc_vt_block / vt_plain_index spelled out: the calls changed the instruction order of these kernels)
        QT* vt = (QT*)ep.v + plane + bh * 64 * ep.t_pad;
#pragma unroll
        for (int i = 0; i < NC; ++i) El<QT>::st(vt + vt_tiled_index(e + i, t), x[i]);
      } else {
        QT* vt = (QT*)ep.v + plane + (bh * 64 + e) * ep.t_pad + t;
#pragma unroll
        for (int i = 0; i < NC; ++i) El<QT>::st(vt + (size_t)i * ep.t_pad, x[i]);
      }
    };
    typedef typename IO<T>::A AT;
    if (IO<T>::split && ep.qkv_mode == 1) put((float*)nullptr, 0, v);
    else {
      if constexpr (IO<T>::split) {                // the encoder attention's Q / K / V^T are IEEE-half planes in BOTH split modes:
#pragma unroll                                     // saturate like every other split operand (inf - inf = NaN in the lo plane otherwise)
        for (int i = 0; i < NC; ++i) v[i] = H16<AT>::sat(v[i]);
      }
      put((AT*)nullptr, 0, v);
      if (IO<T>::split && ep.qkv_mode == 2) {      // lo plane: x - rn(x)
        float lo[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) lo[i] = v[i] - El<AT>::rnd(v[i]);
        put((AT*)nullptr, ep.qkv_plane, lo);
      }
    }
  } else if constexpr (EPI == EPI_KV_CROSS) {
    const int d = ep.d_model, sec = n0 / d, nn = n0 - sec * d, h = nn >> 6, e = nn & 63;
    const int b = m / ep.t_len, t = m - b * ep.t_len;
    const int bs = ep.slot_map ? ep.slot_map[b] : b;
    // packed rows: the row's lanes are consecutive — 16 threads of the split-K reduction (NC = 4) or 8 lanes of an LDS-staged epilogue
    // (NC = 8: lane & 7 = column group)
    if (IO<T>::split && ep.kv24 == 2) {
      st_bfp_row<2, NC>(CrossKv<2>::block((unsigned char*)(sec == 0 ? ep.k : ep.v), (size_t)bs * ep.n_heads + h, ep.t_len), ep.t_len, t, e, *(const float(*)[NC])v, e == 0);
    } else if (IO<T>::split && ep.kv24 == 3) {
      st_bfp_row<3, NC>(CrossKv<3>::block((unsigned char*)(sec == 0 ? ep.k : ep.v), (size_t)bs * ep.n_heads + h, ep.t_len), ep.t_len, t, e, *(const float(*)[NC])v, e == 0);
    } else {
      PT* dst = (PT*)(sec == 0 ? ep.k : ep.v) + (((size_t)bs * ep.n_heads + h) * ep.t_len + t) * 64 + e;
      VecN<PT, NC>::st(dst, v);
    }
  } else if constexpr (EPI == EPI_F32) {
    VecN<float, NC>::st(ep.out_f32 + (size_t)m * ep.ldc + n0, v);
  } else if constexpr (EPI == EPI_QKV_DEC) {
    const int d = ep.d_model, sec = n0 / d, nn = n0 - sec * d, h = nn >> 6, e = nn & 63;
    if (sec == 0) {
#pragma unroll
      for (int i = 0; i < NC; ++i) v[i] *= ep.scale;
      VecN<PT, NC>::st((PT*)ep.q + (size_t)m * d + nn, v);
    } else {
      const int slot = m / ep.pos_div, beam = m - slot * ep.pos_div;
      if (ep.idle_ptr[slot]) return;
      const int pos = ep.pos_ptr[slot];
      const int unit = ep.kv_pt[(size_t)slot * ep.kv_npg + pos / KV_PAGE];
      PT* dst = (PT*)(sec == 1 ? ep.k : ep.v) + kv_page_row((size_t)unit, ep.pos_div, beam, ep.n_heads, h, pos) * 64 + e;
      VecN<PT, NC>::st(dst, v);
    }
  } else if constexpr (EPI == EPI_SCALE) {
#pragma unroll
    for (int i = 0; i < NC; ++i) v[i] *= ep.scale;
    VecN<PT, NC>::st((PT*)ep.out + (size_t)m * ep.ldc + n0, v);
  }
}

}  // namespace wseg
