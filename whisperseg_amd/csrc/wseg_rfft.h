// The workgroup's real FFT in LDS, as measure_chunk_kernel (one frame at a time) and patch_frames_kernel (F frames side by side)
// take it.  n_fft windowed real samples are laid down as M = n_fft / 2 complex points z[m] = x[2m] + i x[2m + 1] (a flat copy); a
// radix-2 decimation-in-frequency pass per power of two — stage sh = log2(M) - 1 down to 0, a barrier behind each, the callers' —
// leaves Z in bit-reversed order, and the unpack step
//     X[k] = E + W_n^k O,   E = (Z[k] + conj Z[M - k]) / 2,   O = (Z[k] - conj Z[M - k]) / 2i
// reads Z[k] and Z[M - k] through the bit reversal: no reordering pass.  `twiddle` is the log-mel descriptor's table, W_n^k for
// k < M.  The floating-point expressions are the ones the device tests' bits rest on (-ffp-contract=off): leave them as written.
// The sizes are plain C++ (the plan headers use them); the device pieces exist where hipcc compiles the file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace wseg {

inline bool rfft_size_ok(int32_t n_fft) { return n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096 || n_fft == 8192; }
inline int rfft_size_check(int32_t n_fft, char* msg, size_t msg_len) {      // -> 0, or -1 with the argument's name in msg
  return rfft_size_ok(n_fft) ? 0 : (snprintf(msg, msg_len, "n_fft must be 512, 1024, 2048, 4096 or 8192 (got %d)", (int)n_fft), -1);
}
inline int rfft_log2_half(int32_t n_fft) {           // n_fft / 2 = 2^log2_half
  int log2_half = 0;
  while ((2 << log2_half) < n_fft) ++log2_half;
  return log2_half;
}

#if defined(__HIPCC__)
// Butterfly b (0 <= b < M / 2) of stage sh of ONE transform, whose M points start at zz: half-size h = 2^sh, the pair zz[i0],
// zz[i0 + h] with W_{2h}^j = W_n^{j n / 2h}.  A stage is this for every b of every frame that lies in LDS, then a barrier.
__device__ __forceinline__ void rfft_dif_butterfly(float2* zz, const float2* __restrict__ twiddle, int n_fft, int sh, int b) {
  const int h = 1 << sh, tstep = n_fft >> (sh + 1);
  const int j = b & (h - 1);
  const int i0 = ((b >> sh) << (sh + 1)) + j, i1 = i0 + h;
  const float2 a = zz[i0], q = zz[i1], w = twiddle[j * tstep];
  const float dr = a.x - q.x, di = a.y - q.y;
  zz[i0] = make_float2(a.x + q.x, a.y + q.y);
  zz[i1] = make_float2(dr * w.x - di * w.y, dr * w.y + di * w.x);
}

// Bin k (0 <= k <= M = 2^log2_half) of the transformed frame at zz -> (re, im).
__device__ __forceinline__ void rfft_unpack_bin(const float2* zz, const float2* __restrict__ twiddle, int M, int log2_half, int k, float& re,
                                                float& im) {
  __builtin_assume(M > 0);                           // (so that a caller's literal k = M is known not to be bin 0)
  if (k == 0 || k == M) {                          // E[0] +- O[0], both real
    const float2 a = zz[0];
    re = k == 0 ? a.x + a.y : a.x - a.y;
    im = 0.0f;
  } else {
    const float2 a = zz[__brev((unsigned)k) >> (32 - log2_half)], q = zz[__brev((unsigned)(M - k)) >> (32 - log2_half)];
    const float er = 0.5f * (a.x + q.x), ei = 0.5f * (a.y - q.y);
    const float orr = 0.5f * (a.y + q.y), oi = -0.5f * (a.x - q.x);
    const float2 w = twiddle[k];
    re = er + (orr * w.x - oi * w.y);
    im = ei + (orr * w.y + oi * w.x);
  }
}
#endif

}  // namespace wseg
