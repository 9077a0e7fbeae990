// The index arithmetic of the polyphase resampler, in one place: the chain of an output (resample_range, what resample_kernel
// computes inline) and the validation of a range call (resample_range_check, wseg_resample_planar_range_f32).  Plain C++ with no HIP
// dependency, so that a host-only program can run it under a sanitizer (tools/resample_range_check.cpp); the kernels of
// wseg_resample.hip compile the same resample_range for the device.
#pragma once
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define WSEG_RANGE_FN __host__ __device__ __forceinline__
#else
#define WSEG_RANGE_FN inline
#endif

namespace wseg {

struct ResampleRange { long long c, k_c, k_lo, k_hi; };      // k_c: floor(c / up), the k of tap c mod up

// Output m multiplies x[k_lo .. k_hi] (nothing when k_hi < k_lo); n_in enters only as the clamp k_hi <= n_in - 1.
WSEG_RANGE_FN ResampleRange resample_range(long long m, long long n_in, int n_h, int up, int down, int pre_pad, int pre_remove) {
  ResampleRange r;
  r.c = (m + pre_remove) * (long long)down - pre_pad;
  r.k_c = r.c / up;
  if (r.c < 0) r.k_c = -((-r.c + up - 1) / up);
  const long long lo_num = r.c - n_h + 1;
  r.k_lo = lo_num <= 0 ? 0 : (lo_num + up - 1) / up;
  r.k_hi = r.k_c > n_in - 1 ? n_in - 1 : r.k_c;
  return r;
}

// Whether outputs [m_first, m_first + m_count) of a recording of n_in frames can be computed from the segment
// [x_first, x_first + x_frames) alone: k_lo(m_first) >= x_first and min(k_c(last), n_in - 1) < x_first + x_frames (k_lo and k_c are
// monotone in m, so both ends suffice).  The ratio's integers are taken as validated (positive up / down / n_taps, non-negative
// pre_pad / pre_remove).  -> 0, or -1 with the offending range in msg.  No product here leaves int64: the output index is bounded
// first.
inline int resample_range_check(int64_t x_first, int64_t x_frames, int64_t n_in, int32_t n_taps, int32_t up, int32_t down, int32_t pre_pad,
                                int32_t pre_remove, int64_t m_first, int64_t m_count, char* msg, size_t msg_len) {
  const int64_t kIndexMax = (int64_t)1 << 61;
  if (m_first < 0 || m_count < 0 || x_first < 0 || x_frames < 0 || n_in < 0) {
    snprintf(msg, msg_len, "m_first %lld, m_count %lld, x_first %lld, x_frames %lld and n_in %lld must not be negative", (long long)m_first,
             (long long)m_count, (long long)x_first, (long long)x_frames, (long long)n_in);
    return -1;
  }
  if (x_first > n_in || x_frames > n_in - x_first) {
    snprintf(msg, msg_len, "the segment [%lld, %lld + %lld) does not lie inside the recording's %lld frames", (long long)x_first,
             (long long)x_first, (long long)x_frames, (long long)n_in);
    return -1;
  }
  if (m_first > kIndexMax || m_count > kIndexMax || (m_first + m_count + pre_remove) > kIndexMax / down) {
    snprintf(msg, msg_len, "the output range [%lld, %lld + %lld) times down = %d leaves the 64-bit index range", (long long)m_first,
             (long long)m_first, (long long)m_count, (int)down);
    return -1;
  }
  if (m_count == 0) return 0;
  const ResampleRange a = resample_range(m_first, n_in, n_taps, up, down, pre_pad, pre_remove);
  const ResampleRange b = resample_range(m_first + m_count - 1, n_in, n_taps, up, down, pre_pad, pre_remove);
  if (a.k_lo < x_first) {
    snprintf(msg, msg_len, "output %lld reads from input %lld on, before the segment's first frame %lld", (long long)m_first,
             (long long)a.k_lo, (long long)x_first);
    return -1;
  }
  if (b.k_hi >= x_first + x_frames) {
    snprintf(msg, msg_len, "output %lld reads up to input %lld, past the segment's end %lld + %lld", (long long)(m_first + m_count - 1),
             (long long)b.k_hi, (long long)x_first, (long long)x_frames);
    return -1;
  }
  return 0;
}

}  // namespace wseg
