// Per-segment fundamental frequency from the resident PCM (wseg_pitch_frames_f64): a YIN contour of every row a segmenter returns,
// one (period, d'(tau), voiced) triple per frame of 2 tau_max samples lying wholly inside the row's samples [s0, s1).
// whisperseg_amd/pitch.py::frames_host is the definition, in float64 with every sum in a stated order; this file takes the same
// float64 steps in the same order, so the output has the definition's BITS — for every workgroup size and every grid.  No atomics,
// no inline assembly.
//
// pitch_frame_kernel    a work item is a frame; the segment table's prefix of frames per segment maps an item to its segment
//   (wseg_segments.h), the grid is capped and strides over the items.  The workgroup (64, 128 or 256 lanes, picked from tau_max in
//   wseg_pitch_plan.h) lays the frame down in LDS (2 tau_max float32, 16 KiB at the largest range), three floats in and with zeros
//   around it, so that every wide read below is aligned and stays inside the array.
//   difference    d(tau) = sum_i (x[i] - x[i + tau])^2, i = 0 .. tau_max - 1.  Lanes own lags: a lane carries the FOUR consecutive
//     lags 4 g + 1 .. 4 g + 4 of a group g through one pass over i, four i at a time — the 4 x 4 terms of such a step read x[i .. i + 3]
//     (the same address in every lane: a broadcast) and the seven samples x[i + 4 g + 1 .. i + 4 g + 7], which sit in a sliding
//     window of eight registers that one 16-byte LDS read refills: 16 terms (48 fp64 operations) per wide read, where a lane per
//     lag would pay two reads a term.  Each lag's chain is sequential in i, the square and the addition rounded separately
//     (-ffp-contract=off), whoever owns the lag.  Lags beyond tau_max of the last group read the zeros and are dropped.
//   prefix sum    run(tau) of d(1 .. tau) in the definition's two levels: a lane per block of 64 lags adds its block up from the
//     block's first lag, one lane adds the (at most 32) block totals into bases, run = base + inner; the frame is dead by then and
//     its LDS holds the inner sums.  Every lane then turns its lags' d into d' = (d tau) / run (1 where run is 0) in place.
//   dip           the first lag under the threshold and the lowest minimiser, both by a tree over the lanes (comparisons only: no
//     rounding, no order); one lane walks the descent, fits the parabola and writes the three floats.
// The triple is rate-free — the kernel never sees a sampling rate; pitch.py scales.
#include <vector>
#include "wseg_common.h"
#include "wseg_pitch_plan.h"
#include "wseg_staging.h"

namespace wseg {

constexpr int kPitchFront = 3;                                                    // floats in front of the frame: x[j] lies at sh[3 + j]
constexpr int kPitchShFloats = 2 * kPitchMaxLag + 16;                             // front + frame + zeros behind (the reads reach 2 tau_max + 6)
static_assert(kPitchShFloats * 4 >= kPitchMaxLag * 8, "the inner sums of the prefix take the frame's place");
constexpr int kPitchNoLag = 0x7fffffff;

struct PitchBest { double v; int i; };

__global__ __launch_bounds__(kPitchMaxLanes) void pitch_frame_kernel(const float* __restrict__ pcm, const long long* __restrict__ table, int n_seg,
                                                                     long long total_frames, int tau_min, int tau_max, int hop,
                                                                     double threshold, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float sh[kPitchShFloats];
  __shared__ double dn[kPitchMaxLag];                // d(tau), then d'(tau), at tau - 1
  __shared__ double base[kPitchMaxBlocks];
  __shared__ int first_below[kPitchMaxLanes];
  __shared__ PitchBest best[kPitchMaxLanes];
  const int tid = threadIdx.x, lanes = blockDim.x;
  const long long* __restrict__ prefix = table + 2 * (long long)n_seg;
  const int width = 2 * tau_max;
  const int groups = (tau_max + kPitchLagsPerLane - 1) / kPitchLagsPerLane;
  const int blocks = (tau_max + kPitchBlock - 1) / kPitchBlock;
  const int full = tau_max & ~3;                     // the i taken four at a time
  double* const inner = reinterpret_cast<double*>(sh);
  for (long long item = blockIdx.x; item < total_frames; item += gridDim.x) {
    const int lo = segment_of_item(prefix, n_seg, item);
    const float* __restrict__ x = pcm + table[2 * lo] + (item - prefix[lo]) * hop;      // x[j], 0 <= j < width, is all this item may read
    for (int j = tid; j < width + 16; j += lanes) {
      const int k = j - kPitchFront;
      sh[j] = (k >= 0 && k < width) ? x[k] : 0.0f;
    }
    __syncthreads();
    for (int g = tid; g < groups; g += lanes) {
      const float* __restrict__ w = sh + 4 * g + 4;  // w[i + k] = x[i + (4 g + 1) + k]; 16-byte aligned at every i % 4 == 0
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      double win[8];
      {
        const float4 v = *reinterpret_cast<const float4*>(w);
        win[0] = v.x; win[1] = v.y; win[2] = v.z; win[3] = v.w;
      }
      for (int i = 0; i < full; i += 4) {
        const float4 v = *reinterpret_cast<const float4*>(w + i + 4);
        win[4] = v.x; win[5] = v.y; win[6] = v.z; win[7] = v.w;
        const double xi[4] = {sh[kPitchFront + i], sh[kPitchFront + i + 1], sh[kPitchFront + i + 2], sh[kPitchFront + i + 3]};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double t = xi[a] - win[a + r];
            acc[r] = acc[r] + t * t;
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) win[k] = win[4 + k];
      }
      for (int i = full; i < tau_max; ++i) {
        const double xi = sh[kPitchFront + i];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double t = xi - (double)w[i + r];
          acc[r] = acc[r] + t * t;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * g + r < tau_max) dn[4 * g + r] = acc[r];
    }
    __syncthreads();                                 // the frame is dead: its place takes the inner sums
    if (tid < blocks) {
      const int k1 = min(tau_max, kPitchBlock * (tid + 1));
      double s = 0.0;
      for (int k = kPitchBlock * tid; k < k1; ++k) {
        s = s + dn[k];
        inner[k] = s;
      }
      base[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int b = 0; b < blocks; ++b) {
        const double t = base[b];
        base[b] = s;
        s = s + t;
      }
    }
    __syncthreads();
    for (int k = tid; k < tau_max; k += lanes) {
      const double run = base[k / kPitchBlock] + inner[k];
      dn[k] = run > 0.0 ? (dn[k] * (double)(k + 1)) / run : 1.0;
    }
    __syncthreads();
    // candidates tau_min .. tau_max - 1: the first one under the threshold, and the lowest minimiser
    const int last = tau_max - 1;
    int first = kPitchNoLag;
    PitchBest mine = {__longlong_as_double(0x7ff0000000000000LL), kPitchNoLag};
    for (int tau = tau_min + tid; tau <= last; tau += lanes) {
      const double v = dn[tau - 1];
      if (v < threshold && first == kPitchNoLag) first = tau;
      if (v < mine.v) { mine.v = v; mine.i = tau; }
    }
    first_below[tid] = first;
    best[tid] = mine;
    __syncthreads();
    for (int s = lanes >> 1; s > 0; s >>= 1) {
      if (tid < s) {
        first_below[tid] = min(first_below[tid], first_below[tid + s]);
        const PitchBest a = best[tid], b = best[tid + s];
        if (b.v < a.v || (b.v == a.v && b.i < a.i)) best[tid] = b;
      }
      __syncthreads();
    }
    if (tid == 0) {
      int tau = first_below[0];
      const bool voiced = tau != kPitchNoLag;
      if (voiced) {
        while (tau + 1 <= last && dn[tau] < dn[tau - 1]) ++tau;
      } else {
        tau = best[0].i == kPitchNoLag ? tau_min : best[0].i;      // (no candidate compares below +inf only with non-finite input)
      }
      const double a = dn[tau - 2], b = dn[tau - 1], c = dn[tau];
      const double den = (a - 2.0 * b) + c;
      double shift = 0.0;
      if (den > 0.0) {
        shift = (0.5 * (a - c)) / den;
        shift = shift < -0.5 ? -0.5 : shift > 0.5 ? 0.5 : shift;
      }
      float* __restrict__ row = out + 3 * item;
      row[0] = (float)((double)tau + shift);
      row[1] = (float)b;
      row[2] = voiced ? 1.0f : 0.0f;
    }
    __syncthreads();                                 // sh, dn and the trees are laid down anew
  }
}

}  // namespace wseg

using namespace wseg;

extern "C" size_t wseg_pitch_scratch_bytes(const int64_t* bounds_host, int32_t n_seg, int32_t tau_max, int32_t hop) {
  PitchPlan plan;
  char msg[200];
  if (pitch_plan(bounds_host, n_seg, tau_max, hop, -1, kPitchGridCap, &plan, nullptr, msg, sizeof(msg))) {
    set_error("wseg_pitch_scratch_bytes: %s", msg);
    return 0;
  }
  return (size_t)plan.scratch_bytes;
}

extern "C" int wseg_pitch_frames_f64(const float* pcm, int64_t n, const int64_t* bounds_host, int32_t n_seg, int32_t tau_min, int32_t tau_max,
                                     int32_t hop, double threshold, void* scratch, size_t scratch_bytes, float* out, void* stream_) {
  const char* fn = "wseg_pitch_frames_f64";
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0) { set_error("%s: n is negative", fn); return WSEG_ERR_INVALID; }
  PitchPlan plan;
  char msg[200];
  if (pitch_args_check(tau_min, tau_max, hop, threshold, msg, sizeof(msg))) { set_error("%s: %s", fn, msg); return WSEG_ERR_INVALID; }
  std::vector<int64_t> prefix((size_t)(n_seg > 0 ? n_seg : 0) + 1);
  if (pitch_plan(bounds_host, n_seg, tau_max, hop, n, grid_cap_env("WSEG_PITCH_GRID", kPitchGridCap, kPitchGridCap), &plan, prefix.data(), msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (n_seg == 0 || plan.total_frames == 0) return WSEG_OK;
  if (const int rc = device_buffers_check(fn, pcm, n, out, scratch, scratch_bytes, plan.scratch_bytes)) return rc;      // (a frame: n > 0)
  if (const int rc = staging_upload((size_t)plan.table_bytes, scratch, stream, fn,
                                    [&](void* host) { segment_table_fill(host, bounds_host, n_seg, prefix.data()); }))
    return rc;
  hipLaunchKernelGGL(pitch_frame_kernel, dim3((unsigned)plan.grid), dim3((unsigned)plan.lanes), 0, stream, pcm,
                     static_cast<const long long*>(scratch), (int)n_seg, (long long)plan.total_frames, (int)tau_min, (int)tau_max, (int)hop,
                     threshold, out);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}
