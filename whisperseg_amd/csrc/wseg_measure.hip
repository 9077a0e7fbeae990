// Per-segment acoustic measurements from the resident PCM (wseg_measure_segments_f32): for every row a segmenter returns, eight
// numbers taken from the float32 samples [s0, s1) of the recording the front-end saw — level (max |x|, rms, zero crossings) and
// the shape of the power spectrum P[k] = sum over frames |rfft(hann * frame)[k]|^2 inside a band (peak bin, centroid, the 5 % and
// 95 % points of the cumulated power, entropy).  whisperseg_amd/measure.py::measure_host is the definition, in float64; this file
// computes the FFT in fp32 and every sum over frames, samples or bins in fp64, in a fixed order: the same input gives the same
// bits on every run and for every grid size.  No atomics, no inline assembly; the front-end's FFT (wseg_logmel.hip: one wave per
// frame, tied to its mel stage) is left alone — the transform here is the workgroup's.
//
// measure_chunk_kernel    a work item is a (segment, chunk) pair, a chunk 64 consecutive frames of the segment (the last chunk the
//   rest; wseg_measure_plan.h); the segment table's prefix of chunks per segment maps an item to its segment (wseg_segments.h),
//   the grid is capped and strides over the items.  A workgroup of 256 lanes transforms one frame at a time in LDS with the
//   real FFT of wseg_rfft.h (decimation in frequency, unpacked through the bit reversal): one code path for 512 .. 8192, 32 KiB of LDS at the
//   largest size, the twiddles (the log-mel descriptor's table, W_n^k for k < n_fft / 2) and the window read from global memory,
//   where every frame of every workgroup finds them in cache.  Lane t owns bins t, t + 256, ...: at most 17 at 8192, kept as fp64
//   registers over the chunk's frames and written once.  A sample is loaded with one guard, index < s1 (indices start at s0), by
//   4-byte loads only: nothing in front of s0 and nothing at or behind s1 is ever read.
//   The chunk also owns the samples [s0 + 64 c hop, s0 + 64 (c + 1) hop) of its segment (the last chunk: up to s1) and writes
//   their max |x|, sum x^2 (fp64) and sign changes — the pair (i - 1, i) belongs to the owner of i, and i = s0 has no pair.
// measure_finish_kernel   one workgroup per segment: adds the chunks' partials in chunk order, then block reductions and one block
//   prefix sum over the band's bins, all fp64, give the row.
// The row is rate-free — the kernels never see a sampling rate: crossings as a count, frequencies in bins; measure.py scales.
#include <vector>
#include "wseg_common.h"
#include "wseg_measure_plan.h"
#include "wseg_staging.h"

namespace wseg {

constexpr int kMeasureLanes = 256;
constexpr int kMeasureMaxHalf = 4096;                                             // complex points of the 8192-point transform
constexpr int kMeasureBinsPerLane = (kMeasureMaxHalf + kMeasureLanes) / kMeasureLanes;      // 17: bins 0 .. 4096 over 256 lanes

// Reductions over the workgroup through `buf` (256 slots), a tree in a fixed order; every lane gets the result.
template <class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T* buf, Op op) {
  const int t = threadIdx.x;
  __syncthreads();                                   // the reduction before may still be read
  buf[t] = v;
  __syncthreads();
  for (int s = kMeasureLanes / 2; s > 0; s >>= 1) {
    if (t < s) buf[t] = op(buf[t], buf[t + s]);
    __syncthreads();
  }
  return buf[0];
}
__device__ __forceinline__ double block_sum(double v, double* buf) {
  return block_reduce(v, buf, [](double a, double b) { return a + b; });
}

__global__ __launch_bounds__(kMeasureLanes) void measure_chunk_kernel(const float* __restrict__ pcm, const long long* __restrict__ table, int n_seg,
                                                                      long long total_chunks, int n_fft, int log2_half,
                                                                      const float* __restrict__ window, const float2* __restrict__ twiddle,
                                                                      double* __restrict__ partial) {
  __shared__ float2 z[kMeasureMaxHalf];
  __shared__ double red[kMeasureLanes];
  const int tid = threadIdx.x;
  const int M = n_fft >> 1, hop = n_fft >> 2;
  const long long* __restrict__ prefix = table + 2 * (long long)n_seg;
  const long long chunk_doubles = M + 1 + kMeasureTimeSlots;
  float* const zf = reinterpret_cast<float*>(z);
  for (long long item = blockIdx.x; item < total_chunks; item += gridDim.x) {
    const int lo = segment_of_item(prefix, n_seg, item);
    const long long s0 = table[2 * lo], len = table[2 * lo + 1] - s0;
    const long long c = item - prefix[lo], n_chunks = prefix[lo + 1] - prefix[lo];
    const long long n_frames = len <= n_fft ? 1 : 1 + (len - n_fft + hop - 1) / hop;
    const long long j0 = c * kMeasureChunkFrames;
    const int nf = (int)min((long long)kMeasureChunkFrames, n_frames - j0);
    const float* __restrict__ x = pcm + s0;          // x[i], 0 <= i < len, is all this item may read
    double P[kMeasureBinsPerLane];
#pragma unroll
    for (int r = 0; r < kMeasureBinsPerLane; ++r) P[r] = 0.0;
    for (int f = 0; f < nf; ++f) {
      const long long base = (j0 + f) * hop;
      for (int i = tid; i < n_fft; i += kMeasureLanes) {
        const long long p = base + i;
        zf[i] = p < len ? x[p] * window[i] : 0.0f;
      }
      __syncthreads();
      for (int sh = log2_half - 1; sh >= 0; --sh) {   // decimation in frequency: half-size 2^sh from M / 2 down to 1
        for (int b = tid; b < (M >> 1); b += kMeasureLanes) rfft_dif_butterfly(z, twiddle, n_fft, sh, b);
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < kMeasureBinsPerLane; ++r) {
        const int k = tid + kMeasureLanes * r;
        if (k <= M) {
          float re, im;
          rfft_unpack_bin(z, twiddle, M, log2_half, k, re, im);
          P[r] += (double)re * (double)re + (double)im * (double)im;
        }
      }
      __syncthreads();                               // z is laid down anew
    }
    // the samples this chunk owns
    const long long t_lo = j0 * hop, t_hi = c == n_chunks - 1 ? len : (j0 + kMeasureChunkFrames) * hop;
    float mx = 0.0f;
    double ss = 0.0;
    long long crossings = 0;
    for (long long i = t_lo + tid; i < t_hi; i += kMeasureLanes) {
      const float v = x[i];
      mx = fmaxf(mx, fabsf(v));
      ss += (double)v * (double)v;
      if (i > 0) crossings += (v < 0.0f) != (x[i - 1] < 0.0f);
    }
    ss = block_sum(ss, red);
    mx = block_reduce(mx, reinterpret_cast<float*>(red), [](float a, float b) { return fmaxf(a, b); });
    crossings = block_reduce(crossings, reinterpret_cast<long long*>(red), [](long long a, long long b) { return a + b; });
    double* __restrict__ dst = partial + item * chunk_doubles;
#pragma unroll
    for (int r = 0; r < kMeasureBinsPerLane; ++r) {
      const int k = tid + kMeasureLanes * r;
      if (k <= M) dst[k] = P[r];
    }
    if (tid == 0) {
      dst[M + 1] = ss;
      dst[M + 2] = (double)mx;
      dst[M + 3] = __longlong_as_double(crossings);
    }
    __syncthreads();                                 // red is read to here
  }
}

struct PeakBin { double v; int i; };

__global__ __launch_bounds__(kMeasureLanes) void measure_finish_kernel(const long long* __restrict__ table, int n_seg, int n_fft, int k_lo, int k_hi,
                                                                       const double* __restrict__ partial, float* __restrict__ out) {
  __shared__ double B[kMeasureMaxHalf];              // the band's bins (at most n_fft / 2: DC is never in it)
  __shared__ double red[kMeasureLanes];
  __shared__ PeakBin peak[kMeasureLanes];
  __shared__ double lane_sum[kMeasureLanes + 1];
  __shared__ double quantile[2];
  const int tid = threadIdx.x;
  const int seg = blockIdx.x;
  const long long* __restrict__ prefix = table + 2 * (long long)n_seg;
  const long long len = table[2 * seg + 1] - table[2 * seg];
  const long long c0 = prefix[seg], n_chunks = prefix[seg + 1] - c0;
  float* __restrict__ row = out + 8 * (long long)seg;
  const float nan = __uint_as_float(0x7fc00000u);
  if (len == 0) {                                    // (uniform over the workgroup)
    if (tid < 8) row[tid] = nan;
    return;
  }
  const int M = n_fft >> 1, nb = k_hi - k_lo + 1;
  const long long chunk_doubles = M + 1 + kMeasureTimeSlots;
  const double* __restrict__ src = partial + c0 * chunk_doubles;
  for (int i = tid; i < nb; i += kMeasureLanes) {
    double s = 0.0;
    for (long long c = 0; c < n_chunks; ++c) s += src[c * chunk_doubles + k_lo + i];
    B[i] = s;
  }
  double ss = 0.0;                                   // every lane adds the same three numbers per chunk, in chunk order
  float mx = 0.0f;
  long long crossings = 0;
  for (long long c = 0; c < n_chunks; ++c) {
    const double* __restrict__ t = src + c * chunk_doubles + M + 1;
    ss += t[0];
    mx = fmaxf(mx, (float)t[1]);
    crossings += __double_as_longlong(t[2]);
  }
  if (tid == 0) quantile[0] = quantile[1] = __longlong_as_double(0x7ff8000000000000LL);
  __syncthreads();
  // total, weighted total and the lowest maximiser: lane t over bins t, t + 256, ..., then the trees
  double total = 0.0, moment = 0.0;
  PeakBin best = {-1.0, 0};
  for (int i = tid; i < nb; i += kMeasureLanes) {
    const double b = B[i];
    total += b;
    moment += (double)(k_lo + i) * b;
    if (b > best.v) { best.v = b; best.i = i; }
  }
  total = block_sum(total, red);
  moment = block_sum(moment, red);
  best = block_reduce(best, peak, [](PeakBin a, PeakBin b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; });
  double h = 0.0;
  for (int i = tid; i < nb; i += kMeasureLanes) {
    const double p = B[i] / total;
    if (p > 0.0) h += p * log(p);
  }
  h = block_sum(h, red);
  // cumulated power: lane t walks the bins [t per, (t + 1) per); C[i] = (sum of the lanes before) + (the lane's running sum), which is
  // monotone in i and continues exactly from one lane to the next, so each of the two targets is crossed in exactly one bin
  const int per = (nb + kMeasureLanes - 1) / kMeasureLanes;
  const int i_lo = min(nb, tid * per), i_hi = min(nb, i_lo + per);
  double mine = 0.0;
  for (int i = i_lo; i < i_hi; ++i) mine += B[i];
  lane_sum[tid + 1] = mine;
  __syncthreads();
  if (tid == 0) {
    lane_sum[0] = 0.0;
    for (int t = 1; t <= kMeasureLanes; ++t) lane_sum[t] += lane_sum[t - 1];
  }
  __syncthreads();
  if (total > 0.0) {
    const double before = lane_sum[tid], t05 = 0.05 * total, t95 = 0.95 * total;
    double run = 0.0, prev = before;
    for (int i = i_lo; i < i_hi; ++i) {
      run += B[i];
      const double cum = before + run;
      if (prev < t05 && cum >= t05) quantile[0] = (double)(k_lo + i) - 0.5 + (t05 - prev) / B[i];
      if (prev < t95 && cum >= t95) quantile[1] = (double)(k_lo + i) - 0.5 + (t95 - prev) / B[i];
      prev = cum;
    }
  }
  __syncthreads();
  if (tid == 0) {
    row[0] = mx;
    row[1] = (float)sqrt(ss / (double)len);
    row[2] = (float)crossings;
    const bool spectral = total > 0.0;
    row[3] = spectral ? (float)(k_lo + best.i) : nan;
    row[4] = spectral ? (float)(moment / total) : nan;
    row[5] = spectral ? (float)quantile[0] : nan;
    row[6] = spectral ? (float)quantile[1] : nan;
    row[7] = spectral ? (float)(-h / log((double)nb)) : nan;
  }
}

}  // namespace wseg

using namespace wseg;

extern "C" size_t wseg_measure_scratch_bytes(const int64_t* bounds_host, int32_t n_seg, int32_t n_fft) {
  MeasurePlan plan;
  char msg[200];
  if (measure_plan(bounds_host, n_seg, n_fft, -1, kMeasureGridCap, &plan, nullptr, msg, sizeof(msg))) {
    set_error("wseg_measure_scratch_bytes: %s", msg);
    return 0;
  }
  return (size_t)plan.scratch_bytes;
}

extern "C" int wseg_measure_segments_f32(const float* pcm, int64_t n, const int64_t* bounds_host, int32_t n_seg, int32_t n_fft, int32_t k_lo,
                                         int32_t k_hi, const float* window, const float* twiddle, void* scratch, size_t scratch_bytes,
                                         float* out, void* stream_) {
  const char* fn = "wseg_measure_segments_f32";
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0) { set_error("%s: n is negative", fn); return WSEG_ERR_INVALID; }
  MeasurePlan plan;
  char msg[200];
  std::vector<int64_t> prefix((size_t)(n_seg > 0 ? n_seg : 0) + 1);
  if (measure_plan(bounds_host, n_seg, n_fft, n, grid_cap_env("WSEG_MEASURE_GRID", kMeasureGridCap, 65535), &plan, prefix.data(), msg, sizeof(msg)) ||
      measure_band_check(n_fft, k_lo, k_hi, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (n_seg == 0) return WSEG_OK;
  if (const int rc = device_buffers_check(fn, pcm, n, out, scratch, scratch_bytes, plan.scratch_bytes)) return rc;
  if (!window || !twiddle || ((uintptr_t)twiddle & 7)) { set_error("%s: window and twiddle (8-byte aligned) must be device pointers", fn); return WSEG_ERR_INVALID; }
  if (const int rc = staging_upload((size_t)plan.table_bytes, scratch, stream, fn,
                                    [&](void* host) { segment_table_fill(host, bounds_host, n_seg, prefix.data()); }))
    return rc;
  const long long* table = static_cast<const long long*>(scratch);
  double* partial = reinterpret_cast<double*>(static_cast<char*>(scratch) + plan.partial_offset);
  if (plan.grid > 0) {
    hipLaunchKernelGGL(measure_chunk_kernel, dim3((unsigned)plan.grid), dim3(kMeasureLanes), 0, stream, pcm, table, (int)n_seg,
                       (long long)plan.total_chunks, (int)n_fft, rfft_log2_half(n_fft), window, reinterpret_cast<const float2*>(twiddle), partial);
    WSEG_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(measure_finish_kernel, dim3((unsigned)n_seg), dim3(kMeasureLanes), 0, stream, table, (int)n_seg, (int)n_fft, (int)k_lo,
                     (int)k_hi, partial, out);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}
