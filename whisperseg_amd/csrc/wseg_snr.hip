// Per-segment signal-to-noise ratio from the resident PCM: a band-energy track over every whole frame of the recording
// (wseg_frame_energy_f32), and per row of a segmenter's output the mean and the maximum of its frames' energies and the noise
// floor of its window, an exact order statistic of the track (wseg_snr_rows_f64).  whisperseg_amd/snr.py holds the definition, in
// float64; here the FFT is fp32 and the band sum fp64 in a fixed order, the selection is exact (integers only) and a row's sum is
// fp64: the same input gives the same bits on every run and for every grid.  No inline assembly.
//
// snr_frames_kernel        a work item is a GROUP of G = 4096 / (n_fft / 2) consecutive frames (16 at n_fft 512 .. 1 at 8192;
//   wseg_snr_plan.h), the grid is capped and strides over the groups.  The samples a group spans — (G - 1) hop + n_fft, a frame shares
//   three quarters of its samples with its neighbours — are loaded ONCE into LDS (a group of one frame has nothing to share and is
//   laid down straight from global memory), guarded by the end of the recording's last whole frame: no sample at or behind it is
//   read.  The frames are laid down windowed as n_fft / 2 complex points each, G side by side, and transformed by the real FFT of
//   wseg_rfft.h as patch_frames_kernel does (2048 butterflies a pass, 8 a lane).  The 256 / G lanes of a frame then walk the band's
//   bins k_lo .. k_hi, re^2 + im^2 in fp64, and a tree over those lanes in a fixed order gives E[j], rounded to float32 once.
// snr_select_kernel        a workgroup per SHORT window (at most kSnrSplit frames): the keys — the float32 bit patterns, which order
//   non-negative floats as their values do; every NaN is 0xFFFFFFFF and sorts last — are loaded once into LDS and the rank-r key is
//   found by a radix select in four 8-bit passes from the top byte down: a 256-bin histogram of the keys that share the bytes found
//   so far (integer atomics in LDS), a scan over the bins, the bin that holds the rank.
// snr_split_pass_kernel    pass p of the same select for the LONG windows, a work item a chunk of kSnrSplit frames: the workgroup
//   finds the bytes of the passes before p from the window's finished histograms in the scratch (every chunk of a window finds the
//   same: integers), counts its chunk in LDS and adds its bins to the window's histogram of pass p with 64-bit integer atomics —
//   integer addition has no order.  Four launches, one per pass, whatever the data.
// snr_split_finish_kernel  a workgroup per long window: the four bytes from the four histograms -> the key.
// snr_rows_kernel          a wave per row: the fp64 sum of its frames' energies over their count, their maximum (NaN if a frame is
//   NaN, as numpy's max), and its window's key as a value -> float64 (S, M, N).
#include <vector>
#include "wseg_common.h"
#include "wseg_snr_plan.h"
#include "wseg_staging.h"

namespace wseg {

struct SnrTrackArgs {
  const float* pcm;
  long long read_end;              // no sample at or behind it is loaded
  long long frames, groups;
  int n_fft, log2_half, log2_group, k_lo, k_hi;
  const float* window;
  const float2* twiddle;
  float* track;
};

__global__ __launch_bounds__(kSnrLanes) void snr_frames_kernel(SnrTrackArgs a) {
  __shared__ float2 z[kSnrFrameSlots];
  __shared__ float stage[kSnrStageFloats];
  __shared__ double red[kSnrLanes];
  const int tid = threadIdx.x;
  const int n_fft = a.n_fft, M = n_fft >> 1, hop = n_fft >> 2, lg = a.log2_half;
  const int G = 1 << a.log2_group;
  const int lanes_per_frame = kSnrLanes >> a.log2_group;
  const float* __restrict__ window = a.window;
  const float2* __restrict__ twiddle = a.twiddle;
  float* const zf = reinterpret_cast<float*>(z);
  for (long long item = blockIdx.x; item < a.groups; item += gridDim.x) {
    const long long g0 = item * G;
    const long long base = g0 * hop;                 // the group's first sample
    if (G > 1) {
      const int span = (G - 1) * hop + n_fft;        // <= kSnrStageFloats
      for (int i = tid; i < span; i += kSnrLanes) {
        const long long p = base + i;
        stage[i] = p < a.read_end ? a.pcm[p] : 0.0f;
      }
      __syncthreads();
      for (int idx = tid; idx < 2 * kSnrFrameSlots; idx += kSnrLanes) {
        const int fr = idx >> (lg + 1), i = idx & (n_fft - 1);
        zf[idx] = stage[fr * hop + i] * window[i];
      }
    } else {
      for (int i = tid; i < n_fft; i += kSnrLanes) {
        const long long p = base + i;
        zf[i] = p < a.read_end ? a.pcm[p] * window[i] : 0.0f;
      }
    }
    __syncthreads();
    for (int sh = lg - 1; sh >= 0; --sh) {           // decimation in frequency: half-size 2^sh from M / 2 down to 1; butterfly bb of frame fr
      for (int b = tid; b < kSnrFrameSlots / 2; b += kSnrLanes) {
        const int fr = b >> (lg - 1), bb = b & ((M >> 1) - 1);
        rfft_dif_butterfly(z + (fr << lg), twiddle, n_fft, sh, bb);
      }
      __syncthreads();
    }
    // the band of frame fr: its lanes take the bins in turns, then a tree over them
    const int fr = tid / lanes_per_frame, sub = tid - fr * lanes_per_frame;
    const float2* __restrict__ zz = z + (fr << lg);
    double acc = 0.0;
    for (int k = a.k_lo + sub; k <= a.k_hi; k += lanes_per_frame) {
      float re, im;
      rfft_unpack_bin(zz, twiddle, M, lg, k, re, im);
      acc = acc + ((double)re * (double)re + (double)im * (double)im);
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = lanes_per_frame >> 1; s > 0; s >>= 1) {
      if (sub < s) red[tid] = red[tid] + red[tid + s];
      __syncthreads();
    }
    if (sub == 0 && g0 + fr < a.frames) a.track[g0 + fr] = (float)red[tid];
    __syncthreads();                                 // stage, z and red are laid down anew
  }
}

// ---- the exact selection -------------------------------------------------------------------------------------------------------------
constexpr uint32_t kSnrNanKey = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t snr_key(float v) { return v != v ? kSnrNanKey : __float_as_uint(v); }

struct SnrDigit {
  unsigned long long scan[2 * 256];
  unsigned long long rank;
  int digit;
};

// Lane t hands in the count of bin t; every lane gets the bin that holds rank r (0 <= r < the sum of the counts) and r becomes the
// rank inside that bin.  An inclusive scan over the 256 bins in eight doubling steps: integers, no order.
__device__ __forceinline__ int snr_digit(unsigned long long count, unsigned long long& r, SnrDigit& sh) {
  const int tid = threadIdx.x;
  __syncthreads();                                   // the digit before may still be read
  sh.scan[tid] = count;
  __syncthreads();
  int src = 0;
  for (int off = 1; off < 256; off <<= 1) {
    const unsigned long long v = sh.scan[src + tid] + (tid >= off ? sh.scan[src + tid - off] : 0ull);
    sh.scan[(src ^ 256) + tid] = v;
    src ^= 256;
    __syncthreads();
  }
  const unsigned long long upto = sh.scan[src + tid], before = upto - count;
  if (before <= r && r < upto) {                     // exactly one lane
    sh.digit = tid;
    sh.rank = r - before;
  }
  __syncthreads();
  r = sh.rank;
  return sh.digit;
}

__global__ __launch_bounds__(kSnrLanes) void snr_select_kernel(const float* __restrict__ track, const long long* __restrict__ uwin,
                                                               const long long* __restrict__ short_list, int n_short, uint32_t* __restrict__ key_out) {
  __shared__ uint32_t keys[kSnrSplit];
  __shared__ uint32_t hist[256];
  __shared__ SnrDigit dg;
  const int tid = threadIdx.x;
  for (int item = blockIdx.x; item < n_short; item += gridDim.x) {
    const long long u = short_list[item];
    const long long w0 = uwin[3 * u];
    const int len = (int)(uwin[3 * u + 1] - w0);     // 1 .. kSnrSplit
    unsigned long long r = (unsigned long long)uwin[3 * u + 2];
    for (int i = tid; i < len; i += kSnrLanes) keys[i] = snr_key(track[w0 + i]);
    uint32_t prefix = 0, mask = 0;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      hist[tid] = 0;
      __syncthreads();                               // (the first pass: the keys are down too)
      for (int i = tid; i < len; i += kSnrLanes) {
        const uint32_t k = keys[i];
        if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
      }
      __syncthreads();
      const int digit = snr_digit(hist[tid], r, dg);
      prefix |= (uint32_t)digit << shift;
      mask |= 255u << shift;
    }
    if (tid == 0) key_out[u] = prefix;
    __syncthreads();                                 // keys and hist are laid down anew
  }
}

__global__ __launch_bounds__(kSnrLanes) void snr_split_pass_kernel(const float* __restrict__ track, const long long* __restrict__ uwin,
                                                                   const long long* __restrict__ long_list, const long long* __restrict__ long_prefix,
                                                                   int n_long, long long total_chunks, int pass,
                                                                   unsigned long long* __restrict__ hist_all) {
  __shared__ uint32_t hist[256];
  __shared__ SnrDigit dg;
  const int tid = threadIdx.x;
  for (long long item = blockIdx.x; item < total_chunks; item += gridDim.x) {
    const int li = segment_of_item(long_prefix, n_long, item);
    const long long u = long_list[li], chunk = item - long_prefix[li];
    const long long w0 = uwin[3 * u], w1 = uwin[3 * u + 1];
    unsigned long long r = (unsigned long long)uwin[3 * u + 2];
    unsigned long long* __restrict__ mine = hist_all + (long long)li * 4 * 256;
    uint32_t prefix = 0, mask = 0;
    for (int q = 0; q < pass; ++q) {                 // the bytes the passes before found
      const int digit = snr_digit(mine[q * 256 + tid], r, dg);
      prefix |= (uint32_t)digit << (24 - 8 * q);
      mask |= 255u << (24 - 8 * q);
    }
    const int shift = 24 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    const long long lo = w0 + chunk * kSnrSplit, hi = min(w1, lo + (long long)kSnrSplit);
    for (long long i = lo + tid; i < hi; i += kSnrLanes) {
      const uint32_t k = snr_key(track[i]);
      if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (hist[tid]) atomicAdd(&mine[pass * 256 + tid], (unsigned long long)hist[tid]);
    __syncthreads();                                 // hist is laid down anew
  }
}

__global__ __launch_bounds__(kSnrLanes) void snr_split_finish_kernel(const long long* __restrict__ uwin, const long long* __restrict__ long_list, int n_long,
                                                                     const unsigned long long* __restrict__ hist_all, uint32_t* __restrict__ key_out) {
  __shared__ SnrDigit dg;
  const int tid = threadIdx.x;
  for (int li = blockIdx.x; li < n_long; li += gridDim.x) {
    const long long u = long_list[li];
    unsigned long long r = (unsigned long long)uwin[3 * u + 2];
    const unsigned long long* __restrict__ mine = hist_all + (long long)li * 4 * 256;
    uint32_t prefix = 0;
    for (int q = 0; q < 4; ++q) prefix |= (uint32_t)snr_digit(mine[q * 256 + tid], r, dg) << (24 - 8 * q);
    if (tid == 0) key_out[u] = prefix;
  }
}

__global__ __launch_bounds__(kSnrRowLanes) void snr_rows_kernel(const float* __restrict__ track, const long long* __restrict__ rows, int n_seg,
                                                                const uint32_t* __restrict__ key, double* __restrict__ out) {
  __shared__ double sum[kSnrRowLanes];
  __shared__ float top[kSnrRowLanes];
  const int tid = threadIdx.x;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
    const long long j0 = rows[3 * (long long)seg], j1 = rows[3 * (long long)seg + 1];
    double s = 0.0;
    float m = __uint_as_float(0xff800000u);          // -inf: a lane without a frame adds nothing to the maximum
    bool any_nan = false;
    for (long long j = j0 + tid; j < j1; j += kSnrRowLanes) {
      const float v = track[j];
      s = s + (double)v;
      any_nan = any_nan || v != v;
      m = fmaxf(m, v);
    }
    sum[tid] = s;
    top[tid] = any_nan ? __uint_as_float(0x7fc00000u) : m;
    __syncthreads();
    for (int h = kSnrRowLanes >> 1; h > 0; h >>= 1) {
      if (tid < h) {
        sum[tid] = sum[tid] + sum[tid + h];
        const float x = top[tid], y = top[tid + h];
        top[tid] = (x != x || y != y) ? __uint_as_float(0x7fc00000u) : fmaxf(x, y);
      }
      __syncthreads();
    }
    if (tid == 0) {
      double* __restrict__ row = out + 3 * (long long)seg;
      if (j1 > j0) {
        const uint32_t k = key[rows[3 * (long long)seg + 2]];
        row[0] = sum[0] / (double)(j1 - j0);
        row[1] = (double)top[0];
        row[2] = k == kSnrNanKey ? nan : (double)__uint_as_float(k);
      } else {                                       // a row without a frame
        row[0] = row[1] = row[2] = nan;
      }
    }
    __syncthreads();                                 // sum and top are laid down anew
  }
}

}  // namespace wseg

using namespace wseg;

extern "C" int64_t wseg_frame_energy_frames(int64_t n, int32_t n_fft) {
  SnrTrackPlan plan;
  char msg[200];
  if (snr_track_plan(n, n_fft, 0, 0, kSnrGridCap, &plan, msg, sizeof(msg))) {
    set_error("wseg_frame_energy_frames: %s", msg);
    return -1;
  }
  return plan.frames;
}

extern "C" int wseg_frame_energy_f32(const float* pcm, int64_t n, int32_t n_fft, int32_t k_lo, int32_t k_hi, const float* window,
                                     const float* twiddle, float* track_out, void* stream_) {
  const char* fn = "wseg_frame_energy_f32";
  hipStream_t stream = (hipStream_t)stream_;
  SnrTrackPlan plan;
  char msg[200];
  if (snr_track_plan(n, n_fft, k_lo, k_hi, grid_cap_env("WSEG_SNR_GRID", kSnrGridCap, kSnrGridCap), &plan, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (plan.frames == 0) return WSEG_OK;
  if (!pcm || ((uintptr_t)pcm & 3)) { set_error("%s: pcm must be a float32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!track_out || ((uintptr_t)track_out & 3)) { set_error("%s: track_out must be a float32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!window || !twiddle || ((uintptr_t)twiddle & 7)) { set_error("%s: window and twiddle (8-byte aligned) must be device pointers", fn); return WSEG_ERR_INVALID; }
  SnrTrackArgs a;
  a.pcm = pcm;
  a.read_end = plan.read_end;
  a.frames = plan.frames;
  a.groups = plan.groups;
  a.n_fft = n_fft;
  a.log2_half = plan.log2_half;
  a.log2_group = plan.log2_group;
  a.k_lo = k_lo;
  a.k_hi = k_hi;
  a.window = window;
  a.twiddle = reinterpret_cast<const float2*>(twiddle);
  a.track = track_out;
  hipLaunchKernelGGL(snr_frames_kernel, dim3((unsigned)plan.grid), dim3(kSnrLanes), 0, stream, a);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}

extern "C" size_t wseg_snr_rows_scratch_bytes(int64_t J, const int64_t* table_host, int32_t n_seg, const int64_t* windows_host, int32_t n_win) {
  SnrRowsPlan plan;
  char msg[200];
  if (snr_rows_plan(J, table_host, n_seg, windows_host, n_win, kSnrGridCap, &plan, nullptr, msg, sizeof(msg))) {
    set_error("wseg_snr_rows_scratch_bytes: %s", msg);
    return 0;
  }
  return (size_t)plan.scratch_bytes;
}

extern "C" int wseg_snr_rows_f64(const float* track, int64_t J, const int64_t* table_host, int32_t n_seg, const int64_t* windows_host, int32_t n_win,
                                 void* scratch, size_t scratch_bytes, double* rows_out, void* stream_) {
  const char* fn = "wseg_snr_rows_f64";
  hipStream_t stream = (hipStream_t)stream_;
  SnrRowsPlan plan;
  char msg[200];
  std::vector<int64_t> table;
  if (snr_rows_plan(J, table_host, n_seg, windows_host, n_win, grid_cap_env("WSEG_SNR_GRID", kSnrGridCap, kSnrGridCap), &plan, &table, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (n_seg == 0) return WSEG_OK;
  if ((J > 0 && !track) || ((uintptr_t)track & 3)) { set_error("%s: track must be a float32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!rows_out || ((uintptr_t)rows_out & 7)) { set_error("%s: rows_out must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < (size_t)plan.scratch_bytes) {
    set_error("%s: scratch must be an 8-byte aligned device buffer of at least %lld bytes (got %zu)", fn, (long long)plan.scratch_bytes, scratch_bytes);
    return WSEG_ERR_INVALID;
  }
  if (const int rc = staging_upload((size_t)plan.table_bytes, scratch, stream, fn,
                                    [&](void* host) { memcpy(host, table.data(), (size_t)plan.table_bytes); }))
    return rc;
  const long long* rows = static_cast<const long long*>(scratch);
  const long long* uwin = rows + 3 * (long long)n_seg;
  const long long* short_list = uwin + 3 * (long long)plan.n_unique;
  const long long* long_list = short_list + plan.n_short;
  const long long* long_prefix = long_list + plan.n_long;
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(static_cast<char*>(scratch) + plan.hist_offset);
  uint32_t* key = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + plan.key_offset);
  if (plan.n_short > 0) {
    hipLaunchKernelGGL(snr_select_kernel, dim3((unsigned)plan.short_grid), dim3(kSnrLanes), 0, stream, track, uwin, short_list, (int)plan.n_short, key);
    WSEG_LAUNCH_CHECK();
  }
  if (plan.n_long > 0) {
    WSEG_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)plan.hist_bytes, stream));
    for (int pass = 0; pass < 4; ++pass) {
      hipLaunchKernelGGL(snr_split_pass_kernel, dim3((unsigned)plan.long_grid), dim3(kSnrLanes), 0, stream, track, uwin, long_list, long_prefix,
                         (int)plan.n_long, (long long)plan.long_chunks, pass, hist);
      WSEG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(snr_split_finish_kernel, dim3((unsigned)plan.finish_grid), dim3(kSnrLanes), 0, stream, uwin, long_list, (int)plan.n_long, hist, key);
    WSEG_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(snr_rows_kernel, dim3((unsigned)plan.rows_grid), dim3(kSnrRowLanes), 0, stream, track, rows, (int)n_seg, key, rows_out);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}
