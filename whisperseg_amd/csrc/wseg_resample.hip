// Polyphase FIR resampler (rational up/down): y[m] = sum_k h[(m + pre_remove) * down - pre_pad - k * up] * x[k].
// the reference resamples with librosa.load(path, sr=target) before segment()
// (scripts/segment.py:48,61; evaluate.py:58) — an un-pinned third-party resampler.  This kernel implements the standard
// Kaiser-windowed-sinc polyphase structure (filter designed on the host, see whisperseg_amd/resample.py).
// Traffic: 4 B in per input sample + 4 B out per output sample; the taps (<= 35 KiB) stay in L1/L2.  Not HBM-bound, though: one
// lane walks its chain with two dependent-latency global loads per fmaf (measured 0.17-0.47 TB/s of signal moved on an MI355X,
// DESIGN.md §8).  resample_planar_kernel further down stages both operands in LDS; this kernel stays as the arithmetic's definition.
#include "wseg_common.h"
#include "wseg_resample_range.h"

namespace wseg {

__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, long long n_in, const float* __restrict__ h, int n_h,
                                                       int up, int down, int pre_pad, int pre_remove, float* __restrict__ y,
                                                       long long n_out) {
  for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < n_out; m += (long long)gridDim.x * 256) {
    const long long c = (m + pre_remove) * (long long)down - pre_pad;
    long long k_hi = c / up;                       // floor (c >= -pre_pad; handle negatives below)
    if (c < 0) k_hi = -((-c + up - 1) / up);
    long long lo_num = c - n_h + 1;
    long long k_lo = lo_num <= 0 ? 0 : (lo_num + up - 1) / up;
    if (k_hi > n_in - 1) k_hi = n_in - 1;
    float acc = 0.f;
    for (long long k = k_lo; k <= k_hi; ++k) acc = fmaf(h[c - k * up], x[k], acc);
    y[m] = acc;
  }
}


// ---- all planes of a recording in one launch (wseg_resample_planar_f32) -------------------------------------------------------
// resample_kernel above leaves everything to the caches: every x sample is fetched by about n_taps / down lanes and every tap by
// every lane, two global loads per fmaf with the fmaf waiting for both.  Here a workgroup takes a TILE of consecutive outputs of
// one plane; the tile's input window — k_lo of its first output to k_hi of its last — comes into LDS once (16-byte loads on the
// plane's own 16-byte grid, dword loads at the two ragged ends), and the taps are copied to LDS once per workgroup when they fit,
// PHASE-MAJOR: tw[c mod up][j] = h[c mod up + j * up], a lane walks one row, and the rows are padded to an odd length so that
// the lanes' rows start on different banks.  The grid is capped, so a workgroup stages the table once for the several tiles it
// takes.  A table that does not fit is read from global memory in h's own order, as resample_kernel reads it: at one step of the
// chain all lanes read inside one stretch of `up` floats (c - k_lo * up lies in (n_taps - 1 - up, n_taps - 1]), a dozen cache lines,
// where a phase-major table in global memory scatters the 64 lanes of a wave over 64 lines (measured: 2.7 times slower than
// resample_kernel at 250 k -> 44.1 k, profiles/resample_planar_ab.txt).  Each output is resample_kernel's fmaf chain — same c, k_lo,
// k_hi, same order, nothing multiplied outside [k_lo, k_hi] — hence the same bits, whichever of the four variants runs.
// The kernel takes a RANGE of outputs and a SEGMENT of each plane (wseg_resample_planar_range_f32): x points at input sample x_first of
// plane 0, the tiles are cut from m_first on, and n_in — the recording's length — still enters only as the clamp of k_hi.  The host
// has checked that every chain of the range lies inside the segment; a tile's window is k_lo of its first output to k_hi of its last,
// so no load — the 16-byte ones included, which are taken only where all four floats lie inside the window, on the 16-byte grid of
// the ADDRESS, whatever the segment's alignment — leaves the segment.  A file resampled piece by piece (wavio.StreamResampler) is a
// sequence of such calls; the whole-recording call is the range [0, n_out) over the segment [0, n_in).
constexpr int kResampleMaxTile = 1024;             // outputs per tile, at most (a multiple of 64)
constexpr int kResampleWindowMax = 4096;           // floats of a staged input window (16 KiB)
constexpr int kResampleTapsMax = 10240;            // floats of a staged tap table, padded rows included (40 KiB)
constexpr int kResampleGridCap = 2048;             // 8 workgroups per CU; more tiles take the grid stride (resample.PLANAR_GRID_CAP)

struct ResamplePlan {
  int tile, window, x_staged, taps_staged, row, row_lds;
  size_t lds_bytes;
};

// Host arithmetic of the launch, a function of the ratio and the filter length alone.
static ResamplePlan resample_plan(int n_taps, int up, int down) {
  ResamplePlan p;
  p.row = (n_taps + up - 1) / up;                  // taps of a phase
  p.row_lds = p.row | 1;
  p.taps_staged = (long long)up * p.row_lds <= kResampleTapsMax;
  auto window = [&](int t) { return ((long long)(t - 1) * down + up - 1) / up + p.row + 2; };
  p.tile = kResampleMaxTile;                       // whole passes of the 256 lanes while they fit, then 192 / 128 / 64
  while (p.tile > 64 && window(p.tile) > kResampleWindowMax) p.tile -= p.tile > 256 ? 256 : 64;
  p.x_staged = window(p.tile) <= kResampleWindowMax;
  if (!p.x_staged) p.tile = 256;                   // one output per lane, x read from global memory
  p.window = (int)(p.x_staged ? window(p.tile) : 0);
  // the staged window starts on the 16-byte grid of its plane: up to 3 floats in front, rounded up to whole groups of four
  p.lds_bytes = (p.x_staged ? (size_t)((p.window + 3 + 3) / 4 * 4) * 4 : 0) + (p.taps_staged ? (size_t)up * p.row_lds * 4 : 0);
  return p;
}

template <bool XS, bool TS>
__global__ __launch_bounds__(256) void resample_planar_kernel(const float* __restrict__ x, long long x_first, long long n_in, long long x_stride,
                                                              int n_planes, const float* __restrict__ h, int n_h, int row_lds, int up,
                                                              int down, int pre_pad, int pre_remove, float* __restrict__ y,
                                                              long long m_first, long long m_count, long long y_stride, int tile,
                                                              int window_floats) {
  extern __shared__ float4 resample_lds[];
  float* xw = reinterpret_cast<float*>(resample_lds);
  float* tw = xw + window_floats;
  const int tid = threadIdx.x;
  if constexpr (TS) {
    for (int i = tid; i < n_h; i += 256) {
      const int j = i / up;
      tw[(i - j * up) * row_lds + j] = h[i];
    }
  }
  const long long n_tiles = (m_count + tile - 1) / tile;
  const long long n_items = n_tiles * n_planes;
  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const long long plane = item / n_tiles;
    const long long t0 = (item - plane * n_tiles) * tile;
    const long long m0 = m_first + t0;
    const int n_tile = (int)min((long long)tile, m_count - t0);
    const float* __restrict__ xp = x + plane * x_stride - x_first;      // xp[k] is input sample k, for the k of the segment
    float* __restrict__ yp = y + plane * y_stride;
    long long s0 = 0;                              // the input sample at xw[0]
    if constexpr (XS) {
      const long long w0 = resample_range(m0, n_in, n_h, up, down, pre_pad, pre_remove).k_lo;
      const long long w1 = resample_range(m0 + n_tile - 1, n_in, n_h, up, down, pre_pad, pre_remove).k_hi;
      s0 = w0 - (long long)(((uintptr_t)(xp + w0) >> 2) & 3);
      const int groups = w1 >= w0 ? (int)((w1 - s0) / 4 + 1) : 0;
      __syncthreads();                             // the tile before has been computed (and, the first time, nothing: harmless)
      for (int g = tid; g < groups; g += 256) {
        const long long k = s0 + 4 * g;
        if (k >= w0 && k + 3 <= w1) {
          reinterpret_cast<float4*>(xw)[g] = *reinterpret_cast<const float4*>(xp + k);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) xw[4 * g + i] = (k + i >= w0 && k + i <= w1) ? xp[k + i] : 0.f;
        }
      }
    }
    __syncthreads();                               // the window (and, the first time, the taps) are in place
    for (int o = tid; o < n_tile; o += 256) {
      const ResampleRange r = resample_range(m0 + o, n_in, n_h, up, down, pre_pad, pre_remove);
      float acc = 0.f;
      if (r.k_hi >= r.k_lo) {
        const int n = (int)(r.k_hi - r.k_lo + 1);
        const float* __restrict__ xs = XS ? xw + (int)(r.k_lo - s0) : xp + r.k_lo;
        // tap c - k * up of the chain's first k, and the step to the next: row c mod up of the staged table, backwards from
        // column k_c - k_lo, or h itself
        const int ph = (int)(r.c - r.k_c * up);
        const float* __restrict__ t = TS ? tw + ph * row_lds + (int)(r.k_c - r.k_lo) : h + (r.c - r.k_lo * up);
        const int step = TS ? 1 : up;
        for (int i = 0; i < n; ++i, t -= step) acc = fmaf(*t, xs[i], acc);
      }
      yp[m0 + o] = acc;
    }
  }
}

}  // namespace wseg

using namespace wseg;

extern "C" int wseg_resample_f32(const float* x, int64_t n_in, const float* taps, int32_t n_taps, int32_t up, int32_t down,
                                 int32_t pre_pad, int32_t pre_remove, float* y, int64_t n_out, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (!x || !taps || !y || n_in < 0 || n_out < 0 || up <= 0 || down <= 0 || n_taps <= 0) { set_error("wseg_resample_f32: bad argument"); return WSEG_ERR_INVALID; }
  if (n_out == 0) return WSEG_OK;
  long long blocks = (n_out + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, (long long)n_in, taps, n_taps, up, down, pre_pad,
                     pre_remove, y, (long long)n_out);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}

static int resample_check(const char* who, int64_t n_in, int64_t n_out, int32_t n_taps, int32_t up, int32_t down, int32_t pre_pad,
                          int32_t pre_remove) {
  if (n_in < 0 || n_out < 0 || up <= 0 || down <= 0 || n_taps <= 0 || pre_pad < 0 || pre_remove < 0) {
    set_error("%s: n_in, n_out, pre_pad and pre_remove must not be negative; up, down and n_taps must be positive", who);
    return WSEG_ERR_INVALID;
  }
  return WSEG_OK;
}

extern "C" int wseg_debug_resample_plan(int64_t n_in, int64_t n_out, int32_t n_taps, int32_t up, int32_t down, int32_t pre_pad,
                                        int32_t pre_remove, int32_t* tile, int32_t* window, int32_t* x_staged, int32_t* taps_staged) {
  if (int e = resample_check("wseg_debug_resample_plan", n_in, n_out, n_taps, up, down, pre_pad, pre_remove)) return e;
  if (!tile || !window || !x_staged || !taps_staged) { set_error("wseg_debug_resample_plan: null result pointer"); return WSEG_ERR_INVALID; }
  const ResamplePlan p = resample_plan(n_taps, up, down);
  *tile = p.tile; *window = p.window; *x_staged = p.x_staged; *taps_staged = p.taps_staged;
  return WSEG_OK;
}

// The range call under the name of the entry point that was called: every check, then the launch.
static int resample_planar_range(const char* who, const float* x, int64_t x_first, int64_t x_frames, int64_t x_plane_stride, int32_t n_planes,
                                 int64_t n_in, const float* taps, int32_t n_taps, int32_t up, int32_t down, int32_t pre_pad,
                                 int32_t pre_remove, float* y, int64_t m_first, int64_t m_count, int64_t y_plane_stride, hipStream_t s) {
  if (!x || !taps || !y || (((uintptr_t)x | (uintptr_t)taps | (uintptr_t)y) & 3)) {
    set_error("%s: x, taps and y must be float32 device pointers", who); return WSEG_ERR_INVALID;
  }
  if (int e = resample_check(who, n_in, 0, n_taps, up, down, pre_pad, pre_remove)) return e;
  if (n_planes < 1 || n_planes > 64) { set_error("%s: n_planes must be 1..64 (got %d)", who, n_planes); return WSEG_ERR_INVALID; }
  char why[256];
  if (resample_range_check(x_first, x_frames, n_in, n_taps, up, down, pre_pad, pre_remove, m_first, m_count, why, sizeof(why))) {
    set_error("%s: %s", who, why); return WSEG_ERR_INVALID;
  }
  // y is the base of the whole output: its planes are at least as long as the last output written
  if (n_planes > 1 && (x_plane_stride < x_frames || y_plane_stride < m_first + m_count)) {
    set_error("%s: plane strides (%lld, %lld) are shorter than the planes (%lld, %lld)", who, (long long)x_plane_stride,
              (long long)y_plane_stride, (long long)x_frames, (long long)(m_first + m_count));
    return WSEG_ERR_INVALID;
  }
  if (m_count == 0) return WSEG_OK;
  const long long xs = n_planes > 1 ? x_plane_stride : 0, ys = n_planes > 1 ? y_plane_stride : 0;
  if (n_in == 0) {                                 // no sample, no chain: zeros, without a kernel
    for (int p = 0; p < n_planes; ++p) WSEG_HIP_CHECK(hipMemsetAsync(y + (size_t)p * ys + m_first, 0, (size_t)m_count * 4, s));
    return WSEG_OK;
  }
  const ResamplePlan p = resample_plan(n_taps, up, down);
  const long long items = (m_count + p.tile - 1) / p.tile * n_planes;
  const dim3 grid((unsigned)(items < kResampleGridCap ? items : kResampleGridCap));
  const int window_floats = p.x_staged ? (p.window + 3 + 3) / 4 * 4 : 0;
#define WSEG_RESAMPLE(XS, TS) hipLaunchKernelGGL((resample_planar_kernel<XS, TS>), grid, dim3(256), p.lds_bytes, s, x, (long long)x_first,     \
                                                 (long long)n_in, xs, (int)n_planes, taps, (int)n_taps, p.row_lds, (int)up, (int)down,        \
                                                 (int)pre_pad, (int)pre_remove, y, (long long)m_first, (long long)m_count, ys, p.tile,        \
                                                 window_floats)
  if (p.x_staged && p.taps_staged) WSEG_RESAMPLE(true, true);
  else if (p.x_staged) WSEG_RESAMPLE(true, false);
  else if (p.taps_staged) WSEG_RESAMPLE(false, true);
  else WSEG_RESAMPLE(false, false);
#undef WSEG_RESAMPLE
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}

extern "C" int wseg_resample_planar_range_f32(const float* x, int64_t x_first, int64_t x_frames, int64_t x_plane_stride, int32_t n_planes,
                                              int64_t n_in, const float* taps, int32_t n_taps, int32_t up, int32_t down, int32_t pre_pad,
                                              int32_t pre_remove, float* y, int64_t m_first, int64_t m_count, int64_t y_plane_stride,
                                              void* stream_) {
  return resample_planar_range("wseg_resample_planar_range_f32", x, x_first, x_frames, x_plane_stride, n_planes, n_in, taps, n_taps, up, down,
                               pre_pad, pre_remove, y, m_first, m_count, y_plane_stride, (hipStream_t)stream_);
}

// The whole recording: the range [0, n_out) over the segment [0, n_in).
extern "C" int wseg_resample_planar_f32(const float* x, int64_t n_in, int64_t x_plane_stride, int32_t n_planes, const float* taps,
                                        int32_t n_taps, int32_t up, int32_t down, int32_t pre_pad, int32_t pre_remove, float* y,
                                        int64_t n_out, int64_t y_plane_stride, void* stream_) {
  return resample_planar_range("wseg_resample_planar_f32", x, 0, n_in, x_plane_stride, n_planes, n_in, taps, n_taps, up, down, pre_pad,
                               pre_remove, y, 0, n_out, y_plane_stride, (hipStream_t)stream_);
}
