// Per-segment log-mel patches from the resident PCM (wseg_patches_f32): for every row a segmenter returns, one picture of
// n_mels x width values — `width` frames at the segment's own spacing, frame c centred on s0 + ((2c + 1) L) / (2 width), through
// periodic Hann -> |rfft|^2 -> the front-end's Slaney bank -> log10 -> the front-end's per-picture normalisation
// (max(v, V - 8) + 4) / 4 with V the picture's maximum.  whisperseg_amd/patches.py::patches_host is the definition, in float64;
// this file computes the FFT and the mel projection in fp32, every sum in a fixed order: the same input gives the same bits on
// every run, for every grid size and for a segment whatever other segments share the call.  The only atomic is the ordered-uint
// maximum of a picture (a maximum has no order).  No inline assembly; the front-end's and the measurements' kernels are left alone.
//
// patch_frames_kernel   the frames of a call are numbered g = segment * width + c and a work item is F = 4096 / (n_fft / 2)
//   consecutive frames (16 at n_fft 512 .. 1 at 8192; wseg_patch_plan.h), so that a workgroup of 256 lanes always transforms 4096
//   complex points of LDS (32 KiB) at a time and no lane idles in a butterfly pass — the work item is finer than a segment, one
//   long segment at width 256 spreads over the grid.  The grid is capped and strides over the items.  Per item: F lanes work out
//   their frame's segment, column and centre (int64, the only divisions); the frames are laid down windowed as n_fft / 2 complex
//   points z[m] = x[2m] + i x[2m + 1] with every index outside [0, n) read as zero — one guard, no sample outside the recording
//   is loaded; the real FFT of wseg_rfft.h, F frames side by side: a decimation-in-frequency pass per power of two (2048
//   butterflies a pass, 8 a lane) leaves Z bit-reversed and the unpack step reads Z[k], Z[M - k] through the bit reversal;
//   |X[k]|^2 goes to a second LDS array (F rows of n_fft / 2 + 1 floats: an odd stride, so lanes on consecutive frames of one
//   filter hit distinct banks); lane (filter m, frame) then walks the filter's contiguous bins with one fmaf chain, writes log10
//   into out[segment][m][c] and keeps the frame's maximum, which the workgroup folds to ONE atomic per frame.
//   Twiddles, window and the bank are read from global memory, where every item of every workgroup finds them in cache.
//   LDS: 32 KiB + 16.1 KiB + 1.3 KiB = 49.4 KiB, three workgroups a CU.
// patch_finish_kernel   normalises the written values in place from the segment's maximum: elementwise, grid-stride.
#include "wseg_common.h"
#include "wseg_patch_plan.h"
#include "wseg_staging.h"

namespace wseg {

constexpr int kPatchLanes = 256;
constexpr int kPatchMaxFrames = kPatchFrameSlots / 256;      // 16: frames of an item at the smallest transform (n_fft 512)

struct PatchArgs {
  wseg_logmel_desc d;              // hop and n_cols are not read
  const float* pcm;
  long long n;
  const long long* table;          // [n_seg][2]: s0, s1 (wseg_segments.h)
  int width;
  int log2_half;                   // n_fft / 2 = 2^log2_half
  int log2_fpi;                    // frames per item = 2^log2_fpi
  long long total_frames, total_items;
  float* out;                      // [n_seg][n_mels][width]
  uint32_t* vmax;                  // [n_seg] ordered uint, zeroed
};

__global__ __launch_bounds__(kPatchLanes) void patch_frames_kernel(PatchArgs a) {
  __shared__ float2 z[kPatchFrameSlots];
  __shared__ float pw[kPatchFrameSlots + kPatchMaxFrames];      // F rows of M + 1
  __shared__ float red[kPatchLanes];
  __shared__ long long f_base[kPatchMaxFrames];                 // sample index of point 0 of the frame (may be negative)
  __shared__ long long f_out[kPatchMaxFrames];                  // offset of out[segment][0][c], -1: no such frame
  __shared__ int f_seg[kPatchMaxFrames];
  const int tid = threadIdx.x;
  const int n_fft = a.d.n_fft, M = n_fft >> 1, lg = a.log2_half, n_mels = a.d.n_mels, W = a.width;
  const int F = 1 << a.log2_fpi;
  const float* __restrict__ window = a.d.window;
  const float2* __restrict__ twiddle = reinterpret_cast<const float2*>(a.d.twiddle);
  float* const zf = reinterpret_cast<float*>(z);
  for (long long item = blockIdx.x; item < a.total_items; item += gridDim.x) {
    if (tid < F) {
      const long long g = item * F + tid;
      if (g < a.total_frames) {
        const long long seg = g / W;
        const long long c = g - seg * W;
        const long long s0 = a.table[2 * seg], L = a.table[2 * seg + 1] - s0;
        f_base[tid] = s0 + ((2 * c + 1) * L) / (2 * (long long)W) - M;
        f_out[tid] = seg * n_mels * W + c;
        f_seg[tid] = (int)seg;
      } else {                                       // behind the last frame of the call: every index is in front of the recording
        f_base[tid] = -(long long)n_fft;
        f_out[tid] = -1;
        f_seg[tid] = 0;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < 2 * kPatchFrameSlots; idx += kPatchLanes) {
      const int fr = idx >> (lg + 1), i = idx & (n_fft - 1);
      const long long p = f_base[fr] + i;
      zf[idx] = (p >= 0 && p < a.n) ? a.pcm[p] * window[i] : 0.0f;
    }
    __syncthreads();
    for (int sh = lg - 1; sh >= 0; --sh) {           // decimation in frequency: half-size 2^sh from M / 2 down to 1; butterfly bb of frame fr
      for (int b = tid; b < kPatchFrameSlots / 2; b += kPatchLanes) {
        const int fr = b >> (lg - 1), bb = b & ((M >> 1) - 1);
        rfft_dif_butterfly(z + (fr << lg), twiddle, n_fft, sh, bb);
      }
      __syncthreads();
    }
    // |X[k]|^2;  the lane of k = 0 also writes k = M
    for (int idx = tid; idx < kPatchFrameSlots; idx += kPatchLanes) {
      const int fr = idx >> lg, k = idx & (M - 1);
      const float2* __restrict__ zz = z + (fr << lg);
      float* __restrict__ pp = pw + fr * (M + 1);
      float re, im;                                  // (bins 0 and M: im = 0, and adding + 0 to a square changes no bit)
      __builtin_assume(k != M);                      // (k < M: the unpack's test for bin M is dead here)
      rfft_unpack_bin(zz, twiddle, M, lg, k, re, im);
      pp[k] = re * re + im * im;
      if (k == 0) {
        rfft_unpack_bin(zz, twiddle, M, lg, M, re, im);
        pp[M] = re * re + im * im;
      }
    }
    __syncthreads();
    // mel projection + log10: lane = (filter, frame), consecutive lanes on consecutive frames = consecutive columns of one output row.
    // 256 is a multiple of F, so a lane keeps its frame over the rounds and its running maximum is that frame's.
    float vmx = -3.0e38f;
    for (int idx = tid; idx < (n_mels << a.log2_fpi); idx += kPatchLanes) {
      const int m = idx >> a.log2_fpi, fr = idx & (F - 1);
      const long long o = f_out[fr];
      if (o >= 0) {
        const int k0 = min(max(a.d.mel_start[m], 0), M);
        const int cnt = min(a.d.mel_count[m], M + 1 - k0);      // the bank is the caller's: never past the spectrum
        const float* __restrict__ wt = a.d.mel_weight + a.d.mel_offset[m];
        const float* __restrict__ p = pw + fr * (M + 1) + k0;
        float acc = 0.0f;
        for (int k = 0; k < cnt; ++k) acc = fmaf(wt[k], p[k], acc);
        // mel floor: max(1e-10, x) then log10; log10(1e-10) is exactly -10 (as the front-end's kernels)
        const float v = acc > 1e-10f ? log10f(acc) : -10.0f;
        a.out[o + (long long)m * W] = v;
        vmx = fmaxf(vmx, v);
      }
    }
    red[tid] = vmx;
    __syncthreads();
    if (tid < F && f_out[tid] >= 0) {
      float v = red[tid];
      for (int j = tid + F; j < kPatchLanes; j += F) v = fmaxf(v, red[j]);
      atomicMax(&a.vmax[f_seg[tid]], f2ord(v));
    }
    __syncthreads();                                 // the frame table, z, pw and red are laid down anew
  }
}

// out = (max(out, V - 8) + 4) / 4 in place, V the maximum of the value's segment; a round of a workgroup is 4 x 256 consecutive values
__global__ __launch_bounds__(kPatchLanes) void patch_finish_kernel(const uint32_t* __restrict__ vmax, float* __restrict__ out, long long total_values,
                                                                   int per_segment) {
  for (long long base = (long long)blockIdx.x * kPatchFinishPerGroup; base < total_values; base += (long long)gridDim.x * kPatchFinishPerGroup) {
#pragma unroll
    for (int u = 0; u < kPatchFinishPerGroup / kPatchLanes; ++u) {
      const long long idx = base + u * kPatchLanes + threadIdx.x;
      if (idx < total_values) {
        const float floorv = ord2f(vmax[idx / per_segment]) - 8.0f;
        out[idx] = (fmaxf(out[idx], floorv) + 4.0f) / 4.0f;
      }
    }
  }
}

}  // namespace wseg

using namespace wseg;

extern "C" size_t wseg_patches_scratch_bytes(int32_t n_seg, int32_t n_mels, int32_t width) {
  PatchPlan plan;
  char msg[200];
  if (patch_plan_sizes(n_seg, n_mels, width, 512, kPatchGridCap, &plan, msg, sizeof(msg))) {      // (the scratch does not depend on n_fft)
    set_error("wseg_patches_scratch_bytes: %s", msg);
    return 0;
  }
  return (size_t)plan.scratch_bytes;
}

extern "C" int wseg_patches_f32(const wseg_logmel_desc* d, const float* pcm, int64_t n, const int64_t* bounds_host, int32_t n_seg, int32_t width,
                                void* scratch, size_t scratch_bytes, float* out, void* stream_) {
  const char* fn = "wseg_patches_f32";
  hipStream_t stream = (hipStream_t)stream_;
  if (!d) { set_error("%s: d is null", fn); return WSEG_ERR_INVALID; }
  if (n < 0) { set_error("%s: n is negative", fn); return WSEG_ERR_INVALID; }
  if (n_seg > 0 && !bounds_host) { set_error("%s: bounds_host is null for n_seg = %d", fn, (int)n_seg); return WSEG_ERR_INVALID; }
  PatchPlan plan;
  char msg[200];
  if (patch_plan(SegmentBoundsArray{bounds_host}, n_seg, d->n_mels, width, d->n_fft, n, grid_cap_env("WSEG_PATCH_GRID", kPatchGridCap, 65535), &plan, msg,
                 sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (n_seg == 0) return WSEG_OK;
  if (!d->window || !d->twiddle || ((uintptr_t)d->twiddle & 7) || !d->mel_start || !d->mel_count || !d->mel_offset || !d->mel_weight) {
    set_error("%s: d must hold device pointers to window, twiddle (8-byte aligned) and the four mel tables", fn);
    return WSEG_ERR_INVALID;
  }
  if (const int rc = device_buffers_check(fn, pcm, n, out, scratch, scratch_bytes, plan.scratch_bytes)) return rc;
  if (const int rc = staging_upload((size_t)plan.table_bytes, scratch, stream, fn,
                                    [&](void* host) { segment_table_fill(host, bounds_host, n_seg, nullptr); }))
    return rc;
  PatchArgs a;
  a.d = *d;
  a.pcm = pcm;
  a.n = n;
  a.table = static_cast<const long long*>(scratch);
  a.width = width;
  a.log2_half = rfft_log2_half(d->n_fft);
  a.log2_fpi = 0;
  while ((1 << a.log2_fpi) < plan.frames_per_item) ++a.log2_fpi;
  a.total_frames = plan.total_frames;
  a.total_items = plan.total_items;
  a.out = out;
  a.vmax = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + plan.vmax_offset);
  WSEG_HIP_CHECK(hipMemsetAsync(a.vmax, 0, (size_t)plan.vmax_bytes, stream));      // the lowest ordered value
  hipLaunchKernelGGL(patch_frames_kernel, dim3((unsigned)plan.grid), dim3(kPatchLanes), 0, stream, a);
  WSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(patch_finish_kernel, dim3((unsigned)plan.finish_grid), dim3(kPatchLanes), 0, stream, a.vmax, out, (long long)plan.total_values,
                     (int)(plan.n_mels * plan.width));
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}
