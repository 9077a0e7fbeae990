// The host arithmetic of the per-segment log-mel patches (wseg_patches_scratch_bytes / wseg_patches_f32), in one place: the
// validation of a call, the work items of patch_frames_kernel, the grids and the layout of the scratch the two kernels of
// wseg_patch.hip share.  Plain C++ with no HIP dependency, so that a host-only program can run it under a sanitizer
// (tools/patch_plan_check.cpp).
//
// A segment [s0, s1) of L = s1 - s0 samples gives `width` frames of n_fft samples, frame c centred on s0 + ((2c + 1) L) / (2 width)
// (whisperseg_amd/patches.py::patches_host).  The frames of a call are numbered g = segment * width + c; a WORK ITEM is
// kPatchFrameSlots / (n_fft / 2) consecutive frames — 16 at n_fft 512, 1 at 8192: what fills the workgroup's 4096 complex points
// of LDS — whatever segments they belong to.  Scratch, in this order:
//   int64    table[n_seg][2]     s0 and L of every segment
//   (padded to kPatchAlign bytes, at least one pad)
//   uint32   vmax[n_seg]         the largest log10 mel value of a segment's patch as an ordered uint (zeroed by the call)
//   (padded to kPatchAlign bytes, at least one pad)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace wseg {

constexpr int kPatchFrameSlots = 4096;         // complex points of LDS a workgroup transforms at a time: one 8192-point frame, 16 of 512
constexpr int kPatchMaxWidth = 256;            // columns of a patch
constexpr int kPatchMaxMels = 96;              // filters (the front-end's limit)
constexpr int kPatchAlign = 256;               // bytes
constexpr int kPatchGridCap = 2048;            // workgroups of either kernel: 8 per CU; more items take the grid stride
constexpr int64_t kPatchMaxSamples = (int64_t)1 << 52;      // of a recording: (2 c + 1) L <= 511 * 2^52 < 2^61

struct PatchPlan {
  int32_t n_fft, n_mels, width, n_seg;
  int32_t frames_per_item;         // kPatchFrameSlots / (n_fft / 2)
  int64_t total_frames;            // n_seg * width                          (< 2^39)
  int64_t total_items;             // ceil(total_frames / frames_per_item)
  int64_t total_values;            // n_seg * n_mels * width floats of out   (< 2^46)
  int64_t table_bytes;             // 16 n_seg
  int64_t vmax_offset;             // table_bytes rounded up to kPatchAlign (at least kPatchAlign)
  int64_t vmax_bytes;              // 4 n_seg
  int64_t scratch_bytes;           // vmax_offset + vmax_bytes rounded up to kPatchAlign (at least kPatchAlign)
  int32_t grid;                    // workgroups of patch_frames_kernel (0: no segment)
  int32_t finish_grid;             // workgroups of patch_finish_kernel, kPatchFinishPerGroup values a round
};

constexpr int kPatchFinishPerGroup = 1024;     // values a workgroup of patch_finish_kernel normalises per round (256 lanes x 4)

inline bool patch_n_fft_ok(int32_t n_fft) { return n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096 || n_fft == 8192; }
inline int64_t patch_pad(int64_t bytes) { return bytes <= 0 ? kPatchAlign : (bytes + kPatchAlign - 1) / kPatchAlign * kPatchAlign; }

// The sample column c of a patch of `width` columns is centred on, for the segment (s0, L): integer arithmetic only, the very
// expression of the definition and of the kernel.
inline int64_t patch_centre(int64_t s0, int64_t L, int32_t c, int32_t width) { return s0 + ((2 * (int64_t)c + 1) * L) / (2 * (int64_t)width); }

// The part of the plan that needs no bounds: sizes, counts, scratch layout, grids -> 0, or -1 with the argument's name in msg.
inline int patch_plan_sizes(int32_t n_seg, int32_t n_mels, int32_t width, int32_t n_fft, int64_t grid_cap, PatchPlan* plan, char* msg,
                            size_t msg_len) {
  if (!patch_n_fft_ok(n_fft)) { snprintf(msg, msg_len, "n_fft must be 512, 1024, 2048, 4096 or 8192 (got %d)", (int)n_fft); return -1; }
  if (n_mels < 1 || n_mels > kPatchMaxMels) { snprintf(msg, msg_len, "n_mels must be 1 .. %d (got %d)", kPatchMaxMels, (int)n_mels); return -1; }
  if (width < 1 || width > kPatchMaxWidth) { snprintf(msg, msg_len, "width must be 1 .. %d (got %d)", kPatchMaxWidth, (int)width); return -1; }
  if (n_seg < 0) { snprintf(msg, msg_len, "n_seg is negative (%d)", (int)n_seg); return -1; }
  PatchPlan p;
  p.n_fft = n_fft;
  p.n_mels = n_mels;
  p.width = width;
  p.n_seg = n_seg;
  p.frames_per_item = kPatchFrameSlots / (n_fft / 2);
  p.total_frames = (int64_t)n_seg * width;
  p.total_items = (p.total_frames + p.frames_per_item - 1) / p.frames_per_item;
  p.total_values = p.total_frames * n_mels;
  p.table_bytes = 16 * (int64_t)n_seg;
  p.vmax_offset = patch_pad(p.table_bytes);
  p.vmax_bytes = 4 * (int64_t)n_seg;
  p.scratch_bytes = p.vmax_offset + patch_pad(p.vmax_bytes);
  if (grid_cap < 1) grid_cap = 1;
  const int64_t rounds = (p.total_values + kPatchFinishPerGroup - 1) / kPatchFinishPerGroup;
  p.grid = (int32_t)(p.total_items < grid_cap ? p.total_items : grid_cap);
  p.finish_grid = (int32_t)(rounds < grid_cap ? rounds : grid_cap);
  *plan = p;
  return 0;
}

// Validates the whole call and fills the plan.  `bounds(i, &s0, &s1)` yields segment i (an array in the library, a synthetic
// sequence in the check program: 2^31 - 1 segments need no 32 GiB); every segment must satisfy 0 <= s0 <= s1 <= n, n <= 2^52
// (n < 0: no recording length is known, s1 <= 2^52).  Where `table` is given (2 n_seg entries) it receives s0 and L of every
// segment -> 0, or -1 with the offending argument's name in msg.  n_seg == 0 is valid: no item, both grids 0.
template <class Bounds>
inline int patch_plan(Bounds bounds, int32_t n_seg, int32_t n_mels, int32_t width, int32_t n_fft, int64_t n, int64_t grid_cap, PatchPlan* plan,
                      int64_t* table, char* msg, size_t msg_len) {
  if (patch_plan_sizes(n_seg, n_mels, width, n_fft, grid_cap, plan, msg, msg_len)) return -1;
  if (n > kPatchMaxSamples) { snprintf(msg, msg_len, "n must be at most 2^52 samples (got %lld)", (long long)n); return -1; }
  const int64_t limit = n < 0 ? kPatchMaxSamples : n;
  for (int32_t i = 0; i < n_seg; ++i) {
    int64_t s0, s1;
    bounds(i, &s0, &s1);
    if (s0 < 0 || s1 < s0 || s1 > limit) {
      snprintf(msg, msg_len, "bounds of segment %d must satisfy 0 <= s0 <= s1 <= %lld (got %lld, %lld)", (int)i, (long long)limit,
               (long long)s0, (long long)s1);
      return -1;
    }
    if (table) {
      table[2 * (int64_t)i] = s0;
      table[2 * (int64_t)i + 1] = s1 - s0;
    }
  }
  return 0;
}

// bounds[n_seg][2] as the library gets them
struct PatchBoundsArray {
  const int64_t* p;
  void operator()(int32_t i, int64_t* s0, int64_t* s1) const { *s0 = p[2 * (int64_t)i]; *s1 = p[2 * (int64_t)i + 1]; }
};

}  // namespace wseg
