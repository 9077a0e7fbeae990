// The host arithmetic of the per-segment log-mel patches (wseg_patches_scratch_bytes / wseg_patches_f32), in one place: the
// validation of a call, the work items of patch_frames_kernel, the grids and the layout of the scratch the two kernels of
// wseg_patch.hip share.  Plain C++ with no HIP dependency, so that a host-only program can run it under a sanitizer
// (tools/patch_plan_check.cpp).
//
// A segment [s0, s1) of L = s1 - s0 samples gives `width` frames of n_fft samples, frame c centred on s0 + ((2c + 1) L) / (2 width)
// (whisperseg_amd/patches.py::patches_host).  The frames of a call are numbered g = segment * width + c; a WORK ITEM is
// kPatchFrameSlots / (n_fft / 2) consecutive frames — 16 at n_fft 512, 1 at 8192: what fills the workgroup's 4096 complex points
// of LDS — whatever segments they belong to.  Scratch, in this order:
//   int64    table[n_seg][2]     the segment table, without a prefix (wseg_segments.h)
//   (padded to kPatchAlign bytes, at least one pad)
//   uint32   vmax[n_seg]         the largest log10 mel value of a segment's patch as an ordered uint (zeroed by the call)
//   (padded to kPatchAlign bytes, at least one pad)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "wseg_rfft.h"
#include "wseg_segments.h"

namespace wseg {

constexpr int kPatchFrameSlots = 4096;         // complex points of LDS a workgroup transforms at a time: one 8192-point frame, 16 of 512
constexpr int kPatchMaxWidth = 256;            // columns of a patch
constexpr int kPatchMaxMels = 96;              // filters (the front-end's limit)
constexpr int kPatchAlign = 256;               // bytes
constexpr int kPatchGridCap = 2048;            // workgroups of either kernel: 8 per CU; more items take the grid stride
static_assert((2 * (int64_t)kPatchMaxWidth - 1) * kSegmentMaxSamples < ((int64_t)1 << 62), "(2 c + 1) L of patch_centre stays inside int64");

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

inline int64_t patch_pad(int64_t bytes) { return bytes <= 0 ? kPatchAlign : (bytes + kPatchAlign - 1) / kPatchAlign * kPatchAlign; }

// The sample column c of a patch of `width` columns is centred on, for the segment (s0, L): integer arithmetic only, the very
// expression of the definition and of the kernel.
inline int64_t patch_centre(int64_t s0, int64_t L, int32_t c, int32_t width) { return s0 + ((2 * (int64_t)c + 1) * L) / (2 * (int64_t)width); }

// The part of the plan that needs no bounds: sizes, counts, scratch layout, grids -> 0, or -1 with the argument's name in msg.
inline int patch_plan_sizes(int32_t n_seg, int32_t n_mels, int32_t width, int32_t n_fft, int64_t grid_cap, PatchPlan* plan, char* msg,
                            size_t msg_len) {
  if (rfft_size_check(n_fft, msg, msg_len)) return -1;
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
  p.table_bytes = segment_table_entries(n_seg, false) * 8;
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

// Validates the whole call and fills the plan.  `bounds` is any bounds source of wseg_segments.h, validated against n by segment_check
// -> 0, or -1 with the offending argument's name in msg.  n_seg == 0 is valid: no item, both grids 0.
template <class Bounds>
inline int patch_plan(Bounds bounds, int32_t n_seg, int32_t n_mels, int32_t width, int32_t n_fft, int64_t n, int64_t grid_cap, PatchPlan* plan,
                      char* msg, size_t msg_len) {
  return (patch_plan_sizes(n_seg, n_mels, width, n_fft, grid_cap, plan, msg, msg_len) || segment_check(bounds, n_seg, n, msg, msg_len)) ? -1 : 0;
}

}  // namespace wseg
