// The host arithmetic of the per-segment pitch contour (wseg_pitch_scratch_bytes / wseg_pitch_frames_f64), in one place: the
// validation of a call, the frame count of every segment, the launch geometry and the layout of the scratch pitch_frame_kernel
// reads its table from.  Plain C++ with no HIP dependency, so that a host-only program can run it under a sanitizer
// (tools/pitch_plan_check.cpp).
//
// A segment [s0, s1) of len = s1 - s0 samples is cut into frames of 2 tau_max samples, hop apart, the first at s0, every one of
// them wholly inside the segment:
//   J = 0 for len < 2 tau_max, else 1 + (len - 2 tau_max) / hop                          (whisperseg_amd/pitch.py::frame_count)
// A frame is a work item.  Scratch:
//   int64  table[3 n_seg + 1]     the segment table with the exclusive prefix of the frame counts (wseg_segments.h)
//   (padded to kPitchAlign bytes)
// A lane of the kernel owns kPitchLagsPerLane consecutive lags at a time ("a group": lags 4 g + 1 .. 4 g + 4); the workgroup is the
// smallest power of two of lanes, 64 .. 256, that gives every group of tau_max a lane, or 256 lanes that take the groups in turns.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "wseg_segments.h"

namespace wseg {

constexpr int kPitchMaxLag = 2048;             // the largest tau_max: the frame (2 tau_max float32) then fills 16 KiB of LDS (pitch.py::MAX_LAG)
constexpr int kPitchBlock = 64;                // lags per block of the two-level prefix sum (pitch.py::BLOCK)
constexpr int kPitchMaxBlocks = kPitchMaxLag / kPitchBlock;      // 32
constexpr int kPitchLagsPerLane = 4;           // consecutive lags a lane carries through one pass over the frame
constexpr int kPitchMaxLanes = 256;
constexpr int kPitchAlign = 256;               // bytes the scratch is padded to
constexpr int kPitchGridCap = 2048;            // workgroups: 8 per CU; more frames take the grid stride
constexpr int64_t kPitchMaxFrames = (int64_t)1 << 40;        // of one call, all segments together (2^40 * 12 bytes of output)

struct PitchPlan {
  int32_t tau_max, hop;
  int32_t n_seg;
  int32_t lanes;                   // of a workgroup: 64, 128 or 256
  int32_t groups;                  // ceil(tau_max / 4): the lag groups of a frame
  int32_t blocks;                  // ceil(tau_max / 64): the blocks of the prefix sum
  int64_t total_frames;            // over all segments
  int64_t table_bytes;             // (3 n_seg + 1) int64
  int64_t scratch_bytes;           // table_bytes rounded up to kPitchAlign
  int64_t out_floats;              // 3 total_frames
  int32_t grid;                    // workgroups (0: no frame at all)
};

// Frames of a segment of len samples (len >= 0; tau_max, hop >= 1).
inline int64_t pitch_frames(int64_t len, int32_t tau_max, int32_t hop) {
  const int64_t width = 2 * (int64_t)tau_max;
  return len < width ? 0 : 1 + (len - width) / hop;
}

// The lags, the hop and the threshold of a call -> 0, or -1 with the offending argument's name in msg.
inline int pitch_args_check(int32_t tau_min, int32_t tau_max, int32_t hop, double threshold, char* msg, size_t msg_len) {
  if (tau_min < 2 || tau_max <= tau_min || tau_max > kPitchMaxLag) {
    snprintf(msg, msg_len, "tau_min, tau_max must satisfy 2 <= tau_min < tau_max <= %d (got %d, %d)", kPitchMaxLag, (int)tau_min, (int)tau_max);
    return -1;
  }
  if (hop < 1) { snprintf(msg, msg_len, "hop must be at least 1 (got %d)", (int)hop); return -1; }
  if (!(threshold > 0.0 && threshold < 1.0)) { snprintf(msg, msg_len, "threshold must lie in (0, 1) (got %g)", threshold); return -1; }
  return 0;
}

// What depends on the counts alone (n_seg >= 0, total_frames >= 0, 1 <= tau_max <= kPitchMaxLag, grid_cap >= 1).
inline void pitch_layout(int32_t n_seg, int64_t total_frames, int32_t tau_max, int32_t hop, int64_t grid_cap, PitchPlan* plan) {
  PitchPlan p;
  p.tau_max = tau_max;
  p.hop = hop;
  p.n_seg = n_seg;
  p.groups = (tau_max + kPitchLagsPerLane - 1) / kPitchLagsPerLane;
  p.blocks = (tau_max + kPitchBlock - 1) / kPitchBlock;
  p.lanes = 64;
  while (p.lanes < p.groups && p.lanes < kPitchMaxLanes) p.lanes *= 2;
  p.total_frames = total_frames;
  p.table_bytes = segment_table_entries(n_seg, true) * 8;
  p.scratch_bytes = (p.table_bytes + kPitchAlign - 1) / kPitchAlign * kPitchAlign;
  p.out_floats = 3 * total_frames;
  if (grid_cap < 1) grid_cap = 1;
  if (grid_cap > kPitchGridCap) grid_cap = kPitchGridCap;
  p.grid = (int32_t)(total_frames < grid_cap ? total_frames : grid_cap);
  *plan = p;
}

// Validates tau_max, hop and bounds[n_seg][2] against n (wseg_segments.h::segment_prefix), fills the plan and, where `prefix` is
// given (n_seg + 1 entries), the exclusive prefix of the frame counts -> 0, or -1 with the offending argument's name in msg.
// n_seg == 0 is valid: no frame, grid 0, scratch_bytes = the padded one-entry table.
inline int pitch_plan(const int64_t* bounds, int32_t n_seg, int32_t tau_max, int32_t hop, int64_t n, int64_t grid_cap, PitchPlan* plan,
                      int64_t* prefix, char* msg, size_t msg_len) {
  if (tau_max < 3 || tau_max > kPitchMaxLag) { snprintf(msg, msg_len, "tau_max must be 3 .. %d (got %d)", kPitchMaxLag, (int)tau_max); return -1; }
  if (hop < 1) { snprintf(msg, msg_len, "hop must be at least 1 (got %d)", (int)hop); return -1; }
  int64_t total;
  if (segment_prefix(SegmentBoundsArray{bounds}, n_seg, n, [tau_max, hop](int64_t len) { return pitch_frames(len, tau_max, hop); },
                     kPitchMaxFrames, "frames", prefix, &total, msg, msg_len))
    return -1;
  pitch_layout(n_seg, total, tau_max, hop, grid_cap, plan);
  return 0;
}

}  // namespace wseg
