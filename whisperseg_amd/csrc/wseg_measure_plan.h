// The host arithmetic of the per-segment measurements (wseg_measure_scratch_bytes / wseg_measure_segments_f32), in one place: the
// validation of a call, the chunk count of every segment and the layout of the scratch the two kernels of wseg_measure.hip share.
// Plain C++ with no HIP dependency, so that a host-only program can run it under a sanitizer (tools/measure_plan_check.cpp).
//
// A segment [s0, s1) of len = s1 - s0 samples is cut into frames of n_fft samples, hop = n_fft / 4 apart, the first at s0:
//   J = 0 for len == 0, 1 for 0 < len <= n_fft, else 1 + ceil((len - n_fft) / hop)        (whisperseg_amd/measure.py::frame_count)
// and its frames into CHUNKS of kMeasureChunkFrames = 64 (the last chunk holds the rest): ceil(J / 64) work items of
// measure_chunk_kernel.  Scratch, in this order:
//   int64  table[3 n_seg + 1]     the segment table with the exclusive prefix of the chunk counts (wseg_segments.h)
//   (padded to kMeasureAlign bytes)
//   double partial[total_chunks][n_fft / 2 + 1 + kMeasureTimeSlots]
//                                 a chunk's spectrum P[0 .. n_fft / 2] summed over its frames, then the partials of the samples it
//                                 owns: sum of squares | max |x| | crossing count (each held in a double slot, the count as int64 bits)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "wseg_rfft.h"
#include "wseg_segments.h"

namespace wseg {

constexpr int kMeasureChunkFrames = 64;        // frames of a segment one work item takes (whisperseg_amd/measure.py::CHUNK_FRAMES)
constexpr int kMeasureTimeSlots = 3;           // sum x^2 | max |x| | crossings, behind a chunk's spectrum
constexpr int kMeasureAlign = 256;             // bytes the partials start on behind the table
constexpr int kMeasureGridCap = 2048;          // workgroups of measure_chunk_kernel: 8 per CU; more items take the grid stride
constexpr int64_t kMeasureMaxChunks = (int64_t)1 << 40;       // of one call, all segments together (2^40 * 33 KiB < 2^56 bytes)

struct MeasurePlan {
  int32_t n_fft, hop, n_bins;      // n_bins = n_fft / 2 + 1
  int32_t n_seg;
  int64_t total_chunks;            // over all segments
  int64_t table_bytes;             // (3 n_seg + 1) int64
  int64_t partial_offset;          // table_bytes rounded up to kMeasureAlign
  int64_t chunk_doubles;           // n_bins + kMeasureTimeSlots
  int64_t scratch_bytes;           // partial_offset + total_chunks * chunk_doubles * 8
  int32_t grid;                    // workgroups of measure_chunk_kernel (0: no chunk at all)
};

// Frames of a segment of len samples (len >= 0).
inline int64_t measure_frames(int64_t len, int32_t n_fft) {
  const int64_t hop = n_fft / 4;
  if (len <= 0) return 0;
  if (len <= n_fft) return 1;
  return 1 + (len - n_fft + hop - 1) / hop;
}
inline int64_t measure_chunks(int64_t len, int32_t n_fft) {
  return (measure_frames(len, n_fft) + kMeasureChunkFrames - 1) / kMeasureChunkFrames;
}

// Validates n_fft and bounds[n_seg][2] against n (wseg_segments.h::segment_prefix), fills the plan and, where `prefix` is given
// (n_seg + 1 entries), the exclusive prefix of the chunk counts -> 0, or -1 with the offending argument's name in msg.
// n_seg == 0 is valid: no chunk, grid 0, scratch_bytes = the padded one-entry table.
inline int measure_plan(const int64_t* bounds, int32_t n_seg, int32_t n_fft, int64_t n, int64_t grid_cap, MeasurePlan* plan,
                        int64_t* prefix, char* msg, size_t msg_len) {
  MeasurePlan p;
  if (rfft_size_check(n_fft, msg, msg_len) ||      // (a segment holds at most 2^52 / (64 * 128) = 2^39 chunks)
      segment_prefix(SegmentBoundsArray{bounds}, n_seg, n, [n_fft](int64_t len) { return measure_chunks(len, n_fft); }, kMeasureMaxChunks,
                     "chunks", prefix, &p.total_chunks, msg, msg_len))
    return -1;
  p.n_fft = n_fft;
  p.hop = n_fft / 4;
  p.n_bins = n_fft / 2 + 1;
  p.n_seg = n_seg;
  p.table_bytes = segment_table_entries(n_seg, true) * 8;
  p.partial_offset = (p.table_bytes + kMeasureAlign - 1) / kMeasureAlign * kMeasureAlign;
  p.chunk_doubles = p.n_bins + kMeasureTimeSlots;
  p.scratch_bytes = p.partial_offset + p.total_chunks * p.chunk_doubles * 8;
  if (grid_cap < 1) grid_cap = 1;
  p.grid = (int32_t)(p.total_chunks < grid_cap ? p.total_chunks : grid_cap);
  *plan = p;
  return 0;
}

// The band of the spectral columns: 1 <= k_lo <= k_hi <= n_fft / 2 -> 0, or -1 with the names in msg.
inline int measure_band_check(int32_t n_fft, int32_t k_lo, int32_t k_hi, char* msg, size_t msg_len) {
  if (k_lo < 1 || k_hi < k_lo || k_hi > n_fft / 2) {
    snprintf(msg, msg_len, "k_lo, k_hi must satisfy 1 <= k_lo <= k_hi <= %d (got %d, %d)", (int)(n_fft / 2), (int)k_lo, (int)k_hi);
    return -1;
  }
  return 0;
}

}  // namespace wseg
