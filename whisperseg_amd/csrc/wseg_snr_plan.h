// The host arithmetic of the per-segment signal-to-noise ratio (wseg_frame_energy_f32, wseg_snr_rows_scratch_bytes /
// wseg_snr_rows_f64), in one place: the frame count of a recording, a row's frame range and noise window, the validation of a
// call, the dedup of the (w0, w1, r) triples, the split of long windows, the grids and the layout of the scratch the kernels of
// wseg_snr.hip share.  Plain C++ with no HIP dependency, so that a host-only program can run it under a sanitizer
// (tools/snr_plan_check.cpp).
//
// A recording of n samples has the WHOLE frames j = 0 .. J - 1, frame j = x[j hop : j hop + n_fft], hop = n_fft / 4:
//   J = 0 for n < n_fft, else 1 + (n - n_fft) / hop                                      (whisperseg_amd/snr.py::frame_count)
// snr_frames_kernel's work item is a GROUP of kSnrFrameSlots / (n_fft / 2) consecutive frames (16 at n_fft 512 .. 1 at 8192): what
// fills the workgroup's 4096 complex points of LDS.
// The rows call gets table[n_seg][3] = (j0, j1, window) — the signal frames [j0, j1) of a row and the index of its noise window —
// and windows[n_win][3] = (w0, w1, r): the window's frames [w0, w1) and the rank r, 0 <= r <= w1 - w0 - 1, of the order statistic
// that is its noise floor.  Equal triples are selected ONCE: the plan sorts them and gives every row its unique window.  A unique
// window of at most kSnrSplit frames is SHORT: one workgroup selects it in LDS; a longer one is LONG and cut into chunks of
// kSnrSplit frames, whose 256-bin histograms are added up in the scratch, integer counts (no order).  Scratch, in this order:
//   int64   rows[n_seg][3]        (j0, j1, unique window)
//   int64   uwin[n_unique][3]     (w0, w1, r)
//   int64   short_list[n_short]   unique windows one workgroup takes
//   int64   long_list[n_long]     unique windows that are split
//   int64   long_prefix[n_long + 1]   the exclusive prefix of their chunk counts
//   (padded to kSnrAlign bytes)                                                  — all of the above is ONE staged upload
//   uint64  hist[n_long][4][256]  the long windows' counts per radix pass (zeroed by the call)
//   uint32  key[n_unique]         the selected bit pattern of every unique window
//   (padded to kSnrAlign bytes)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include "wseg_rfft.h"
#include "wseg_segments.h"

namespace wseg {

constexpr int kSnrFrameSlots = 4096;           // complex points of LDS a workgroup transforms at a time: one 8192-point frame, 16 of 512
constexpr int kSnrMaxGroup = kSnrFrameSlots / 256;      // 16: frames of a group at the smallest transform
constexpr int kSnrStageFloats = 5120;          // samples a group of MORE than one frame spans at most: (G - 1) hop + n_fft at n_fft 4096
constexpr int kSnrLanes = 256;
constexpr int kSnrRowLanes = 64;               // of snr_rows_kernel: a wave per row
constexpr int kSnrSplit = 8192;                // frames of a window one workgroup selects in LDS (32 KiB of keys); more: split
constexpr int kSnrAlign = 256;                 // bytes
constexpr int kSnrGridCap = 2048;              // workgroups of any kernel: 8 per CU; more items take the grid stride
constexpr int64_t kSnrMaxFrames = (int64_t)1 << 40;      // of a recording

inline int64_t snr_pad(int64_t bytes) { return (bytes + kSnrAlign - 1) / kSnrAlign * kSnrAlign; }

// Whole frames of a recording of n samples (n >= 0, n_fft a transform size).
inline int64_t snr_frames(int64_t n, int32_t n_fft) {
  const int64_t hop = n_fft / 4;
  return n < n_fft ? 0 : 1 + (n - n_fft) / hop;
}

// The signal frames [j0, j1) of the samples [s0, s1), 0 <= s0 <= s1 <= n, in a recording of J >= 1 frames: the frames wholly
// inside the row, or the one frame centred nearest the row's centre (whisperseg_amd/snr.py::frame_ranges).
inline void snr_signal_frames(int64_t s0, int64_t s1, int32_t n_fft, int64_t J, int64_t* j0, int64_t* j1) {
  const int64_t hop = n_fft / 4;
  int64_t a = (s0 + hop - 1) / hop;
  int64_t b = s1 < n_fft ? 0 : (s1 - n_fft) / hop + 1;
  if (b > J) b = J;
  if (b <= a) {
    const int64_t num = (s0 + s1) / 2 - n_fft / 2 + hop / 2;      // (negative: the first frame)
    int64_t jc = num < 0 ? 0 : num / hop;
    if (jc > J - 1) jc = J - 1;
    a = jc;
    b = jc + 1;
  }
  *j0 = a;
  *j1 = b;
}

// The noise window of the signal frames [j0, j1): the whole recording (context_frames < 0), or c frames to either side.
inline void snr_noise_window(int64_t j0, int64_t j1, int64_t J, int64_t context_frames, int64_t* w0, int64_t* w1) {
  if (context_frames < 0) { *w0 = 0; *w1 = J; return; }
  *w0 = j0 > context_frames ? j0 - context_frames : 0;
  *w1 = j1 < J - context_frames ? j1 + context_frames : J;
}

// r = floor(q (len - 1)), 0 <= q <= 1, len >= 1, in double as Python's floats take it.
inline int64_t snr_rank(double q, int64_t len) { return (int64_t)floor(q * (double)(len - 1)); }

// ---- the track ---------------------------------------------------------------------------------------------------------------------
struct SnrTrackPlan {
  int32_t n_fft, hop, log2_half;
  int32_t group;                   // frames of a work item: kSnrFrameSlots / (n_fft / 2)
  int32_t log2_group;
  int64_t frames;                  // J
  int64_t groups;                  // ceil(J / group)
  int64_t read_end;                // (J - 1) hop + n_fft <= n: no sample at or behind it is loaded (0: no frame)
  int32_t grid;                    // workgroups (0: no frame)
};

// n, n_fft and the band -> 0, or -1 with the offending argument's name in msg.
inline int snr_track_plan(int64_t n, int32_t n_fft, int32_t k_lo, int32_t k_hi, int64_t grid_cap, SnrTrackPlan* plan, char* msg, size_t msg_len) {
  if (rfft_size_check(n_fft, msg, msg_len)) return -1;
  if (n < 0 || n > kSegmentMaxSamples) { snprintf(msg, msg_len, "n must be 0 .. 2^52 samples (got %lld)", (long long)n); return -1; }
  if (k_lo < 0 || k_hi < k_lo || k_hi > n_fft / 2) {
    snprintf(msg, msg_len, "k_lo, k_hi must satisfy 0 <= k_lo <= k_hi <= n_fft / 2 (got %d, %d)", (int)k_lo, (int)k_hi);
    return -1;
  }
  SnrTrackPlan p;
  p.n_fft = n_fft;
  p.hop = n_fft / 4;
  p.log2_half = rfft_log2_half(n_fft);
  p.group = kSnrFrameSlots / (n_fft / 2);
  p.log2_group = 0;
  while ((1 << p.log2_group) < p.group) ++p.log2_group;
  p.frames = snr_frames(n, n_fft);
  if (p.frames > kSnrMaxFrames) { snprintf(msg, msg_len, "n holds more than 2^40 frames"); return -1; }
  p.groups = (p.frames + p.group - 1) / p.group;
  p.read_end = p.frames ? (p.frames - 1) * p.hop + n_fft : 0;
  if (grid_cap < 1) grid_cap = 1;
  if (grid_cap > kSnrGridCap) grid_cap = kSnrGridCap;
  p.grid = (int32_t)(p.groups < grid_cap ? p.groups : grid_cap);
  *plan = p;
  return 0;
}

// ---- the rows ----------------------------------------------------------------------------------------------------------------------
struct SnrRowsPlan {
  int32_t n_seg, n_win;
  int32_t n_unique, n_short, n_long;
  int64_t long_chunks;             // chunks of all long windows
  int64_t table_entries;           // int64 entries of the staged upload
  int64_t table_bytes;
  int64_t hist_offset, hist_bytes; // uint64 [n_long][4][256]
  int64_t key_offset, key_bytes;   // uint32 [n_unique]
  int64_t scratch_bytes;
  int32_t short_grid, long_grid, finish_grid, rows_grid;      // workgroups (0: no launch)
};

// What depends on the counts alone (all >= 0, n_unique = n_short + n_long).
inline void snr_rows_layout(int32_t n_seg, int32_t n_win, int32_t n_short, int32_t n_long, int64_t long_chunks, int64_t grid_cap, SnrRowsPlan* plan) {
  SnrRowsPlan p;
  p.n_seg = n_seg;
  p.n_win = n_win;
  p.n_short = n_short;
  p.n_long = n_long;
  p.n_unique = n_short + n_long;
  p.long_chunks = long_chunks;
  p.table_entries = 3 * (int64_t)n_seg + 3 * (int64_t)p.n_unique + n_short + n_long + ((int64_t)n_long + 1);
  p.table_bytes = p.table_entries * 8;
  p.hist_offset = snr_pad(p.table_bytes);
  p.hist_bytes = (int64_t)n_long * 4 * 256 * 8;
  p.key_offset = p.hist_offset + p.hist_bytes;
  p.key_bytes = 4 * (int64_t)p.n_unique;
  p.scratch_bytes = p.key_offset + snr_pad(p.key_bytes);
  if (grid_cap < 1) grid_cap = 1;
  if (grid_cap > kSnrGridCap) grid_cap = kSnrGridCap;
  p.short_grid = (int32_t)(n_short < grid_cap ? n_short : grid_cap);
  p.long_grid = (int32_t)(long_chunks < grid_cap ? long_chunks : grid_cap);
  p.finish_grid = (int32_t)(n_long < grid_cap ? n_long : grid_cap);
  p.rows_grid = (int32_t)(n_seg < grid_cap ? n_seg : grid_cap);
  *plan = p;
}

struct SnrFrameRanges {            // a bounds source of wseg_segments.h over the first two of every three entries
  const int64_t* p;
  void operator()(int32_t i, int64_t* s0, int64_t* s1) const { *s0 = p[3 * (int64_t)i]; *s1 = p[3 * (int64_t)i + 1]; }
};

// Validates table[n_seg][3] and windows[n_win][3] against J (wseg_segments.h: 0 <= j0 <= j1 <= J, 0 <= w0 <= w1 <= J), every rank
// against its window (0 <= r <= w1 - w0 - 1: a window holds a frame) and every row's window index against n_win; dedups the
// triples and fills the plan and, where `table` is given, the int64 entries of the upload (table_entries of them) -> 0, or -1 with
// the offending argument's name in msg.  n_seg == 0 is valid: no launch.
inline int snr_rows_plan(int64_t J, const int64_t* rows, int32_t n_seg, const int64_t* windows, int32_t n_win, int64_t grid_cap, SnrRowsPlan* plan,
                         std::vector<int64_t>* table, char* msg, size_t msg_len) {
  if (J < 0 || J > kSnrMaxFrames) { snprintf(msg, msg_len, "J must be 0 .. 2^40 frames (got %lld)", (long long)J); return -1; }
  if (n_win < 0) { snprintf(msg, msg_len, "n_win is negative (%d)", (int)n_win); return -1; }
  if (n_seg > 0 && !rows) { snprintf(msg, msg_len, "table is null for n_seg = %d", (int)n_seg); return -1; }
  if (n_win > 0 && !windows) { snprintf(msg, msg_len, "windows is null for n_win = %d", (int)n_win); return -1; }
  if (segment_check(SnrFrameRanges{rows}, n_seg, J, msg, msg_len)) return -1;
  char inner[160];
  if (segment_check(SnrFrameRanges{windows}, n_win, J, inner, sizeof(inner))) { snprintf(msg, msg_len, "windows: %s", inner); return -1; }
  for (int32_t i = 0; i < n_win; ++i) {
    const int64_t len = windows[3 * (int64_t)i + 1] - windows[3 * (int64_t)i], r = windows[3 * (int64_t)i + 2];
    if (r < 0 || r > len - 1) {
      snprintf(msg, msg_len, "the rank r of window %d must satisfy 0 <= r <= w1 - w0 - 1 = %lld (got %lld)", (int)i, (long long)(len - 1), (long long)r);
      return -1;
    }
  }
  for (int32_t i = 0; i < n_seg; ++i) {
    const int64_t w = rows[3 * (int64_t)i + 2];
    if (w < 0 || w >= n_win) { snprintf(msg, msg_len, "the window of row %d must be 0 .. n_win - 1 = %d (got %lld)", (int)i, (int)n_win - 1, (long long)w); return -1; }
  }
  // the dedup: the windows' indices sorted by their triple; equal neighbours share a unique window, numbered in sorted order
  std::vector<int32_t> order((size_t)n_win), unique_of((size_t)n_win);
  for (int32_t i = 0; i < n_win; ++i) order[(size_t)i] = i;
  auto triple_less = [windows](int32_t a, int32_t b) {
    const int64_t* x = windows + 3 * (int64_t)a;
    const int64_t* y = windows + 3 * (int64_t)b;
    return x[0] != y[0] ? x[0] < y[0] : x[1] != y[1] ? x[1] < y[1] : x[2] < y[2];
  };
  std::sort(order.begin(), order.end(), triple_less);
  std::vector<int32_t> first;      // of every unique window: a window that has its triple
  for (int32_t k = 0; k < n_win; ++k) {
    if (k == 0 || triple_less(order[(size_t)k - 1], order[(size_t)k])) first.push_back(order[(size_t)k]);
    unique_of[(size_t)order[(size_t)k]] = (int32_t)first.size() - 1;
  }
  int32_t n_short = 0, n_long = 0;
  int64_t long_chunks = 0;
  for (const int32_t w : first) {
    const int64_t len = windows[3 * (int64_t)w + 1] - windows[3 * (int64_t)w];
    if (len <= kSnrSplit) ++n_short; else { ++n_long; long_chunks += (len + kSnrSplit - 1) / kSnrSplit; }
  }
  snr_rows_layout(n_seg, n_win, n_short, n_long, long_chunks, grid_cap, plan);
  if (!table) return 0;
  table->assign((size_t)plan->table_entries, 0);
  int64_t* t = table->data();
  for (int32_t i = 0; i < n_seg; ++i) {
    t[3 * (int64_t)i] = rows[3 * (int64_t)i];
    t[3 * (int64_t)i + 1] = rows[3 * (int64_t)i + 1];
    t[3 * (int64_t)i + 2] = unique_of[(size_t)rows[3 * (int64_t)i + 2]];
  }
  int64_t* uwin = t + 3 * (int64_t)n_seg;
  int64_t* short_list = uwin + 3 * (int64_t)plan->n_unique;
  int64_t* long_list = short_list + n_short;
  int64_t* long_prefix = long_list + n_long;
  int32_t s = 0, l = 0;
  int64_t chunks = 0;
  for (int32_t u = 0; u < plan->n_unique; ++u) {
    const int64_t* w = windows + 3 * (int64_t)first[(size_t)u];
    uwin[3 * (int64_t)u] = w[0];
    uwin[3 * (int64_t)u + 1] = w[1];
    uwin[3 * (int64_t)u + 2] = w[2];
    const int64_t len = w[1] - w[0];
    if (len <= kSnrSplit) {
      short_list[s++] = u;
    } else {
      long_list[l] = u;
      long_prefix[l++] = chunks;
      chunks += (len + kSnrSplit - 1) / kSnrSplit;
    }
  }
  long_prefix[n_long] = chunks;
  return 0;
}

}  // namespace wseg
