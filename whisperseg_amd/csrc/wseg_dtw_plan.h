// The host arithmetic of the nearest-neighbour search under banded dynamic time warping (wseg_dtw_scratch_bytes / wseg_dtw_knn_f32 /
// wseg_dtw_pairs_f64), in one place: the validation of a call, the padded step count, the sequences of a tile, the query and
// candidate tiles, the candidate splits, the grids under the cap and the layout of the scratch the kernels of wseg_dtw.hip share.
// Plain C++ with no HIP dependency, so that a host-only program can run it under a sanitizer (tools/dtw_plan_check.cpp).
//
// A row is a sequence of `steps` columns of `channels` values, time fastest: row[ch * steps + t].  dtw_select_kernel treats every
// COLUMN as a row of a 128 x 128 dot-product tile, the steps of a sequence padded to kDtwBlock = 32 or to 64 (zero-filled columns
// the dynamic program never enters), so a tile holds seqs = 128 / padded = 4 or 2 query sequences against as many candidates.
// A WORK ITEM is (query tile, split): seqs query sequences against the candidate tiles [split * tiles_per_split,
// (split + 1) * tiles_per_split).  Splits exist so that few query rows still fill the chip: as many as bring the items to the
// grid cap, never more than there are candidate tiles, none of them empty.  Every (row, split) leaves its L = k + kDtwExtra best
// keys in scratch.  Scratch, in this order, every region padded to kDtwAlign bytes (at least one pad):
//   float    qnorm[m][steps]                   |q_i[:, a]|^2 as the channel-ordered fmaf chain
//   float    xnorm[n][steps]                   |x_j[:, b]|^2, the same
//   uint64   keys[m_tiles * seqs][splits][L]   (ordered G^ << 32) | j, ascending; all ones: no candidate
// The keys region is SIZED for min(m4 * n_tiles, m4 + 4 cap) rows of lists, m4 = m rounded up to 4 — a bound of
// m_tiles * seqs * splits (m_tiles * seqs <= m4, splits <= n_tiles, m_tiles * splits <= m_tiles + cap) that grows with m, n, k,
// steps and the cap, so that wseg_dtw_scratch_bytes is monotone although the split count is not — and a call under a smaller cap
// ($WSEG_DTW_GRID) fits the size reported for the default one.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace wseg {

constexpr int kDtwTile = 128;                  // columns of a tile on either side
constexpr int kDtwBlock = 32;                  // the steps of a sequence are padded to one or two accumulator blocks
constexpr int kDtwMaxSteps = 64;               // T
constexpr int kDtwMaxChannels = 128;           // C
constexpr int kDtwMaxK = 64;                   // neighbours per row
constexpr int kDtwExtra = 8;                   // candidates kept beyond k for the exact re-rank
constexpr int kDtwMaxL = kDtwMaxK + kDtwExtra; // entries of a row's list
constexpr int kDtwAlign = 256;                 // bytes
constexpr int kDtwGridCap = 2048;              // workgroups of dtw_select_kernel; more items take the grid stride
constexpr int kDtwFinishPerCap = 8;            // single-wave workgroups of dtw_finish_kernel / dtw_pairs_kernel per unit of the cap
constexpr int64_t kDtwMaxRows = INT32_MAX;     // of queries and of corpus: indices are int32

struct DtwPlan {
  int64_t m, n;
  int32_t channels, steps, k, L;
  int32_t padded;                  // 32 or 64
  int32_t seqs;                    // sequences of a tile on either side: 128 / padded
  int64_t m_tiles, n_tiles;        // ceil(m / seqs), ceil(n / seqs)
  int32_t splits;                  // candidate splits, 1 .. min(n_tiles, cap)        (0: no candidate tile)
  int32_t tiles_per_split;         // ceil(n_tiles / splits); (splits - 1) * tiles_per_split < n_tiles: no split is empty
  int64_t items;                   // m_tiles * splits
  int32_t grid;                    // workgroups of dtw_select_kernel, min(items, cap)
  int32_t finish_grid;             // workgroups of dtw_finish_kernel, one query row at a time each
  int32_t norm_grid;               // workgroups (256 columns a round) of dtw_norms_kernel over the (m + n) * steps columns
  int64_t qnorm_offset, qnorm_bytes, xnorm_offset, xnorm_bytes, keys_offset, keys_bytes, keys_capacity, scratch_bytes;
};

inline int64_t dtw_pad(int64_t bytes) { return bytes <= 0 ? kDtwAlign : (bytes + kDtwAlign - 1) / kDtwAlign * kDtwAlign; }

// channels, steps and (band >= 0: checked; band < 0: not given) -> 0, or -1 with the argument's name in msg
inline int dtw_check_shape(int32_t channels, int32_t steps, int32_t band, char* msg, size_t msg_len) {
  if (channels < 1 || channels > kDtwMaxChannels) { snprintf(msg, msg_len, "channels must be 1 .. %d (got %d)", kDtwMaxChannels, (int)channels); return -1; }
  if (steps < 1 || steps > kDtwMaxSteps) { snprintf(msg, msg_len, "steps must be 1 .. %d (got %d)", kDtwMaxSteps, (int)steps); return -1; }
  if (band >= steps) { snprintf(msg, msg_len, "band must be 0 .. steps - 1 = %d (got %d)", (int)steps - 1, (int)band); return -1; }
  return 0;
}

// the grid of the single-wave kernels over `work` rows or pairs under the cap
inline int32_t dtw_wave_grid(int64_t work, int64_t grid_cap) {
  if (grid_cap < 1) grid_cap = 1;
  if (grid_cap > kDtwGridCap) grid_cap = kDtwGridCap;
  const int64_t cap = grid_cap * kDtwFinishPerCap;
  return (int32_t)(work < 0 ? 0 : work < cap ? work : cap);
}

// Validates the sizes of a call and fills the plan -> 0, or -1 with the argument's name in msg.  m == 0 and n == 0 are valid.
inline int dtw_plan(int64_t m, int64_t n, int32_t channels, int32_t steps, int32_t k, int64_t grid_cap, DtwPlan* plan, char* msg, size_t msg_len) {
  if (k < 1 || k > kDtwMaxK) { snprintf(msg, msg_len, "k must be 1 .. %d (got %d)", kDtwMaxK, (int)k); return -1; }
  if (dtw_check_shape(channels, steps, -1, msg, msg_len)) return -1;
  if (m < 0 || m > kDtwMaxRows) { snprintf(msg, msg_len, "m must be 0 .. 2^31 - 1 (got %lld)", (long long)m); return -1; }
  if (n < 0 || n > kDtwMaxRows) { snprintf(msg, msg_len, "n must be 0 .. 2^31 - 1 (got %lld)", (long long)n); return -1; }
  if (grid_cap < 1) grid_cap = 1;
  if (grid_cap > kDtwGridCap) grid_cap = kDtwGridCap;
  DtwPlan p;
  p.m = m;
  p.n = n;
  p.channels = channels;
  p.steps = steps;
  p.k = k;
  p.L = k + kDtwExtra;
  p.padded = steps <= kDtwBlock ? kDtwBlock : 2 * kDtwBlock;
  p.seqs = kDtwTile / p.padded;
  p.m_tiles = (m + p.seqs - 1) / p.seqs;
  p.n_tiles = (n + p.seqs - 1) / p.seqs;
  if (p.m_tiles == 0 || p.n_tiles == 0) {
    p.splits = 0;
    p.tiles_per_split = 0;
  } else {
    int64_t want = (grid_cap + p.m_tiles - 1) / p.m_tiles;       // splits that bring the items to the cap
    if (want > p.n_tiles) want = p.n_tiles;
    p.tiles_per_split = (int32_t)((p.n_tiles + want - 1) / want);
    p.splits = (int32_t)((p.n_tiles + p.tiles_per_split - 1) / p.tiles_per_split);
  }
  p.items = p.m_tiles * p.splits;
  p.grid = (int32_t)(p.items < grid_cap ? p.items : grid_cap);
  p.finish_grid = dtw_wave_grid(m, grid_cap);
  const int64_t norm_rounds = ((m + n) * steps + 255) / 256;
  p.norm_grid = (int32_t)(norm_rounds < grid_cap ? norm_rounds : grid_cap);
  const int64_t m4 = (m + 3) / 4 * 4;
  const int64_t pairs = m4 * p.n_tiles, capped = m4 + 4 * grid_cap;
  const int64_t rows_bound = pairs < capped ? pairs : capped;
  p.qnorm_offset = 0;
  p.qnorm_bytes = 4 * m * steps;
  p.xnorm_offset = dtw_pad(p.qnorm_bytes);
  p.xnorm_bytes = 4 * n * steps;
  p.keys_offset = p.xnorm_offset + dtw_pad(p.xnorm_bytes);
  p.keys_bytes = p.items * p.seqs * p.L * 8;
  p.keys_capacity = rows_bound * p.L * 8;
  p.scratch_bytes = p.keys_offset + dtw_pad(p.keys_capacity);
  *plan = p;
  return 0;
}

}  // namespace wseg
