// The host arithmetic of the nearest-neighbour search under banded dynamic time warping (wseg_dtw_scratch_bytes / wseg_dtw_knn_f32 /
// wseg_dtw_pairs_f64), in one place: the validation of a call, the padded step count, the sequences of a tile, the query and
// candidate tiles and the layout of the scratch the kernels of wseg_dtw.hip share; the candidate splits, the grids under the cap and
// the bound that sizes the keys are wseg_select_plan.h's.  Plain C++ with no HIP dependency, so that a host-only program can run it
// under a sanitizer (tools/dtw_plan_check.cpp).
//
// A row is a sequence of `steps` columns of `channels` values, time fastest: row[ch * steps + t].  dtw_select_kernel treats every
// COLUMN as a row of a 128 x 128 dot-product tile, the steps of a sequence padded to kDtwBlock = 32 or to 64 (zero-filled columns
// the dynamic program never enters), so a tile holds seqs = 128 / padded = 4 or 2 query sequences against as many candidates.
// A WORK ITEM is (query tile, split): seqs query sequences against a split of the candidate tiles.  Every (row, split) leaves its
// L = k + kDtwExtra best keys in scratch.  Scratch, in this order, every region padded to kDtwAlign bytes (at least one pad):
//   float    qnorm[m][steps]                   |q_i[:, a]|^2 as the channel-ordered fmaf chain
//   float    xnorm[n][steps]                   |x_j[:, b]|^2, the same
//   uint64   keys[m_tiles * seqs][splits][L]   (ordered G^ << 32) | j, ascending; all ones: no candidate
// The keys region is SIZED for min(m4 * n_tiles, m4 + 4 cap) rows of lists, m4 = m rounded up to 4 (sel_lists_bound; m_tiles * seqs
// <= m4 whatever the padding), so that wseg_dtw_scratch_bytes is monotone in m, n, k, steps and the cap, and a call under a smaller
// cap ($WSEG_DTW_GRID) fits the size reported for the default one.
#pragma once
#include "wseg_select_plan.h"

namespace wseg {

constexpr int kDtwTile = kSelTile;             // columns of a tile on either side
constexpr int kDtwBlock = 32;                  // the steps of a sequence are padded to one or two accumulator blocks
constexpr int kDtwMaxSteps = 64;               // T
constexpr int kDtwMaxChannels = 128;           // C
constexpr int kDtwMaxK = 64;                   // neighbours per row
constexpr int kDtwExtra = kSelExtra;             // candidates kept beyond k for the exact re-rank
constexpr int kDtwMaxL = kDtwMaxK + kDtwExtra; // entries of a row's list
constexpr int kDtwAlign = kSelAlign;             // bytes
constexpr int kDtwGridCap = kSelGridCap;       // workgroups of dtw_select_kernel
constexpr int kDtwFinishPerCap = kSelFinishPerCap;     // single-wave workgroups of dtw_finish_kernel / dtw_pairs_kernel per unit of the cap
constexpr int64_t kDtwMaxRows = kSelMaxRows;   // of queries and of corpus

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

// channels, steps and (band >= 0: checked; band < 0: not given) -> 0, or -1 with the argument's name in msg
inline int dtw_check_shape(int32_t channels, int32_t steps, int32_t band, char* msg, size_t msg_len) {
  if (channels < 1 || channels > kDtwMaxChannels) { snprintf(msg, msg_len, "channels must be 1 .. %d (got %d)", kDtwMaxChannels, (int)channels); return -1; }
  if (steps < 1 || steps > kDtwMaxSteps) { snprintf(msg, msg_len, "steps must be 1 .. %d (got %d)", kDtwMaxSteps, (int)steps); return -1; }
  if (band >= steps) { snprintf(msg, msg_len, "band must be 0 .. steps - 1 = %d (got %d)", (int)steps - 1, (int)band); return -1; }
  return 0;
}

// the grid of the single-wave kernels over `work` rows or pairs under the cap
inline int32_t dtw_wave_grid(int64_t work, int64_t grid_cap) { return sel_wave_grid(work, grid_cap); }

// Validates the sizes of a call and fills the plan -> 0, or -1 with the argument's name in msg.  m == 0 and n == 0 are valid.
inline int dtw_plan(int64_t m, int64_t n, int32_t channels, int32_t steps, int32_t k, int64_t grid_cap, DtwPlan* plan, char* msg, size_t msg_len) {
  if (k < 1 || k > kDtwMaxK) { snprintf(msg, msg_len, "k must be 1 .. %d (got %d)", kDtwMaxK, (int)k); return -1; }
  if (dtw_check_shape(channels, steps, -1, msg, msg_len)) return -1;
  if (sel_check_rows("m", m, msg, msg_len) || sel_check_rows("n", n, msg, msg_len)) return -1;
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
  const SelSplit s = sel_split(p.m_tiles, p.n_tiles, grid_cap);
  p.splits = s.splits;
  p.tiles_per_split = s.tiles_per_split;
  p.items = s.items;
  p.grid = s.grid;
  p.finish_grid = sel_wave_grid(m, grid_cap);
  p.norm_grid = sel_norm_grid((m + n) * steps, grid_cap);
  p.qnorm_offset = 0;
  p.qnorm_bytes = 4 * m * steps;
  p.xnorm_offset = sel_pad(p.qnorm_bytes);
  p.xnorm_bytes = 4 * n * steps;
  p.keys_offset = p.xnorm_offset + sel_pad(p.xnorm_bytes);
  p.keys_bytes = p.items * p.seqs * p.L * 8;
  p.keys_capacity = sel_lists_bound((m + 3) / 4 * 4, p.n_tiles, 4, grid_cap) * p.L * 8;
  p.scratch_bytes = p.keys_offset + sel_pad(p.keys_capacity);
  *plan = p;
  return 0;
}

}  // namespace wseg
