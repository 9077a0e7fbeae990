// The host arithmetic of the nearest-neighbour search (wseg_knn_scratch_bytes / wseg_knn_f32), in one place: the validation of a
// call, the query and candidate tiles and the layout of the scratch the kernels of wseg_knn.hip share; the candidate splits, the
// grids under the cap and the bound that sizes the keys are wseg_select_plan.h's.  Plain C++ with no HIP dependency, so that a
// host-only program can run it under a sanitizer (tools/knn_plan_check.cpp).
//
// A WORK ITEM of the select kernel is (query tile, split): kKnnTile = 128 query rows against a split of the candidate tiles (128
// candidates each).  Every (row, split) leaves its L = k + kKnnExtra best keys in scratch.  Scratch, in this order, every region
// padded to kKnnAlign bytes (at least one pad):
//   float    qnorm[m]                          |q_i|^2 as the k-ordered fmaf chain
//   float    xnorm[n]                          |x_j|^2, the same
//   uint64   keys[m_tiles * 128][splits][L]    (ordered d^ << 32) | j, ascending; all ones: no candidate
// The keys region is SIZED for min(m_tiles * n_tiles, m_tiles + cap) items of 128 rows (sel_lists_bound), so that
// wseg_knn_scratch_bytes is monotone in m, n, k and the cap, and a call under a smaller cap ($WSEG_KNN_GRID) fits the size reported
// for the default one.
#pragma once
#include "wseg_select_plan.h"

namespace wseg {

constexpr int kKnnTile = kSelTile;             // query rows of a work item; candidates of a tile
constexpr int kKnnMaxK = 64;                   // neighbours per row
constexpr int kKnnExtra = kSelExtra;           // candidates kept beyond k for the exact re-rank
constexpr int kKnnMaxL = kKnnMaxK + kKnnExtra; // entries of a row's list
constexpr int kKnnSmallL = kSelSmallL;         // lists up to here (k <= 16) run in the selection kernel with the smaller LDS
constexpr int kKnnMaxD = 20480;                // columns: 80 x 256, the widest patch
constexpr int kKnnAlign = kSelAlign;           // bytes
constexpr int kKnnGridCap = kSelGridCap;       // workgroups of the select kernel
constexpr int kKnnFinishPerCap = kSelFinishPerCap;     // single-wave workgroups of knn_finish_kernel per unit of the cap
constexpr int64_t kKnnMaxRows = kSelMaxRows;   // of queries and of corpus

struct KnnPlan {
  int64_t m, n;
  int32_t d, k, L;
  int64_t m_tiles, n_tiles;        // ceil(m / 128), ceil(n / 128)                    (< 2^24)
  int32_t splits;                  // candidate splits, 1 .. min(n_tiles, cap)        (0: no candidate tile)
  int32_t tiles_per_split;         // ceil(n_tiles / splits); (splits - 1) * tiles_per_split < n_tiles: no split is empty
  int64_t items;                   // m_tiles * splits                                (< 2^24 + cap)
  int32_t grid;                    // workgroups of the select kernel, min(items, cap)
  int32_t finish_grid;             // workgroups of knn_finish_kernel, one query row at a time each
  int32_t norm_grid;               // workgroups (256 rows a round) of the norms kernel over the m + n rows
  int64_t qnorm_offset, qnorm_bytes, xnorm_offset, xnorm_bytes, keys_offset, keys_bytes, keys_capacity, scratch_bytes;
};

// Validates the sizes of a call and fills the plan -> 0, or -1 with the argument's name in msg.  m == 0 and n == 0 are valid.
inline int knn_plan(int64_t m, int64_t n, int32_t d, int32_t k, int64_t grid_cap, KnnPlan* plan, char* msg, size_t msg_len) {
  if (k < 1 || k > kKnnMaxK) { snprintf(msg, msg_len, "k must be 1 .. %d (got %d)", kKnnMaxK, (int)k); return -1; }
  if (d < 1 || d > kKnnMaxD) { snprintf(msg, msg_len, "d must be 1 .. %d (got %d)", kKnnMaxD, (int)d); return -1; }
  if (sel_check_rows("m", m, msg, msg_len) || sel_check_rows("n", n, msg, msg_len)) return -1;
  KnnPlan p;
  p.m = m;
  p.n = n;
  p.d = d;
  p.k = k;
  p.L = k + kKnnExtra;
  p.m_tiles = (m + kKnnTile - 1) / kKnnTile;
  p.n_tiles = (n + kKnnTile - 1) / kKnnTile;
  const SelSplit s = sel_split(p.m_tiles, p.n_tiles, grid_cap);
  p.splits = s.splits;
  p.tiles_per_split = s.tiles_per_split;
  p.items = s.items;
  p.grid = s.grid;
  p.finish_grid = sel_wave_grid(m, grid_cap);
  p.norm_grid = sel_norm_grid(m + n, grid_cap);
  p.qnorm_offset = 0;
  p.qnorm_bytes = 4 * m;
  p.xnorm_offset = sel_pad(p.qnorm_bytes);
  p.xnorm_bytes = 4 * n;
  p.keys_offset = p.xnorm_offset + sel_pad(p.xnorm_bytes);
  p.keys_bytes = p.items * kKnnTile * p.L * 8;
  p.keys_capacity = sel_lists_bound(p.m_tiles * kKnnTile, p.n_tiles, kKnnTile, grid_cap) * p.L * 8;
  p.scratch_bytes = p.keys_offset + sel_pad(p.keys_capacity);
  *plan = p;
  return 0;
}

}  // namespace wseg
