// The host arithmetic of the nearest-neighbour search (wseg_knn_scratch_bytes / wseg_knn_f32), in one place: the validation of a
// call, the query and candidate tiles, the candidate splits, the grids under the cap and the layout of the scratch the kernels of
// wseg_knn.hip share.  Plain C++ with no HIP dependency, so that a host-only program can run it under a sanitizer
// (tools/knn_plan_check.cpp).
//
// A WORK ITEM of knn_select_kernel is (query tile, split): kKnnTile = 128 query rows against the candidate tiles (128 candidates
// each) [split * tiles_per_split, (split + 1) * tiles_per_split).  Splits exist so that few query rows still fill the chip: as
// many as bring the items to the grid cap, never more than there are candidate tiles, none of them empty.  Every (row, split)
// leaves its L = k + kKnnExtra best keys in scratch.  Scratch, in this order, every region padded to kKnnAlign bytes (at least one
// pad):
//   float    qnorm[m]                          |q_i|^2 as the k-ordered fmaf chain
//   float    xnorm[n]                          |x_j|^2, the same
//   uint64   keys[m_tiles * 128][splits][L]    (ordered d^ << 32) | j, ascending; all ones: no candidate
// The keys region is SIZED for min(m_tiles * n_tiles, m_tiles + cap) items of 128 rows — a bound of m_tiles * splits that grows
// with m, n, k and the cap, so that wseg_knn_scratch_bytes is monotone although the split count is not — and a call under a
// smaller cap ($WSEG_KNN_GRID) fits the size reported for the default one.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace wseg {

constexpr int kKnnTile = 128;                  // query rows of a work item; candidates of a tile
constexpr int kKnnMaxK = 64;                   // neighbours per row
constexpr int kKnnExtra = 8;                   // candidates kept beyond k for the exact re-rank
constexpr int kKnnMaxL = kKnnMaxK + kKnnExtra; // entries of a row's list
constexpr int kKnnSmallL = 24;                 // lists up to here (k <= 16) run in the selection kernel with the smaller LDS
constexpr int kKnnMaxD = 20480;                // columns: 80 x 256, the widest patch
constexpr int kKnnAlign = 256;                 // bytes
constexpr int kKnnGridCap = 2048;              // workgroups of knn_select_kernel: 8 per CU; more items take the grid stride
constexpr int kKnnFinishPerCap = 8;            // single-wave workgroups of knn_finish_kernel per unit of the cap
constexpr int64_t kKnnMaxRows = INT32_MAX;     // of queries and of corpus: indices are int32

struct KnnPlan {
  int64_t m, n;
  int32_t d, k, L;
  int64_t m_tiles, n_tiles;        // ceil(m / 128), ceil(n / 128)                    (< 2^24)
  int32_t splits;                  // candidate splits, 1 .. min(n_tiles, cap)        (0: no candidate tile)
  int32_t tiles_per_split;         // ceil(n_tiles / splits); (splits - 1) * tiles_per_split < n_tiles: no split is empty
  int64_t items;                   // m_tiles * splits                                (< 2^24 + cap)
  int32_t grid;                    // workgroups of knn_select_kernel, min(items, cap)
  int32_t finish_grid;             // workgroups of knn_finish_kernel, one query row at a time each
  int32_t norm_grid;               // workgroups (256 rows a round) of knn_norms_kernel over the m + n rows
  int64_t qnorm_offset, qnorm_bytes, xnorm_offset, xnorm_bytes, keys_offset, keys_bytes, keys_capacity, scratch_bytes;
};

inline int64_t knn_pad(int64_t bytes) { return bytes <= 0 ? kKnnAlign : (bytes + kKnnAlign - 1) / kKnnAlign * kKnnAlign; }

// Validates the sizes of a call and fills the plan -> 0, or -1 with the argument's name in msg.  m == 0 and n == 0 are valid.
inline int knn_plan(int64_t m, int64_t n, int32_t d, int32_t k, int64_t grid_cap, KnnPlan* plan, char* msg, size_t msg_len) {
  if (k < 1 || k > kKnnMaxK) { snprintf(msg, msg_len, "k must be 1 .. %d (got %d)", kKnnMaxK, (int)k); return -1; }
  if (d < 1 || d > kKnnMaxD) { snprintf(msg, msg_len, "d must be 1 .. %d (got %d)", kKnnMaxD, (int)d); return -1; }
  if (m < 0 || m > kKnnMaxRows) { snprintf(msg, msg_len, "m must be 0 .. 2^31 - 1 (got %lld)", (long long)m); return -1; }
  if (n < 0 || n > kKnnMaxRows) { snprintf(msg, msg_len, "n must be 0 .. 2^31 - 1 (got %lld)", (long long)n); return -1; }
  if (grid_cap < 1) grid_cap = 1;
  if (grid_cap > kKnnGridCap) grid_cap = kKnnGridCap;
  KnnPlan p;
  p.m = m;
  p.n = n;
  p.d = d;
  p.k = k;
  p.L = k + kKnnExtra;
  p.m_tiles = (m + kKnnTile - 1) / kKnnTile;
  p.n_tiles = (n + kKnnTile - 1) / kKnnTile;
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
  const int64_t finish_cap = grid_cap * kKnnFinishPerCap;
  p.finish_grid = (int32_t)(m < finish_cap ? m : finish_cap);
  const int64_t norm_rounds = (m + n + 255) / 256;
  p.norm_grid = (int32_t)(norm_rounds < grid_cap ? norm_rounds : grid_cap);
  const int64_t pairs = p.m_tiles * p.n_tiles, capped = p.m_tiles + grid_cap;
  const int64_t items_bound = pairs < capped ? pairs : capped;
  p.qnorm_offset = 0;
  p.qnorm_bytes = 4 * m;
  p.xnorm_offset = knn_pad(p.qnorm_bytes);
  p.xnorm_bytes = 4 * n;
  p.keys_offset = p.xnorm_offset + knn_pad(p.xnorm_bytes);
  p.keys_bytes = p.items * kKnnTile * p.L * 8;
  p.keys_capacity = items_bound * kKnnTile * p.L * 8;
  p.scratch_bytes = p.keys_offset + knn_pad(p.keys_capacity);
  *plan = p;
  return 0;
}

}  // namespace wseg
