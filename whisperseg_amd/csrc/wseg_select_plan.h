// The host arithmetic that the distance-tile selections share (wseg_knn_plan.h, wseg_mst_plan.h, wseg_dtw_plan.h; the device side
// is wseg_select.h): the candidate splits of a work item, the grids under the cap, the padding of a scratch region and the bound
// that sizes the keys.  Plain C++ with no HIP dependency; the three plans call it and the stand-alone programs that check them
// under a sanitizer (tools/knn_plan_check.cpp, mst_plan_check.cpp, dtw_plan_check.cpp) check it through them.
//
// A WORK ITEM of a select kernel is (query tile, split): the rows of one query tile against the candidate tiles
// [split * tiles_per_split, (split + 1) * tiles_per_split).  Splits exist so that few query rows still fill the chip: as many as
// bring the items to the grid cap, never more than there are candidate tiles, none of them empty.  Every (row, split) leaves its
// L best keys in scratch; the finish kernel, a wave per row, merges them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace wseg {

constexpr int kSelTile = 128;                  // rows (or columns) of a dot-product tile on either side
constexpr int kSelExtra = 8;                   // candidates kept beyond those reported, for the exact re-rank
constexpr int kSelSmallL = 24;                 // lists up to here leave the LDS for two workgroups a CU
constexpr int kSelAlign = 256;                 // bytes
constexpr int kSelGridCap = 2048;              // workgroups of a select kernel: 8 per CU; more items take the grid stride
constexpr int kSelFinishPerCap = 8;            // single-wave workgroups of a finish kernel per unit of the cap
constexpr int64_t kSelMaxRows = INT32_MAX;     // of queries and of corpus: indices are int32

struct SelSplit {
  int32_t splits;                  // candidate splits, 1 .. min(n_tiles, cap)        (0: no query or no candidate tile)
  int32_t tiles_per_split;         // ceil(n_tiles / splits); (splits - 1) * tiles_per_split < n_tiles: no split is empty
  int64_t items;                   // m_tiles * splits                                (<= m_tiles + cap)
  int32_t grid;                    // workgroups of the select kernel, min(items, cap)
};

inline int64_t sel_clamp_cap(int64_t grid_cap) { return grid_cap < 1 ? 1 : grid_cap > kSelGridCap ? kSelGridCap : grid_cap; }

// a scratch region of `bytes` takes this many: a multiple of kSelAlign, at least one
inline int64_t sel_pad(int64_t bytes) { return bytes <= 0 ? kSelAlign : (bytes + kSelAlign - 1) / kSelAlign * kSelAlign; }

// a row count of a call -> 0, or -1 with the argument's name in msg
inline int sel_check_rows(const char* name, int64_t rows, char* msg, size_t msg_len) {
  if (rows >= 0 && rows <= kSelMaxRows) return 0;
  snprintf(msg, msg_len, "%s must be 0 .. 2^31 - 1 (got %lld)", name, (long long)rows);
  return -1;
}

inline SelSplit sel_split(int64_t m_tiles, int64_t n_tiles, int64_t grid_cap) {
  grid_cap = sel_clamp_cap(grid_cap);
  SelSplit s;
  if (m_tiles == 0 || n_tiles == 0) {
    s.splits = 0;
    s.tiles_per_split = 0;
  } else {
    int64_t want = (grid_cap + m_tiles - 1) / m_tiles;           // splits that bring the items to the cap
    if (want > n_tiles) want = n_tiles;
    s.tiles_per_split = (int32_t)((n_tiles + want - 1) / want);
    s.splits = (int32_t)((n_tiles + s.tiles_per_split - 1) / s.tiles_per_split);
  }
  s.items = m_tiles * s.splits;
  s.grid = (int32_t)(s.items < grid_cap ? s.items : grid_cap);
  return s;
}

// the grid of the single-wave kernels (a finish kernel, dtw_pairs_kernel) over `work` rows or pairs under the cap
inline int32_t sel_wave_grid(int64_t work, int64_t grid_cap) {
  const int64_t cap = sel_clamp_cap(grid_cap) * kSelFinishPerCap;
  return (int32_t)(work < 0 ? 0 : work < cap ? work : cap);
}

// the grid of a norms kernel (256 rows or columns a round) over `work` of them under the cap
inline int32_t sel_norm_grid(int64_t work, int64_t grid_cap) {
  const int64_t rounds = (work + 255) / 256, cap = sel_clamp_cap(grid_cap);
  return (int32_t)(rounds < cap ? rounds : cap);
}

// The keys region is SIZED for min(rows * n_tiles, rows + per_cap * cap) lists, `rows` the query rows rounded up to whole tiles
// (per_cap: the most rows of a tile) — a bound of rows * splits (splits <= n_tiles, m_tiles * splits <= m_tiles + cap) that grows
// with every size and with the cap, so that a scratch size is monotone although the split count is not, and a call under a smaller
// cap (the test knobs) fits the size reported for the default one.
inline int64_t sel_lists_bound(int64_t rows, int64_t n_tiles, int64_t per_cap, int64_t grid_cap) {
  const int64_t pairs = rows * n_tiles, capped = rows + per_cap * sel_clamp_cap(grid_cap);
  return pairs < capped ? pairs : capped;
}

}  // namespace wseg
