// The host arithmetic of the principal-component kernels (wseg_pca_scratch_bytes / wseg_pca_moments_f64 / wseg_pca_project_f64), in
// one place: the validation of a call, the column tiles of the Gram matrix, the row splits, the grids under the cap and the layout of
// the scratch.  Plain C++ with no HIP dependency, so that a host-only program can run it under a sanitizer
// (tools/pca_plan_check.cpp); the two index functions the kernels share with the host carry WSEG_PCA_HD.
//
// The Gram matrix S = X^T X of d columns is cut into BLOCKS of kPcaBlock = 64 columns, nb = ceil(d / 64) of them a side.  A TILE is
// a pair of blocks (bi, bj) with bi <= bj — only the tiles on and above the diagonal are computed, nb (nb + 1) / 2 of them, numbered
// row by row: (0, 0), (0, 1) .. (0, nb - 1), (1, 1) .. — and the mirror is written from the same values.  Few columns are few tiles,
// so the n rows are cut into SPLITS of rows_per_split rows (a multiple of the row chunk kPcaChunk = 32; the last split may be short,
// none is empty).  The split count is a function of (n, d) ALONE: as many as bring tiles * splits to kPcaTargetItems, never more than
// one per kPcaMinSplitRows rows.  A WORK ITEM of pca_moments_kernel is (split, tile), item = split * tiles + tile; the grid strides
// over the items, so the cap ($WSEG_PCA_GRID) only changes which workgroup takes which item.
// With one split an item writes S (and the column sums, from the diagonal tiles) directly.  With more, every item leaves its 64 x 64
// partial tile — and a diagonal tile its 64 partial column sums — in the scratch, and pca_finish_kernel adds them in ascending split
// order.  Scratch, in this order, both regions padded to kPcaAlign bytes (at least one pad):
//   double   partial[items][64][64]        item = split * tiles + tile
//   double   sums[splits][nb][64]
// The regions are SIZED for min(tiles * ceil(n / 256), tiles + 1024, 2048) items — a bound of tiles * splits (splits > 1 only where
// tiles < 1024) that grows with n and d, so that wseg_pca_scratch_bytes is monotone although the split count is not.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define WSEG_PCA_HD __host__ __device__
#else
#define WSEG_PCA_HD
#endif

namespace wseg {

constexpr int kPcaMaxD = 8192;                 // columns: the float64 Gram matrix is then 512 MiB
constexpr int kPcaMaxR = 64;                   // components of a projection
constexpr int kPcaBlock = 64;                  // columns of a block: 4 MFMA tiles of 16, one 16-row strip per wave
constexpr int kPcaChunk = 32;                  // rows of the LDS image of the moments kernel: 8 k-steps of 4
constexpr int kPcaRowTile = 64;                // rows of a work item of the projection: 16 per wave
constexpr int kPcaColChunk = 32;               // columns of the LDS image of the projection: 8 k-steps of 4
constexpr int kPcaMinSplitRows = 256;          // no split is planned shorter than this
constexpr int kPcaTargetItems = 1024;          // tiles * splits the row splits aim for: 4 workgroups per CU
constexpr int kPcaGridCap = 2048;              // workgroups of a launch; more items take the grid stride
constexpr int kPcaAlign = 256;                 // bytes
constexpr int64_t kPcaMaxRows = INT32_MAX;

struct PcaPlan {
  int64_t n;
  int32_t d, r;
  int32_t nb;                      // ceil(d / 64)                                      (<= 128)
  int32_t tiles;                   // nb (nb + 1) / 2                                   (<= 8256)
  int32_t splits;                  // 1 .. min(ceil(1024 / tiles), ceil(n / 256))
  int64_t rows_per_split;          // a multiple of 32; (splits - 1) * rows_per_split < n
  int64_t items;                   // tiles * splits                                    (< tiles + 1024)
  int32_t grid;                    // workgroups of pca_moments_kernel, min(items, cap)
  int32_t finish_grid;             // workgroups of pca_finish_kernel, min(tiles, cap); 0 with one split
  int64_t row_tiles;               // ceil(n / 64): the items of the projection
  int32_t project_grid;            // min(row_tiles, cap)
  int64_t capacity_items;          // what the scratch is sized for
  int64_t partial_offset, partial_bytes, sums_offset, sums_bytes, scratch_bytes;
};

inline int64_t pca_pad(int64_t bytes) { return bytes <= 0 ? kPcaAlign : (bytes + kPcaAlign - 1) / kPcaAlign * kPcaAlign; }

// tile -> (bi, bj), bi <= bj, of nb blocks a side: row bi of the triangle holds nb - bi tiles
WSEG_PCA_HD inline void pca_tile_blocks(int nb, int tile, int* bi, int* bj) {
  int row = 0;
  while (tile >= nb - row) { tile -= nb - row; ++row; }
  *bi = row;
  *bj = row + tile;
}

// the rows [begin, end) of a split
WSEG_PCA_HD inline void pca_split_rows(long long n, long long rows_per_split, int split, long long* begin, long long* end) {
  const long long b = (long long)split * rows_per_split, e = b + rows_per_split;
  *begin = b < n ? b : n;
  *end = e < n ? e : n;
}

// Validates the sizes of a moments call and fills the plan -> 0, or -1 with the argument's name in msg.
inline int pca_plan(int64_t n, int32_t d, int64_t grid_cap, PcaPlan* plan, char* msg, size_t msg_len) {
  if (d < 1 || d > kPcaMaxD) { snprintf(msg, msg_len, "d must be 1 .. %d (got %d)", kPcaMaxD, (int)d); return -1; }
  if (n < 1 || n > kPcaMaxRows) { snprintf(msg, msg_len, "n must be 1 .. 2^31 - 1 (got %lld)", (long long)n); return -1; }
  if (grid_cap < 1) grid_cap = 1;
  if (grid_cap > kPcaGridCap) grid_cap = kPcaGridCap;
  PcaPlan p = {};
  p.n = n;
  p.d = d;
  p.nb = (d + kPcaBlock - 1) / kPcaBlock;
  p.tiles = p.nb * (p.nb + 1) / 2;
  const int64_t want = (kPcaTargetItems + p.tiles - 1) / p.tiles;                   // splits that bring the items to the target
  const int64_t by_rows = (n + kPcaMinSplitRows - 1) / kPcaMinSplitRows;
  const int64_t s = want < by_rows ? want : by_rows;                                // >= 1
  p.rows_per_split = ((n + s - 1) / s + kPcaChunk - 1) / kPcaChunk * kPcaChunk;
  p.splits = (int32_t)((n + p.rows_per_split - 1) / p.rows_per_split);
  p.items = (int64_t)p.tiles * p.splits;
  p.grid = (int32_t)(p.items < grid_cap ? p.items : grid_cap);
  p.finish_grid = p.splits > 1 ? (int32_t)(p.tiles < grid_cap ? p.tiles : grid_cap) : 0;
  p.row_tiles = (n + kPcaRowTile - 1) / kPcaRowTile;
  p.project_grid = (int32_t)(p.row_tiles < grid_cap ? p.row_tiles : grid_cap);
  int64_t bound = p.tiles * by_rows;
  if (bound > p.tiles + kPcaTargetItems) bound = p.tiles + kPcaTargetItems;
  if (bound > 2 * kPcaTargetItems) bound = 2 * kPcaTargetItems;
  p.capacity_items = bound;
  p.partial_offset = 0;
  p.partial_bytes = p.splits > 1 ? p.items * kPcaBlock * kPcaBlock * 8 : 0;
  p.sums_offset = pca_pad(bound * kPcaBlock * kPcaBlock * 8);
  p.sums_bytes = p.splits > 1 ? (int64_t)p.splits * p.nb * kPcaBlock * 8 : 0;
  p.scratch_bytes = p.sums_offset + pca_pad(bound * kPcaBlock * 8);
  *plan = p;
  return 0;
}

// Validates the sizes of a projection and fills n, d, r, row_tiles and project_grid -> 0, or -1 with the argument's name in msg.
inline int pca_project_plan(int64_t n, int32_t d, int32_t r, int64_t grid_cap, PcaPlan* plan, char* msg, size_t msg_len) {
  if (r < 1 || r > kPcaMaxR) { snprintf(msg, msg_len, "r must be 1 .. %d (got %d)", kPcaMaxR, (int)r); return -1; }
  if (pca_plan(n, d, grid_cap, plan, msg, msg_len)) return -1;
  plan->r = r;
  return 0;
}

}  // namespace wseg
