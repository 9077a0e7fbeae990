// The host arithmetic of one Boruvka round of the mutual-reachability minimum spanning tree (wseg_mst_scratch_bytes /
// wseg_mst_round_f32), in one place: the validation of a call, the row tiles, the candidate splits, the grids under the cap and
// the layout of the scratch the kernels of wseg_mst.hip share.  Plain C++ with no HIP dependency, so that a host-only program can
// run it under a sanitizer (tools/mst_plan_check.cpp).  It follows wseg_knn_plan.h with queries == corpus.
//
// A WORK ITEM of mst_select_kernel is (row tile, split): kMstTile = 128 rows against the candidate tiles (128 candidates each)
// [split * tiles_per_split, (split + 1) * tiles_per_split).  Splits exist so that few rows still fill the chip: as many as bring
// the items to the grid cap, never more than there are tiles, none of them empty.  Every (row, split) leaves its kMstL = 1 + 8 best
// keys in scratch.  Scratch, in this order, every region padded to kMstAlign bytes (at least one pad):
//   float    norm[n]                          |x_i|^2 as the c-ordered fmaf chain
//   uint64   keys[tiles * 128][splits][9]     (ordered w^ << 32) | j, ascending; all ones: no candidate
// The keys region is SIZED for min(tiles * tiles, tiles + cap) items of 128 rows — a bound of tiles * splits that grows with n and
// the cap, so that wseg_mst_scratch_bytes is monotone although the split count is not — and a call under a smaller cap
// ($WSEG_MST_GRID) fits the size reported for the default one.  The size does not depend on d.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace wseg {

constexpr int kMstTile = 128;                  // rows of a work item; candidates of a tile
constexpr int kMstExtra = 8;                   // candidates kept beyond the one for the exact re-rank
constexpr int kMstL = 1 + kMstExtra;           // entries of a row's list
constexpr int kMstMaxD = 20480;                // columns: 80 x 256, the widest patch
constexpr int kMstAlign = 256;                 // bytes
constexpr int kMstGridCap = 2048;              // workgroups of mst_select_kernel: 8 per CU; more items take the grid stride
constexpr int kMstFinishPerCap = 8;            // single-wave workgroups of mst_finish_kernel per unit of the cap
constexpr int64_t kMstMaxRows = INT32_MAX;     // indices are int32

struct MstPlan {
  int64_t n;
  int32_t d;
  int64_t tiles;                   // ceil(n / 128)                                   (<= 2^24)
  int32_t splits;                  // candidate splits, 1 .. min(tiles, cap)          (0: no row)
  int32_t tiles_per_split;         // ceil(tiles / splits); (splits - 1) * tiles_per_split < tiles: no split is empty
  int64_t items;                   // tiles * splits                                  (<= 2^24 + cap)
  int32_t grid;                    // workgroups of mst_select_kernel, min(items, cap)
  int32_t finish_grid;             // workgroups of mst_finish_kernel, one row at a time each
  int32_t norm_grid;               // workgroups (256 rows a round) of mst_norms_kernel
  int64_t norm_offset, norm_bytes, keys_offset, keys_bytes, keys_capacity, scratch_bytes;
};

inline int64_t mst_pad(int64_t bytes) { return bytes <= 0 ? kMstAlign : (bytes + kMstAlign - 1) / kMstAlign * kMstAlign; }

// Validates the sizes of a call and fills the plan -> 0, or -1 with the argument's name in msg.  n == 0 is valid.
inline int mst_plan(int64_t n, int32_t d, int64_t grid_cap, MstPlan* plan, char* msg, size_t msg_len) {
  if (d < 1 || d > kMstMaxD) { snprintf(msg, msg_len, "d must be 1 .. %d (got %d)", kMstMaxD, (int)d); return -1; }
  if (n < 0 || n > kMstMaxRows) { snprintf(msg, msg_len, "n must be 0 .. 2^31 - 1 (got %lld)", (long long)n); return -1; }
  if (grid_cap < 1) grid_cap = 1;
  if (grid_cap > kMstGridCap) grid_cap = kMstGridCap;
  MstPlan p;
  p.n = n;
  p.d = d;
  p.tiles = (n + kMstTile - 1) / kMstTile;
  if (p.tiles == 0) {
    p.splits = 0;
    p.tiles_per_split = 0;
  } else {
    int64_t want = (grid_cap + p.tiles - 1) / p.tiles;           // splits that bring the items to the cap
    if (want > p.tiles) want = p.tiles;
    p.tiles_per_split = (int32_t)((p.tiles + want - 1) / want);
    p.splits = (int32_t)((p.tiles + p.tiles_per_split - 1) / p.tiles_per_split);
  }
  p.items = p.tiles * p.splits;
  p.grid = (int32_t)(p.items < grid_cap ? p.items : grid_cap);
  const int64_t finish_cap = grid_cap * kMstFinishPerCap;
  p.finish_grid = (int32_t)(n < finish_cap ? n : finish_cap);
  const int64_t norm_rounds = (n + 255) / 256;
  p.norm_grid = (int32_t)(norm_rounds < grid_cap ? norm_rounds : grid_cap);
  const int64_t pairs = p.tiles * p.tiles, capped = p.tiles + grid_cap;
  const int64_t items_bound = pairs < capped ? pairs : capped;
  p.norm_offset = 0;
  p.norm_bytes = 4 * n;
  p.keys_offset = mst_pad(p.norm_bytes);
  p.keys_bytes = p.items * kMstTile * kMstL * 8;
  p.keys_capacity = items_bound * kMstTile * kMstL * 8;
  p.scratch_bytes = p.keys_offset + mst_pad(p.keys_capacity);
  *plan = p;
  return 0;
}

}  // namespace wseg
