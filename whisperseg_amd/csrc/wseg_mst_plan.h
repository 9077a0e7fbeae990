// The host arithmetic of one Boruvka round of the mutual-reachability minimum spanning tree (wseg_mst_scratch_bytes /
// wseg_mst_round_f32), in one place: the validation of a call, the row tiles and the layout of the scratch the kernels of
// wseg_mst.hip share; the candidate splits, the grids under the cap and the bound that sizes the keys are wseg_select_plan.h's,
// with queries == corpus.  Plain C++ with no HIP dependency, so that a host-only program can run it under a sanitizer
// (tools/mst_plan_check.cpp).
//
// A WORK ITEM of the select kernel is (row tile, split): kMstTile = 128 rows against a split of the candidate tiles (128 candidates
// each).  Every (row, split) leaves its kMstL = 1 + 8 best keys in scratch.  Scratch, in this order, every region padded to
// kMstAlign bytes (at least one pad):
//   float    norm[n]                          |x_i|^2 as the c-ordered fmaf chain
//   uint64   keys[tiles * 128][splits][9]     (ordered w^ << 32) | j, ascending; all ones: no candidate
// The keys region is SIZED for min(tiles * tiles, tiles + cap) items of 128 rows (sel_lists_bound), so that wseg_mst_scratch_bytes
// is monotone in n and the cap, and a call under a smaller cap ($WSEG_MST_GRID) fits the size reported for the default one.  The
// size does not depend on d.
#pragma once
#include "wseg_select_plan.h"

namespace wseg {

constexpr int kMstTile = kSelTile;             // rows of a work item; candidates of a tile
constexpr int kMstExtra = kSelExtra;           // candidates kept beyond the one for the exact re-rank
constexpr int kMstL = 1 + kMstExtra;           // entries of a row's list
constexpr int kMstMaxD = 20480;                // columns: 80 x 256, the widest patch
constexpr int kMstAlign = kSelAlign;           // bytes
constexpr int kMstGridCap = kSelGridCap;       // workgroups of the select kernel
constexpr int kMstFinishPerCap = kSelFinishPerCap;     // single-wave workgroups of mst_finish_kernel per unit of the cap
constexpr int64_t kMstMaxRows = kSelMaxRows;   // indices are int32

struct MstPlan {
  int64_t n;
  int32_t d;
  int64_t tiles;                   // ceil(n / 128)                                   (<= 2^24)
  int32_t splits;                  // candidate splits, 1 .. min(tiles, cap)          (0: no row)
  int32_t tiles_per_split;         // ceil(tiles / splits); (splits - 1) * tiles_per_split < tiles: no split is empty
  int64_t items;                   // tiles * splits                                  (<= 2^24 + cap)
  int32_t grid;                    // workgroups of the select kernel, min(items, cap)
  int32_t finish_grid;             // workgroups of mst_finish_kernel, one row at a time each
  int32_t norm_grid;               // workgroups (256 rows a round) of the norms kernel
  int64_t norm_offset, norm_bytes, keys_offset, keys_bytes, keys_capacity, scratch_bytes;
};

// Validates the sizes of a call and fills the plan -> 0, or -1 with the argument's name in msg.  n == 0 is valid.
inline int mst_plan(int64_t n, int32_t d, int64_t grid_cap, MstPlan* plan, char* msg, size_t msg_len) {
  if (d < 1 || d > kMstMaxD) { snprintf(msg, msg_len, "d must be 1 .. %d (got %d)", kMstMaxD, (int)d); return -1; }
  if (sel_check_rows("n", n, msg, msg_len)) return -1;
  MstPlan p;
  p.n = n;
  p.d = d;
  p.tiles = (n + kMstTile - 1) / kMstTile;
  const SelSplit s = sel_split(p.tiles, p.tiles, grid_cap);
  p.splits = s.splits;
  p.tiles_per_split = s.tiles_per_split;
  p.items = s.items;
  p.grid = s.grid;
  p.finish_grid = sel_wave_grid(n, grid_cap);
  p.norm_grid = sel_norm_grid(n, grid_cap);
  p.norm_offset = 0;
  p.norm_bytes = 4 * n;
  p.keys_offset = sel_pad(p.norm_bytes);
  p.keys_bytes = p.items * kMstTile * kMstL * 8;
  p.keys_capacity = sel_lists_bound(p.tiles * kMstTile, p.tiles, kMstTile, grid_cap) * kMstL * 8;
  p.scratch_bytes = p.keys_offset + sel_pad(p.keys_capacity);
  *plan = p;
  return 0;
}

}  // namespace wseg
