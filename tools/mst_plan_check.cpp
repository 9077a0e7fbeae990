// Host-only check of the validation and launch plan of wseg_mst_scratch_bytes / wseg_mst_round_f32 (whisperseg_amd/csrc/
// wseg_mst_plan.h: plain C++, no HIP) over the limits: n in {0, 1, 127, 128, 129, ..., 2^31 - 1}, d in {1, 20 480} and every grid cap
// from 1 to the default: the arithmetic must stay inside int64 and int32, and the plan must keep what the kernels rely on.  Build it
// under the host sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/mst_plan_check.cpp \
//       -o mst_plan_check && ./mst_plan_check
//
// It fails unless: the tiles cover the rows with less than one tile to spare; the splits are 1 .. min(tiles, cap), none of them
// empty, and together cover every tile; the grids are 1 .. cap (the finish grid 1 .. 8 cap) and never more than their work (0
// without work); the two scratch regions follow each other on their alignment without overlap and fit in the reported size, the keys
// of the last (row, split) and the last element of the rows stay inside int64; the size under a smaller cap never exceeds the size
// under the default cap (what wseg_mst_scratch_bytes reports) and the reported size is monotone in n and the same for every d.
// Invalid sizes must be rejected with the argument's name.  Prints one line per d.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "../whisperseg_amd/csrc/wseg_mst_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

int main() {
  int bad = 0;
  const int64_t sizes[] = {0, 1, 2, 127, 128, 129, 255, 256, 257, 1000, 4096, 100000, 262144, 262145, 10000000, INT32_MAX};
  int64_t reported[sizeof(sizes) / sizeof(sizes[0])] = {};
  for (const int32_t d : {1, kMstMaxD}) {
    int fails = 0;
    int64_t plans = 0, before = 0;
    int at = 0;
    for (const int64_t n : sizes) {
      MstPlan whole;
      if (mst_plan(n, d, kMstGridCap, &whole, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; continue; }
      if (whole.scratch_bytes < before) { std::printf("  not monotone in n at %lld\n", (long long)n); ++fails; }
      before = whole.scratch_bytes;
      if (d != 1 && reported[at] != whole.scratch_bytes) { std::printf("  the size depends on d at n %lld\n", (long long)n); ++fails; }
      reported[at++] = whole.scratch_bytes;
      for (int64_t cap = 1; cap <= kMstGridCap; ++cap) {
        MstPlan p;
        if (mst_plan(n, d, cap, &p, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; break; }
        ++plans;
        bool ok = p.n == n && p.d == d && p.tiles * kMstTile >= n && (p.tiles == 0 ? n == 0 : (p.tiles - 1) * kMstTile < n);
        if (n == 0) {
          ok = ok && p.splits == 0 && p.items == 0 && p.grid == 0 && p.keys_bytes == 0 && p.finish_grid == 0 && p.norm_grid == 0;
        } else {
          ok = ok && p.splits >= 1 && p.splits <= cap && p.splits <= p.tiles && p.tiles_per_split >= 1 &&
               (int64_t)p.splits * p.tiles_per_split >= p.tiles && (int64_t)(p.splits - 1) * p.tiles_per_split < p.tiles &&
               p.items == p.tiles * p.splits && p.grid >= 1 && p.grid <= cap && p.grid <= p.items &&
               p.finish_grid >= 1 && p.finish_grid <= cap * kMstFinishPerCap && p.finish_grid <= n &&
               p.norm_grid >= 1 && p.norm_grid <= cap && (int64_t)(p.norm_grid - 1) * 256 < n;
        }
        // the regions: in order, aligned, no overlap, inside the reported size
        ok = ok && p.norm_offset == 0 && p.norm_bytes == 4 * n && p.keys_offset % kMstAlign == 0 && p.keys_offset >= p.norm_offset + p.norm_bytes &&
             p.keys_bytes == p.items * kMstTile * kMstL * 8 && p.keys_bytes <= p.keys_capacity &&
             p.scratch_bytes >= p.keys_offset + p.keys_capacity && p.scratch_bytes % kMstAlign == 0 && p.scratch_bytes > 0;
        // the last key the selection kernel writes and the finish kernel reads: row tiles * 128 - 1, the last split, entry L - 1
        if (p.items > 0) {
          const int64_t last = ((p.tiles * kMstTile - 1) * p.splits + (p.splits - 1)) * kMstL + (kMstL - 1);
          ok = ok && last >= 0 && (last + 1) * 8 == p.keys_bytes;
        }
        // element offsets the kernels form, and the grid-stride's last step
        ok = ok && n * (int64_t)d <= INT64_MAX / 4 && p.items + cap < INT64_MAX && n + cap * 256 < INT64_MAX;
        // what wseg_mst_scratch_bytes reports (the default cap) holds every smaller cap's plan
        ok = ok && p.scratch_bytes <= whole.scratch_bytes;
        if (!ok) { std::printf("  a broken plan: n %lld, d %d, cap %lld\n", (long long)n, (int)d, (long long)cap); ++fails; break; }
      }
    }
    MstPlan p;
    if (mst_plan(5, d, kMstGridCap, &p, msg, sizeof(msg)) || mst_plan(5, d, 0, &p, msg, sizeof(msg)) || p.grid != 1 ||
        mst_plan(5, d, INT64_MAX, &p, msg, sizeof(msg)) || p.grid != 1 || mst_plan(5, d, INT64_MIN, &p, msg, sizeof(msg)) || p.grid != 1 ||
        !rejected(mst_plan(-1, d, 1, &p, msg, sizeof(msg)), "n must") || !rejected(mst_plan((int64_t)INT32_MAX + 1, d, 1, &p, msg, sizeof(msg)), "n must") ||
        !rejected(mst_plan(INT64_MIN, d, 1, &p, msg, sizeof(msg)), "n must") || !rejected(mst_plan(INT64_MAX, d, 1, &p, msg, sizeof(msg)), "n must") ||
        !rejected(mst_plan(5, 0, 1, &p, msg, sizeof(msg)), "d must") || !rejected(mst_plan(5, kMstMaxD + 1, 1, &p, msg, sizeof(msg)), "d must") ||
        !rejected(mst_plan(5, INT32_MIN, 1, &p, msg, sizeof(msg)), "d must") || !rejected(mst_plan(5, INT32_MAX, 1, &p, msg, sizeof(msg)), "d must")) {
      std::printf("  valid input is refused or invalid input accepted (%s)\n", msg); ++fails;
    }
    std::printf("d %5d: %lld plans up to 2^31 - 1 rows, caps 1 .. %d: %s\n", (int)d, (long long)plans, kMstGridCap, fails ? "FAILED" : "ok");
    bad += fails;
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
