// Host-only check of the validation and launch plan of wseg_pca_scratch_bytes / wseg_pca_moments_f64 / wseg_pca_project_f64
// (whisperseg_amd/csrc/wseg_pca_plan.h: plain C++, no HIP) over a grid of (n, d, cap) up to the limits n = 2^31 - 1, d = 8192: the
// arithmetic must stay inside int64 and int32, and the plan must keep what the launches rely on.  Build it under the host sanitizer
// and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/pca_plan_check.cpp \
//       -o pca_plan_check && ./pca_plan_check
//
// It fails unless: the tiles (bi, bj) of pca_tile_blocks cover the triangle bi <= bj < nb exactly once, in the documented order; the
// splits of pca_split_rows cover the rows 0 .. n - 1 exactly once, none empty, every one but the last a multiple of the row chunk;
// the split count, the rows of a split and the scratch size do not depend on the cap; the grids are 1 .. the cap and never larger
// than the items; the partial tiles and the partial sums of a plan with more than one split lie in their regions, which neither
// overlap nor exceed the reported size; the size is positive, aligned and monotone in n and in d; the largest element offsets
// (n * d floats, items * 4096 doubles) stay inside int64.  Invalid sizes must be rejected with the argument's name.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../whisperseg_amd/csrc/wseg_pca_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

int main() {
  int bad = 0;
  const int64_t rows[] = {1, 2, 3, 5, 31, 32, 33, 63, 65, 255, 256, 257, 511, 513, 1027, 4096, 100000, 1000000, 1048577, 123456789, INT32_MAX};
  const int32_t cols[] = {1, 15, 16, 17, 63, 64, 65, 80, 127, 128, 129, 130, 640, 1280, 2560, 2561, 2879, 2880, 2881, 5120, 8191, 8192};
  const int64_t caps[] = {1, 3, 256, kPcaGridCap, 1000000};
  const size_t n_rows = sizeof(rows) / sizeof(rows[0]), n_cols = sizeof(cols) / sizeof(cols[0]);
  std::vector<int64_t> size_of(n_rows * n_cols, 0);
  int64_t plans = 0, most_items = 0, most_splits = 0;
  for (size_t a = 0; a < n_rows; ++a) {
    for (size_t b = 0; b < n_cols; ++b) {
      const int64_t n = rows[a];
      const int32_t d = cols[b];
      PcaPlan first = {};
      for (const int64_t cap : caps) {
        PcaPlan p;
        if (pca_plan(n, d, cap, &p, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++bad; continue; }
        ++plans;
        const int64_t eff = cap < kPcaGridCap ? cap : kPcaGridCap;
        bool ok = p.n == n && p.d == d && p.nb == (d + kPcaBlock - 1) / kPcaBlock && p.tiles == p.nb * (p.nb + 1) / 2;
        // the splits: every row once, none empty, chunk multiples
        ok = ok && p.splits >= 1 && p.rows_per_split >= 1 && p.rows_per_split % kPcaChunk == 0 && (int64_t)(p.splits - 1) * p.rows_per_split < n &&
             (int64_t)p.splits * p.rows_per_split >= n && p.splits <= (n + kPcaMinSplitRows - 1) / kPcaMinSplitRows &&
             (int64_t)p.splits * p.tiles < p.tiles + kPcaTargetItems;
        long long next = 0;
        for (int s = 0; ok && s < p.splits; ++s) {
          long long r0, r1;
          pca_split_rows(n, p.rows_per_split, s, &r0, &r1);
          ok = r0 == next && r1 > r0 && r1 <= n && (r0 % kPcaChunk == 0);
          next = r1;
        }
        ok = ok && next == n;
        // the tiles: the triangle once, row by row
        if (ok && cap == caps[0]) {
          int want_i = 0, want_j = 0;
          for (int t = 0; ok && t < p.tiles; ++t) {
            int bi, bj;
            pca_tile_blocks(p.nb, t, &bi, &bj);
            ok = bi == want_i && bj == want_j && bi <= bj && bj < p.nb;
            if (++want_j == p.nb) { ++want_i; want_j = want_i; }
          }
          ok = ok && want_i == p.nb;
        }
        // the grids
        ok = ok && p.items == (int64_t)p.tiles * p.splits && p.grid >= 1 && p.grid <= eff && p.grid <= p.items && (p.grid == p.items || p.grid == eff) &&
             (p.splits > 1 ? p.finish_grid >= 1 && p.finish_grid <= eff && p.finish_grid <= p.tiles : p.finish_grid == 0) &&
             p.row_tiles == (n + kPcaRowTile - 1) / kPcaRowTile && p.project_grid >= 1 && p.project_grid <= eff && p.project_grid <= p.row_tiles;
        // the scratch: regions inside, apart, aligned
        ok = ok && p.scratch_bytes > 0 && p.scratch_bytes % kPcaAlign == 0 && p.partial_offset == 0 && p.sums_offset % kPcaAlign == 0 &&
             p.partial_offset + p.partial_bytes <= p.sums_offset && p.sums_offset + p.sums_bytes <= p.scratch_bytes &&
             p.scratch_bytes <= ((int64_t)2 * kPcaTargetItems * (kPcaBlock * kPcaBlock + kPcaBlock) * 8 + 2 * kPcaAlign);
        if (p.splits > 1) {
          ok = ok && p.items <= p.capacity_items && p.partial_bytes == p.items * kPcaBlock * kPcaBlock * 8 &&
               p.sums_bytes == (int64_t)p.splits * p.nb * kPcaBlock * 8 && (int64_t)p.splits * p.nb <= p.capacity_items;
        } else {
          ok = ok && p.partial_bytes == 0 && p.sums_bytes == 0;
        }
        // the cap changes the grids alone
        if (cap == caps[0]) first = p;
        ok = ok && p.splits == first.splits && p.rows_per_split == first.rows_per_split && p.scratch_bytes == first.scratch_bytes &&
             p.sums_offset == first.sums_offset && p.items == first.items;
        // the offsets a lane forms
        ok = ok && n <= INT64_MAX / ((int64_t)d * 4) && p.items <= INT64_MAX / (kPcaBlock * kPcaBlock * 8) && (int64_t)d * d * 8 <= INT64_MAX / 2;
        if (!ok) { std::printf("  a broken plan: n %lld, d %d, cap %lld\n", (long long)n, (int)d, (long long)cap); ++bad; }
        if (p.items > most_items) most_items = p.items;
        if (p.splits > most_splits) most_splits = p.splits;
        size_of[a * n_cols + b] = p.scratch_bytes;
        for (int32_t r : {1, 15, 16, 17, 33, 64}) {
          PcaPlan q;
          if (pca_project_plan(n, d, r, cap, &q, msg, sizeof(msg)) || q.r != r || q.project_grid != p.project_grid || q.row_tiles != p.row_tiles) {
            std::printf("  a broken projection plan: n %lld, d %d, r %d\n", (long long)n, (int)d, (int)r);
            ++bad;
          }
        }
      }
      if (a && size_of[a * n_cols + b] < size_of[(a - 1) * n_cols + b]) { std::printf("  not monotone in n at n %lld, d %d\n", (long long)n, (int)d); ++bad; }
      if (b && size_of[a * n_cols + b] < size_of[a * n_cols + b - 1]) { std::printf("  not monotone in d at n %lld, d %d\n", (long long)n, (int)d); ++bad; }
    }
  }
  PcaPlan p;
  if (!rejected(pca_plan(0, 5, 1, &p, msg, sizeof(msg)), "n must") || !rejected(pca_plan(-1, 5, 1, &p, msg, sizeof(msg)), "n must") ||
      !rejected(pca_plan((int64_t)INT32_MAX + 1, 5, 1, &p, msg, sizeof(msg)), "n must") || !rejected(pca_plan(INT64_MIN, 5, 1, &p, msg, sizeof(msg)), "n must") ||
      !rejected(pca_plan(INT64_MAX, 5, 1, &p, msg, sizeof(msg)), "n must") || !rejected(pca_plan(5, 0, 1, &p, msg, sizeof(msg)), "d must") ||
      !rejected(pca_plan(5, kPcaMaxD + 1, 1, &p, msg, sizeof(msg)), "d must") || !rejected(pca_plan(5, INT32_MIN, 1, &p, msg, sizeof(msg)), "d must") ||
      !rejected(pca_plan(5, INT32_MAX, 1, &p, msg, sizeof(msg)), "d must") || !rejected(pca_project_plan(5, 5, 0, 1, &p, msg, sizeof(msg)), "r must") ||
      !rejected(pca_project_plan(5, 5, kPcaMaxR + 1, 1, &p, msg, sizeof(msg)), "r must") || !rejected(pca_project_plan(5, 5, INT32_MIN, 1, &p, msg, sizeof(msg)), "r must") ||
      !rejected(pca_project_plan(0, 5, 3, 1, &p, msg, sizeof(msg)), "n must") || !rejected(pca_project_plan(5, 0, 3, 1, &p, msg, sizeof(msg)), "d must") ||
      pca_plan(5, 5, INT64_MIN, &p, msg, sizeof(msg)) || p.grid != 1 || pca_plan(5, 5, INT64_MAX, &p, msg, sizeof(msg))) {
    std::printf("  valid input is refused or invalid input accepted (%s)\n", msg);
    ++bad;
  }
  std::printf("%lld plans up to 2^31 - 1 rows of 8192 columns: at most %lld items, %lld splits\n", (long long)plans, (long long)most_items, (long long)most_splits);
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
