// Host-only check of the validation and launch plan of wseg_knn_scratch_bytes / wseg_knn_f32 (whisperseg_amd/csrc/wseg_knn_plan.h:
// plain C++, no HIP) over the limits: m, n in {0, 1, 63, 64, 65, 2^31 - 1}, d in {1, 20 480}, k in {1, 64} and every grid cap from 1
// to the default: the arithmetic must stay inside int64 and int32, and the plan must keep what the kernels rely on.  Build it under
// the host sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/knn_plan_check.cpp \
//       -o knn_plan_check && ./knn_plan_check
//
// It fails unless: the tiles cover the rows with less than one tile to spare; the splits are 1 .. min(candidate tiles, cap), none of
// them empty, and together cover every candidate tile; the grids are 1 .. cap (the finish grid 1 .. 8 cap) and never more than
// their work (0 without work); the three scratch regions follow each other on their alignment without overlap and fit in the
// reported size, the keys of the last (row, split) and the last elements of queries, corpus and the outputs stay inside int64; the
// size under a smaller cap never exceeds the size under the default cap (what wseg_knn_scratch_bytes reports) and the reported size
// is monotone in m, n and k.  Invalid sizes must be rejected with the argument's name.  Prints one line per (d, k).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "../whisperseg_amd/csrc/wseg_knn_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

int main() {
  int bad = 0;
  const int64_t sizes[] = {0, 1, 63, 64, 65, INT32_MAX};
  for (const int32_t d : {1, kKnnMaxD}) {
    for (const int32_t k : {1, kKnnMaxK}) {
      int fails = 0;
      int64_t plans = 0;
      for (const int64_t m : sizes) {
        for (const int64_t n : sizes) {
          KnnPlan whole;
          if (knn_plan(m, n, d, k, kKnnGridCap, &whole, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; continue; }
          for (int64_t cap = 1; cap <= kKnnGridCap; ++cap) {
            KnnPlan p;
            if (knn_plan(m, n, d, k, cap, &p, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; break; }
            ++plans;
            bool ok = p.m == m && p.n == n && p.d == d && p.k == k && p.L == k + kKnnExtra && p.L <= kKnnMaxL &&
                      p.m_tiles * kKnnTile >= m && (p.m_tiles == 0 ? m == 0 : (p.m_tiles - 1) * kKnnTile < m) &&
                      p.n_tiles * kKnnTile >= n && (p.n_tiles == 0 ? n == 0 : (p.n_tiles - 1) * kKnnTile < n);
            if (m == 0 || n == 0) {
              ok = ok && p.splits == 0 && p.items == 0 && p.grid == 0 && p.keys_bytes == 0;
            } else {
              ok = ok && p.splits >= 1 && p.splits <= cap && p.splits <= p.n_tiles && p.tiles_per_split >= 1 &&
                   (int64_t)p.splits * p.tiles_per_split >= p.n_tiles && (int64_t)(p.splits - 1) * p.tiles_per_split < p.n_tiles &&
                   p.items == p.m_tiles * p.splits && p.grid >= 1 && p.grid <= cap && p.grid <= p.items;
            }
            ok = ok && (m == 0 ? p.finish_grid == 0 : (p.finish_grid >= 1 && p.finish_grid <= cap * kKnnFinishPerCap && p.finish_grid <= m));
            ok = ok && (m + n == 0 ? p.norm_grid == 0 : (p.norm_grid >= 1 && p.norm_grid <= cap && (int64_t)(p.norm_grid - 1) * 256 < m + n));
            // the regions: in order, aligned, no overlap, inside the reported size
            ok = ok && p.qnorm_offset == 0 && p.qnorm_bytes == 4 * m && p.xnorm_offset % kKnnAlign == 0 && p.xnorm_offset >= p.qnorm_offset + p.qnorm_bytes &&
                 p.xnorm_bytes == 4 * n && p.keys_offset % kKnnAlign == 0 && p.keys_offset >= p.xnorm_offset + p.xnorm_bytes &&
                 p.keys_bytes == p.items * kKnnTile * p.L * 8 && p.keys_bytes <= p.keys_capacity &&
                 p.scratch_bytes >= p.keys_offset + p.keys_capacity && p.scratch_bytes % kKnnAlign == 0 && p.scratch_bytes > 0;
            // the last key the selection kernel writes and the finish kernel reads: row m_tiles * 128 - 1, the last split, entry L - 1
            if (p.items > 0) {
              const int64_t last = ((p.m_tiles * kKnnTile - 1) * p.splits + (p.splits - 1)) * p.L + (p.L - 1);
              ok = ok && last >= 0 && (last + 1) * 8 == p.keys_bytes;
            }
            // element offsets the kernels form, and the grid-stride's last step
            ok = ok && m * (int64_t)d <= INT64_MAX / 4 && n * (int64_t)d <= INT64_MAX / 4 && m * (int64_t)k <= INT64_MAX / 4 &&
                 p.items + cap < INT64_MAX && (m + n) + cap * 256 < INT64_MAX;
            // what wseg_knn_scratch_bytes reports (the default cap) holds every smaller cap's plan
            ok = ok && p.scratch_bytes <= whole.scratch_bytes;
            if (!ok) { std::printf("  a broken plan: m %lld, n %lld, d %d, k %d, cap %lld\n", (long long)m, (long long)n, (int)d, (int)k, (long long)cap); ++fails; break; }
          }
        }
      }
      // monotone in m, n and k under the default cap — although the split count is not
      int64_t before_m = 0;
      for (const int64_t m : {0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4096, 100000, 131072, 131073, 10000000, (int)INT32_MAX}) {
        int64_t before_n = 0;
        for (const int64_t n : {0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4096, 100000, 131072, 131073, 10000000, (int)INT32_MAX}) {
          KnnPlan p, q;
          if (knn_plan(m, n, d, k, kKnnGridCap, &p, msg, sizeof(msg))) { ++fails; continue; }
          if (p.scratch_bytes < before_n) { std::printf("  not monotone in n at m %lld, n %lld\n", (long long)m, (long long)n); ++fails; }
          before_n = p.scratch_bytes;
          if (k < kKnnMaxK && (knn_plan(m, n, d, k + 1, kKnnGridCap, &q, msg, sizeof(msg)) || q.scratch_bytes < p.scratch_bytes)) {
            std::printf("  not monotone in k at m %lld, n %lld\n", (long long)m, (long long)n); ++fails;
          }
          if (n == INT32_MAX) {
            if (p.scratch_bytes < before_m) { std::printf("  not monotone in m at m %lld\n", (long long)m); ++fails; }
            before_m = p.scratch_bytes;
          }
        }
      }
      KnnPlan p;
      if (knn_plan(5, 5, d, k, kKnnGridCap, &p, msg, sizeof(msg)) || knn_plan(5, 5, d, k, 0, &p, msg, sizeof(msg)) || p.grid != 1 ||
          knn_plan(5, 5, d, k, INT64_MAX, &p, msg, sizeof(msg)) || p.grid != 1 ||
          !rejected(knn_plan(-1, 5, d, k, 1, &p, msg, sizeof(msg)), "m must") || !rejected(knn_plan((int64_t)INT32_MAX + 1, 5, d, k, 1, &p, msg, sizeof(msg)), "m must") ||
          !rejected(knn_plan(5, -1, d, k, 1, &p, msg, sizeof(msg)), "n must") || !rejected(knn_plan(5, (int64_t)INT32_MAX + 1, d, k, 1, &p, msg, sizeof(msg)), "n must") ||
          !rejected(knn_plan(5, INT64_MIN, d, k, 1, &p, msg, sizeof(msg)), "n must") || !rejected(knn_plan(INT64_MAX, 5, d, k, 1, &p, msg, sizeof(msg)), "m must") ||
          !rejected(knn_plan(5, 5, 0, k, 1, &p, msg, sizeof(msg)), "d must") || !rejected(knn_plan(5, 5, kKnnMaxD + 1, k, 1, &p, msg, sizeof(msg)), "d must") ||
          !rejected(knn_plan(5, 5, INT32_MIN, k, 1, &p, msg, sizeof(msg)), "d must") || !rejected(knn_plan(5, 5, INT32_MAX, k, 1, &p, msg, sizeof(msg)), "d must") ||
          !rejected(knn_plan(5, 5, d, 0, 1, &p, msg, sizeof(msg)), "k must") || !rejected(knn_plan(5, 5, d, kKnnMaxK + 1, 1, &p, msg, sizeof(msg)), "k must") ||
          !rejected(knn_plan(5, 5, d, INT32_MIN, 1, &p, msg, sizeof(msg)), "k must") || !rejected(knn_plan(5, 5, d, INT32_MAX, 1, &p, msg, sizeof(msg)), "k must")) {
        std::printf("  valid input is refused or invalid input accepted (%s)\n", msg); ++fails;
      }
      std::printf("d %5d, k %2d: %lld plans up to 2^31 - 1 rows on both sides, caps 1 .. %d: %s\n", (int)d, (int)k, (long long)plans, kKnnGridCap,
                  fails ? "FAILED" : "ok");
      bad += fails;
    }
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
