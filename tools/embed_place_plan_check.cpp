// Host-only check of the validation and launch plan of wseg_embed_place_f64 (whisperseg_amd/csrc/wseg_embed_plan.h::embed_place_plan:
// plain C++, no HIP) over the limits: m in {0, 1, 63, 64, 65, ..., 2^31 - 1} new rows, corpora of 1 .. 2^31 - 1 vertices, both dims,
// epoch ranges at the edges of 1 .. 2^31 - 1: the arithmetic must stay inside int64 and int32, and the plan must keep what the launch
// and a lane rely on.  Build it under the host sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/embed_place_plan_check.cpp \
//       -o embed_place_plan_check && ./embed_place_plan_check
//
// It fails unless: the grid is 1 .. the cap, never more than the new rows need (0 without one: nothing is launched), and its
// stride's last step stays inside int64; the plan carries the call's sizes and epochs; the largest offsets a lane forms (m * dim and
// n * dim elements, (t + 1) * rate, the counter's (t * 64 + q) * 16 + s before the key is added) stay inside int64; the window of a
// row a lane reads — entries e0 + q with q < 64 and 0 <= e0 + q < min(e1, nnz) — is computed without overflow for any int64 e0, e1
// and lies inside 0 .. nnz.  Invalid sizes, ranges and parameters must be rejected with the argument's name; m == 0 is valid with
// any corpus, m > 0 needs n >= 1.  Prints one line per dim.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "../whisperseg_amd/csrc/wseg_embed_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

static int plan_of(int64_t m, int64_t nnz, int64_t n, int32_t dim, int64_t t0, int64_t t1, int64_t total, EmbedPlacePlan* p, double lr = 1.0,
                   double a = 1.5, double b = 0.9, double gamma = 1.0, int32_t n_neg = 5) {
  return embed_place_plan(m, nnz, n, dim, t0, t1, total, lr, a, b, gamma, n_neg, p, msg, sizeof(msg));
}

// the window of a row as embed_place_kernel computes it: (first entry, its position in the row, the position it stops at)
struct Window { int64_t first, q_first, q_end; };

static Window window_of(int64_t e0, int64_t e1, int64_t nnz) {
  if (e1 > nnz) e1 = nnz;
  if (e1 < 0) e1 = 0;
  const int64_t first = e0 < 0 ? 0 : e0;
  const int64_t q_first = e0 < 0 ? (e0 < -(int64_t)kEmbedPlaceRow ? (int64_t)kEmbedPlaceRow : -e0) : 0;
  int64_t q_end = q_first + (e1 - first);
  if (q_end > kEmbedPlaceRow) q_end = kEmbedPlaceRow;
  return {first, q_first, q_end};
}

int main() {
  int bad = 0;
  const int64_t sizes[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 4096, 100000, 1048576, 1048577, 10000000, INT32_MAX};
  const int64_t corpora[] = {1, 2, 20000, INT32_MAX};
  const int64_t ranges[][3] = {{0, 1, 1}, {0, 2, 2}, {0, 100, 100}, {0, 20, 50}, {20, 50, 50}, {49, 50, 50}, {7, 8, 200},
                               {0, kEmbedMaxEpochs, kEmbedMaxEpochs}, {kEmbedMaxEpochs - 1, kEmbedMaxEpochs, kEmbedMaxEpochs}};
  for (const int32_t dim : {2, 3}) {
    int fails = 0;
    int64_t plans = 0;
    for (const int64_t m : sizes) {
      for (const int64_t n : corpora) {
        for (const auto& r : ranges) {
          EmbedPlacePlan p;
          const int64_t nnz = m * kEmbedPlaceRow < kEmbedMaxNnz ? m * kEmbedPlaceRow : kEmbedMaxNnz;
          if (plan_of(m, nnz, n, dim, r[0], r[1], r[2], &p)) { std::printf("  rejected: %s\n", msg); ++fails; continue; }
          ++plans;
          bool ok = p.m == m && p.n == n && p.nnz == nnz && p.dim == dim && p.t0 == r[0] && p.t1 == r[1] && p.total == r[2];
          ok = ok && (m == 0 ? p.grid == 0 : p.grid >= 1 && p.grid <= kEmbedGridCap && (int64_t)(p.grid - 1) * kEmbedLanes < m) &&
               (int64_t)p.grid * kEmbedLanes >= (m < (int64_t)kEmbedGridCap * kEmbedLanes ? m : (int64_t)kEmbedGridCap * kEmbedLanes) &&
               m + (int64_t)kEmbedGridCap * kEmbedLanes < INT64_MAX;
          ok = ok && m * (int64_t)dim <= INT64_MAX / 8 && n * (int64_t)dim <= INT64_MAX / 8 && ((uint64_t)m + 1) * 8 < ((uint64_t)1 << 40);
          // the schedule's products and the counter before the key is added (the sum with the key wraps in uint64 by design)
          ok = ok && (uint64_t)r[2] * 65536u < ((uint64_t)1 << 48) &&
               ((uint64_t)r[2] * kEmbedPlaceRow + kEmbedPlaceRow) * kEmbedMaxNeg + kEmbedMaxNeg < ((uint64_t)1 << 48);
          // a negative sample: ((h >> 32) * n) >> 32 < n, the product inside uint64
          ok = ok && ((((uint64_t)UINT32_MAX * (uint64_t)n) >> 32) < (uint64_t)n);
          if (!ok) { std::printf("  a broken plan: m %lld, n %lld, dim %d, epochs %lld .. %lld of %lld\n", (long long)m, (long long)n, (int)dim, (long long)r[0], (long long)r[1], (long long)r[2]); ++fails; }
        }
      }
    }
    // the window of a row, whatever indptr holds
    const int64_t ends[] = {INT64_MIN, INT64_MIN + 1, -((int64_t)1 << 40), -65, -64, -63, -3, -1, 0, 1, 5, 63, 64, 65, 100, 163, 164, 165, (int64_t)1 << 38, INT64_MAX - 1, INT64_MAX};
    for (const int64_t nnz : {(int64_t)0, (int64_t)1, (int64_t)100, (int64_t)164, kEmbedMaxNnz}) {
      for (const int64_t e0 : ends) {
        for (const int64_t e1 : ends) {
          const Window w = window_of(e0, e1, nnz);
          bool ok = w.q_first >= 0 && w.q_first <= kEmbedPlaceRow && w.q_end <= kEmbedPlaceRow && w.first >= 0;
          if (w.q_first < w.q_end) {                     // what is read: first .. first + (q_end - q_first) - 1
            const int64_t last = w.first + (w.q_end - 1 - w.q_first);
            ok = ok && last < nnz && last < e1 && w.first >= e0 && (e0 >= 0 ? w.first - e0 == w.q_first : w.first == 0 && w.q_first == -e0);
          }
          // nothing that counts is left out: an entry e in [max(e0, 0), min(e1, nnz)) with e - e0 < 64 lies in the window
          if (e0 > -(int64_t)kEmbedPlaceRow && e0 < nnz && e1 > 0 && e1 > e0) {
            const int64_t lo = e0 < 0 ? 0 : e0, hi_a = e1 < nnz ? e1 : nnz, hi_b = e0 + kEmbedPlaceRow, hi = hi_a < hi_b ? hi_a : hi_b;
            if (lo < hi) ok = ok && w.first == lo && w.q_end - w.q_first == hi - lo;
          }
          if (!ok) { std::printf("  a broken window: row %lld .. %lld of %lld entries\n", (long long)e0, (long long)e1, (long long)nnz); ++fails; }
        }
      }
    }
    EmbedPlacePlan p;
    const double inf = INFINITY, nan = NAN;
    if (plan_of(5, 0, 1, dim, 0, 1, 1, &p) || plan_of(0, 0, 0, dim, 0, 1, 1, &p) || plan_of(0, 0, 7, dim, 0, 1, 1, &p) ||
        plan_of(5, 8, 3, dim, 0, 1, 1, &p, 1.0, 0.0, 1.0, 0.0, 0) || plan_of(5, 8, 3, dim, 0, 1, 1, &p, -1.0, 1.0, 1.0, -1.0, 16) ||
        !rejected(plan_of(-1, 0, 3, dim, 0, 1, 1, &p), "m must") || !rejected(plan_of((int64_t)INT32_MAX + 1, 0, 3, dim, 0, 1, 1, &p), "m must") ||
        !rejected(plan_of(INT64_MIN, 0, 3, dim, 0, 1, 1, &p), "m must") || !rejected(plan_of(INT64_MAX, 0, 3, dim, 0, 1, 1, &p), "m must") ||
        !rejected(plan_of(5, 8, 0, dim, 0, 1, 1, &p), "n must") || !rejected(plan_of(5, 8, -1, dim, 0, 1, 1, &p), "n must") ||
        !rejected(plan_of(0, 0, -1, dim, 0, 1, 1, &p), "n must") || !rejected(plan_of(5, 8, (int64_t)INT32_MAX + 1, dim, 0, 1, 1, &p), "n must") ||
        !rejected(plan_of(5, 8, INT64_MIN, dim, 0, 1, 1, &p), "n must") || !rejected(plan_of(5, 8, INT64_MAX, dim, 0, 1, 1, &p), "n must") ||
        !rejected(plan_of(5, -1, 3, dim, 0, 1, 1, &p), "nnz must") || !rejected(plan_of(5, kEmbedMaxNnz + 1, 3, dim, 0, 1, 1, &p), "nnz must") ||
        !rejected(plan_of(5, INT64_MAX, 3, dim, 0, 1, 1, &p), "nnz must") || !rejected(plan_of(5, INT64_MIN, 3, dim, 0, 1, 1, &p), "nnz must") ||
        !rejected(plan_of(5, 8, 3, 1, 0, 1, 1, &p), "dim must") || !rejected(plan_of(5, 8, 3, 4, 0, 1, 1, &p), "dim must") ||
        !rejected(plan_of(5, 8, 3, INT32_MIN, 0, 1, 1, &p), "dim must") || !rejected(plan_of(5, 8, 3, INT32_MAX, 0, 1, 1, &p), "dim must") ||
        !rejected(plan_of(5, 8, 3, dim, 0, 1, 0, &p), "total_epochs") || !rejected(plan_of(5, 8, 3, dim, 0, 1, kEmbedMaxEpochs + 1, &p), "total_epochs") ||
        !rejected(plan_of(5, 8, 3, dim, 0, 1, INT64_MIN, &p), "total_epochs") || !rejected(plan_of(5, 8, 3, dim, 0, 1, INT64_MAX, &p), "total_epochs") ||
        !rejected(plan_of(5, 8, 3, dim, -1, 1, 5, &p), "t0") || !rejected(plan_of(5, 8, 3, dim, 1, 1, 5, &p), "t0") || !rejected(plan_of(5, 8, 3, dim, 2, 1, 5, &p), "t0") ||
        !rejected(plan_of(5, 8, 3, dim, 0, 6, 5, &p), "t0") || !rejected(plan_of(5, 8, 3, dim, INT64_MIN, INT64_MAX, 5, &p), "t0") ||
        !rejected(plan_of(5, 8, 3, dim, INT64_MAX, INT64_MIN, 5, &p), "t0") ||
        !rejected(plan_of(5, 8, 3, dim, 0, 1, 1, &p, 1, 1, 1, 1, -1), "n_neg") || !rejected(plan_of(5, 8, 3, dim, 0, 1, 1, &p, 1, 1, 1, 1, 17), "n_neg") ||
        !rejected(plan_of(5, 8, 3, dim, 0, 1, 1, &p, nan), "lr must") || !rejected(plan_of(5, 8, 3, dim, 0, 1, 1, &p, inf), "lr must") ||
        !rejected(plan_of(5, 8, 3, dim, 0, 1, 1, &p, 1, nan), "a must") || !rejected(plan_of(5, 8, 3, dim, 0, 1, 1, &p, 1, -0.5), "a must") ||
        !rejected(plan_of(5, 8, 3, dim, 0, 1, 1, &p, 1, 1, 0.0), "b must") || !rejected(plan_of(5, 8, 3, dim, 0, 1, 1, &p, 1, 1, inf), "b must") ||
        !rejected(plan_of(5, 8, 3, dim, 0, 1, 1, &p, 1, 1, 1, nan), "gamma must") || !rejected(plan_of(5, 8, 3, dim, 0, 1, 1, &p, 1, 1, 1, -inf), "gamma must")) {
      std::printf("  valid input is refused or invalid input accepted (%s)\n", msg); ++fails;
    }
    std::printf("dim %d: %lld plans up to 2^31 - 1 new rows, vertices and epochs: %s\n", (int)dim, (long long)plans, fails ? "FAILED" : "ok");
    bad += fails;
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
