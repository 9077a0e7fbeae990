// Host-only check of the validation and launch plan of wseg_embed_scratch_bytes / wseg_embed_epochs_f64 (whisperseg_amd/csrc/
// wseg_embed_plan.h: plain C++, no HIP) over the limits: n in {0, 1, 63, 64, 65, ..., 2^31 - 1}, both dims, epoch ranges at the
// edges of 1 .. 2^31 - 1: the arithmetic must stay inside int64 and int32, and the plan must keep what the launches rely on.  Build
// it under the host sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/embed_plan_check.cpp \
//       -o embed_plan_check && ./embed_plan_check
//
// It fails unless: the grid is 1 .. the cap, never more than the vertices need (0 without a vertex), and its stride's last step stays
// inside int64; the scratch holds n * dim doubles, is aligned, positive and monotone in n and dim; the last epoch of every range
// writes y_out, consecutive epochs alternate, every epoch reads what the one before it wrote (the first one y_in) and none reads the
// buffer it writes; the largest offsets a lane forms (n * dim elements, (t + 1) * rate) stay inside int64.  Invalid sizes, ranges and
// parameters must be rejected with the argument's name.  Prints one line per dim.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "../whisperseg_amd/csrc/wseg_embed_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

static int plan_of(int64_t n, int64_t nnz, int32_t dim, int64_t t0, int64_t t1, int64_t total, EmbedPlan* p, double lr = 1.0, double a = 1.5,
                   double b = 0.9, double gamma = 1.0, int32_t n_neg = 5) {
  return embed_plan(n, nnz, dim, t0, t1, total, lr, a, b, gamma, n_neg, p, msg, sizeof(msg));
}

int main() {
  int bad = 0;
  const int64_t sizes[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 4096, 100000, 1048576, 1048577, 10000000, INT32_MAX};
  const int64_t ranges[][3] = {{0, 1, 1}, {0, 2, 2}, {0, 50, 50}, {0, 20, 50}, {20, 50, 50}, {49, 50, 50}, {7, 8, 200}, {7, 9, 200}, {0, 200, 200},
                               {0, kEmbedMaxEpochs, kEmbedMaxEpochs}, {kEmbedMaxEpochs - 1, kEmbedMaxEpochs, kEmbedMaxEpochs},
                               {kEmbedMaxEpochs - 3, kEmbedMaxEpochs, kEmbedMaxEpochs}};
  int64_t smaller[sizeof(sizes) / sizeof(sizes[0])] = {};
  for (const int32_t dim : {2, 3}) {
    int fails = 0;
    int64_t plans = 0, before = 0;
    int at = 0;
    for (const int64_t n : sizes) {
      for (const auto& r : ranges) {
        EmbedPlan p;
        if (plan_of(n, n ? kEmbedMaxNnz : 0, dim, r[0], r[1], r[2], &p)) { std::printf("  rejected: %s\n", msg); ++fails; continue; }
        ++plans;
        bool ok = p.n == n && p.dim == dim && p.t0 == r[0] && p.t1 == r[1] && p.total == r[2];
        ok = ok && (n == 0 ? p.grid == 0 : p.grid >= 1 && p.grid <= kEmbedGridCap && (int64_t)(p.grid - 1) * kEmbedLanes < n) &&
             (int64_t)p.grid * kEmbedLanes >= (n < (int64_t)kEmbedGridCap * kEmbedLanes ? n : (int64_t)kEmbedGridCap * kEmbedLanes) &&
             n + (int64_t)kEmbedGridCap * kEmbedLanes < INT64_MAX;
        ok = ok && p.scratch_bytes >= n * dim * 8 && p.scratch_bytes % kEmbedAlign == 0 && p.scratch_bytes > 0 &&
             p.scratch_bytes < n * dim * 8 + 2 * kEmbedAlign && n * (int64_t)dim <= INT64_MAX / 8;
        // the ping-pong: the first epochs and the last epochs of the range (a range may hold 2^31 - 1 of them)
        ok = ok && embed_writes(p, p.t1 - 1) == 1 && p.first_to_out == embed_writes(p, p.t0) && embed_reads(p, p.t0) == 2;
        for (const int64_t from : {p.t0, p.t1 - 64 > p.t0 ? p.t1 - 64 : p.t0}) {
          for (int64_t t = from; t < p.t1 && t < from + 64; ++t) {
            const int w = embed_writes(p, t), rd = embed_reads(p, t);
            ok = ok && (w == 0 || w == 1) && rd != w && (t == p.t0 ? rd == 2 : rd == embed_writes(p, t - 1) && w != embed_writes(p, t - 1));
          }
        }
        // the schedule's products and the counter's first factor
        ok = ok && (uint64_t)r[2] * 65536u < ((uint64_t)1 << 48) && p.nnz <= kEmbedMaxNnz;
        if (!ok) { std::printf("  a broken plan: n %lld, dim %d, epochs %lld .. %lld of %lld\n", (long long)n, (int)dim, (long long)r[0], (long long)r[1], (long long)r[2]); ++fails; }
      }
      EmbedPlan s;
      if (embed_sizes(n, dim, &s, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; continue; }
      if (s.scratch_bytes < before) { std::printf("  not monotone in n at %lld\n", (long long)n); ++fails; }
      before = s.scratch_bytes;
      if (dim == 3 && s.scratch_bytes < smaller[at]) { std::printf("  not monotone in dim at n %lld\n", (long long)n); ++fails; }
      smaller[at++] = s.scratch_bytes;
    }
    EmbedPlan p;
    const double inf = INFINITY, nan = NAN;
    if (plan_of(5, 0, dim, 0, 1, 1, &p) || plan_of(5, 8, dim, 0, 1, 1, &p, 1.0, 0.0, 1.0, 0.0, 0) || plan_of(5, 8, dim, 0, 1, 1, &p, -1.0, 1.0, 1.0, -1.0, 16) ||
        !rejected(plan_of(-1, 0, dim, 0, 1, 1, &p), "n must") || !rejected(plan_of((int64_t)INT32_MAX + 1, 0, dim, 0, 1, 1, &p), "n must") ||
        !rejected(plan_of(INT64_MIN, 0, dim, 0, 1, 1, &p), "n must") || !rejected(plan_of(INT64_MAX, 0, dim, 0, 1, 1, &p), "n must") ||
        !rejected(plan_of(5, -1, dim, 0, 1, 1, &p), "nnz must") || !rejected(plan_of(5, kEmbedMaxNnz + 1, dim, 0, 1, 1, &p), "nnz must") ||
        !rejected(plan_of(5, INT64_MAX, dim, 0, 1, 1, &p), "nnz must") || !rejected(plan_of(5, INT64_MIN, dim, 0, 1, 1, &p), "nnz must") ||
        !rejected(plan_of(5, 8, 1, 0, 1, 1, &p), "dim must") || !rejected(plan_of(5, 8, 4, 0, 1, 1, &p), "dim must") ||
        !rejected(plan_of(5, 8, INT32_MIN, 0, 1, 1, &p), "dim must") || !rejected(plan_of(5, 8, INT32_MAX, 0, 1, 1, &p), "dim must") ||
        !rejected(plan_of(5, 8, dim, 0, 1, 0, &p), "total_epochs") || !rejected(plan_of(5, 8, dim, 0, 1, kEmbedMaxEpochs + 1, &p), "total_epochs") ||
        !rejected(plan_of(5, 8, dim, 0, 1, INT64_MIN, &p), "total_epochs") || !rejected(plan_of(5, 8, dim, 0, 1, INT64_MAX, &p), "total_epochs") ||
        !rejected(plan_of(5, 8, dim, -1, 1, 5, &p), "t0") || !rejected(plan_of(5, 8, dim, 1, 1, 5, &p), "t0") || !rejected(plan_of(5, 8, dim, 2, 1, 5, &p), "t0") ||
        !rejected(plan_of(5, 8, dim, 0, 6, 5, &p), "t0") || !rejected(plan_of(5, 8, dim, INT64_MIN, INT64_MAX, 5, &p), "t0") ||
        !rejected(plan_of(5, 8, dim, INT64_MAX, INT64_MIN, 5, &p), "t0") ||
        !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, 1, 1, 1, 1, -1), "n_neg") || !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, 1, 1, 1, 1, 17), "n_neg") ||
        !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, nan), "lr must") || !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, inf), "lr must") ||
        !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, 1, nan), "a must") || !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, 1, -0.5), "a must") ||
        !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, 1, -inf), "a must") || !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, 1, 1, 0.0), "b must") ||
        !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, 1, 1, nan), "b must") || !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, 1, 1, inf), "b must") ||
        !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, 1, 1, 1, nan), "gamma must") || !rejected(plan_of(5, 8, dim, 0, 1, 1, &p, 1, 1, 1, -inf), "gamma must")) {
      std::printf("  valid input is refused or invalid input accepted (%s)\n", msg); ++fails;
    }
    std::printf("dim %d: %lld plans up to 2^31 - 1 vertices and epochs: %s\n", (int)dim, (long long)plans, fails ? "FAILED" : "ok");
    bad += fails;
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
