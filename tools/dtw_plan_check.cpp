// Host-only check of the validation and launch plan of wseg_dtw_scratch_bytes / wseg_dtw_knn_f32 / wseg_dtw_pairs_f64
// (whisperseg_amd/csrc/wseg_dtw_plan.h: plain C++, no HIP) over the limits: m, n in {0, 1, 2, 3, 4, 5, 2^31 - 1}, channels in
// {1, 128}, steps in {1, 32, 33, 64}, k in {1, 64} and every grid cap from 1 to the default: the arithmetic must stay inside int64
// and int32, and the plan must keep what the kernels rely on.  Build it under the host sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/dtw_plan_check.cpp \
//       -o dtw_plan_check && ./dtw_plan_check
//
// It fails unless: the steps are padded to 32 or 64 and a tile holds 128 / padded sequences; the tiles cover the rows with less than
// one tile to spare; the splits are 1 .. min(candidate tiles, cap), none of them empty, and together cover every candidate tile; the
// grids are 1 .. cap (the finish grid 1 .. 8 cap) and never more than their work (0 without work); the three scratch regions follow
// each other on their alignment without overlap and fit in the reported size, the keys of the last (row, split) and the last
// elements of queries, corpus, norms and the outputs stay inside int64; the size under a smaller cap never exceeds the size under
// the default cap (what wseg_dtw_scratch_bytes reports) and the reported size is monotone in m, n, steps and k.  Invalid sizes must
// be rejected with the argument's name.  Prints one line per (channels, steps, k).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "../whisperseg_amd/csrc/wseg_dtw_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

int main() {
  int bad = 0;
  const int64_t sizes[] = {0, 1, 2, 3, 4, 5, INT32_MAX};
  const int64_t ladder[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000, 4096, 100000, 131072, 131073, 10000000, INT32_MAX};
  for (const int32_t c : {1, kDtwMaxChannels}) {
    for (const int32_t t : {1, kDtwBlock, kDtwBlock + 1, kDtwMaxSteps}) {
      for (const int32_t k : {1, kDtwMaxK}) {
        int fails = 0;
        int64_t plans = 0;
        for (const int64_t m : sizes) {
          for (const int64_t n : sizes) {
            DtwPlan whole;
            if (dtw_plan(m, n, c, t, k, kDtwGridCap, &whole, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; continue; }
            for (int64_t cap = 1; cap <= kDtwGridCap; ++cap) {
              DtwPlan p;
              if (dtw_plan(m, n, c, t, k, cap, &p, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; break; }
              ++plans;
              bool ok = p.m == m && p.n == n && p.channels == c && p.steps == t && p.k == k && p.L == k + kDtwExtra && p.L <= kDtwMaxL &&
                        (p.padded == kDtwBlock || p.padded == 2 * kDtwBlock) && p.padded >= t && p.padded - t < kDtwBlock &&
                        p.seqs * p.padded == kDtwTile && p.seqs <= 4 &&
                        p.m_tiles * p.seqs >= m && (p.m_tiles == 0 ? m == 0 : (p.m_tiles - 1) * p.seqs < m) &&
                        p.n_tiles * p.seqs >= n && (p.n_tiles == 0 ? n == 0 : (p.n_tiles - 1) * p.seqs < n);
              if (m == 0 || n == 0) {
                ok = ok && p.splits == 0 && p.items == 0 && p.grid == 0 && p.keys_bytes == 0;
              } else {
                ok = ok && p.splits >= 1 && p.splits <= cap && p.splits <= p.n_tiles && p.tiles_per_split >= 1 &&
                     (int64_t)p.splits * p.tiles_per_split >= p.n_tiles && (int64_t)(p.splits - 1) * p.tiles_per_split < p.n_tiles &&
                     p.items == p.m_tiles * p.splits && p.grid >= 1 && p.grid <= cap && p.grid <= p.items;
              }
              ok = ok && (m == 0 ? p.finish_grid == 0 : (p.finish_grid >= 1 && p.finish_grid <= cap * kDtwFinishPerCap && p.finish_grid <= m));
              ok = ok && p.finish_grid == dtw_wave_grid(m, cap);
              ok = ok && (m + n == 0 ? p.norm_grid == 0 : (p.norm_grid >= 1 && p.norm_grid <= cap && (int64_t)(p.norm_grid - 1) * 256 < (m + n) * t));
              // the regions: in order, aligned, no overlap, inside the reported size
              ok = ok && p.qnorm_offset == 0 && p.qnorm_bytes == 4 * m * t && p.xnorm_offset % kDtwAlign == 0 &&
                   p.xnorm_offset >= p.qnorm_offset + p.qnorm_bytes && p.xnorm_bytes == 4 * n * t && p.keys_offset % kDtwAlign == 0 &&
                   p.keys_offset >= p.xnorm_offset + p.xnorm_bytes && p.keys_bytes == p.items * p.seqs * p.L * 8 &&
                   p.keys_bytes <= p.keys_capacity && p.scratch_bytes >= p.keys_offset + p.keys_capacity &&
                   p.scratch_bytes % kDtwAlign == 0 && p.scratch_bytes > 0;
              // the last key the selection kernel writes and the finish kernel reads: row m_tiles * seqs - 1, the last split, entry L - 1
              if (p.items > 0) {
                const int64_t last = ((p.m_tiles * p.seqs - 1) * p.splits + (p.splits - 1)) * p.L + (p.L - 1);
                ok = ok && last >= 0 && (last + 1) * 8 == p.keys_bytes;
              }
              // element offsets the kernels form, and the grid-stride's last step
              const int64_t d = (int64_t)c * t;
              ok = ok && m * d <= INT64_MAX / 4 && n * d <= INT64_MAX / 4 && m * (int64_t)k <= INT64_MAX / 4 &&
                   p.items + cap < INT64_MAX && (m + n) * t + cap * 256 < INT64_MAX && (p.m_tiles + 1) * p.seqs * (int64_t)t < INT64_MAX;
              // what wseg_dtw_scratch_bytes reports (the default cap) holds every smaller cap's plan
              ok = ok && p.scratch_bytes <= whole.scratch_bytes;
              if (!ok) {
                std::printf("  a broken plan: m %lld, n %lld, channels %d, steps %d, k %d, cap %lld\n", (long long)m, (long long)n, (int)c, (int)t, (int)k, (long long)cap);
                ++fails;
                break;
              }
            }
          }
        }
        // monotone in m, n, steps and k under the default cap — although the split count and the sequences of a tile are not
        int64_t before_m = 0;
        for (const int64_t m : ladder) {
          int64_t before_n = 0;
          for (const int64_t n : ladder) {
            DtwPlan p, q;
            if (dtw_plan(m, n, c, t, k, kDtwGridCap, &p, msg, sizeof(msg))) { ++fails; continue; }
            if (p.scratch_bytes < before_n) { std::printf("  not monotone in n at m %lld, n %lld\n", (long long)m, (long long)n); ++fails; }
            before_n = p.scratch_bytes;
            if (k < kDtwMaxK && (dtw_plan(m, n, c, t, k + 1, kDtwGridCap, &q, msg, sizeof(msg)) || q.scratch_bytes < p.scratch_bytes)) {
              std::printf("  not monotone in k at m %lld, n %lld\n", (long long)m, (long long)n); ++fails;
            }
            if (t < kDtwMaxSteps && (dtw_plan(m, n, c, t + 1, k, kDtwGridCap, &q, msg, sizeof(msg)) || q.scratch_bytes < p.scratch_bytes)) {
              std::printf("  not monotone in steps at m %lld, n %lld\n", (long long)m, (long long)n); ++fails;
            }
            if (n == INT32_MAX) {
              if (p.scratch_bytes < before_m) { std::printf("  not monotone in m at m %lld\n", (long long)m); ++fails; }
              before_m = p.scratch_bytes;
            }
          }
        }
        DtwPlan p;
        if (dtw_plan(5, 5, c, t, k, kDtwGridCap, &p, msg, sizeof(msg)) || dtw_plan(5, 5, c, t, k, 0, &p, msg, sizeof(msg)) || p.grid != 1 ||
            dtw_plan(5, 5, c, t, k, INT64_MAX, &p, msg, sizeof(msg)) || p.grid > p.items ||
            !rejected(dtw_plan(-1, 5, c, t, k, 1, &p, msg, sizeof(msg)), "m must") || !rejected(dtw_plan((int64_t)INT32_MAX + 1, 5, c, t, k, 1, &p, msg, sizeof(msg)), "m must") ||
            !rejected(dtw_plan(5, -1, c, t, k, 1, &p, msg, sizeof(msg)), "n must") || !rejected(dtw_plan(5, (int64_t)INT32_MAX + 1, c, t, k, 1, &p, msg, sizeof(msg)), "n must") ||
            !rejected(dtw_plan(5, INT64_MIN, c, t, k, 1, &p, msg, sizeof(msg)), "n must") || !rejected(dtw_plan(INT64_MAX, 5, c, t, k, 1, &p, msg, sizeof(msg)), "m must") ||
            !rejected(dtw_plan(5, 5, 0, t, k, 1, &p, msg, sizeof(msg)), "channels must") || !rejected(dtw_plan(5, 5, kDtwMaxChannels + 1, t, k, 1, &p, msg, sizeof(msg)), "channels must") ||
            !rejected(dtw_plan(5, 5, INT32_MIN, t, k, 1, &p, msg, sizeof(msg)), "channels must") || !rejected(dtw_plan(5, 5, INT32_MAX, t, k, 1, &p, msg, sizeof(msg)), "channels must") ||
            !rejected(dtw_plan(5, 5, c, 0, k, 1, &p, msg, sizeof(msg)), "steps must") || !rejected(dtw_plan(5, 5, c, kDtwMaxSteps + 1, k, 1, &p, msg, sizeof(msg)), "steps must") ||
            !rejected(dtw_plan(5, 5, c, INT32_MIN, k, 1, &p, msg, sizeof(msg)), "steps must") || !rejected(dtw_plan(5, 5, c, INT32_MAX, k, 1, &p, msg, sizeof(msg)), "steps must") ||
            !rejected(dtw_plan(5, 5, c, t, 0, 1, &p, msg, sizeof(msg)), "k must") || !rejected(dtw_plan(5, 5, c, t, kDtwMaxK + 1, 1, &p, msg, sizeof(msg)), "k must") ||
            !rejected(dtw_plan(5, 5, c, t, INT32_MIN, 1, &p, msg, sizeof(msg)), "k must") || !rejected(dtw_plan(5, 5, c, t, INT32_MAX, 1, &p, msg, sizeof(msg)), "k must") ||
            dtw_check_shape(c, t, 0, msg, sizeof(msg)) || dtw_check_shape(c, t, t - 1, msg, sizeof(msg)) || dtw_check_shape(c, t, -1, msg, sizeof(msg)) ||
            !rejected(dtw_check_shape(c, t, t, msg, sizeof(msg)), "band must") || !rejected(dtw_check_shape(c, t, INT32_MAX, msg, sizeof(msg)), "band must") ||
            dtw_wave_grid(0, kDtwGridCap) != 0 || dtw_wave_grid(-5, kDtwGridCap) != 0 || dtw_wave_grid(7, 0) != 7 || dtw_wave_grid(INT32_MAX, 0) != kDtwFinishPerCap ||
            dtw_wave_grid(INT64_MAX, INT64_MAX) != kDtwGridCap * kDtwFinishPerCap) {
          std::printf("  valid input is refused or invalid input accepted (%s)\n", msg); ++fails;
        }
        std::printf("channels %3d, steps %2d, k %2d: %lld plans up to 2^31 - 1 rows on both sides, caps 1 .. %d: %s\n", (int)c, (int)t, (int)k,
                    (long long)plans, kDtwGridCap, fails ? "FAILED" : "ok");
        bad += fails;
      }
    }
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
