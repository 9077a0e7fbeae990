// Host-only check of the range validation of wseg_resample_planar_range_f32 (whisperseg_amd/csrc/wseg_resample_range.h: plain C++,
// no HIP), over the ratios of the resampler's tests and recordings of 1, 17, 3000 and 2^40 frames: the index arithmetic must stay
// inside int64 and answer as the definition says.  Build it under the host sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/resample_range_check.cpp \
//       -o resample_range_check && ./resample_range_check
//
// For every (ratio, n_in) it takes the whole range and cuts of it at a few outputs, gives each cut its minimal segment — k_lo of its
// first output to k_hi of its last — and fails unless the check accepts that segment, rejects it with one frame less at either end
// (where that frame is read), and rejects negative, outsized and overflowing arguments.  Prints one line per (ratio, n_in).
#include <cstdio>
#include <cstdint>
#include <numeric>
#include "../whisperseg_amd/csrc/wseg_resample_range.h"

using wseg::resample_range;
using wseg::resample_range_check;

int main() {
  const long long ratios[][2] = {{48000, 16000}, {44100, 16000}, {16000, 44100}, {32000, 48000}, {300000, 250000}, {300000, 16000},
                                 {250000, 44100}, {8000, 16000}, {300000, 4000}, {2500000, 44100}};
  const int64_t lengths[] = {1, 17, 3000, (int64_t)1 << 40};
  char msg[256];
  int bad = 0;
  for (const auto& r : ratios) {
    const long long g = std::gcd(r[0], r[1]);
    const int up = (int)(r[1] / g), down = (int)(r[0] / g);
    // the filter of whisperseg_amd/resample.py (filter_half_len, _ratio); any positive integers would serve the arithmetic checked here
    const int half_len = 10 * (up > down ? up : down), n_taps = 2 * half_len + 1;
    const int pre_pad = down - half_len % down, pre_remove = (half_len + pre_pad) / down;
    for (const int64_t n_in : lengths) {
      const int64_t n_out = (int64_t)(((__int128)n_in * up + down - 1) / down);
      auto ok = [&](int64_t x_first, int64_t x_frames, int64_t m_first, int64_t m_count) {
        return resample_range_check(x_first, x_frames, n_in, n_taps, up, down, pre_pad, pre_remove, m_first, m_count, msg, sizeof(msg)) == 0;
      };
      int fails = 0, cuts = 0;
      if (!ok(0, n_in, 0, n_out)) { std::printf("  the whole range is rejected: %s\n", msg); ++fails; }
      const int64_t marks[] = {0, 1, n_out / 3, n_out / 2, n_out - 1, n_out};
      for (int i = 0; i + 1 < 6; ++i) {
        const int64_t m0 = marks[i], m1 = marks[i + 1];
        if (m0 < 0 || m1 <= m0 || m1 > n_out) continue;
        ++cuts;
        const auto a = resample_range(m0, n_in, n_taps, up, down, pre_pad, pre_remove);
        const auto b = resample_range(m1 - 1, n_in, n_taps, up, down, pre_pad, pre_remove);
        const int64_t x0 = a.k_lo, x1 = (b.k_hi + 1 > x0 ? b.k_hi + 1 : x0);      // an empty chain at the end: an empty tail
        if (x1 > n_in || x0 > n_in) { std::printf("  outputs [%lld, %lld): segment [%lld, %lld) leaves the recording\n", (long long)m0, (long long)m1, (long long)x0, (long long)x1); ++fails; continue; }
        if (!ok(x0, x1 - x0, m0, m1 - m0)) { std::printf("  outputs [%lld, %lld): the minimal segment is rejected: %s\n", (long long)m0, (long long)m1, msg); ++fails; }
        if (x0 + 1 <= x1 && ok(x0 + 1, x1 - x0 - 1, m0, m1 - m0)) { std::printf("  outputs [%lld, %lld): accepted without the first frame\n", (long long)m0, (long long)m1); ++fails; }
        if (b.k_hi >= x0 && ok(x0, x1 - x0 - 1, m0, m1 - m0)) { std::printf("  outputs [%lld, %lld): accepted without the last frame\n", (long long)m0, (long long)m1); ++fails; }
      }
      if (ok(0, n_in, -1, 1) || ok(0, n_in, 0, -1) || ok(-1, n_in, 0, 0) || ok(0, -1, 0, 0) || ok(1, n_in, 0, 0) || ok(0, n_in + 1, 0, 0)) {
        std::printf("  a negative or outsized argument is accepted\n"); ++fails;
      }
      if (ok(0, n_in, INT64_MAX - 4, 2) || ok(0, n_in, 0, INT64_MAX) || ok(0, n_in, INT64_MAX / down, 1)) {
        std::printf("  an output range that overflows is accepted\n"); ++fails;
      }
      if (!ok(0, n_in, n_out, 0) || !ok(0, 0, 0, 0)) { std::printf("  an empty range is rejected: %s\n", msg); ++fails; }
      std::printf("%7lld -> %6lld Hz, n_in %14lld, n_out %14lld: %d cuts, %s\n", r[0], r[1], (long long)n_in, (long long)n_out, cuts,
                  fails ? "FAILED" : "ok");
      bad += fails;
    }
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
