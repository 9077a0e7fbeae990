// Host-only check of the validation and launch plan of wseg_measure_scratch_bytes / wseg_measure_segments_f32
// (whisperseg_amd/csrc/wseg_measure_plan.h: plain C++, no HIP), over all five FFT sizes and segments from nothing to 2^40 frames:
// the arithmetic must stay inside int64 and int32, and the plan must keep what the two kernels rely on.  Build it under the host
// sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/measure_plan_check.cpp \
//       -o measure_plan_check && ./measure_plan_check
//
// For every n_fft it asks for the plan of segments whose lengths sit around every step of the frame and chunk counts (one frame,
// the second frame, the seam of two chunks, 2^31 samples, 2^40 frames), alone and all together at odd starts, and fails unless:
// frames and chunks agree with a count made another way (the frames' starts, walked); the last frame starts inside the segment
// and reaches its end, the last chunk's own samples start inside it — what measure_chunk_kernel's loops assume; the prefix is
// the running sum; the partials start on their alignment behind the table and the scratch holds exactly table + chunks; the grid
// is 1 .. cap and never more than the chunks; the byte offsets of the last chunk's last double and of the last sample stay inside
// int64.  Invalid bounds, sizes, counts and bands must be rejected with the argument's name.  Prints one line per n_fft.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../whisperseg_amd/csrc/wseg_measure_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

// Frames of a segment, from the definition's wording: frame j exists if it is the first, or if frame j - 1 ends before the segment does.
static int64_t frames_by_definition(int64_t len, int64_t n_fft) {
  if (len <= 0) return 0;
  const int64_t hop = n_fft / 4;
  if (len <= n_fft) return 1;
  // the smallest J >= 1 with (J - 1) * hop + n_fft >= len, found by bisection (no division: another route than the header's)
  int64_t lo = 1, hi = len / hop + 2;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((mid - 1) * hop + n_fft >= len) hi = mid; else lo = mid + 1;
  }
  return lo;
}

int main() {
  int bad = 0;
  for (const int32_t n_fft : {512, 1024, 2048, 4096, 8192}) {
    const int64_t hop = n_fft / 4, bins = n_fft / 2 + 1;
    int fails = 0;
    std::vector<int64_t> lengths = {0, 1, 7};
    for (const int64_t centre : {(int64_t)n_fft, n_fft + hop, n_fft + 63 * hop, n_fft + 127 * hop, (int64_t)1 << 31, ((int64_t)1 << 31) * hop,
                                 n_fft + (((int64_t)1 << 40) - 1) * hop})
      for (int64_t d = -1; d <= 1; ++d) lengths.push_back(centre + d);
    std::vector<int64_t> bounds, prefix(lengths.size() + 1);
    int64_t expected_chunks = 0;
    for (size_t i = 0; i < lengths.size(); ++i) {
      const int64_t len = lengths[i], s0 = 2 * (int64_t)i + 1;
      bounds.push_back(s0);
      bounds.push_back(s0 + len);
      const int64_t J = frames_by_definition(len, n_fft);
      if (measure_frames(len, n_fft) != J) { std::printf("  %lld samples: %lld frames, expected %lld\n", (long long)len, (long long)measure_frames(len, n_fft), (long long)J); ++fails; }
      const int64_t C = measure_chunks(len, n_fft);
      if (C != (J + kMeasureChunkFrames - 1) / kMeasureChunkFrames) { std::printf("  %lld samples: %lld chunks\n", (long long)len, (long long)C); ++fails; }
      if (len > 0) {
        // the kernel's loops: the last frame starts inside the segment and reaches its end; the last chunk owns at least one sample
        const int64_t last_start = (J - 1) * hop, own_start = (C - 1) * kMeasureChunkFrames * hop;
        if (!(last_start < len && last_start + n_fft >= len && own_start < len && (C == 1 || (C - 1) * kMeasureChunkFrames < J))) {
          std::printf("  %lld samples: the last frame or chunk lies outside\n", (long long)len); ++fails;
        }
      }
      expected_chunks += C;
      // the segment alone, with and without a recording length
      MeasurePlan p;
      const int64_t one[2] = {s0, s0 + len};
      if (measure_plan(one, 1, n_fft, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)) || p.total_chunks != C ||
          measure_plan(one, 1, n_fft, s0 + len, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)) || p.total_chunks != C) {
        std::printf("  %lld samples alone: %s\n", (long long)len, msg); ++fails;
      }
      if (!rejected(measure_plan(one, 1, n_fft, s0 + len - 1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") && s0 + len - 1 >= 0) {
        std::printf("  %lld samples: a segment behind the recording's end is accepted\n", (long long)len); ++fails;
      }
    }
    MeasurePlan p;
    const int32_t n_seg = (int32_t)lengths.size();
    for (const int64_t cap : {(int64_t)kMeasureGridCap, (int64_t)1, (int64_t)3, (int64_t)65535}) {
      if (measure_plan(bounds.data(), n_seg, n_fft, -1, cap, &p, prefix.data(), msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; continue; }
      bool ok = p.n_fft == n_fft && p.hop == hop && p.n_bins == bins && p.n_seg == n_seg && p.total_chunks == expected_chunks &&
                p.table_bytes == (3 * (int64_t)n_seg + 1) * 8 && p.partial_offset >= p.table_bytes && p.partial_offset % kMeasureAlign == 0 &&
                p.partial_offset - p.table_bytes < kMeasureAlign && p.chunk_doubles == bins + kMeasureTimeSlots &&
                p.scratch_bytes == p.partial_offset + p.total_chunks * p.chunk_doubles * 8 && p.grid >= 1 && p.grid <= cap && p.grid <= p.total_chunks;
      int64_t run = 0;
      for (int32_t i = 0; i < n_seg; ++i) {
        ok = ok && prefix[i] == run;
        run += measure_chunks(lengths[i], n_fft);
      }
      ok = ok && prefix[n_seg] == run && run == p.total_chunks;
      // the last double of the last chunk and the last sample read, as byte offsets
      const int64_t last_double = p.partial_offset + ((p.total_chunks - 1) * p.chunk_doubles + p.chunk_doubles - 1) * 8;
      ok = ok && last_double + 8 == p.scratch_bytes && bounds.back() <= INT64_MAX / 4;
      if (!ok) { std::printf("  a broken plan at grid cap %lld\n", (long long)cap); ++fails; }
    }
    // no segments; segments without samples
    if (measure_plan(nullptr, 0, n_fft, 0, kMeasureGridCap, &p, prefix.data(), msg, sizeof(msg)) || p.grid != 0 || p.total_chunks != 0 ||
        p.scratch_bytes != kMeasureAlign || prefix[0] != 0) { std::printf("  no segments: %s\n", msg); ++fails; }
    const int64_t empty[4] = {5, 5, 0, 0};
    if (measure_plan(empty, 2, n_fft, 5, kMeasureGridCap, &p, prefix.data(), msg, sizeof(msg)) || p.grid != 0 || p.total_chunks != 0 || prefix[2] != 0) {
      std::printf("  empty segments: %s\n", msg); ++fails;
    }
    // what must be refused
    const int64_t reversed[2] = {9, 8}, negative[2] = {-1, 8}, huge[2] = {0, kSegmentMaxSamples + 1}, fine[2] = {0, 8};
    std::vector<int64_t> many;
    for (int i = 0; i < 8; ++i) { many.push_back(0); many.push_back(kSegmentMaxSamples); }
    if (!rejected(measure_plan(reversed, 1, n_fft, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
        !rejected(measure_plan(negative, 1, n_fft, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
        !rejected(measure_plan(huge, 1, n_fft, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
        !rejected(measure_plan(fine, 1, n_fft, 7, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
        !rejected(measure_plan(fine, 1, n_fft, INT64_MAX, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "n must") ||
        !rejected(measure_plan(nullptr, 1, n_fft, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
        !rejected(measure_plan(fine, -1, n_fft, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "n_seg") ||
        !rejected(measure_plan(fine, INT32_MIN, n_fft, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "n_seg") ||
        !rejected(measure_plan(fine, 1, n_fft + 1, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "n_fft") ||
        !rejected(measure_plan(fine, 1, n_fft * 32, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "n_fft") ||
        !rejected(measure_plan(fine, 1, 0, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "n_fft") ||
        !rejected(measure_plan(fine, 1, -n_fft, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "n_fft") ||
        (n_fft <= 1024 && !rejected(measure_plan(many.data(), 8, n_fft, -1, kMeasureGridCap, &p, nullptr, msg, sizeof(msg)), "chunks"))) {
      std::printf("  invalid input is accepted (%s)\n", msg); ++fails;
    }
    if (measure_band_check(n_fft, 1, n_fft / 2, msg, sizeof(msg)) || measure_band_check(n_fft, 7, 7, msg, sizeof(msg)) ||
        !rejected(measure_band_check(n_fft, 0, 5, msg, sizeof(msg)), "k_lo") || !rejected(measure_band_check(n_fft, 6, 5, msg, sizeof(msg)), "k_hi") ||
        !rejected(measure_band_check(n_fft, 1, n_fft / 2 + 1, msg, sizeof(msg)), "k_hi") ||
        !rejected(measure_band_check(n_fft, INT32_MIN, INT32_MAX, msg, sizeof(msg)), "k_lo")) {
      std::printf("  a band is misjudged (%s)\n", msg); ++fails;
    }
    std::printf("n_fft %4d: %zu segments up to 2^40 frames, %lld chunks of %lld doubles: %s\n", (int)n_fft, lengths.size(),
                (long long)expected_chunks, (long long)(bins + kMeasureTimeSlots), fails ? "FAILED" : "ok");
    bad += fails;
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
