// Host-only check of the validation and launch plan of wseg_pitch_scratch_bytes / wseg_pitch_frames_f64
// (whisperseg_amd/csrc/wseg_pitch_plan.h: plain C++, no HIP), over lag ranges from three to 2048 lags, hops from one sample to
// 2^31 - 1, segments from nothing to 2^40 samples and counts up to 2^31 - 1 segments: the arithmetic must stay inside int64 and
// int32, and the plan must keep what the kernel relies on.  Build it under the host sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/pitch_plan_check.cpp \
//       -o pitch_plan_check && ./pitch_plan_check
//
// For every (tau_max, hop) it asks for the plan of segments whose lengths sit around every step of the frame count (no frame, one,
// the second, 2^31 samples, 2^40 samples), alone and all together at odd starts, and fails unless: the frame count agrees with a
// count made another way (the frames' starts, bisected); the last frame lies wholly inside the segment and no further frame would
// — what pitch_frame_kernel's loads assume; the prefix is the running sum; the table is (3 n_seg + 1) int64 and the scratch its
// padded size; the workgroup is 64, 128 or 256 lanes, a power of two, with a lane per lag group wherever 256 lanes suffice; the
// blocks of the prefix sum number at most 32; the grid is 1 .. cap and never more than the frames; the byte offset of the last
// output float stays inside int64.  The layout is checked for 2^31 - 1 segments and 2^40 frames without walking that many
// bounds.  Every rejected argument must be rejected with its name.  Prints one line per (tau_max, hop).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "../whisperseg_amd/csrc/wseg_pitch_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

// Frames of a segment, from the definition's wording: frame j exists if its 2 tau_max samples, hop apart from s0, end inside the segment.
static int64_t frames_by_definition(int64_t len, int64_t tau_max, int64_t hop) {
  const int64_t width = 2 * tau_max;
  if (len < width) return 0;
  // the largest J >= 1 with (J - 1) * hop + width <= len, found by bisection (no division: another route than the header's)
  int64_t lo = 1, hi = (len - width) / 1 + 2;          // J = hi is never a frame (hop >= 1)
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    const __int128 end = (__int128)(mid - 1) * hop + width;
    if (end <= len) lo = mid; else hi = mid;
  }
  return lo;
}

int main() {
  int bad = 0;
  for (const int32_t tau_max : {3, 4, 50, 64, 65, 255, 256, 257, 1021, 1024, 2047, 2048}) {
    for (const int32_t hop : {1, 2, 17, tau_max / 2 + 1, 2 * tau_max, 4096, INT32_MAX}) {
      const int64_t width = 2 * (int64_t)tau_max;
      int fails = 0;
      std::vector<int64_t> lengths = {0, 1, width - 1, width, width + 1, width + hop - 1, width + (int64_t)hop, width + (int64_t)hop + 1,
                                      width + 7 * (int64_t)hop + hop / 2};
      // (2^40 samples at hop 1 or 2 hold more frames than one call takes: those lengths are checked alone, as refusals, below)
      for (const int64_t centre : {(int64_t)1 << 31, (int64_t)1 << 40})
        for (int64_t d = -1; d <= 1; ++d)
          if (pitch_frames(centre + d, tau_max, hop) <= kPitchMaxFrames / 8) lengths.push_back(centre + d);
      std::vector<int64_t> bounds, prefix(lengths.size() + 1);
      int64_t expected = 0;
      for (size_t i = 0; i < lengths.size(); ++i) {
        const int64_t len = lengths[i], s0 = 2 * (int64_t)i + 1;
        bounds.push_back(s0);
        bounds.push_back(s0 + len);
        const int64_t J = frames_by_definition(len, tau_max, hop);
        if (pitch_frames(len, tau_max, hop) != J) {
          std::printf("  %lld samples: %lld frames, expected %lld\n", (long long)len, (long long)pitch_frames(len, tau_max, hop), (long long)J); ++fails;
        }
        if (J > 0) {
          // the kernel's loads: the last frame ends inside the segment, one more would not
          const __int128 last_end = (__int128)(J - 1) * hop + width;
          if (!(last_end <= len && last_end + hop > len)) { std::printf("  %lld samples: the last frame lies outside\n", (long long)len); ++fails; }
        }
        expected += J;
        PitchPlan p;
        const int64_t one[2] = {s0, s0 + len};
        if (pitch_plan(one, 1, tau_max, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)) || p.total_frames != J ||
            pitch_plan(one, 1, tau_max, hop, s0 + len, kPitchGridCap, &p, nullptr, msg, sizeof(msg)) || p.total_frames != J) {
          std::printf("  %lld samples alone: %s\n", (long long)len, msg); ++fails;
        }
        if (!rejected(pitch_plan(one, 1, tau_max, hop, s0 + len - 1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "bounds")) {
          std::printf("  %lld samples: a segment behind the recording's end is accepted\n", (long long)len); ++fails;
        }
      }
      PitchPlan p;
      const int32_t n_seg = (int32_t)lengths.size();
      for (const int64_t cap : {(int64_t)kPitchGridCap, (int64_t)1, (int64_t)3, (int64_t)65535, (int64_t)0, (int64_t)-7}) {
        if (pitch_plan(bounds.data(), n_seg, tau_max, hop, -1, cap, &p, prefix.data(), msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; continue; }
        const int64_t top = cap < 1 ? 1 : cap > kPitchGridCap ? kPitchGridCap : cap;
        bool ok = p.tau_max == tau_max && p.hop == hop && p.n_seg == n_seg && p.total_frames == expected &&
                  p.table_bytes == (3 * (int64_t)n_seg + 1) * 8 && p.scratch_bytes >= p.table_bytes && p.scratch_bytes % kPitchAlign == 0 &&
                  p.scratch_bytes - p.table_bytes < kPitchAlign && p.out_floats == 3 * expected && p.grid >= 1 && p.grid <= top &&
                  p.grid <= p.total_frames && (p.grid == top || p.grid == p.total_frames);
        ok = ok && p.groups == (tau_max + 3) / 4 && p.groups * kPitchLagsPerLane >= tau_max && (p.groups - 1) * kPitchLagsPerLane < tau_max;
        ok = ok && p.blocks == (tau_max + 63) / 64 && p.blocks >= 1 && p.blocks <= kPitchMaxBlocks && p.blocks <= p.lanes;
        ok = ok && (p.lanes == 64 || p.lanes == 128 || p.lanes == 256) && (p.lanes >= p.groups || p.lanes == kPitchMaxLanes) &&
             (p.lanes == 64 || p.lanes / 2 < p.groups);
        // the widest LDS read of the kernel: floats 4 g + 4 + i + 7 with g < groups, i <= (tau_max & ~3) - 4, inside 2 tau_max + 16 floats
        ok = ok && 4 * (p.groups - 1) + 4 + ((tau_max & ~3) - 4 > 0 ? (tau_max & ~3) - 4 : 0) + 7 < 2 * tau_max + 16;
        int64_t run = 0;
        for (int32_t i = 0; i < n_seg; ++i) {
          ok = ok && prefix[i] == run;
          run += pitch_frames(lengths[i], tau_max, hop);
        }
        ok = ok && prefix[n_seg] == run && run == p.total_frames;
        ok = ok && p.out_floats <= INT64_MAX / 4 && bounds.back() <= INT64_MAX / 4;
        if (!ok) { std::printf("  a broken plan at grid cap %lld\n", (long long)cap); ++fails; }
      }
      // no segments; segments without a frame
      if (pitch_plan(nullptr, 0, tau_max, hop, 0, kPitchGridCap, &p, prefix.data(), msg, sizeof(msg)) || p.grid != 0 || p.total_frames != 0 ||
          p.scratch_bytes != kPitchAlign || prefix[0] != 0) { std::printf("  no segments: %s\n", msg); ++fails; }
      const int64_t empty[4] = {5, 5, 0, width - 1};
      if (pitch_plan(empty, 2, tau_max, hop, width - 1, kPitchGridCap, &p, prefix.data(), msg, sizeof(msg)) || p.grid != 0 || p.total_frames != 0 ||
          prefix[2] != 0) { std::printf("  empty segments: %s\n", msg); ++fails; }
      // the layout at the largest counts, without walking the bounds
      pitch_layout(INT32_MAX, kPitchMaxFrames, tau_max, hop, kPitchGridCap, &p);
      if (p.table_bytes != (3 * (int64_t)INT32_MAX + 1) * 8 || p.scratch_bytes < p.table_bytes || p.scratch_bytes % kPitchAlign ||
          p.out_floats != 3 * kPitchMaxFrames || p.out_floats > INT64_MAX / 4 || p.grid != kPitchGridCap) {
        std::printf("  a broken layout at 2^31 - 1 segments\n"); ++fails;
      }
      // what must be refused
      const int64_t reversed[2] = {9, 8}, negative[2] = {-1, 8}, huge[2] = {0, kSegmentMaxSamples + 1}, fine[2] = {0, width};
      const int64_t full[2] = {0, kSegmentMaxSamples};
      if (!rejected(pitch_plan(reversed, 1, tau_max, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
          !rejected(pitch_plan(negative, 1, tau_max, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
          !rejected(pitch_plan(huge, 1, tau_max, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
          !rejected(pitch_plan(fine, 1, tau_max, hop, width - 1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
          !rejected(pitch_plan(fine, 1, tau_max, hop, INT64_MAX, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "n must") ||
          !rejected(pitch_plan(nullptr, 1, tau_max, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
          !rejected(pitch_plan(fine, -1, tau_max, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "n_seg") ||
          !rejected(pitch_plan(fine, INT32_MIN, tau_max, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "n_seg") ||
          !rejected(pitch_plan(fine, 1, 2, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "tau_max") ||
          !rejected(pitch_plan(fine, 1, 0, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "tau_max") ||
          !rejected(pitch_plan(fine, 1, -tau_max, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "tau_max") ||
          !rejected(pitch_plan(fine, 1, kPitchMaxLag + 1, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "tau_max") ||
          !rejected(pitch_plan(fine, 1, INT32_MAX, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "tau_max") ||
          !rejected(pitch_plan(fine, 1, tau_max, 0, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "hop") ||
          !rejected(pitch_plan(fine, 1, tau_max, -hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "hop") ||
          !rejected(pitch_plan(fine, 1, tau_max, INT32_MIN, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "hop") ||
          (hop <= 2 && !rejected(pitch_plan(full, 1, tau_max, hop, -1, kPitchGridCap, &p, nullptr, msg, sizeof(msg)), "frames"))) {
        std::printf("  invalid input is accepted (%s)\n", msg); ++fails;
      }
      const double nan = std::nan("");
      if (pitch_args_check(2, tau_max, hop, 0.1, msg, sizeof(msg)) || pitch_args_check(tau_max - 1, tau_max, hop, 0.999, msg, sizeof(msg)) ||
          !rejected(pitch_args_check(1, tau_max, hop, 0.1, msg, sizeof(msg)), "tau_min") ||
          !rejected(pitch_args_check(INT32_MIN, tau_max, hop, 0.1, msg, sizeof(msg)), "tau_min") ||
          !rejected(pitch_args_check(tau_max, tau_max, hop, 0.1, msg, sizeof(msg)), "tau_max") ||
          !rejected(pitch_args_check(tau_max + 1, tau_max, hop, 0.1, msg, sizeof(msg)), "tau_max") ||
          !rejected(pitch_args_check(2, kPitchMaxLag + 1, hop, 0.1, msg, sizeof(msg)), "tau_max") ||
          !rejected(pitch_args_check(2, INT32_MAX, hop, 0.1, msg, sizeof(msg)), "tau_max") ||
          !rejected(pitch_args_check(2, tau_max, 0, 0.1, msg, sizeof(msg)), "hop") ||
          !rejected(pitch_args_check(2, tau_max, INT32_MIN, 0.1, msg, sizeof(msg)), "hop") ||
          !rejected(pitch_args_check(2, tau_max, hop, 0.0, msg, sizeof(msg)), "threshold") ||
          !rejected(pitch_args_check(2, tau_max, hop, 1.0, msg, sizeof(msg)), "threshold") ||
          !rejected(pitch_args_check(2, tau_max, hop, -0.1, msg, sizeof(msg)), "threshold") ||
          !rejected(pitch_args_check(2, tau_max, hop, nan, msg, sizeof(msg)), "threshold") ||
          !rejected(pitch_args_check(2, tau_max, hop, INFINITY, msg, sizeof(msg)), "threshold")) {
        std::printf("  the lags, the hop or the threshold are misjudged (%s)\n", msg); ++fails;
      }
      std::printf("tau_max %4d hop %10d: %zu segments up to 2^40 samples, %lld frames, %d lanes: %s\n", (int)tau_max, (int)hop, lengths.size(),
                  (long long)expected, (int)p.lanes, fails ? "FAILED" : "ok");
      bad += fails;
    }
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
