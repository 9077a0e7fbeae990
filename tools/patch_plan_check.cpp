// Host-only check of the validation and launch plan of wseg_patches_scratch_bytes / wseg_patches_f32
// (whisperseg_amd/csrc/wseg_patch_plan.h: plain C++, no HIP), over all five FFT sizes, widths 1 .. 256, segment counts from none to
// 2^31 - 1 (a synthetic sequence, no array) and samples up to 2^52: the arithmetic must stay inside int64 and int32, and the plan
// must keep what the two kernels rely on.  Build it under the host sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/patch_plan_check.cpp \
//       -o patch_plan_check && ./patch_plan_check
//
// For every n_fft it fails unless: a work item's frames fill the workgroup's 4096 complex points exactly; the items cover the
// n_seg * width frames with less than one item to spare; both grids are 1 .. cap and never more than their work (0 without a
// segment); the maxima follow the table on their alignment and the scratch holds exactly both; the offsets of the last table entry,
// the last value of out and the last frame's last sample stay inside int64; every column centre lies in [s0, s1) (at s0 for an
// empty segment) and never moves backwards from one column to the next, up to s1 = 2^52 at width 256; the table written for the
// device is (s0, s1).  Invalid sizes, counts, widths and bounds must be rejected with the argument's name.  Prints one line per n_fft.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../whisperseg_amd/csrc/wseg_patch_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

// Segment i of a synthetic call of n_seg segments that ends at `top`: starts spread over [0, top], lengths from 0 up to everything left.
struct Synthetic {
  int64_t top;
  int32_t n_seg;
  void operator()(int32_t i, int64_t* s0, int64_t* s1) const {
    const int64_t step = n_seg > 1 ? top / (n_seg - 1) : 0;
    *s0 = i == n_seg - 1 ? top : step * i;
    switch (i % 4) {
      case 0: *s1 = *s0; break;
      case 1: *s1 = *s0 + (top - *s0 > 0 ? 1 : 0); break;
      case 2: *s1 = *s0 + (top - *s0) / 2; break;
      default: *s1 = top;
    }
  }
};

int main() {
  int bad = 0;
  const int64_t top = kSegmentMaxSamples;
  for (const int32_t n_fft : {512, 1024, 2048, 4096, 8192}) {
    int fails = 0;
    int64_t plans = 0;
    for (const int32_t width : {1, 2, 5, 32, 255, 256}) {
      for (const int32_t n_mels : {1, 80, 96}) {
        for (const int32_t n_seg : {0, 1, 15, 16, 17, 1000, 65537, INT32_MAX}) {
          for (const int64_t cap : {(int64_t)kPatchGridCap, (int64_t)1, (int64_t)3, (int64_t)65535}) {
            PatchPlan p;
            if (patch_plan_sizes(n_seg, n_mels, width, n_fft, cap, &p, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; continue; }
            ++plans;
            const int64_t frames = (int64_t)n_seg * width;
            bool ok = p.n_fft == n_fft && p.n_mels == n_mels && p.width == width && p.n_seg == n_seg &&
                      (int64_t)p.frames_per_item * (n_fft / 2) == kPatchFrameSlots && p.frames_per_item >= 1 && p.frames_per_item <= 16 &&
                      256 % p.frames_per_item == 0 && p.total_frames == frames && p.total_items * p.frames_per_item >= frames &&
                      (p.total_items == 0 ? frames == 0 : (p.total_items - 1) * p.frames_per_item < frames) &&
                      p.total_values == frames * n_mels && p.table_bytes == 16 * (int64_t)n_seg && p.vmax_offset >= p.table_bytes &&
                      p.vmax_offset % kPatchAlign == 0 && p.vmax_offset >= kPatchAlign && p.vmax_offset - p.table_bytes <= kPatchAlign &&
                      p.vmax_bytes == 4 * (int64_t)n_seg && p.scratch_bytes >= p.vmax_offset + p.vmax_bytes && p.scratch_bytes % kPatchAlign == 0 &&
                      p.scratch_bytes - (p.vmax_offset + p.vmax_bytes) <= kPatchAlign;
            const int64_t rounds = (p.total_values + kPatchFinishPerGroup - 1) / kPatchFinishPerGroup;
            if (n_seg == 0) ok = ok && p.grid == 0 && p.finish_grid == 0;
            else ok = ok && p.grid >= 1 && p.grid <= cap && p.grid <= p.total_items && p.finish_grid >= 1 && p.finish_grid <= cap && p.finish_grid <= rounds;
            // byte offsets the kernels form: the last value of out, the last round's last index, the last item's last frame number
            ok = ok && p.total_values <= INT64_MAX / 4 && (rounds + cap) <= INT64_MAX / kPatchFinishPerGroup &&
                 (p.total_items + cap) <= INT64_MAX / p.frames_per_item && (int64_t)n_mels * width <= INT32_MAX;
            if (!ok) { std::printf("  a broken plan: n_seg %d, n_mels %d, width %d, cap %lld\n", (int)n_seg, (int)n_mels, (int)width, (long long)cap); ++fails; }
          }
        }
      }
      // column centres: inside the segment, never backwards, for lengths around the width and up to 2^52
      for (const int64_t L : {(int64_t)0, (int64_t)1, (int64_t)width - 1, (int64_t)width, (int64_t)width + 1, (int64_t)1001, (int64_t)1 << 31, top - 1, top}) {
        if (L < 0) continue;
        for (const int64_t s0 : {(int64_t)0, (int64_t)7, top - L}) {
          if (s0 + L > top) continue;
          int64_t before = s0;
          bool ok = true;
          for (int32_t c = 0; c < width; ++c) {
            const int64_t t = patch_centre(s0, L, c, width);
            ok = ok && t >= before && (L == 0 ? t == s0 : (t >= s0 && t < s0 + L));
            before = t;
            // the first and the last sample index of the frame, as the kernel forms them
            ok = ok && t - n_fft / 2 >= -(int64_t)n_fft && t - n_fft / 2 + n_fft - 1 <= top + n_fft;
          }
          // the middle column of an odd width sits on the middle sample
          if (width % 2 == 1 && L > 0) ok = ok && patch_centre(s0, L, width / 2, width) == s0 + L / 2;
          if (!ok) { std::printf("  width %d, s0 %lld, L %lld: a centre outside the segment\n", (int)width, (long long)s0, (long long)L); ++fails; }
        }
      }
    }
    // the whole call: the device's table of (s0, s1) for a small call, then 2^31 - 1 synthetic segments up to 2^52 without a table
    {
      const Synthetic small{top, 1001};
      std::vector<int64_t> table(2 * 1001), array(2 * 1001);
      for (int32_t i = 0; i < 1001; ++i) small(i, &array[2 * i], &array[2 * i + 1]);
      PatchPlan p;
      if (patch_plan(small, 1001, 80, 256, n_fft, top, kPatchGridCap, &p, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; }
      segment_table_fill(table.data(), array.data(), 1001, nullptr);
      for (int32_t i = 0; i < 1001; ++i) {
        int64_t s0, s1;
        small(i, &s0, &s1);
        if (table[2 * i] != s0 || table[2 * i + 1] != s1 || s0 < 0 || s1 < s0 || s1 > top) { std::printf("  the table of segment %d\n", (int)i); ++fails; break; }
      }
      if (n_fft == 512 || n_fft == 8192) {         // (two billion segments take a few seconds: the walk does not depend on n_fft)
        const Synthetic huge{top, INT32_MAX};
        if (patch_plan(huge, INT32_MAX, 96, 256, n_fft, -1, kPatchGridCap, &p, msg, sizeof(msg)) || p.total_frames != (int64_t)INT32_MAX * 256 ||
            p.total_values != (int64_t)INT32_MAX * 256 * 96 || p.grid != kPatchGridCap) { std::printf("  2^31 - 1 segments: %s\n", msg); ++fails; }
        if (!rejected(patch_plan(huge, INT32_MAX, 96, 256, n_fft, top - 1, kPatchGridCap, &p, msg, sizeof(msg)), "bounds")) {
          std::printf("  2^31 - 1 segments: a segment behind the recording's end is accepted\n"); ++fails;
        }
      }
    }
    // what must be refused
    const int64_t reversed[2] = {9, 8}, negative[2] = {-1, 8}, huge_one[2] = {0, kSegmentMaxSamples + 1}, fine[2] = {0, 8};
    PatchPlan p;
    auto plan = [&](const int64_t* b, int32_t n_seg, int32_t n_mels, int32_t width, int32_t nf, int64_t n) {
      return patch_plan(SegmentBoundsArray{b}, n_seg, n_mels, width, nf, n, kPatchGridCap, &p, msg, sizeof(msg));
    };
    if (plan(fine, 1, 80, 32, n_fft, 8) || plan(fine, 1, 80, 32, n_fft, -1) || plan(nullptr, 0, 80, 32, n_fft, 0) ||
        !rejected(plan(reversed, 1, 80, 32, n_fft, -1), "bounds") || !rejected(plan(negative, 1, 80, 32, n_fft, -1), "bounds") ||
        !rejected(plan(huge_one, 1, 80, 32, n_fft, -1), "bounds") || !rejected(plan(fine, 1, 80, 32, n_fft, 7), "bounds") ||
        !rejected(plan(fine, 1, 80, 32, n_fft, INT64_MAX), "n must") || !rejected(plan(fine, -1, 80, 32, n_fft, -1), "n_seg") ||
        !rejected(plan(fine, INT32_MIN, 80, 32, n_fft, -1), "n_seg") || !rejected(plan(fine, 1, 80, 32, n_fft + 1, -1), "n_fft") ||
        !rejected(plan(fine, 1, 80, 32, n_fft * 32, -1), "n_fft") || !rejected(plan(fine, 1, 80, 32, 0, -1), "n_fft") ||
        !rejected(plan(fine, 1, 80, 32, -n_fft, -1), "n_fft") || !rejected(plan(fine, 1, 80, 32, 256, -1), "n_fft") ||
        !rejected(plan(fine, 1, 80, 0, n_fft, -1), "width") || !rejected(plan(fine, 1, 80, 257, n_fft, -1), "width") ||
        !rejected(plan(fine, 1, 80, INT32_MIN, n_fft, -1), "width") || !rejected(plan(fine, 1, 80, INT32_MAX, n_fft, -1), "width") ||
        !rejected(plan(fine, 1, 0, 32, n_fft, -1), "n_mels") || !rejected(plan(fine, 1, 97, 32, n_fft, -1), "n_mels") ||
        !rejected(plan(fine, 1, INT32_MIN, 32, n_fft, -1), "n_mels")) {
      std::printf("  valid input is refused or invalid input accepted (%s)\n", msg); ++fails;
    }
    std::printf("n_fft %4d: %lld plans up to 2^31 - 1 segments of 256 columns, centres up to 2^52: %s\n", (int)n_fft, (long long)plans,
                fails ? "FAILED" : "ok");
    bad += fails;
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
