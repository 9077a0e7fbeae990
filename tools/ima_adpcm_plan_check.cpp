// Host-only check of the validation and launch plan of wseg_ima_adpcm_to_mono_f32 / wseg_ima_adpcm_to_planar_f32
// (whisperseg_amd/csrc/wseg_ima_adpcm_plan.h: plain C++, no HIP), over block sizes from the smallest (8 bytes per channel) to the
// largest (65 532 bytes per channel), 1 / 2 / 64 channels and recordings of one block up to 2^40 frames: the arithmetic must stay inside int64
// and int32, and the plan must keep what the kernel relies on.  Build it under the host sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/ima_adpcm_plan_check.cpp \
//       -o ima_adpcm_plan_check && ./ima_adpcm_plan_check
//
// For every (channels, block size, length) it asks for the plan of the whole blocks with the last one cut to one frame, to all but
// one and not at all, and fails unless: the block geometry is the format's; the groups cover the blocks exactly once; the rows of
// a group fit the LDS image at an odd stride that holds a pass's dwords; the passes cover the data dwords; the byte and frame
// offsets of the last group, computed as the kernel computes them, stay inside int64; frame counts outside the last block, bad
// block sizes, channel counts and planar ranges are rejected with the argument's name.  Prints one line per (channels, block size).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "../whisperseg_amd/csrc/wseg_ima_adpcm_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

int main() {
  const int channel_counts[] = {1, 2, 64};
  const int64_t lengths[] = {1, 1000, (int64_t)1 << 31, (int64_t)1 << 40};      // frames, at least
  int bad = 0;
  for (const int ch : channel_counts) {
    // bytes per channel of a block: the smallest, the usual powers of two, odd dword counts, the largest (one channel: what the 16-bit nBlockAlign allows)
    const int largest = kAdpcmMaxChannelBytes;
    const int per_channel[] = {8, 12, 36, 116, 120, 256, 1024, 2048, largest - 4, largest};
    for (const int pc : per_channel) {
      if (pc < 8 || pc > largest) continue;
      const int32_t block_bytes = pc * ch;
      const int32_t spb = 2 * (pc - 4) + 1;
      int fails = 0;
      AdpcmPlan p;
      for (const int64_t frames : lengths) {
        const int64_t n_blocks = (frames + spb - 1) / spb;
        for (const int64_t n_frames : {(n_blocks - 1) * spb + 1, n_blocks * spb - 1, n_blocks * spb}) {
          if (n_frames <= (n_blocks - 1) * spb) continue;      // (spb - 1 == 0 never happens: spb >= 9)
          if (ima_adpcm_plan(n_blocks, block_bytes, ch, n_frames, &p, msg, sizeof(msg))) { std::printf("  rejected: %s\n", msg); ++fails; continue; }
          const int pass_dwords = p.data_dwords < kAdpcmPassDwords ? p.data_dwords : kAdpcmPassDwords;
          bool ok = p.block_dwords * 4 == block_bytes && p.block_frames == spb && p.data_dwords * 8 + 1 == spb &&
                    p.group_blocks == kAdpcmLanes / ch && p.group_blocks * ch <= kAdpcmLanes &&
                    p.n_groups * p.group_blocks >= n_blocks && (p.n_groups - 1) * p.group_blocks < n_blocks &&
                    p.grid >= 1 && p.grid <= kAdpcmGridCap && p.grid <= p.n_groups &&
                    (p.row_stride & 1) && p.row_stride >= ch * (pass_dwords + 1) &&
                    (int64_t)p.group_blocks * p.row_stride <= kAdpcmImageDwords &&
                    (int64_t)(p.n_passes - 1) * kAdpcmPassDwords < p.data_dwords && (int64_t)p.n_passes * kAdpcmPassDwords >= p.data_dwords;
          // the kernel's offsets of the last block: dwords of raw, frames of out
          const int64_t last = n_blocks - 1;
          const int64_t dword = last * p.block_dwords + p.block_dwords, frame = last * p.block_frames + p.block_frames;
          ok = ok && dword > 0 && frame >= n_frames && dword <= INT64_MAX / 4;
          if (!ok) { std::printf("  a broken plan for %lld blocks, %lld frames\n", (long long)n_blocks, (long long)n_frames); ++fails; }
        }
        if (!rejected(ima_adpcm_plan(n_blocks, block_bytes, ch, n_blocks * spb + 1, &p, msg, sizeof(msg)), "n_frames") ||
            !rejected(ima_adpcm_plan(n_blocks, block_bytes, ch, (n_blocks - 1) * spb, &p, msg, sizeof(msg)), "n_frames") ||
            !rejected(ima_adpcm_plan(n_blocks, block_bytes, ch, -1, &p, msg, sizeof(msg)), "n_frames") ||
            !rejected(ima_adpcm_plan(n_blocks, block_bytes, ch, INT64_MAX, &p, msg, sizeof(msg)), "n_frames")) {
          std::printf("  a frame count outside the last block is accepted\n"); ++fails;
        }
      }
      if (ima_adpcm_plan(0, block_bytes, ch, 0, &p, msg, sizeof(msg)) || p.grid != 0 || p.n_groups != 0) { std::printf("  no blocks: %s\n", msg); ++fails; }
      if (!rejected(ima_adpcm_plan(0, block_bytes, ch, 1, &p, msg, sizeof(msg)), "n_frames") ||
          !rejected(ima_adpcm_plan(-1, block_bytes, ch, 0, &p, msg, sizeof(msg)), "n_blocks") ||
          !rejected(ima_adpcm_plan(INT64_MAX, block_bytes, ch, INT64_MAX, &p, msg, sizeof(msg)), "n_blocks") ||
          !rejected(ima_adpcm_plan(((int64_t)1 << 40) + 1, block_bytes, ch, 1, &p, msg, sizeof(msg)), "n_blocks")) {
        std::printf("  a bad block count is accepted\n"); ++fails;
      }
      if ((ch > 1 && !rejected(ima_adpcm_plan(1, block_bytes + 4, ch, 1, &p, msg, sizeof(msg)), "block_bytes")) ||      // (one channel: any multiple of 4 from 8 on is a block)
          !rejected(ima_adpcm_plan(1, block_bytes + 2, ch, 1, &p, msg, sizeof(msg)), "block_bytes") ||
          !rejected(ima_adpcm_plan(1, 4 * ch, ch, 1, &p, msg, sizeof(msg)), "block_bytes") ||
          !rejected(ima_adpcm_plan(1, 0, ch, 1, &p, msg, sizeof(msg)), "block_bytes") ||
          !rejected(ima_adpcm_plan(1, -block_bytes, ch, 1, &p, msg, sizeof(msg)), "block_bytes") ||
          !rejected(ima_adpcm_plan(1, INT32_MAX, ch, 1, &p, msg, sizeof(msg)), "block_bytes") ||
          !rejected(ima_adpcm_plan(1, (kAdpcmMaxChannelBytes + 4) * ch, ch, 1, &p, msg, sizeof(msg)), "block_bytes") ||
          !rejected(ima_adpcm_plan(1, block_bytes, 0, 1, &p, msg, sizeof(msg)), "channels") ||
          !rejected(ima_adpcm_plan(1, block_bytes, 65, 1, &p, msg, sizeof(msg)), "channels") ||
          !rejected(ima_adpcm_plan(1, block_bytes, -1, 1, &p, msg, sizeof(msg)), "channels")) {
        std::printf("  a bad block size or channel count is accepted (%s)\n", msg); ++fails;
      }
      const int64_t n = (int64_t)1 << 40;
      if (planar_range_check(ch, n, 0, ch, n, msg, sizeof(msg)) || planar_range_check(ch, n, ch - 1, 1, 0, msg, sizeof(msg)) ||
          !rejected(planar_range_check(ch, n, ch, 1, n, msg, sizeof(msg)), "first_channel") ||
          !rejected(planar_range_check(ch, n, -1, 1, n, msg, sizeof(msg)), "first_channel") ||
          !rejected(planar_range_check(ch, n, 0, ch + 1, n, msg, sizeof(msg)), "n_out_channels") ||
          !rejected(planar_range_check(ch, n, 0, 0, n, msg, sizeof(msg)), "n_out_channels") ||
          !rejected(planar_range_check(ch, n, ch - 1, 2, n, msg, sizeof(msg)), "n_out_channels") ||
          (ch > 1 && !rejected(planar_range_check(ch, n, 0, 2, n - 1, msg, sizeof(msg)), "plane_stride"))) {
        std::printf("  a planar range is misjudged (%s)\n", msg); ++fails;
      }
      std::printf("%2d channels, blocks of %5d bytes (%6d frames): %d passes, rows %4d dwords apart, %3d blocks a group: %s\n", ch, (int)block_bytes,
                  (int)spb, (int)p.n_passes, (int)p.row_stride, (int)p.group_blocks, fails ? "FAILED" : "ok");
      bad += fails;
    }
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
