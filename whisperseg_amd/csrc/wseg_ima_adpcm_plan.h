// The host arithmetic of the IMA ADPCM decode (wseg_ima_adpcm_to_mono_f32 / wseg_ima_adpcm_to_planar_f32), in one place: the
// validation of a call and the launch plan the kernel of wseg_ingest.hip is started with — and planar_range_check, the argument
// check of every planar entry point of that file.  Plain C++ with no HIP dependency, so that a host-only program can run it under
// a sanitizer (tools/ima_adpcm_plan_check.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>

namespace wseg {

constexpr int kAdpcmLanes = 256;           // lanes of a workgroup: one chain — a (block, channel) pair — per lane
constexpr int kAdpcmSliceDwords = 4;       // data dwords of a chain per slice: 32 samples, transposed through LDS and stored as runs
constexpr int kAdpcmPassDwords = 28;       // data dwords of a chain per pass of the LDS image: seven slices
constexpr int kAdpcmGridCap = 1024;        // workgroups; longer streams take the grid stride (whisperseg_amd/wavio.py::ADPCM_GRID_CAP)
constexpr int kAdpcmMaxChannelBytes = 65532;      // of a block, per channel (a file's nBlockAlign is a 16-bit field for all channels together)
constexpr int kAdpcmImageDwords = kAdpcmLanes * (kAdpcmPassDwords + 2);      // rows of ch * 29 dwords (| 1) for floor(256 / ch) blocks
constexpr int kAdpcmStageStride = 8 * kAdpcmSliceDwords + 1;                 // a chain's floats of a slice: the block's first sample + 32

struct AdpcmPlan {
  int32_t block_dwords;        // block_bytes / 4
  int32_t data_dwords;         // of one channel of a block: block_bytes / (4 channels) - 1
  int32_t block_frames;        // samples per block and channel: 8 data_dwords + 1
  int32_t group_blocks;        // blocks a workgroup takes at a time: floor(256 / channels)
  int32_t n_passes;            // image passes over a block: ceil(data_dwords / kAdpcmPassDwords)
  int32_t row_stride;          // dwords between the image rows of two blocks: the row's dwords | 1 (an odd stride: no bank is hit twice)
  int32_t grid;                // workgroups
  int64_t n_groups;            // ceil(n_blocks / group_blocks)
};

// Validates the arguments both entry points share and fills the plan -> 0, or -1 with the offending argument's name in msg.
// n_blocks == 0 is valid (n_frames must be 0 then; the plan's grid is 0: nothing is launched).  No product leaves int64.
inline int ima_adpcm_plan(int64_t n_blocks, int32_t block_bytes, int32_t channels, int64_t n_frames, AdpcmPlan* plan, char* msg,
                          size_t msg_len) {
  if (channels < 1 || channels > 64) { snprintf(msg, msg_len, "channels must be 1..64 (got %d)", (int)channels); return -1; }
  if (block_bytes <= 4 * channels || block_bytes > kAdpcmMaxChannelBytes * channels || (block_bytes - 4 * channels) % (4 * channels)) {
    snprintf(msg, msg_len, "block_bytes must be 4 * channels * (1 + k) for a k >= 1 and at most %d per channel (got %d for %d channels)",
             kAdpcmMaxChannelBytes, (int)block_bytes, (int)channels);
    return -1;
  }
  AdpcmPlan p;
  p.block_dwords = block_bytes / 4;
  p.data_dwords = block_bytes / (4 * channels) - 1;
  p.block_frames = 8 * p.data_dwords + 1;
  // n_blocks * block_bytes (below 2^22) and n_blocks * block_frames (below 2^17) stay inside int64
  if (n_blocks < 0 || n_blocks > ((int64_t)1 << 40)) {
    snprintf(msg, msg_len, "n_blocks must be 0..2^40 (got %lld)", (long long)n_blocks);
    return -1;
  }
  const int64_t most = n_blocks * p.block_frames, least = n_blocks ? most - p.block_frames + 1 : 0;
  if (n_frames < least || n_frames > most) {
    snprintf(msg, msg_len, "n_frames must be %lld..%lld for %lld blocks of %d frames (got %lld)", (long long)least, (long long)most,
             (long long)n_blocks, (int)p.block_frames, (long long)n_frames);
    return -1;
  }
  p.group_blocks = kAdpcmLanes / channels;
  p.n_passes = (p.data_dwords + kAdpcmPassDwords - 1) / kAdpcmPassDwords;
  const int32_t pass_dwords = p.data_dwords < kAdpcmPassDwords ? p.data_dwords : kAdpcmPassDwords;
  p.row_stride = (channels * (pass_dwords + 1)) | 1;
  p.n_groups = (n_blocks + p.group_blocks - 1) / p.group_blocks;
  p.grid = (int32_t)(p.n_groups < kAdpcmGridCap ? p.n_groups : kAdpcmGridCap);
  *plan = p;
  return 0;
}

// The arguments every planar entry point has beside its mono sibling's — wseg_pcm_to_planar_f32 / wseg_samples_to_planar_f32 and,
// after ima_adpcm_plan, wseg_ima_adpcm_to_planar_f32 — -> 0, or -1 with the argument's name in msg.
inline int planar_range_check(int32_t channels, int64_t n_frames, int32_t first_channel, int32_t n_out_channels, int64_t plane_stride,
                                  char* msg, size_t msg_len) {
  if (first_channel < 0 || first_channel >= channels) {
    snprintf(msg, msg_len, "first_channel must be 0..%d (got %d)", (int)channels - 1, (int)first_channel);
    return -1;
  }
  if (n_out_channels < 1 || n_out_channels > channels - first_channel) {
    snprintf(msg, msg_len, "n_out_channels must be 1..%d behind channel %d (got %d)", (int)(channels - first_channel), (int)first_channel,
             (int)n_out_channels);
    return -1;
  }
  if (n_out_channels > 1 && plane_stride < n_frames) {
    snprintf(msg, msg_len, "plane_stride (%lld) is shorter than the %lld frames of a plane", (long long)plane_stride, (long long)n_frames);
    return -1;
  }
  return 0;
}

}  // namespace wseg
