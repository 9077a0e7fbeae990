// Audio sample decode (audio ingest): interleaved frames exactly as they sit in the sample chunk of a WAVE /
// RF64, AIFF / AIFF-C or AU file -> float32 mono.  Replaces the decoding half of `librosa.load(path, sr=None)` (reference
// scripts/segment.py:48,61; evaluate.py:58), i.e. what whisperseg_amd/wavio.py::load_wav / load_audio do with numpy on the host,
// and produces the same float32 bits:
//   u8 (x - 128) / 128 | s16 x / 2^15 | s24 sign-extended / 2^23 | s32 one int -> float32 rounding, then the exact scale 2^-31
//   f32 copied | f64 one round-to-nearest-even conversion (beyond the float32 range: +-inf)
//   wseg_sample_encoding 6..13 (whisperseg_amd/wavio.py::load_audio): s8 x / 128 | s16be / s24be / s32be / f32be / f64be the bytes
//   swapped in registers, then as their little-endian siblings | u-law / A-law the G.711 expansion to int16 (integer arithmetic in
//   registers, no table), then x / 2^15
//   channels > 1: numpy's mean(axis=1) of the float32 samples of a frame — the sum starts from +0 (so a frame of -0.0 samples
//   gives +0.0), runs left to right for fewer than 8 channels and in numpy's pairwise order from 8 channels on (eight strided
//   partial sums, combined as a tree, the last channels % 8 samples added one by one), then ONE division by float(channels).
// A pure stream (HBM-bound: 1..8 bytes in per sample, 4 bytes out per frame).  The unit of work is a GROUP of four output frames:
// one lane, one 16-byte store.  A group's bytes start on a dword for every frame size, so a lane reads the aligned dwords that
// cover its group (16-byte loads where the group is a multiple of 16 bytes) and takes samples apart in registers; the last
// n_frames % 4 frames are read byte by byte by one lane.  No LDS, no scratch; all indexing is 64-bit.
// wseg_pcm_to_planar_f32 (further down) keeps the channels apart instead of averaging them, through an LDS image of a tile of frames.
// wseg_ima_adpcm_to_mono_f32 / _planar_f32 (last) decode the one block codec of the ingest, IMA ADPCM: one sequential chain per lane.
#include <type_traits>
#include "wseg_common.h"
#include "wseg_ima_adpcm_plan.h"

namespace wseg {

constexpr int kBytes[14] = {1, 2, 3, 4, 4, 8, 1, 2, 3, 4, 4, 8, 1, 1};      // bytes per sample of wseg_sample_encoding

// G.711 code -> int16 (ITU-T G.711's expansion, as libsndfile and CPython's audioop tabulate it).
__device__ __forceinline__ int ulaw_to_s16(uint32_t b) {
  const uint32_t u = ~b & 0xffu;
  const int t = (int)((((u & 15u) << 3) + 0x84u) << ((u & 0x70u) >> 4));
  return (u & 0x80u) ? 0x84 - t : t - 0x84;
}
__device__ __forceinline__ int alaw_to_s16(uint32_t b) {
  const uint32_t a = (b ^ 0x55u) & 0xffu;
  const uint32_t s = (a & 0x70u) >> 4;
  uint32_t t = (a & 15u) << 4;
  t = s ? (t + 0x108u) << (s - 1) : t + 8u;
  return (a & 0x80u) ? (int)t : -(int)t;
}

// Sample at byte `b` (a multiple of the sample size for the 1- and 2-byte encodings, of 4 for the 4- and 8-byte ones, any for
// s24 / s24be) of the dword array `w`.  With a register array and a compile-time `b` this is shifts only.
template <int FMT, class W>
__device__ __forceinline__ float sample_at(const W& w, long long b) {
  const long long d = b >> 2;
  const int sh = (int)(b & 3) * 8;
  if constexpr (FMT == WSEG_PCM_U8) {
    return ((float)((w[d] >> sh) & 0xffu) - 128.0f) / 128.0f;
  } else if constexpr (FMT == WSEG_PCM_S16) {
    return (float)(int16_t)(w[d] >> sh) / 32768.0f;
  } else if constexpr (FMT == WSEG_PCM_S24) {
    uint32_t v = w[d] >> sh;
    if (sh > 8) v |= w[d + 1] << (32 - sh);        // the sample ends in the next dword (which exists: it holds the sample's last byte)
    return (float)((int32_t)(v << 8) >> 8) / 8388608.0f;
  } else if constexpr (FMT == WSEG_PCM_S32) {
    return (float)(int32_t)w[d] * 4.656612873077393e-10f;      // 2^-31: exact, no result is subnormal
  } else if constexpr (FMT == WSEG_PCM_F32) {
    return __uint_as_float(w[d]);
  } else if constexpr (FMT == WSEG_PCM_F64) {
    return (float)__longlong_as_double((long long)(((unsigned long long)w[d + 1] << 32) | w[d]));
  } else if constexpr (FMT == WSEG_ENC_S8) {
    return (float)(int8_t)(w[d] >> sh) / 128.0f;
  } else if constexpr (FMT == WSEG_ENC_S16BE) {
    const uint32_t v = w[d] >> sh;
    return (float)(int16_t)(((v & 0xffu) << 8) | ((v >> 8) & 0xffu)) / 32768.0f;
  } else if constexpr (FMT == WSEG_ENC_S24BE) {
    uint32_t v = w[d] >> sh;
    if (sh > 8) v |= w[d + 1] << (32 - sh);        // as for s24: the sample ends in the next dword
    return (float)((int32_t)__builtin_bswap32(v) >> 8) / 8388608.0f;      // the swap puts the three bytes on top: the shift sign-extends
  } else if constexpr (FMT == WSEG_ENC_S32BE) {
    return (float)(int32_t)__builtin_bswap32(w[d]) * 4.656612873077393e-10f;
  } else if constexpr (FMT == WSEG_ENC_F32BE) {
    return __uint_as_float(__builtin_bswap32(w[d]));
  } else if constexpr (FMT == WSEG_ENC_F64BE) {
    return (float)__longlong_as_double((long long)(((unsigned long long)__builtin_bswap32(w[d]) << 32) | __builtin_bswap32(w[d + 1])));
  } else if constexpr (FMT == WSEG_ENC_ULAW) {
    return (float)ulaw_to_s16(w[d] >> sh) / 32768.0f;
  } else {
    static_assert(FMT == WSEG_ENC_ALAW, "unknown sample encoding");
    return (float)alaw_to_s16(w[d] >> sh) / 32768.0f;
  }
}

// The tail's view of raw: dword d assembled from byte loads, never touching a byte the sample does not own.
template <int FMT>
__device__ __forceinline__ float sample_bytes(const uint8_t* __restrict__ raw, long long b) {
  constexpr int B = kBytes[FMT];
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < B; ++i) {
    const uint32_t v = raw[b + i];
    if (i < 4) lo |= v << (8 * i); else hi |= v << (8 * (i - 4));
  }
  const uint32_t w[2] = {lo, hi};
  return sample_at<FMT>(w, 0);
}

// numpy's add.reduce over the channels of one frame, then the mean.  get(c): float32 sample of channel c.
template <int CH, class Get>
__device__ __forceinline__ float frame_mean(int ch, Get get) {
  if constexpr (CH == 1) {
    return get(0);
  } else if constexpr (CH == 2) {
    return (0.0f + (get(0) + get(1))) / 2.0f;
  } else {
    float s;
    if (ch < 8) {
      s = get(0);
      for (int c = 1; c < ch; ++c) s += get(c);
    } else {
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = get(j);
      int c = 8;
      for (; c < ch - (ch & 7); c += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += get(c + j);
      }
      s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      for (; c < ch; ++c) s += get(c);
    }
    return (0.0f + s) / (float)ch;
  }
}

template <int N>
struct Dwords {
  uint32_t v[N];
  __device__ __forceinline__ uint32_t operator[](long long i) const { return v[i]; }
};

// The N dwords of a group at p (a multiple of 4 N bytes behind a 16-byte aligned base): the widest loads that alignment allows.
template <int N>
__device__ __forceinline__ Dwords<N> load_group(const uint32_t* __restrict__ p) {
  Dwords<N> r;
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
      const uint4 q = reinterpret_cast<const uint4*>(p)[i];
      r.v[4 * i] = q.x; r.v[4 * i + 1] = q.y; r.v[4 * i + 2] = q.z; r.v[4 * i + 3] = q.w;
    }
  } else if constexpr (N % 2 == 0) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      const uint2 q = reinterpret_cast<const uint2*>(p)[i];
      r.v[2 * i] = q.x; r.v[2 * i + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) r.v[i] = p[i];
  }
  return r;
}

// CH = 1 / 2: unrolled bodies over a register copy of the group; CH = 0: any channel count, dwords fetched sample by sample.
template <int FMT, int CH>
__global__ __launch_bounds__(256) void pcm_to_mono_kernel(const void* __restrict__ raw_, long long n_frames, int ch,
                                                          float* __restrict__ out, int out_aligned) {
  constexpr int B = kBytes[FMT];
  const uint32_t* __restrict__ raw = static_cast<const uint32_t*>(raw_);
  const long long n_groups = n_frames >> 2;
  const long long frame_bytes = (long long)(CH ? CH : ch) * B;
  const long long stride = (long long)gridDim.x * 256;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += stride) {
    float y[4];
    if constexpr (CH != 0) {
      constexpr int N = CH * B;                    // dwords of a group = bytes of a frame
      const Dwords<N> w = load_group<N>(raw + g * N);
#pragma unroll
      for (int f = 0; f < 4; ++f)
        y[f] = frame_mean<CH>(CH, [&](int c) { return sample_at<FMT>(w, (long long)((f * CH + c) * B)); });
    } else {
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const long long b0 = (4 * g + f) * frame_bytes;
        y[f] = frame_mean<0>(ch, [&](int c) { return sample_at<FMT>(raw, b0 + (long long)c * B); });
      }
    }
    if (out_aligned) {
      *reinterpret_cast<float4*>(out + 4 * g) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int f = 0; f < 4; ++f) out[4 * g + f] = y[f];
    }
  }
  // the last n_frames % 4 frames: one lane, byte loads
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint8_t* __restrict__ bytes = static_cast<const uint8_t*>(raw_);
    for (long long fr = n_groups << 2; fr < n_frames; ++fr) {
      const long long b0 = fr * frame_bytes;
      out[fr] = frame_mean<CH>(CH ? CH : ch, [&](int c) { return sample_bytes<FMT>(bytes, b0 + (long long)c * B); });
    }
  }
}

template <int FMT>
static void launch_pcm(int ch, dim3 grid, hipStream_t s, const void* raw, long long n_frames, float* out, int out_aligned) {
  if (ch == 1) hipLaunchKernelGGL((pcm_to_mono_kernel<FMT, 1>), grid, dim3(256), 0, s, raw, n_frames, ch, out, out_aligned);
  else if (ch == 2) hipLaunchKernelGGL((pcm_to_mono_kernel<FMT, 2>), grid, dim3(256), 0, s, raw, n_frames, ch, out, out_aligned);
  else hipLaunchKernelGGL((pcm_to_mono_kernel<FMT, 0>), grid, dim3(256), 0, s, raw, n_frames, ch, out, out_aligned);
}

// ---- the channels kept apart (wseg_pcm_to_planar_f32) -------------------------------------------------------------------------
// The mono kernel's CH = 0 path lets every lane walk its own four frames through global memory (a lane stride of four frames:
// coalesced only through the cache).  Here a workgroup takes a TILE of kPlanarTile consecutive frames and goes through it in
// passes of as many frames (a multiple of 16: every pass starts on a 16-byte boundary whatever the frame size) as fit the LDS
// image: the pass's contiguous bytes come in with coalesced 16-byte loads, each byte once, and the planes are taken out of the
// image — an item is (plane, four consecutive frames), consecutive lanes on consecutive groups of one plane, one 16-byte store
// each.  The groups of a plane are laid on ITS 16-byte grid (a plane whose address is m floats behind a 16-byte boundary takes
// frames 4g - m .. 4g - m + 3 as group g), so every plane gets 16-byte stores; the groups cut by the pass's two ends store
// their frames dword by dword.  The image carries one pad dword behind every 16: the lane stride of the de-interleaving reads is
// one frame's bytes in dwords, and frame sizes that are a power of two (s16 x 8: 16 dwords) would put the 32 lanes of a
// ds_read_b32 group on two banks; padded, 16 -> 17 is conflict-free and 4 / 8 / 32 are 2-way.  The price is that the image is
// written dword by dword (its 16-byte pieces are no longer aligned).  Measured (profiles/ingest_planar_ab.txt): 5.3-6.4 TB/s padded
// against 3.6-3.9 TB/s with an unpadded image written by 16-byte LDS stores, for every frame size tried, odd ones included.
constexpr int kPlanarTile = 1024;                  // frames per tile (whisperseg_amd/wavio.py::PLANAR_TILE_FRAMES)
constexpr int kPlanarImage = 16384;                // bytes of a pass: 1024 frames of up to 16 bytes, 32 frames of 512
constexpr int kPlanarGridCap = 2048;               // 8 workgroups per CU; longer streams take the grid stride (wavio.PLANAR_GRID_CAP)

struct PaddedImage {
  const uint32_t* w;
  __device__ __forceinline__ uint32_t operator[](long long d) const { const int i = (int)d; return w[i + (i >> 4)]; }
};

template <int FMT>
__global__ __launch_bounds__(256) void pcm_to_planar_kernel(const void* __restrict__ raw_, long long n_frames, int ch, int first, int n_out,
                                                            float* __restrict__ out, long long plane_stride) {
  constexpr int B = kBytes[FMT];
  __shared__ uint32_t image[kPlanarImage / 4 + kPlanarImage / 64];
  const PaddedImage img{image};
  const uint4* __restrict__ raw = static_cast<const uint4*>(raw_);
  const int frame_bytes = ch * B;                                                  // <= 512
  const int pass_max = min(kPlanarTile, kPlanarImage / frame_bytes / 16 * 16);     // >= 32
  const int slots = pass_max / 4 + 1;                                              // groups of a plane in a pass, at most
  const int n_items = n_out * slots;
  const int tid = threadIdx.x;
  const long long n_tiles = (n_frames + kPlanarTile - 1) / kPlanarTile;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long t0 = tile * kPlanarTile;
    const int n_tile = (int)min((long long)kPlanarTile, n_frames - t0);
    for (int p0 = 0; p0 < n_tile; p0 += pass_max) {
      const int n = min(pass_max, n_tile - p0);
      const long long chunk0 = ((t0 + p0) * frame_bytes) >> 4;                    // (a multiple of 16 frames: exact)
      const int chunks = (n * frame_bytes + 15) >> 4;                              // <= 1024; the file's last one may be cut: raw is readable to there
      uint4 q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (tid + 256 * k < chunks) q[k] = raw[chunk0 + tid + 256 * k];
      __syncthreads();                                                             // the pass before has been taken out
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k;
        if (i < chunks) {
          uint32_t* p = image + 4 * i + (i >> 2);
          p[0] = q[k].x; p[1] = q[k].y; p[2] = q[k].z; p[3] = q[k].w;
        }
      }
      __syncthreads();
      for (int it = tid; it < n_items; it += 256) {
        const int c = it / slots, g = it - c * slots;
        float* __restrict__ plane = out + (long long)c * plane_stride + (t0 + p0);
        const int f0 = 4 * g - (int)(((uintptr_t)plane >> 2) & 3);
        if (f0 >= n) continue;
        const int b0 = f0 * frame_bytes + (first + c) * B;
        if (f0 >= 0 && f0 + 4 <= n) {
          float y[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) y[k] = sample_at<FMT>(img, (long long)(b0 + k * frame_bytes));
          *reinterpret_cast<float4*>(plane + f0) = make_float4(y[0], y[1], y[2], y[3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (f0 + k >= 0 && f0 + k < n) plane[f0 + k] = sample_at<FMT>(img, (long long)(b0 + k * frame_bytes));
        }
      }
    }
  }
}

// ---- IMA ADPCM (wseg_ima_adpcm_to_mono_f32 / wseg_ima_adpcm_to_planar_f32) -------------------------------------------------------
// A block codec: inside a block every sample of a channel follows from the one before it (predictor and step index), so the unit of
// parallel work is a CHAIN, one (block, channel) pair, and a lane runs one chain: block_frames - 1 dependent steps, each with a
// divergent look-up of the step table — which therefore sits in LDS (89 dwords the workgroup fills), not in constant memory.
// A workgroup takes GROUPS of floor(256 / channels) whole blocks, so that every channel of a frame is decoded in the workgroup
// that averages it.  The bytes of a group go through an LDS image in PASSES of kAdpcmPassDwords data dwords per chain (pass 0 with
// the block's headers in front): a row per block, filled by coalesced 16-byte loads — consecutive lanes on consecutive 16-byte
// pieces of one block's stretch, then of the next block's; only a piece that straddles the end of a stretch (blocks that are no
// multiple of 16 bytes, or the seam of two passes) is fetched by both sides, each keeping its own dwords.  The rows are an odd
// number of dwords apart: the chains of a one-channel file read the image at a lane stride of one row, and block sizes are
// typically powers of two (the pad of PaddedImage above, per row instead of per 16 dwords).
// A chain advances in SLICES of four dwords = 32 samples, written as floats to its row of the stage (33 floats: slice 0 also holds
// the block's first sample, which is the header's predictor; an odd stride again).  Behind a barrier the slice leaves as contiguous
// runs: an item is (plane, block, four frames on the PLANE's 16-byte grid), consecutive lanes on consecutive items of one run, a
// 16-byte store each and dword stores at the run's cut ends — as in pcm_to_planar_kernel; block starts b * block_frames are odd
// offsets, so the grid is taken from the address.  The mono mix averages the stage's rows of a block with frame_mean (numpy's order).
// All trip counts (groups, passes, slices) are uniform over the workgroup; lanes without a chain only pass the barriers.
__device__ const int kImaSteps[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157,
    173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707,
    1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635,
    13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

// MONO: every channel's chain runs and the frames' means go to out; else the chains of channels first .. first + n_sel - 1 go to
// planes plane_stride floats apart.
template <bool MONO>
__global__ __launch_bounds__(256) void ima_adpcm_kernel(const void* __restrict__ raw_, long long n_blocks, int ch, long long n_frames, int first,
                                                        int n_sel, float* __restrict__ out, long long plane_stride, AdpcmPlan plan) {
  __shared__ uint32_t image[kAdpcmImageDwords];
  __shared__ float stage[kAdpcmLanes * kAdpcmStageStride];
  __shared__ int steps[89];
  const int tid = threadIdx.x;
  if (tid < 89) steps[tid] = kImaSteps[tid];                   // (read behind the barrier that follows the first image fill)
  const uint4* __restrict__ raw = static_cast<const uint4*>(raw_);
  const int rs = plan.row_stride, nd = plan.data_dwords;
  const int chains = MONO ? ch : n_sel;                        // chains per block
  const int my_block = tid / chains, my_c = (MONO ? 0 : first) + (tid - my_block * chains);
  float* const my_stage = stage + tid * kAdpcmStageStride;     // (tid = my_block * chains + the chain's number in its block)
  for (long long grp = blockIdx.x; grp < plan.n_groups; grp += gridDim.x) {
    const long long b0 = grp * plan.group_blocks;
    const int gb = (int)min((long long)plan.group_blocks, n_blocks - b0);
    const bool has_chain = my_block < gb;
    int pred = 0, idx = 0;
    for (int pass = 0; pass < plan.n_passes; ++pass) {
      const int j0 = pass * kAdpcmPassDwords, nj = min(kAdpcmPassDwords, nd - j0);
      const int lo = pass ? ch * (1 + j0) : 0, len = ch * (1 + j0 + nj) - lo;    // the stretch [lo, lo + len) of a block's dwords
      const int pieces = (4 * len + 27) >> 4;                  // the 16-byte pieces it can touch, wherever it starts
      for (int i = tid; i < gb * pieces; i += 256) {
        const int r = i / pieces, k = i - r * pieces;
        const long long d_lo = (b0 + r) * plan.block_dwords + lo;
        const long long piece = (d_lo >> 2) + k;
        const int rel = (int)((piece << 2) - d_lo);            // -3 .. : the piece's first dword, counted from the stretch's
        if (rel < len) {                                       // (the piece starts inside the block: raw is readable to its end)
          const uint4 q = raw[piece];
          const uint32_t v[4] = {q.x, q.y, q.z, q.w};
          uint32_t* row = image + r * rs;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (rel + e >= 0 && rel + e < len) row[rel + e] = v[e];
        }
      }
      __syncthreads();
      if (pass == 0 && has_chain) {                            // the chain's header: int16 predictor, u8 step index, u8 reserved
        const uint32_t h = image[my_block * rs + my_c];
        pred = (int)(int16_t)(h & 0xffffu);
        idx = min((int)((h >> 16) & 0xffu), 88);
      }
      const int base = my_block * rs + (pass ? 0 : ch) + my_c;  // the chain's data dword j0 + j at base + j * ch
      for (int s = 0; 4 * s < nj; ++s) {
        const int nq = min(kAdpcmSliceDwords, nj - 4 * s);
        const bool first_slice = pass == 0 && s == 0;
        if (has_chain) {
          if (first_slice) my_stage[0] = (float)pred / 32768.0f;
          for (int q = 0; q < nq; ++q) {
            const uint32_t w = image[base + (4 * s + q) * ch];
#pragma unroll
            for (int e = 0; e < 8; ++e) {                      // low nibble first
              const int d = (int)((w >> (4 * e)) & 15u);
              const int step = steps[idx];
              int diff = step >> 3;
              if (d & 4) diff += step;
              if (d & 2) diff += step >> 1;
              if (d & 1) diff += step >> 2;
              pred = (d & 8) ? pred - diff : pred + diff;
              pred = min(max(pred, -32768), 32767);
              idx += (d & 4) ? ((d & 3) << 1) + 2 : -1;
              idx = min(max(idx, 0), 88);
              my_stage[1 + 8 * q + e] = (float)pred / 32768.0f;
            }
          }
        }
        __syncthreads();
        // the slice's run of a block: samples [r0, r0 + run) of the block, at stage offset so of the chains' rows
        const int r0 = first_slice ? 0 : 1 + 8 * (j0 + 4 * s), so = first_slice ? 0 : 1, run = 8 * nq + (first_slice ? 1 : 0);
        const int n_items = (MONO ? 1 : n_sel) * gb * 9;        // 33 frames and up to 3 in front of them: nine groups of four
        for (int it = tid; it < n_items; it += 256) {
          const int row = it / 9, g = it - row * 9;
          const int p = row / gb, bl = row - p * gb;            // plane-major: consecutive rows are consecutive blocks of one plane
          const long long f_first = (b0 + bl) * plan.block_frames + r0;
          const int n = (int)min((long long)run, n_frames - f_first);      // n_frames cuts the last block (n <= 0: nothing left)
          float* __restrict__ dst = out + p * plane_stride + f_first;
          const int f0 = 4 * g - (int)(((uintptr_t)dst >> 2) & 3);
          if (f0 >= n) continue;
          const float* src = stage + (bl * chains + p) * kAdpcmStageStride + so;
          auto value = [&](int f) {
            if (!MONO || ch == 1) return src[f];
            return frame_mean<0>(ch, [&](int c) { return src[c * kAdpcmStageStride + f]; });
          };
          if (f0 >= 0 && f0 + 4 <= n) {
            *reinterpret_cast<float4*>(dst + f0) = make_float4(value(f0), value(f0 + 1), value(f0 + 2), value(f0 + 3));
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (f0 + k >= 0 && f0 + k < n) dst[f0 + k] = value(f0 + k);
          }
        }
        __syncthreads();                                       // the stage, and behind the last slice the image, may be rewritten
      }
    }
  }
}

}  // namespace wseg

using namespace wseg;

// The first checks of every entry point, in this order (`what`: the name of its format / encoding argument, whose codes are
// 0..last; nullptr: it has none); samples_to_mono / samples_to_planar / ima_adpcm_decode do the rest.
static bool head_ok(const char* fn, const void* raw, const float* out, int32_t channels, const char* what = nullptr, int32_t code = 0,
                    int32_t last = 0) {
  if (!raw || ((uintptr_t)raw & 15)) { set_error("%s: raw must be a 16-byte aligned device pointer", fn); return false; }
  if (!out || ((uintptr_t)out & 3)) { set_error("%s: out must be a float32 device pointer", fn); return false; }
  if (channels < 1 || channels > 64) { set_error("%s: channels must be 1..64 (got %d)", fn, channels); return false; }
  if (what && (code < 0 || code > last)) { set_error("%s: unknown %s %d", fn, what, code); return false; }
  return true;
}

// THE list of the encodings (wseg_sample_encoding): f(std::integral_constant<int, E>()) for the E that `code` is, so that f has
// the encoding as a compile-time constant -> whether it is one of them.
template <int... E>
struct Encodings {};
using AllEncodings = Encodings<WSEG_PCM_U8, WSEG_PCM_S16, WSEG_PCM_S24, WSEG_PCM_S32, WSEG_PCM_F32, WSEG_PCM_F64, WSEG_ENC_S8, WSEG_ENC_S16BE,
                               WSEG_ENC_S24BE, WSEG_ENC_S32BE, WSEG_ENC_F32BE, WSEG_ENC_F64BE, WSEG_ENC_ULAW, WSEG_ENC_ALAW>;
template <class F, int... E>
static bool with_encoding(int code, F f, Encodings<E...>) {
  return ((code == E && (f(std::integral_constant<int, E>()), true)) || ...);
}

// The remaining checks and the launch of wseg_pcm_to_mono_f32 / wseg_samples_to_mono_f32 (`fn`: the entry point's name for the
// messages; the caller has checked the code, 0..13).
static int samples_to_mono(const char* fn, const void* raw, int64_t n_frames, int32_t channels, int32_t code, float* out, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (n_frames < 0) { set_error("%s: n_frames is negative", fn); return WSEG_ERR_INVALID; }
  if (n_frames == 0) return WSEG_OK;
  long long blocks = ((n_frames >> 2) + 255) / 256;
  if (blocks < 1) blocks = 1;                      // fewer than four frames: the tail lane alone
  if (blocks > 8192) blocks = 8192;                // 32 workgroups per CU; longer streams take the grid stride
  const dim3 grid((unsigned)blocks);
  const int out_aligned = ((uintptr_t)out & 15) == 0;
  with_encoding(code, [&](auto fmt) { launch_pcm<decltype(fmt)::value>(channels, grid, s, raw, n_frames, out, out_aligned); }, AllEncodings());
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}

static int samples_to_planar(const char* fn, const void* raw, int64_t n_frames, int32_t channels, int32_t code, int32_t first_channel,
                             int32_t n_out_channels, float* out, int64_t plane_stride, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (n_frames < 0) { set_error("%s: n_frames is negative", fn); return WSEG_ERR_INVALID; }
  char msg[200];
  if (planar_range_check(channels, n_frames, first_channel, n_out_channels, plane_stride, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (n_frames == 0) return WSEG_OK;
  long long blocks = (n_frames + kPlanarTile - 1) / kPlanarTile;
  if (blocks > kPlanarGridCap) blocks = kPlanarGridCap;
  const dim3 grid((unsigned)blocks);
  const long long stride = n_out_channels > 1 ? plane_stride : 0;
  with_encoding(code, [&](auto fmt) {
    hipLaunchKernelGGL((pcm_to_planar_kernel<decltype(fmt)::value>), grid, dim3(256), 0, s, raw, (long long)n_frames, (int)channels, (int)first_channel,
                       (int)n_out_channels, out, stride);
  }, AllEncodings());
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}

extern "C" int wseg_pcm_to_mono_f32(const void* raw, int64_t n_frames, int32_t channels, int32_t format, float* out, void* stream) {
  if (!head_ok("wseg_pcm_to_mono_f32", raw, out, channels, "format", format, WSEG_PCM_F64)) return WSEG_ERR_INVALID;
  return samples_to_mono("wseg_pcm_to_mono_f32", raw, n_frames, channels, format, out, stream);
}

extern "C" int wseg_samples_to_mono_f32(const void* raw, int64_t n_frames, int32_t channels, int32_t encoding, float* out, void* stream) {
  if (!head_ok("wseg_samples_to_mono_f32", raw, out, channels, "encoding", encoding, WSEG_ENC_ALAW)) return WSEG_ERR_INVALID;
  return samples_to_mono("wseg_samples_to_mono_f32", raw, n_frames, channels, encoding, out, stream);
}

extern "C" int wseg_pcm_to_planar_f32(const void* raw, int64_t n_frames, int32_t channels, int32_t format, int32_t first_channel,
                                      int32_t n_out_channels, float* out, int64_t plane_stride, void* stream) {
  if (!head_ok("wseg_pcm_to_planar_f32", raw, out, channels, "format", format, WSEG_PCM_F64)) return WSEG_ERR_INVALID;
  return samples_to_planar("wseg_pcm_to_planar_f32", raw, n_frames, channels, format, first_channel, n_out_channels, out, plane_stride, stream);
}

extern "C" int wseg_samples_to_planar_f32(const void* raw, int64_t n_frames, int32_t channels, int32_t encoding, int32_t first_channel,
                                          int32_t n_out_channels, float* out, int64_t plane_stride, void* stream) {
  if (!head_ok("wseg_samples_to_planar_f32", raw, out, channels, "encoding", encoding, WSEG_ENC_ALAW)) return WSEG_ERR_INVALID;
  return samples_to_planar("wseg_samples_to_planar_f32", raw, n_frames, channels, encoding, first_channel, n_out_channels, out, plane_stride, stream);
}

// The checks and the launch of both IMA ADPCM entry points (planar: n_out_channels >= 1; mono: 0).
static int ima_adpcm_decode(const char* fn, const void* raw, int64_t n_blocks, int32_t block_bytes, int32_t channels, int64_t n_frames,
                            int32_t first_channel, int32_t n_out_channels, bool mono, float* out, int64_t plane_stride, void* stream_) {
  if (!head_ok(fn, raw, out, channels)) return WSEG_ERR_INVALID;
  AdpcmPlan plan;
  char msg[200];
  if (ima_adpcm_plan(n_blocks, block_bytes, channels, n_frames, &plan, msg, sizeof(msg)) ||
      (!mono && planar_range_check(channels, n_frames, first_channel, n_out_channels, plane_stride, msg, sizeof(msg)))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (n_blocks == 0) return WSEG_OK;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((unsigned)plan.grid);
  if (mono) {
    hipLaunchKernelGGL((ima_adpcm_kernel<true>), grid, dim3(kAdpcmLanes), 0, s, raw, (long long)n_blocks, (int)channels, (long long)n_frames, 0,
                       (int)channels, out, 0LL, plan);
  } else {
    hipLaunchKernelGGL((ima_adpcm_kernel<false>), grid, dim3(kAdpcmLanes), 0, s, raw, (long long)n_blocks, (int)channels, (long long)n_frames,
                       (int)first_channel, (int)n_out_channels, out, n_out_channels > 1 ? (long long)plane_stride : 0LL, plan);
  }
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}

extern "C" int wseg_ima_adpcm_to_mono_f32(const void* raw, int64_t n_blocks, int32_t block_bytes, int32_t channels, int64_t n_frames,
                                          float* out, void* stream) {
  return ima_adpcm_decode("wseg_ima_adpcm_to_mono_f32", raw, n_blocks, block_bytes, channels, n_frames, 0, 0, true, out, 0, stream);
}

extern "C" int wseg_ima_adpcm_to_planar_f32(const void* raw, int64_t n_blocks, int32_t block_bytes, int32_t channels, int64_t n_frames,
                                            int32_t first_channel, int32_t n_out_channels, float* out, int64_t plane_stride, void* stream) {
  return ima_adpcm_decode("wseg_ima_adpcm_to_planar_f32", raw, n_blocks, block_bytes, channels, n_frames, first_channel, n_out_channels,
                          false, out, plane_stride, stream);
}
