// Principal components of float32 rows (wseg_pca_moments_f64 / wseg_pca_project_f64): the two O(N D^2) / O(N D r) steps of
// whisperseg_amd/pca.py on the fp64 matrix cores (v_mfma_f64_16x16x4_f64); the covariance, the eigen-decomposition and the
// conventions are host work there.  pca.py::moments_host / project_host are the definitions (numpy, float64).  A float32 value
// converts to float64 exactly and the product of two such values is exact in float64, so every rounding here is one of an addition:
// on inputs whose partial sums are exact the results are the definition's bits, elsewhere they stay inside the bounds
// tests/pca_cases.py derives.  No N x D float64 copy exists.  The host arithmetic — validation, tiles, splits, grids, the scratch —
// is wseg_pca_plan.h.  No inline assembly, no atomics; the build has -ffp-contract=off.
//
// The instruction: D[16][16] += A[16][4] B[4][16] in float64; lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15],
// one double each, and holds four results: D[row = (l >> 4) + 4 * reg][col = l & 15], reg 0 .. 3 (NOT the f32 map).
//
// pca_moments_kernel   a workgroup of 4 waves per work item (split, tile): the 64 x 64 tile (bi, bj), bi <= bj, of S = X^T X over the
//   rows of the split.  The reduction runs over rows, four a k-step: with A[i][k] = x[n0 + k][64 bi + i] and B[k][j] =
//   x[n0 + k][64 bj + j] both operands are the same access — 16 consecutive floats per quarter-wave — so an LDS image of a 32-row
//   chunk in its natural layout (rows 80 floats apart: the four quarter-waves hit four bank groups) serves both without a transpose.
//   Wave w owns the 16-row strip w of the tile: one converted A fragment against four B fragments, 16 accumulator values a lane.
//   On a diagonal tile a fifth product against a B of ones leaves the column sums of the strip in every column of its result.  The
//   next chunk is fetched into registers while the current one is multiplied.  Rows beyond the split and columns beyond d are zeros
//   in the image and contribute exact zeros.  With one split the tile is written to S — element (i, j), i <= j, and its mirror from
//   the same register — with more, to the scratch.
// pca_finish_kernel    adds the partial tiles and partial sums of the splits in ascending split order and writes S, both triangles
//   from one value, and the sums.
// pca_project_kernel<NT>   Z = (X - mean) V for r <= 64 columns: a workgroup per 64 rows, wave w its rows 16 w .. 16 w + 15, NT =
//   ceil(r / 16) 16-column tiles.  A[i][k] = x[n0 + i][c0 + k] - mean[c0 + k] is strided by d across lanes, so a chunk of 32 columns
//   goes through LDS (rows 36 floats apart), with that chunk of the basis and of the mean (zeros beyond d and r) beside it; the next
//   chunk of all three is fetched into registers while the current one is multiplied.
#include "wseg_common.h"
#include "wseg_pca_plan.h"

namespace wseg {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int kPcaLanes = 256;                 // 4 waves
constexpr int kPcaImgStride = 80;              // floats between the rows of the moments image
constexpr int kPcaXStride = 36;                // floats between the rows of the projection's image
constexpr int kPcaTileElems = kPcaBlock * kPcaBlock;

struct PcaMomentsArgs {
  const float* rows;               // [n][d]
  long long n, rows_per_split, items;
  int d, nb, tiles, splits;
  double* sum;                     // [d]
  double* gram;                    // [d][d]
  double* partial;                 // [items][64][64]   (splits > 1)
  double* sums;                    // [splits][nb][64]  (splits > 1)
};

__device__ __forceinline__ f64x4 pca_mfma(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(kPcaLanes) void pca_moments_kernel(PcaMomentsArgs p) {
  __shared__ float img[2][kPcaChunk * kPcaImgStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = lane & 15, q = lane >> 4;
  const int load_col = threadIdx.x & 63, load_row = threadIdx.x >> 6;
  for (long long item = blockIdx.x; item < p.items; item += gridDim.x) {
    const int split = (int)(item / p.tiles), tile = (int)(item - (long long)split * p.tiles);
    int bi, bj;
    pca_tile_blocks(p.nb, tile, &bi, &bj);
    long long r0, r1;
    pca_split_rows(p.n, p.rows_per_split, split, &r0, &r1);
    const bool diag = bi == bj;
    const int ca = bi * kPcaBlock + load_col, cb = bj * kPcaBlock + load_col;
    float ra[8], rb[8];
    auto fetch = [&](long long base) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const long long row = base + load_row + 4 * i;
        const bool in = row < r1;
        ra[i] = in && ca < p.d ? p.rows[row * p.d + ca] : 0.0f;
        rb[i] = diag ? ra[i] : (in && cb < p.d ? p.rows[row * p.d + cb] : 0.0f);
      }
    };
    f64x4 acc[4], ones;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    ones = f64x4{0.0, 0.0, 0.0, 0.0};
    fetch(r0);
    for (long long base = r0; base < r1; base += kPcaChunk) {
      __syncthreads();                                   // the chunk before this one has been read
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        img[0][(load_row + 4 * i) * kPcaImgStride + load_col] = ra[i];
        img[1][(load_row + 4 * i) * kPcaImgStride + load_col] = rb[i];
      }
      __syncthreads();
      if (base + kPcaChunk < r1) fetch(base + kPcaChunk);
#pragma unroll
      for (int kk = 0; kk < kPcaChunk / 4; ++kk) {
        const int at = (kk * 4 + q) * kPcaImgStride + lo;
        const double a = (double)img[0][at + wave * 16];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = pca_mfma(a, (double)img[1][at + t * 16], acc[t]);
        if (diag) ones = pca_mfma(a, 1.0, ones);
      }
    }
    const int strip = wave * 16 + q;                     // + 4 * reg: the row of a result inside the tile
    if (p.splits == 1) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int gi = bi * kPcaBlock + strip + 4 * reg, gj = bj * kPcaBlock + t * 16 + lo;
          if (gi < p.d && gj < p.d && (!diag || gi <= gj)) {
            p.gram[(long long)gi * p.d + gj] = acc[t][reg];
            p.gram[(long long)gj * p.d + gi] = acc[t][reg];
          }
        }
      }
      if (diag && lo == 0) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int c = bi * kPcaBlock + strip + 4 * reg;
          if (c < p.d) p.sum[c] = ones[reg];
        }
      }
    } else {
      double* out = p.partial + item * kPcaTileElems;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) out[(strip + 4 * reg) * kPcaBlock + t * 16 + lo] = acc[t][reg];
      }
      if (diag && lo == 0) {
        double* s = p.sums + ((long long)split * p.nb + bi) * kPcaBlock;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) s[strip + 4 * reg] = ones[reg];
      }
    }
  }
}

__global__ __launch_bounds__(kPcaLanes) void pca_finish_kernel(PcaMomentsArgs p) {
  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    int bi, bj;
    pca_tile_blocks(p.nb, tile, &bi, &bj);
    const bool diag = bi == bj;
    for (int e = threadIdx.x; e < kPcaTileElems; e += kPcaLanes) {
      const int i = e >> 6, j = e & 63;
      const int gi = bi * kPcaBlock + i, gj = bj * kPcaBlock + j;
      if (gi >= p.d || gj >= p.d || (diag && i > j)) continue;
      const double* from = p.partial + (long long)tile * kPcaTileElems + e;
      double v = from[0];
      for (int s = 1; s < p.splits; ++s) v += from[(long long)s * p.tiles * kPcaTileElems];
      p.gram[(long long)gi * p.d + gj] = v;
      p.gram[(long long)gj * p.d + gi] = v;
    }
    if (diag && threadIdx.x < kPcaBlock) {
      const int c = bi * kPcaBlock + threadIdx.x;
      if (c < p.d) {
        const double* from = p.sums + (long long)bi * kPcaBlock + threadIdx.x;
        double v = from[0];
        for (int s = 1; s < p.splits; ++s) v += from[(long long)s * p.nb * kPcaBlock];
        p.sum[c] = v;
      }
    }
  }
}

struct PcaProjectArgs {
  const float* rows;               // [n][d]
  long long n, row_tiles;
  int d, r;
  const double* mean;              // [d]
  const double* basis;             // [d][r]
  double* out;                     // [n][r]
};

template <int NT>
__global__ __launch_bounds__(kPcaLanes, 2) void pca_project_kernel(PcaProjectArgs p) {
  constexpr int kWidth = 16 * NT;                                  // columns of the basis image
  constexpr int kPer = kPcaColChunk * kWidth / kPcaLanes;          // doubles of it a lane fetches
  __shared__ float xs[kPcaRowTile * kPcaXStride];
  __shared__ double bs[kPcaColChunk * kWidth];
  __shared__ double ms[kPcaColChunk];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = lane & 15, q = lane >> 4;
  const int load_col = threadIdx.x & 31, load_row = threadIdx.x >> 5;
  for (long long tile = blockIdx.x; tile < p.row_tiles; tile += gridDim.x) {
    const long long n0 = tile * kPcaRowTile;
    float rx[8];
    double rb[kPer], rm;
    auto fetch = [&](int c0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const long long n = n0 + load_row + 8 * i;
        rx[i] = n < p.n && c0 + load_col < p.d ? p.rows[n * p.d + c0 + load_col] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int e = (int)threadIdx.x + kPcaLanes * i, k = e / kWidth, j = e % kWidth;
        rb[i] = c0 + k < p.d && j < p.r ? p.basis[(long long)(c0 + k) * p.r + j] : 0.0;
      }
      rm = threadIdx.x < kPcaColChunk && c0 + (int)threadIdx.x < p.d ? p.mean[c0 + threadIdx.x] : 0.0;
    };
    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    for (int c0 = 0; c0 < p.d; c0 += kPcaColChunk) {
      __syncthreads();                                   // the chunk before this one has been read
#pragma unroll
      for (int i = 0; i < 8; ++i) xs[(load_row + 8 * i) * kPcaXStride + load_col] = rx[i];
#pragma unroll
      for (int i = 0; i < kPer; ++i) bs[threadIdx.x + kPcaLanes * i] = rb[i];
      if (threadIdx.x < kPcaColChunk) ms[threadIdx.x] = rm;
      __syncthreads();
      if (c0 + kPcaColChunk < p.d) fetch(c0 + kPcaColChunk);
#pragma unroll
      for (int kk = 0; kk < kPcaColChunk / 4; ++kk) {
        const int k = kk * 4 + q;
        const double a = (double)xs[(wave * 16 + lo) * kPcaXStride + k] - ms[k];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = pca_mfma(a, bs[k * kWidth + t * 16 + lo], acc[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const long long n = n0 + wave * 16 + q + 4 * reg;
        const int j = t * 16 + lo;
        if (n < p.n && j < p.r) p.out[n * p.r + j] = acc[t][reg];
      }
    }
  }
}

static bool pca_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace wseg

using namespace wseg;

extern "C" size_t wseg_pca_scratch_bytes(int64_t n, int32_t d) {
  PcaPlan plan;
  char msg[200];
  if (pca_plan(n, d, kPcaGridCap, &plan, msg, sizeof(msg))) {
    set_error("wseg_pca_scratch_bytes: %s", msg);
    return 0;
  }
  return (size_t)plan.scratch_bytes;
}

extern "C" int wseg_pca_moments_f64(const float* rows, int64_t n, int32_t d, double* sum, double* gram, void* scratch, size_t scratch_bytes,
                                    void* stream_) {
  const char* fn = "wseg_pca_moments_f64";
  hipStream_t stream = (hipStream_t)stream_;
  PcaPlan plan;
  char msg[200];
  if (pca_plan(n, d, grid_cap_env("WSEG_PCA_GRID", kPcaGridCap, kPcaGridCap), &plan, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (!rows || ((uintptr_t)rows & 3)) { set_error("%s: rows must be a float32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!sum || ((uintptr_t)sum & 7)) { set_error("%s: sum must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!gram || ((uintptr_t)gram & 7)) { set_error("%s: gram must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < (size_t)plan.scratch_bytes) {
    set_error("%s: scratch must be an 8-byte aligned device buffer of at least %lld bytes (got %zu)", fn, (long long)plan.scratch_bytes, scratch_bytes);
    return WSEG_ERR_INVALID;
  }
  const size_t rows_bytes = (size_t)n * (size_t)d * 4, sum_bytes = (size_t)d * 8, gram_bytes = (size_t)d * (size_t)d * 8;
  const size_t used = (size_t)plan.scratch_bytes;
  if (pca_overlap(rows, rows_bytes, sum, sum_bytes) || pca_overlap(rows, rows_bytes, gram, gram_bytes) || pca_overlap(rows, rows_bytes, scratch, used) ||
      pca_overlap(sum, sum_bytes, gram, gram_bytes) || pca_overlap(sum, sum_bytes, scratch, used) || pca_overlap(gram, gram_bytes, scratch, used)) {
    set_error("%s: rows, sum, gram and scratch must not overlap", fn);
    return WSEG_ERR_INVALID;
  }
  PcaMomentsArgs args;
  args.rows = rows;
  args.n = n;
  args.rows_per_split = plan.rows_per_split;
  args.items = plan.items;
  args.d = d;
  args.nb = plan.nb;
  args.tiles = plan.tiles;
  args.splits = plan.splits;
  args.sum = sum;
  args.gram = gram;
  args.partial = reinterpret_cast<double*>(static_cast<char*>(scratch) + plan.partial_offset);
  args.sums = reinterpret_cast<double*>(static_cast<char*>(scratch) + plan.sums_offset);
  hipLaunchKernelGGL(pca_moments_kernel, dim3((unsigned)plan.grid), dim3(kPcaLanes), 0, stream, args);
  WSEG_LAUNCH_CHECK();
  if (plan.splits > 1) {
    hipLaunchKernelGGL(pca_finish_kernel, dim3((unsigned)plan.finish_grid), dim3(kPcaLanes), 0, stream, args);
    WSEG_LAUNCH_CHECK();
  }
  return WSEG_OK;
}

extern "C" int wseg_pca_project_f64(const float* rows, int64_t n, int32_t d, const double* mean, const double* basis, int32_t r, double* out,
                                    void* stream_) {
  const char* fn = "wseg_pca_project_f64";
  hipStream_t stream = (hipStream_t)stream_;
  PcaPlan plan;
  char msg[200];
  if (pca_project_plan(n, d, r, grid_cap_env("WSEG_PCA_GRID", kPcaGridCap, kPcaGridCap), &plan, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (!rows || ((uintptr_t)rows & 3)) { set_error("%s: rows must be a float32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!mean || ((uintptr_t)mean & 7)) { set_error("%s: mean must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!basis || ((uintptr_t)basis & 7)) { set_error("%s: basis must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!out || ((uintptr_t)out & 7)) { set_error("%s: out must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  const size_t out_bytes = (size_t)n * (size_t)r * 8;
  if (pca_overlap(out, out_bytes, rows, (size_t)n * (size_t)d * 4) || pca_overlap(out, out_bytes, mean, (size_t)d * 8) ||
      pca_overlap(out, out_bytes, basis, (size_t)d * (size_t)r * 8)) {
    set_error("%s: out must not overlap rows, mean or basis", fn);
    return WSEG_ERR_INVALID;
  }
  PcaProjectArgs args;
  args.rows = rows;
  args.n = n;
  args.row_tiles = plan.row_tiles;
  args.d = d;
  args.r = r;
  args.mean = mean;
  args.basis = basis;
  args.out = out;
  const dim3 grid((unsigned)plan.project_grid), lanes(kPcaLanes);
  switch ((r + 15) / 16) {                               // the 16-column tiles of the result
    case 1: hipLaunchKernelGGL(pca_project_kernel<1>, grid, lanes, 0, stream, args); break;
    case 2: hipLaunchKernelGGL(pca_project_kernel<2>, grid, lanes, 0, stream, args); break;
    case 3: hipLaunchKernelGGL(pca_project_kernel<3>, grid, lanes, 0, stream, args); break;
    default: hipLaunchKernelGGL(pca_project_kernel<4>, grid, lanes, 0, stream, args); break;
  }
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}
