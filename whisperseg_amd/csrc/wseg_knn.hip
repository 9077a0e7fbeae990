// k nearest neighbours of every query row among the corpus rows under the squared Euclidean distance (wseg_knn_f32): the graph that
// clustering, embedding and "calls like this one" start from, over the per-segment patches or any float32 rows.  The m x n matrix of
// distances never exists.  whisperseg_amd/neighbors.py::neighbors_host is the definition (numpy, float64, direct form, total order
// (distance, index)); the host arithmetic — tiles, splits, grids, scratch — is wseg_knn_plan.h.  No inline assembly, no atomics.
//
// knn_norms_kernel    |row|^2 of every query and corpus row as ONE k-ordered fmaf chain over c = 0 .. d - 1 (a lane per row).
// knn_select_kernel   a work item is 128 query rows against one split of the candidate tiles (128 candidates each); the grid strides
//   over the items.  Per candidate tile the 128 x 128 dot products come from v_mfma_f32_32x32x2_f32 — the loop of
//   gemm_f32_mfma_kernel with 4 x 2 waves of 32 query rows x 64 candidates (two accumulators) each: both operands streamed through
//   LDS along d in slabs of 16 (double-buffered, the next slab fetched under the MFMAs, the d tail and rows behind m / n ZERO-FILLED
//   in LDS: no byte outside the two matrices is read).  32 flops per operand byte: the first version, 2 x 2 waves on a 64 x 64 tile
//   at 16 flops per byte, was bound by the L2 at 39 % of the matrix peak.  That
//   instruction is bit for bit a k-ordered fmaf chain and a zero product leaves the chain as it is, so
//       d^(i, j) = fmaf(-2, q_i . x_j, |q_i|^2 + |x_j|^2)
//   has ONE value whatever the tiling, the grid, the split or the run.  Every query row keeps a sorted list of the L = k + 8
//   smallest keys (ordered-uint d^ << 32 | j: one 64-bit compare is the total order (d^, j)) in LDS; after a tile a lane inserts
//   those of its 32 values that beat the row's worst entry — rare after the first tiles.  The four lanes that hold values of one
//   row go one after the other (wave column 0 then 1 between barriers, lane half 0 then 1 inside a wave); keys are distinct and
//   the order is total, so the list does not depend on who came first.  Each (row, split) writes its list to scratch.
//   LDS: 2 x 2 x 16 x 132 floats of slabs (33.0 KiB) + 128 norms + the lists: 128 x 24 keys (24.0 KiB; k <= 16) = 57.5 KiB, two
//   workgroups a CU at 128 registers (four waves a SIMD: the launch bounds) — or 128 x 72 keys (72.0 KiB) = 105.5 KiB, one workgroup a CU.
// knn_finish_kernel   a wave per query row: merges the splits' lists into the L smallest keys (L rounds of "smallest key above the
//   last one", a wave minimum each), recomputes the DIRECT form sum (q - x)^2 of those candidates with fp64 accumulation (lanes
//   stride over c, one fixed xor tree), orders them by (float32 of that sum, j) — the value it reports, so that equal reported
//   distances have ascending indices — and writes the first k; -1 / +inf where candidates ran out.  The cancellation error of
//   d^ therefore only matters at the boundary of the k + 8 kept candidates and never shows in a distance.
#include "wseg_common.h"
#include "wseg_knn_plan.h"

namespace wseg {

constexpr unsigned long long kKnnNone = ~0ull;       // the key of "no candidate": behind every real key
constexpr int kKnnSelectLanes = 512;                 // knn_select_kernel: 4 x 2 waves, a wave owns 32 query rows x 64 candidates of a tile

struct KnnArgs {
  const float* q;                  // [m][d]
  const float* x;                  // [n][d]
  long long m, n;
  int d, k, L;
  int exclude;                     // 1: candidate j == query row i is none
  int splits, tiles_per_split;
  long long n_tiles, items;
  float* qnorm;                    // [m]
  float* xnorm;                    // [n]
  unsigned long long* keys;        // [m_tiles * 128][splits][L]
  int* index_out;                  // [m][k]
  float* distance_out;             // [m][k]
};

__device__ __forceinline__ unsigned knn_f2ord(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// |row|^2 of rows [0, m) of q then [0, n) of x: acc = fmaf(v, v, acc) over c ascending — the chain the MFMA runs on a product
template <bool VEC>
__global__ __launch_bounds__(256) void knn_norms_kernel(KnnArgs a) {
  const long long rows = a.m + a.n;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long long)gridDim.x * 256) {
    const bool isq = r < a.m;
    const float* __restrict__ p = isq ? a.q + r * a.d : a.x + (r - a.m) * a.d;
    float acc = 0.0f;
    if constexpr (VEC) {
      for (int c = 0; c < a.d; c += 4) {
        const float4 v = *(const float4*)(p + c);
        acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
      }
    } else {
      for (int c = 0; c < a.d; ++c) acc = fmaf(p[c], p[c], acc);
    }
    if (isq) a.qnorm[r] = acc; else a.xnorm[r - a.m] = acc;
  }
}

// the row's sorted list (ascending, L entries) takes `key` if it beats the worst entry; volatile: other lanes of the workgroup
// wrote the list a moment ago
__device__ __forceinline__ void knn_insert(volatile unsigned long long* row, int L, unsigned long long key) {
  if (key >= row[L - 1]) return;
  int p = L - 1;
  while (p > 0) {
    const unsigned long long prev = row[p - 1];
    if (prev <= key) break;
    row[p] = prev;
    --p;
  }
  row[p] = key;
}

template <bool VEC, int LMAX>
__global__ __launch_bounds__(kKnnSelectLanes, LMAX <= kKnnSmallL ? 4 : 2) void knn_select_kernel(KnnArgs a) {
  constexpr int BK = 16, LD = kKnnTile + 4, TJ = 2;
  __shared__ float sQ[2][BK][LD];
  __shared__ float sX[2][BK][LD];
  __shared__ float sxn[kKnnTile];
  __shared__ unsigned long long lists[kKnnTile * LMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int fi = lane & 31, fk = lane >> 5;
  const int lr = tid >> 2, lq = (tid & 3) * 4;           // global loads: row lr of both operands, k offset lq, 4 floats
  const int D = a.d, L = a.L, nk = (D + BK - 1) / BK;
  const int lrow = wm * 32 + fi;                         // the query row of this lane's 32 values, inside the tile
  volatile unsigned long long* const mylist = lists + lrow * L;
  auto load4 = [&](const float* __restrict__ p, int kb) {      // p: the row, null behind the last one
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p && kb < D) {
      if constexpr (VEC) {
        v = *(const float4*)(p + kb);                    // d % 4 == 0: the four are inside the row
      } else {
        v.x = p[kb];
        if (kb + 1 < D) v.y = p[kb + 1];
        if (kb + 2 < D) v.z = p[kb + 2];
        if (kb + 3 < D) v.w = p[kb + 3];
      }
    }
    return v;
  };
  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const long long qt = item / a.splits;
    const int split = (int)(item - qt * a.splits);
    const long long m0 = qt * kKnnTile;
    for (int idx = tid; idx < kKnnTile * L; idx += kKnnSelectLanes) lists[idx] = kKnnNone;
    const bool qok = m0 + lrow < a.m;
    const float qn = qok ? a.qnorm[m0 + lrow] : 0.0f;
    const float* __restrict__ const qp = m0 + lr < a.m ? a.q + (m0 + lr) * D : nullptr;
    const long long t0 = (long long)split * a.tiles_per_split;
    const long long t1 = t0 + a.tiles_per_split < a.n_tiles ? t0 + a.tiles_per_split : a.n_tiles;
    for (long long t = t0; t < t1; ++t) {
      const long long n0 = t * kKnnTile;
      if (tid < kKnnTile) sxn[tid] = n0 + tid < a.n ? a.xnorm[n0 + tid] : 0.0f;
      const float* __restrict__ const xp = n0 + lr < a.n ? a.x + (n0 + lr) * D : nullptr;
      float4 rq = load4(qp, lq), rx = load4(xp, lq);
      auto stage = [&](int b) {
        sQ[b][lq + 0][lr] = rq.x; sQ[b][lq + 1][lr] = rq.y; sQ[b][lq + 2][lr] = rq.z; sQ[b][lq + 3][lr] = rq.w;
        sX[b][lq + 0][lr] = rx.x; sX[b][lq + 1][lr] = rx.y; sX[b][lq + 2][lr] = rx.z; sX[b][lq + 3][lr] = rx.w;
      };
      f32x16 acc[TJ];
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      stage(0);
      __syncthreads();                                   // (also: the cleared lists, the tile's norms)
      for (int kt = 0; kt < nk; ++kt) {
        const int b = kt & 1;
        if (kt + 1 < nk) { rq = load4(qp, (kt + 1) * BK + lq); rx = load4(xp, (kt + 1) * BK + lq); }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {             // lanes 0-31 carry k = kk, lanes 32-63 k = kk + 1: ascending k
          const float qf = sQ[b][kk + fk][lrow];
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(sX[b][kk + fk][wn * 64 + j * 32 + fi], qf, acc[j], 0, 0, 0);
        }
        if (kt + 1 < nk) stage(b ^ 1);
        __syncthreads();
      }
      // Register r of acc[j]: query row lrow, candidate c = wn * 64 + 32 j + 8 (r >> 2) + 4 fk + (r & 3) of the tile.  Value number
      // v = 16 j + r of the lane; `pass` marks those that may beat the row's worst entry (a float compare: a superset — the lists
      // only ever tighten, the insertion compares the keys).  The insertion loop exists once: it picks the marked values one by one.
      auto key_of = [&](int c, float dot) {
        const float dh = fmaf(-2.0f, dot, qn + sxn[c]) + 0.0f;         // (+ 0: no negative zero among the keys)
        return ((unsigned long long)knn_f2ord(dh) << 32) | (unsigned)(n0 + c);
      };
      const int nvalid = a.n - n0 < kKnnTile ? (int)(a.n - n0) : kKnnTile;
      const long long self = m0 + lrow - n0;             // the row's own column in this tile, where it has one
      const int selfc = a.exclude && self >= 0 && self < kKnnTile ? (int)self : -1;
      // the worst entry's d^ (+inf while the list is not full)
      const unsigned wo = (unsigned)(mylist[L - 1] >> 32);
      const float wf = wo == 0xffffffffu ? __uint_as_float(0x7f800000u) : __uint_as_float((wo & 0x80000000u) ? (wo & 0x7fffffffu) : ~wo);
      unsigned pass = 0;
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = wn * 64 + 32 * j + 8 * (r >> 2) + 4 * fk + (r & 3);
          const float dh = fmaf(-2.0f, acc[j][r], qn + sxn[c]);
          const bool ok = (int)qok & (int)(c < nvalid) & (int)(c != selfc) & (int)(dh <= wf);
          pass |= ok ? 1u << (16 * j + r) : 0u;
        }
#pragma unroll 1
      for (int phase = 0; phase < 2; ++phase) {          // the four lanes of a row, one after the other
        if (wn == phase) {
#pragma unroll 1
          for (int h = 0; h < 2; ++h) {
            if (fk == h) {
              while (pass) {
                const int v = __builtin_ctz(pass);
                pass &= pass - 1;
                float dot = 0.0f;
#pragma unroll
                for (int j = 0; j < TJ; ++j)
#pragma unroll
                  for (int r = 0; r < 16; ++r) dot = v == 16 * j + r ? acc[j][r] : dot;
                const int j = v >> 4, r = v & 15;
                knn_insert(mylist, L, key_of(wn * 64 + 32 * j + 8 * (r >> 2) + 4 * fk + (r & 3), dot));
              }
            }
            __builtin_amdgcn_wave_barrier();
          }
        }
        __syncthreads();
      }
    }
    if (t1 <= t0) __syncthreads();                       // (no tile: the cleared lists are written out)
    for (int idx = tid; idx < kKnnTile * L; idx += kKnnSelectLanes) {
      const int row = idx / L, e = idx - row * L;
      a.keys[((m0 + row) * a.splits + split) * L + e] = lists[idx];
    }
    __syncthreads();                                     // the lists are cleared for the next item
  }
}

__global__ __launch_bounds__(64) void knn_finish_kernel(KnnArgs a, int vec) {
  __shared__ unsigned sj[kKnnMaxL];
  __shared__ unsigned long long sk[kKnnMaxL];
  const int lane = threadIdx.x, L = a.L, D = a.d;
  const long long total = (long long)a.splits * L;
  for (long long row = blockIdx.x; row < a.m; row += gridDim.x) {
    const unsigned long long* __restrict__ keys = a.keys + row * total;
    // the L smallest keys of the splits' lists, ascending; keys are distinct but for "none"
    unsigned long long prev = 0;
    int cnt = 0;
    for (int t = 0; t < L; ++t) {
      unsigned long long best = kKnnNone;
      for (long long i = lane; i < total; i += 64) {
        const unsigned long long v = keys[i];
        if ((t == 0 || v > prev) && v < best) best = v;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o < best ? o : best;
      }
      if (best == kKnnNone) break;
      if (lane == 0) sj[t] = (unsigned)best;
      prev = best;
      ++cnt;
    }
    __syncthreads();
    // the direct form with fp64 accumulation, reported as float32
    const float* __restrict__ q = a.q + row * D;
    for (int t = 0; t < cnt; ++t) {
      const unsigned j = sj[t];
      const float* __restrict__ x = a.x + (long long)j * D;
      double s = 0.0;
      if (vec) {
        for (int c = 4 * lane; c < D; c += 256) {
          const float4 qv = *(const float4*)(q + c), xv = *(const float4*)(x + c);
          const double d0 = (double)qv.x - (double)xv.x, d1 = (double)qv.y - (double)xv.y;
          const double d2 = (double)qv.z - (double)xv.z, d3 = (double)qv.w - (double)xv.w;
          s = fma(d0, d0, s); s = fma(d1, d1, s); s = fma(d2, d2, s); s = fma(d3, d3, s);
        }
      } else {
        for (int c = lane; c < D; c += 64) {
          const double df = (double)q[c] - (double)x[c];
          s = fma(df, df, s);
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (lane == 0) sk[t] = ((unsigned long long)knn_f2ord((float)s) << 32) | j;
    }
    __syncthreads();
    // rank by (float32 distance, j): distinct keys, the ranks are a permutation
    for (int t = lane; t < cnt; t += 64) {
      const unsigned long long mine = sk[t];
      int rank = 0;
      for (int u = 0; u < cnt; ++u) rank += sk[u] < mine ? 1 : 0;
      if (rank < a.k) {
        const unsigned o = (unsigned)(mine >> 32);
        a.index_out[row * a.k + rank] = (int)(unsigned)mine;
        a.distance_out[row * a.k + rank] = __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
      }
    }
    for (int t = cnt + lane; t < a.k; t += 64) {
      a.index_out[row * a.k + t] = -1;
      a.distance_out[row * a.k + t] = __uint_as_float(0x7f800000u);
    }
    __syncthreads();                                     // sj and sk are laid down anew
  }
}

// index = -1, distance = +inf over the m x k outputs: a call without candidates
__global__ __launch_bounds__(256) void knn_fill_kernel(int* __restrict__ index_out, float* __restrict__ distance_out, long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    index_out[i] = -1;
    distance_out[i] = __uint_as_float(0x7f800000u);
  }
}

}  // namespace wseg

using namespace wseg;

extern "C" size_t wseg_knn_scratch_bytes(int64_t m, int64_t n, int32_t d, int32_t k) {
  KnnPlan plan;
  char msg[200];
  if (knn_plan(m, n, d, k, kKnnGridCap, &plan, msg, sizeof(msg))) {
    set_error("wseg_knn_scratch_bytes: %s", msg);
    return 0;
  }
  return (size_t)plan.scratch_bytes;
}

extern "C" int wseg_knn_f32(const float* queries, int64_t m, const float* corpus, int64_t n, int32_t d, int32_t k, int32_t exclude_same_index,
                            void* scratch, size_t scratch_bytes, int32_t* index_out, float* distance_out, void* stream_) {
  const char* fn = "wseg_knn_f32";
  hipStream_t stream = (hipStream_t)stream_;
  KnnPlan plan;
  char msg[200];
  // (the grid cap — and with it the candidate splits — is a test knob)
  if (knn_plan(m, n, d, k, grid_cap_env("WSEG_KNN_GRID", kKnnGridCap, kKnnGridCap), &plan, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (exclude_same_index != 0 && exclude_same_index != 1) { set_error("%s: exclude_same_index must be 0 or 1", fn); return WSEG_ERR_INVALID; }
  if (m == 0) return WSEG_OK;
  if (!queries || ((uintptr_t)queries & 3)) { set_error("%s: queries must be a float32 device pointer", fn); return WSEG_ERR_INVALID; }
  if ((n > 0 && !corpus) || ((uintptr_t)corpus & 3)) { set_error("%s: corpus must be a float32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!index_out || ((uintptr_t)index_out & 3)) { set_error("%s: index_out must be an int32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!distance_out || ((uintptr_t)distance_out & 3)) { set_error("%s: distance_out must be a float32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (n == 0) {
    const long long total = (long long)m * k;
    const long long rounds = (total + 255) / 256;
    hipLaunchKernelGGL(knn_fill_kernel, dim3((unsigned)(rounds < kKnnGridCap ? rounds : kKnnGridCap)), dim3(256), 0, stream, (int*)index_out,
                       distance_out, total);
    WSEG_LAUNCH_CHECK();
    return WSEG_OK;
  }
  if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < (size_t)plan.scratch_bytes) {
    set_error("%s: scratch must be an 8-byte aligned device buffer of at least %lld bytes (got %zu)", fn, (long long)plan.scratch_bytes, scratch_bytes);
    return WSEG_ERR_INVALID;
  }
  KnnArgs a;
  a.q = queries;
  a.x = corpus;
  a.m = m;
  a.n = n;
  a.d = d;
  a.k = k;
  a.L = plan.L;
  a.exclude = exclude_same_index;
  a.splits = plan.splits;
  a.tiles_per_split = plan.tiles_per_split;
  a.n_tiles = plan.n_tiles;
  a.items = plan.items;
  a.qnorm = reinterpret_cast<float*>(static_cast<char*>(scratch) + plan.qnorm_offset);
  a.xnorm = reinterpret_cast<float*>(static_cast<char*>(scratch) + plan.xnorm_offset);
  a.keys = reinterpret_cast<unsigned long long*>(static_cast<char*>(scratch) + plan.keys_offset);
  a.index_out = (int*)index_out;
  a.distance_out = distance_out;
  // 16-byte loads where every row starts on 16 bytes
  const bool vec = d % 4 == 0 && !((uintptr_t)queries & 15) && !((uintptr_t)corpus & 15);
  if (vec) hipLaunchKernelGGL(knn_norms_kernel<true>, dim3((unsigned)plan.norm_grid), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(knn_norms_kernel<false>, dim3((unsigned)plan.norm_grid), dim3(256), 0, stream, a);
  WSEG_LAUNCH_CHECK();
  // lists of up to kKnnSmallL entries leave room for two workgroups a CU
  const dim3 grid((unsigned)plan.grid), block(kKnnSelectLanes);
  if (plan.L <= kKnnSmallL) {
    if (vec) hipLaunchKernelGGL((knn_select_kernel<true, kKnnSmallL>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((knn_select_kernel<false, kKnnSmallL>), grid, block, 0, stream, a);
  } else {
    if (vec) hipLaunchKernelGGL((knn_select_kernel<true, kKnnMaxL>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((knn_select_kernel<false, kKnnMaxL>), grid, block, 0, stream, a);
  }
  WSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_finish_kernel, dim3((unsigned)plan.finish_grid), dim3(64), 0, stream, a, vec ? 1 : 0);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}
