// The distance-tile selection, written once for its consumers (wseg_knn.hip, wseg_mst.hip, wseg_dtw.hip): "for every query row the L
// candidates that come first under (value, index), out of an m x n matrix of values that never exists".  The host arithmetic —
// tiles, splits, grids, scratch — is wseg_select_plan.h.  No inline assembly, no atomics.  kNN runs all of it; MST and DTW share the
// keys, the lists' insertion, the norms and fill kernels, the finish's pieces and the entry points' checks, and keep select kernels
// with a tile loop of their own (they say why).  The stages, in the order of a call:
//
// select_norms_kernel   |row|^2 as ONE c-ordered fmaf chain (a lane per row): the chain the MFMA runs on a product.
// sel_tile_product      the 128 x 128 dot products of a query tile and a candidate tile from v_mfma_f32_32x32x2_f32: 4 x 2 waves of 32
//   query rows x 64 candidates (two accumulators) each, both operands streamed through LDS along c in slabs of 16 (double-buffered,
//   the next slab fetched under the MFMAs; what lies behind the operands ZERO-FILLED in LDS by the caller's loader: no byte outside
//   the two matrices is read).  32 flops per operand byte: the first version, 2 x 2 waves on a 64 x 64 tile at 16 flops per byte,
//   was bound by the L2 at 39 % of the matrix peak.  That instruction is bit for bit a c-ordered fmaf chain and a zero product
//   leaves the chain as it is, so a value such as
//       d^(i, j) = fmaf(-2, q_i . x_j, |q_i|^2 + |x_j|^2)
//   has ONE value whatever the tiling, the grid, the split or the run.
// sel_key / sel_insert  a candidate is the key (ordered-uint value << 32) | j: one 64-bit compare is the total order (value, j).
//   Every query row keeps a sorted list of its L smallest keys in LDS.  Keys are distinct and the order is total, so a list does
//   not depend on who came first.  Each (row, split) writes its list to scratch (sel_write_lists).
// select_kernel         the tile loop over those pieces: after a tile a lane marks those of its 32 values that beat the
//   row's worst entry — rare after the first tiles — and the four lanes that hold values of one row insert them one after the other
//   (sel_insert_marked).  What a value is, what a tile stages next to its norms and which candidates are masked is the caller's
//   Score, a compile-time policy.
// The finish, a wave per query row: sel_merge_split_lists merges the splits' lists into the L smallest keys, the caller recomputes
//   those candidates exactly (sel_direct_sq_f64: the DIRECT form sum (q - x)^2 with fp64 accumulation) and sel_rank_and_write
//   orders them by (float32 of that, j) — the value it reports, so that equal reported values have ascending indices — and writes
//   the first k; -1 / +inf where candidates ran out (select_fill_kernel: a call without candidates).  The cancellation error of a
//   selection value therefore only matters at the boundary of the L kept candidates and never shows in a reported value.
//
// A NEW CONSUMER supplies: a host plan over wseg_select_plan.h; a Score for select_kernel (or, where a tile's values need work of
// their own as DTW's do, a kernel of its own over sel_tile_product with its operand loader); the exact value of its finish.
#pragma once
#include "wseg_common.h"
#include "wseg_select_plan.h"

namespace wseg {

constexpr unsigned long long kSelNone = ~0ull;       // the key of "no candidate": behind every real key
constexpr int kSelLanes = 512;                       // a select kernel: 4 x 2 waves, a wave owns 32 query rows x 64 candidates of a tile
constexpr int kSelBK = 16;                           // columns of a slab
constexpr int kSelLD = kSelTile + 4;                 // floats between two columns of a slab in LDS
typedef float SelSlabs[kSelBK][kSelLD];              // one slab of one operand; an operand has two

__device__ __forceinline__ float sel_inf() { return __uint_as_float(0x7f800000u); }

// (+ 0: no negative zero among the keys)
__device__ __forceinline__ unsigned long long sel_key(float value, unsigned j) { return ((unsigned long long)f2ord(value + 0.0f) << 32) | j; }
__device__ __forceinline__ float sel_key_value(unsigned long long key) { return ord2f((unsigned)(key >> 32)); }

// the row's sorted list (ascending, L entries) takes `key` if it beats the worst entry; volatile: other lanes of the workgroup
// wrote the list a moment ago
__device__ __forceinline__ void sel_insert(volatile unsigned long long* row, int L, unsigned long long key) {
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

// Register r of accumulator j of a lane of wave column wn, lane half fk: the candidate of the tile it holds (its query row is
// 32 * (wave row) + (lane & 31))
__device__ __forceinline__ int sel_candidate(int wn, int fk, int j, int r) { return wn * 64 + 32 * j + 8 * (r >> 2) + 4 * fk + (r & 3); }

// |row|^2 of rows [0, m) of q then [0, n) of x: acc = fmaf(v, v, acc) over c ascending
template <bool VEC>
__global__ __launch_bounds__(256) void select_norms_kernel(const float* q, long long m, const float* x, long long n, int d, float* qnorm,
                                                           float* xnorm) {
  const long long rows = m + n;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long long)gridDim.x * 256) {
    const bool isq = r < m;
    const float* __restrict__ p = isq ? q + r * d : x + (r - m) * d;
    float acc = 0.0f;
    if constexpr (VEC) {
      for (int c = 0; c < d; c += 4) {
        const float4 v = *(const float4*)(p + c);
        acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
      }
    } else {
      for (int c = 0; c < d; ++c) acc = fmaf(p[c], p[c], acc);
    }
    if (isq) qnorm[r] = acc; else xnorm[r - m] = acc;
  }
}

// The operand loader of row-major operands [rows][D]: a lane fetches 4 floats of row tid >> 2 of either operand, at column offset
// 4 (tid & 3) of a slab.  VEC: 16-byte loads (D % 4 == 0, rows on 16 bytes); otherwise scalar loads with the D tail.
template <bool VEC>
struct SelRowLoader {
  const float* __restrict__ qp;    // the lane's row of either operand, null behind the last one
  const float* __restrict__ xp;
  int D;
  float4 rq, rx;
  __device__ __forceinline__ float4 load4(const float* __restrict__ p, int kb) const {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p && kb < D) {
      if constexpr (VEC) {
        v = *(const float4*)(p + kb);                    // D % 4 == 0: the four are inside the row
      } else {
        v.x = p[kb];
        if (kb + 1 < D) v.y = p[kb + 1];
        if (kb + 2 < D) v.z = p[kb + 2];
        if (kb + 3 < D) v.w = p[kb + 3];
      }
    }
    return v;
  }
  __device__ __forceinline__ void load(int kt) {
    const int kb = kt * kSelBK + (threadIdx.x & 3) * 4;
    rq = load4(qp, kb);
    rx = load4(xp, kb);
  }
  __device__ __forceinline__ void stage(SelSlabs& sq, SelSlabs& sx) const {
    const int lr = threadIdx.x >> 2, lq = (threadIdx.x & 3) * 4;
    sq[lq + 0][lr] = rq.x; sq[lq + 1][lr] = rq.y; sq[lq + 2][lr] = rq.z; sq[lq + 3][lr] = rq.w;
    sx[lq + 0][lr] = rx.x; sx[lq + 1][lr] = rx.y; sx[lq + 2][lr] = rx.z; sx[lq + 3][lr] = rx.w;
  }
};

// acc[j][r] = q_lrow . x_c, c = sel_candidate(wn, fk, j, r), over nk slabs: `loader.load(kt)` fetches the lane's part of slab kt of
// both operands into registers, `loader.stage(sq, sx)` stores it.  Every lane of the workgroup calls it; it begins by staging
// slab 0 and ends behind a barrier, the slabs read for the last time.  (The first barrier also publishes what the caller wrote to
// LDS before the call: cleared lists, a tile's norms.)
template <typename Loader>
__device__ __forceinline__ void sel_tile_product(Loader& loader, SelSlabs* sQ, SelSlabs* sX, int nk, f32x16 (&acc)[2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const int fi = lane & 31, fk = lane >> 5, lrow = wm * 32 + fi;
  loader.load(0);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  loader.stage(sQ[0], sX[0]);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int b = kt & 1;
    if (kt + 1 < nk) loader.load(kt + 1);
#pragma unroll
    for (int kk = 0; kk < kSelBK; kk += 2) {             // lanes 0-31 carry c = kk, lanes 32-63 c = kk + 1: ascending c
      const float qf = sQ[b][kk + fk][lrow];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(sX[b][kk + fk][wn * 64 + j * 32 + fi], qf, acc[j], 0, 0, 0);
    }
    if (kt + 1 < nk) loader.stage(sQ[b ^ 1], sX[b ^ 1]);
    __syncthreads();
  }
}

// The four lanes that hold values of one query row insert their marked values one after the other: wave column 0 then 1 between
// barriers, lane half 0 then 1 inside a wave.  Bit v = 16 j + r of `pass` marks value acc[j][r]; `key_of(c, dot)` is its key.  The
// insertion loop exists once: it picks the marked values one by one.  Every lane of the workgroup calls it.
template <typename KeyOf>
__device__ __forceinline__ void sel_insert_marked(unsigned pass, const f32x16 (&acc)[2], volatile unsigned long long* mylist, int L, KeyOf key_of) {
  const int wn = (threadIdx.x >> 6) & 1, fk = (threadIdx.x & 63) >> 5;
#pragma unroll 1
  for (int phase = 0; phase < 2; ++phase) {
    if (wn == phase) {
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        if (fk == h) {
          while (pass) {
            const int v = __builtin_ctz(pass);
            pass &= pass - 1;
            float dot = 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int r = 0; r < 16; ++r) dot = v == 16 * j + r ? acc[j][r] : dot;
            sel_insert(mylist, L, key_of(sel_candidate(wn, fk, v >> 4, v & 15), dot));
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    __syncthreads();
  }
}

// the lists of a work item, `rows` x L keys in LDS: cleared at its start, written to scratch [first_row + row][split][L] at its end
__device__ __forceinline__ void sel_clear_lists(unsigned long long* lists, int rows, int L) {
  for (int idx = threadIdx.x; idx < rows * L; idx += kSelLanes) lists[idx] = kSelNone;
}
__device__ __forceinline__ void sel_write_lists(const unsigned long long* lists, int rows, int L, unsigned long long* keys, long long first_row,
                                                int splits, int split) {
  for (int idx = threadIdx.x; idx < rows * L; idx += kSelLanes) {
    const int row = idx / L, e = idx - row * L;
    keys[((first_row + row) * splits + split) * L + e] = lists[idx];
  }
}

struct SelectArgs {
  const float* q;                  // [m][d]
  const float* x;                  // [n][d]
  long long m, n;
  int d, L;
  int splits, tiles_per_split;
  long long n_tiles, items;
  const float* qnorm;              // [m]
  const float* xnorm;              // [n]
  unsigned long long* keys;        // [m_tiles * 128][splits][L]
};

// A work item is 128 query rows against one split of the candidate tiles (128 candidates each); the grid strides over the items.
// Score (passed by value, its members are the caller's extra arguments) states the caller's value:
//   Score::Tile                        what a tile stages in LDS next to its norms, arrays of 128 aligned to 16 bytes
//   Score::Row                         what a lane keeps of its query row
//   stage(args, tile, c, j, in)        lane c of the first 128 fills entry c of the tile from candidate j (in: j < n)
//   row(args, i, ok)                   the query row i of a lane (ok: i < m)
//   enter(row, i, n0)                  ... told that the tile of candidates n0 .. n0 + 127 begins
//   value(row, tile, c, dot)           the value of candidate c of the tile given q_i . x_c
//   masked(row, tile, c)               candidate c of the tile is none for this row, whatever its value
// LDS: 2 x 2 x 16 x 132 floats of slabs (33.0 KiB) + the tile + 128 x LMAX keys.  Up to kSelSmallL entries that leaves room for two
// workgroups a CU at 128 registers (four waves a SIMD: the launch bounds); 72 entries (72.0 KiB) make it one workgroup a CU.
template <bool VEC, int LMAX, typename Score>
__global__ __launch_bounds__(kSelLanes, LMAX <= kSelSmallL ? 4 : 2) void select_kernel(SelectArgs a, Score score) {
  __shared__ SelSlabs sQ[2];
  __shared__ SelSlabs sX[2];
  __shared__ typename Score::Tile tile;
  __shared__ unsigned long long lists[kSelTile * LMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int fi = lane & 31, fk = lane >> 5;
  const int lr = tid >> 2;                               // global loads: row lr of both operands
  const int D = a.d, L = a.L, nk = (D + kSelBK - 1) / kSelBK;
  const int lrow = wm * 32 + fi;                         // the query row of this lane's 32 values, inside the tile
  volatile unsigned long long* const mylist = lists + lrow * L;
  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const long long qt = item / a.splits;
    const int split = (int)(item - qt * a.splits);
    const long long m0 = qt * kSelTile;
    sel_clear_lists(lists, kSelTile, L);
    const bool qok = m0 + lrow < a.m;
    typename Score::Row row = score.row(a, m0 + lrow, qok);
    const float* __restrict__ const qp = m0 + lr < a.m ? a.q + (m0 + lr) * D : nullptr;
    const long long t0 = (long long)split * a.tiles_per_split;
    const long long t1 = t0 + a.tiles_per_split < a.n_tiles ? t0 + a.tiles_per_split : a.n_tiles;
    for (long long t = t0; t < t1; ++t) {
      const long long n0 = t * kSelTile;
      if (tid < kSelTile) score.stage(a, tile, tid, n0 + tid, n0 + tid < a.n);
      SelRowLoader<VEC> loader = {qp, n0 + lr < a.n ? a.x + (n0 + lr) * D : nullptr, D};
      f32x16 acc[2];
      sel_tile_product(loader, sQ, sX, nk, acc);
      // `pass` marks the values that may beat the row's worst entry (a float compare: a superset — the lists only ever tighten,
      // the insertion compares the keys)
      const int nvalid = a.n - n0 < kSelTile ? (int)(a.n - n0) : kSelTile;
      score.enter(row, m0 + lrow, n0);
      // the worst entry's value (+inf while the list is not full)
      const unsigned wo = (unsigned)(mylist[L - 1] >> 32);
      const float wf = wo == 0xffffffffu ? sel_inf() : ord2f(wo);
      // (four neighbouring candidates at a time, one 16-byte LDS read per array of the tile; the scheduling barrier keeps the
      // compiler from fetching all the tile's words ahead, which does not fit 128 registers beside the accumulators)
      unsigned pass = 0;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e, c = sel_candidate(wn, fk, j, r);
            const float w = score.value(row, tile, c, acc[j][r]);
            const bool ok = (int)qok & (int)(c < nvalid) & (int)!score.masked(row, tile, c) & (int)(w <= wf);
            pass |= ok ? 1u << (16 * j + r) : 0u;
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      sel_insert_marked(pass, acc, mylist, L, [&](int c, float dot) { return sel_key(score.value(row, tile, c, dot), (unsigned)(n0 + c)); });
    }
    if (t1 <= t0) __syncthreads();                       // (no tile: the cleared lists are written out)
    sel_write_lists(lists, kSelTile, L, a.keys, m0, a.splits, split);
    __syncthreads();                                     // the lists are cleared for the next item
  }
}

// The L smallest keys of the `total` keys of a row's splits' lists, ascending (L rounds of "smallest key above the last one", a wave
// minimum each; keys are distinct but for "none") -> their count; lane 0 leaves the candidates' indices in sj.  A wave calls it.
__device__ __forceinline__ int sel_merge_split_lists(const unsigned long long* __restrict__ keys, long long total, int L, int lane, unsigned* sj) {
  unsigned long long prev = 0;
  int cnt = 0;
  for (int t = 0; t < L; ++t) {
    unsigned long long best = kSelNone;
    for (long long i = lane; i < total; i += 64) {
      const unsigned long long v = keys[i];
      if ((t == 0 || v > prev) && v < best) best = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off);
      best = o < best ? o : best;
    }
    if (best == kSelNone) break;
    if (lane == 0) sj[t] = (unsigned)best;
    prev = best;
    ++cnt;
  }
  return cnt;
}

// sum_c (q[c] - x[c])^2, the direct form with fp64 accumulation: the lanes of a wave stride over c, one fixed xor tree; every lane
// holds the sum.  vec: 16-byte loads (D % 4 == 0, rows on 16 bytes).
__device__ __forceinline__ double sel_direct_sq_f64(const float* __restrict__ q, const float* __restrict__ x, int D, int vec, int lane) {
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
  return s;
}

// The cnt exact keys sk (float32 value, j) of a row, ranked — distinct keys, the ranks are a permutation —: the first k go to the
// row's outputs, -1 / +inf where candidates ran out.  A wave calls it.
__device__ __forceinline__ void sel_rank_and_write(const unsigned long long* sk, int cnt, int k, int lane, int* __restrict__ index_row,
                                                   float* __restrict__ value_row) {
  for (int t = lane; t < cnt; t += 64) {
    const unsigned long long mine = sk[t];
    int rank = 0;
    for (int u = 0; u < cnt; ++u) rank += sk[u] < mine ? 1 : 0;
    if (rank < k) {
      index_row[rank] = (int)(unsigned)mine;
      value_row[rank] = sel_key_value(mine);
    }
  }
  for (int t = cnt + lane; t < k; t += 64) {
    index_row[t] = -1;
    value_row[t] = sel_inf();
  }
}

// index = -1, value = +inf over the m x k outputs: a call without candidates
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void select_fill_kernel(int* __restrict__ index_out, float* __restrict__ value_out, long long total) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * BLOCK) {
    index_out[i] = -1;
    value_out[i] = sel_inf();
  }
}
inline void sel_launch_fill(int* index_out, float* value_out, long long total, hipStream_t stream) {
  const long long rounds = (total + 255) / 256;
  hipLaunchKernelGGL(select_fill_kernel<256>, dim3((unsigned)(rounds < kSelGridCap ? rounds : kSelGridCap)), dim3(256), 0, stream, index_out,
                     value_out, total);
}

// The entry points' checks of a device pointer to 4-byte elements (what: "a float32" / "an int32"; required: null is an error) and
// of the scratch -> true with the error set
inline bool sel_bad_pointer(const char* fn, const void* p, bool required, const char* name, const char* what) {
  if (!(required && !p) && !((uintptr_t)p & 3)) return false;
  set_error("%s: %s must be %s device pointer", fn, name, what);
  return true;
}
inline bool sel_bad_scratch(const char* fn, const void* scratch, size_t scratch_bytes, int64_t need) {
  if (scratch && !((uintptr_t)scratch & 7) && scratch_bytes >= (size_t)need) return false;
  set_error("%s: scratch must be an 8-byte aligned device buffer of at least %lld bytes (got %zu)", fn, (long long)need, scratch_bytes);
  return true;
}

}  // namespace wseg
