// One Boruvka round of the minimum spanning tree under the mutual-reachability distance (wseg_mst_round_f32): for every row i the
// candidate j of ANOTHER component that comes first in the order (w(i, j), j), w(i, j) = max(core_i, core_j, d(i, j)), d the squared
// Euclidean distance — the N^2 D part of density-based clustering (HDBSCAN, DBSCAN*, robust single linkage) over the per-segment
// patches or any float32 rows.  The n x n matrix never exists.  whisperseg_amd/linkage.py::mst_host is the definition (numpy,
// float64 direct form, strict total order (w, a, b)); linkage.py::mst drives the rounds and keeps the O(n) component bookkeeping on
// the host; the host arithmetic — tiles, splits, grids, scratch — is wseg_mst_plan.h.  No inline assembly, no atomics.
//
// The keys, the sorted lists, the norms kernel, the finish's merge and fp64 direct form and the entry points' checks are
// wseg_select.h's.  mst_select_kernel keeps a tile loop of its own, the one wseg_select.h's select_kernel runs: instantiated from
// the shared kernel a round measured 5 % slower (profiles/select_refactor_ab.txt), so this body stays the one that
// was measured.
//
// select_norms_kernel |row|^2 of every row as ONE c-ordered fmaf chain (a lane per row).
// mst_select_kernel   a work item is 128 rows against one split of the candidate tiles (128 candidates each); the grid strides over
//   the items.  Per candidate tile the 128 x 128 dot products come from v_mfma_f32_32x32x2_f32, 4 x 2 waves of 32 rows x 64
//   candidates (two accumulators) each, both operands streamed through LDS along d in slabs of 16 (double-buffered, the d tail and
//   rows behind n ZERO-FILLED in LDS: no byte outside the matrix is read).  A tile's core[j] and component[j] are staged next to its
//   norms.  That instruction is bit for bit a c-ordered fmaf chain and a zero product leaves the chain as it is, so
//       w^(i, j) = max(core_i, core_j, fmaf(-2, x_i . x_j, |x_i|^2 + |x_j|^2))
//   has ONE value whatever the tiling, the grid, the split or the run.  Candidates of the row's own component (the row itself among
//   them) and candidates behind n are masked.  Every row keeps a sorted list of the L = 1 + 8 smallest keys (ordered-uint w^ << 32 |
//   j: one 64-bit compare is the total order (w^, j)) in LDS, inserted as in select_kernel: keys are distinct and the order is
//   total, so the list does not depend on who came first.  Each (row, split) writes its list to scratch.
//   LDS: 2 x 2 x 16 x 132 floats of slabs (33.0 KiB) + 3 x 128 words of the tile + 128 x 9 keys (9.0 KiB) = 43.5 KiB, two
//   workgroups a CU at 128 registers (four waves a SIMD: the launch bounds).
// mst_finish_kernel   a wave per row: merges the splits' lists into the L smallest keys, recomputes the DIRECT form sum (x_i - x_j)^2
//   of those candidates with fp64 accumulation (sel_direct_sq_f64; (a - b)^2 is symmetric, so d32(i, j) and d32(j, i) have the same
//   bits), forms the exact w = max(core_i, core_j, float32 of that sum) and writes the first under (w, j); -1 / +inf where the row
//   has no candidate.  The cancellation error of w^ therefore only decides WHICH nine candidates are looked at and never shows in a
//   weight.
#include "wseg_mst_plan.h"
#include "wseg_select.h"

namespace wseg {

struct MstArgs {
  const float* x;                  // [n][d]
  long long n;
  int d;
  const float* core;               // [n]
  const int* comp;                 // [n]
  int splits, tiles_per_split;
  long long n_tiles, items;
  float* norm;                     // [n]
  unsigned long long* keys;        // [tiles * 128][splits][L]
  int* index_out;                  // [n]
  float* weight_out;               // [n]
};

template <bool VEC>
__global__ __launch_bounds__(kSelLanes, 4) void mst_select_kernel(MstArgs a) {
  constexpr int BK = 16, LD = kMstTile + 4, TJ = 2, L = kMstL;
  __shared__ float sQ[2][BK][LD];
  __shared__ float sX[2][BK][LD];
  __shared__ __attribute__((aligned(16))) float sxn[kMstTile];
  __shared__ __attribute__((aligned(16))) float sxc[kMstTile];
  __shared__ __attribute__((aligned(16))) int sxk[kMstTile];
  __shared__ unsigned long long lists[kMstTile * L];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int fi = lane & 31, fk = lane >> 5;
  const int lr = tid >> 2, lq = (tid & 3) * 4;           // global loads: row lr of both operands, c offset lq, 4 floats
  const int D = a.d, nk = (D + BK - 1) / BK;
  const int lrow = wm * 32 + fi;                         // the row of this lane's 32 values, inside the tile
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
    const long long m0 = qt * kMstTile;
    for (int idx = tid; idx < kMstTile * L; idx += kSelLanes) lists[idx] = kSelNone;
    const bool qok = m0 + lrow < a.n;
    const float qn = qok ? a.norm[m0 + lrow] : 0.0f;
    const float qc = qok ? a.core[m0 + lrow] : 0.0f;
    const int qk = qok ? a.comp[m0 + lrow] : 0;
    const float* __restrict__ const qp = m0 + lr < a.n ? a.x + (m0 + lr) * D : nullptr;
    const long long t0 = (long long)split * a.tiles_per_split;
    const long long t1 = t0 + a.tiles_per_split < a.n_tiles ? t0 + a.tiles_per_split : a.n_tiles;
    for (long long t = t0; t < t1; ++t) {
      const long long n0 = t * kMstTile;
      if (tid < kMstTile) {
        const bool in = n0 + tid < a.n;
        sxn[tid] = in ? a.norm[n0 + tid] : 0.0f;
        sxc[tid] = in ? a.core[n0 + tid] : 0.0f;
        sxk[tid] = in ? a.comp[n0 + tid] : 0;
      }
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
      __syncthreads();                                   // (also: the cleared lists, the tile's norms, cores and components)
      for (int kt = 0; kt < nk; ++kt) {
        const int b = kt & 1;
        if (kt + 1 < nk) { rq = load4(qp, (kt + 1) * BK + lq); rx = load4(xp, (kt + 1) * BK + lq); }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {             // lanes 0-31 carry c = kk, lanes 32-63 c = kk + 1: ascending c
          const float qf = sQ[b][kk + fk][lrow];
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(sX[b][kk + fk][wn * 64 + j * 32 + fi], qf, acc[j], 0, 0, 0);
        }
        if (kt + 1 < nk) stage(b ^ 1);
        __syncthreads();
      }
      // Register r of acc[j]: row lrow, candidate sel_candidate(wn, fk, j, r) of the tile.  Value number
      // v = 16 j + r of the lane; `pass` marks those that may beat the row's worst entry (a float compare: a superset — the lists
      // only ever tighten, the insertion compares the keys).  The insertion loop exists once: it picks the marked values one by one.
      auto weight_of = [&](int c, float dot) {
        return fmaxf(fmaxf(qc, sxc[c]), fmaf(-2.0f, dot, qn + sxn[c])) + 0.0f;         // (+ 0: no negative zero among the keys)
      };
      const int nvalid = a.n - n0 < kMstTile ? (int)(a.n - n0) : kMstTile;
      // the worst entry's w^ (+inf while the list is not full)
      const unsigned wo = (unsigned)(mylist[L - 1] >> 32);
      const float wf = wo == 0xffffffffu ? sel_inf() : ord2f(wo);
      // (four neighbouring candidates at a time, one 16-byte LDS read per array; the scheduling barrier keeps the compiler from
      // fetching all 96 words ahead, which does not fit 128 registers beside the accumulators)
      unsigned pass = 0;
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c0 = wn * 64 + 32 * j + 8 * g + 4 * fk;
          const float4 n4 = *(const float4*)&sxn[c0], c4 = *(const float4*)&sxc[c0];
          const int4 k4 = *(const int4*)&sxk[c0];
          const float xn[4] = {n4.x, n4.y, n4.z, n4.w}, xc[4] = {c4.x, c4.y, c4.z, c4.w};
          const int xk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float w = fmaxf(fmaxf(qc, xc[e]), fmaf(-2.0f, acc[j][4 * g + e], qn + xn[e]));
            const bool ok = (int)qok & (int)(c0 + e < nvalid) & (int)(xk[e] != qk) & (int)(w <= wf);
            pass |= ok ? 1u << (16 * j + 4 * g + e) : 0u;
          }
          __builtin_amdgcn_sched_barrier(0);
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
                const int c = sel_candidate(wn, fk, v >> 4, v & 15);
                sel_insert(mylist, L, ((unsigned long long)f2ord(weight_of(c, dot)) << 32) | (unsigned)(n0 + c));
              }
            }
            __builtin_amdgcn_wave_barrier();
          }
        }
        __syncthreads();
      }
    }
    if (t1 <= t0) __syncthreads();                       // (no tile: the cleared lists are written out)
    for (int idx = tid; idx < kMstTile * L; idx += kSelLanes) {
      const int row = idx / L, e = idx - row * L;
      a.keys[((m0 + row) * a.splits + split) * L + e] = lists[idx];
    }
    __syncthreads();                                     // the lists are cleared for the next item
  }
}

__global__ __launch_bounds__(64) void mst_finish_kernel(MstArgs a, int vec) {
  __shared__ unsigned sj[kMstL];
  const int lane = threadIdx.x;
  const long long total = (long long)a.splits * kMstL;
  for (long long row = blockIdx.x; row < a.n; row += gridDim.x) {
    const int cnt = sel_merge_split_lists(a.keys + row * total, total, kMstL, lane, sj);
    __syncthreads();
    // the direct form with fp64 accumulation as float32, then the exact weight; the first under (w, j) — every lane holds it
    const float qc = a.core[row];
    unsigned long long first = kSelNone;
    for (int t = 0; t < cnt; ++t) {
      const unsigned j = sj[t];
      const double s = sel_direct_sq_f64(a.x + row * a.d, a.x + (long long)j * a.d, a.d, vec, lane);
      const unsigned long long key = sel_key(fmaxf(fmaxf(qc, a.core[j]), (float)s), j);
      first = key < first ? key : first;
    }
    if (lane == 0) {
      a.index_out[row] = cnt ? (int)(unsigned)first : -1;
      a.weight_out[row] = cnt ? sel_key_value(first) : sel_inf();
    }
    __syncthreads();                                     // sj is laid down anew
  }
}

}  // namespace wseg

using namespace wseg;

extern "C" size_t wseg_mst_scratch_bytes(int64_t n, int32_t d) {
  MstPlan plan;
  char msg[200];
  if (mst_plan(n, d, kMstGridCap, &plan, msg, sizeof(msg))) {
    set_error("wseg_mst_scratch_bytes: %s", msg);
    return 0;
  }
  return (size_t)plan.scratch_bytes;
}

extern "C" int wseg_mst_round_f32(const float* rows, int64_t n, int32_t d, const float* core, const int32_t* component, void* scratch,
                                  size_t scratch_bytes, int32_t* index_out, float* weight_out, void* stream_) {
  const char* fn = "wseg_mst_round_f32";
  hipStream_t stream = (hipStream_t)stream_;
  MstPlan plan;
  char msg[200];
  // (the grid cap — and with it the candidate splits — is a test knob)
  if (mst_plan(n, d, grid_cap_env("WSEG_MST_GRID", kMstGridCap, kMstGridCap), &plan, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (n == 0) return WSEG_OK;
  if (sel_bad_pointer(fn, rows, true, "rows", "a float32") || sel_bad_pointer(fn, core, true, "core", "a float32") ||
      sel_bad_pointer(fn, component, true, "component", "an int32") || sel_bad_pointer(fn, index_out, true, "index_out", "an int32") ||
      sel_bad_pointer(fn, weight_out, true, "weight_out", "a float32") || sel_bad_scratch(fn, scratch, scratch_bytes, plan.scratch_bytes))
    return WSEG_ERR_INVALID;
  MstArgs a;
  a.x = rows;
  a.n = n;
  a.d = d;
  a.core = core;
  a.comp = (const int*)component;
  a.splits = plan.splits;
  a.tiles_per_split = plan.tiles_per_split;
  a.n_tiles = plan.tiles;
  a.items = plan.items;
  a.norm = reinterpret_cast<float*>(static_cast<char*>(scratch) + plan.norm_offset);
  a.keys = reinterpret_cast<unsigned long long*>(static_cast<char*>(scratch) + plan.keys_offset);
  a.index_out = (int*)index_out;
  a.weight_out = weight_out;
  // 16-byte loads where every row starts on 16 bytes
  const bool vec = d % 4 == 0 && !((uintptr_t)rows & 15);
  // (queries == corpus: the norms kernel's second operand is empty)
  const dim3 ngrid((unsigned)plan.norm_grid), nblock(256);
  const float* const none = nullptr;
  if (vec) hipLaunchKernelGGL(select_norms_kernel<true>, ngrid, nblock, 0, stream, rows, (long long)n, none, 0ll, (int)d, a.norm, a.norm);
  else hipLaunchKernelGGL(select_norms_kernel<false>, ngrid, nblock, 0, stream, rows, (long long)n, none, 0ll, (int)d, a.norm, a.norm);
  WSEG_LAUNCH_CHECK();
  const dim3 grid((unsigned)plan.grid), block(kSelLanes);
  if (vec) hipLaunchKernelGGL(mst_select_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(mst_select_kernel<false>, grid, block, 0, stream, a);
  WSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(mst_finish_kernel, dim3((unsigned)plan.finish_grid), dim3(64), 0, stream, a, vec ? 1 : 0);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}
