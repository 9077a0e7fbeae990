// k nearest neighbours of every query row among the corpus rows under banded dynamic time warping (wseg_dtw_knn_f32), and the
// warping distance of a list of pairs (wseg_dtw_pairs_f64).  A row is a sequence of T = steps columns of C = channels values, time
// fastest: row[ch * T + t].  whisperseg_amd/dtw.py::dtw_host is the definition (numpy, float64): the local cost c(a, b) =
// sum_ch (q[ch, a] - x[ch, b])^2 as one sequential chain in ch, G(a, b) = c(a, b) + min(G(a-1, b-1), G(a-1, b), G(a, b-1)) over the
// cells |a - b| <= band, dtw = G(T-1, T-1); the neighbours come in the total order (dtw, index).  The m x n matrix of distances
// never exists.  The host arithmetic — padding, tiles, splits, grids, scratch — is wseg_dtw_plan.h.  The keys, the sorted lists, the
// finish's merge and ranking, the fill kernel and the entry points' checks are wseg_select.h's.  dtw_select_kernel keeps a tile loop
// of its own — sel_tile_product's with a column loader: over the shared function a call measured 3 % slower (DESIGN.md §8,
// profiles/select_refactor_ab.txt), so this body stays the one that was measured.  No inline assembly, no atomics.
//
// dtw_norms_kernel    |column|^2 of every column of every query and corpus row as ONE channel-ordered fmaf chain (a lane a column).
// dtw_select_kernel   every column is a row of dimension C.  A work item is one tile of 128 query columns — 4 sequences padded to 32
//   steps, or 2 padded to 64 — against one split of the candidate tiles (as many sequences each); the grid strides over the items.
//   Per candidate tile the 128 x 128 dot products q_a . x_b come from v_mfma_f32_32x32x2_f32, 4 x 2 waves of 32 query columns x 64
//   candidate columns each: both operands streamed through LDS along the channels in slabs of 16 (double-buffered, the next slab
//   fetched under the MFMAs; the channel tail, the padded steps and the sequences behind m / n ZERO-FILLED in LDS: no byte outside
//   the two matrices is read).  A pair's T x T matrix is one 32 x 32 accumulator block (2 x 2 of them at T > 32); steps below 32 or
//   between 33 and 63 waste matrix work in proportion to the padding — nothing is packed.  That instruction is bit for bit a
//   k-ordered fmaf chain and a zero product leaves the chain as it is, so
//       c^(a, b) = fmaf(-2, q_a . x_b, |q_a|^2 + |x_b|^2)
//   has ONE value whatever the tiling, the grid, the split or the run.  The tile's costs go to LDS (over the slab buffers, free
//   after the channel loop; rows 130 floats apart: the 32 lanes of an LDS group read an anti-diagonal, 129 floats from lane to
//   lane, from 32 different banks, and the stores of the costs are two-way, which their register transfer hides) and the
//   recurrence runs in float32 as an anti-diagonal sweep: a lane per row a of a pair — 16 pairs x 32 lanes, or 4 pairs x 64 lanes
//   of the first four waves — 2 T - 1 steps, the neighbour row's two last values through lane shifts.  Only G^(T-1, T-1) leaves the
//   sweep: one lane per query sequence inserts the tile's keys (ordered-uint G^ << 32 | j: one 64-bit compare is the total order
//   (G^, j)) into the sequence's sorted list of the L = k + 8 smallest.  Keys are distinct and the order is total, so the list
//   does not depend on the order of the tiles.  Each (row, split) writes its list to scratch.
//   LDS: 128 x 130 floats of costs / slabs (65.0 KiB) + 128 norms + 4 x 72 keys + 16 results = 67.8 KiB: two workgroups a CU.
// dtw_finish_kernel   a wave per query row: merges the splits' lists into the L smallest keys, recomputes those candidates by THE
//   DEFINITION in float64 (dtw_pair_f64: a lane per cell of the band, the cell's chain sequential in ch with the difference, the
//   square and the addition rounded one by one — the build pins -ffp-contract=off —, then the sweep in float64), orders them by
//   (float32 of that distance, j) — the value it reports — and writes the first k; -1 / +inf where candidates ran out.  The
//   selection's error therefore only matters at the boundary of the k + 8 kept candidates and never shows in a distance.
// dtw_pairs_kernel    a wave per pair of a caller's list: dtw_pair_f64, reported as float32.
#include "wseg_dtw_plan.h"
#include "wseg_select.h"

namespace wseg {

constexpr int kDtwCostLd = kDtwTile + 2;             // floats between two rows of the costs in LDS

struct DtwArgs {
  const float* q;                  // [m][C * T]
  const float* x;                  // [n][C * T]
  long long m, n;
  int C, T, band, k, L;
  int exclude;                     // 1: candidate j == query row i is none
  int splits, tiles_per_split;
  long long n_tiles, items;
  float* qnorm;                    // [m][T]
  float* xnorm;                    // [n][T]
  unsigned long long* keys;        // [m_tiles * seqs][splits][L]
  int* index_out;                  // [m][k]
  float* distance_out;             // [m][k]
};

// |column|^2 of the columns of q then of x: acc = fmaf(v, v, acc) over ch ascending — the chain the MFMA runs on a product
__global__ __launch_bounds__(256) void dtw_norms_kernel(DtwArgs a) {
  const long long qcols = a.m * a.T, cols = (a.m + a.n) * a.T;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cols; c += (long long)gridDim.x * 256) {
    const bool isq = c < qcols;
    const long long cc = isq ? c : c - qcols;
    const long long row = cc / a.T;
    const int t = (int)(cc - row * a.T);
    const float* __restrict__ p = (isq ? a.q : a.x) + row * ((long long)a.C * a.T) + t;
    float acc = 0.0f;
    for (int ch = 0; ch < a.C; ++ch) {
      const float v = p[(long long)ch * a.T];
      acc = fmaf(v, v, acc);
    }
    if (isq) a.qnorm[cc] = acc; else a.xnorm[cc] = acc;
  }
}

// The recurrence as an anti-diagonal sweep over the costs `crow[b]` = c(a, b) of this lane's row a: at step s the lane holds cell
// (a, s - a); its left neighbour G(a, b - 1) is its own value of the step before, G(a - 1, b) and G(a - 1, b - 1) are lane a - 1's
// values of the last and the last but one step (lane shifts inside groups of `WIDTH` lanes).  Cells outside the band or the T x T
// square are +inf and their costs are not read.  -> G(a, T - 1 + ...) of the last step the lane was inside: lane a = T - 1 returns
// G(T - 1, T - 1).  Every lane of the wave must call it.
template <typename F, int WIDTH>
__device__ __forceinline__ F dtw_sweep(const F* crow, int a, int T, int band) {
  const F inf = (F)__uint_as_float(0x7f800000u);
  F p1 = inf, p2 = inf;
  for (int s = 0; s <= 2 * T - 2; ++s) {
    F u1 = __shfl_up(p1, 1, WIDTH), u2 = __shfl_up(p2, 1, WIDTH);
    if (a == 0) { u1 = inf; u2 = inf; }
    const int b = s - a, off = b - a;
    const bool inside = a < T && b >= 0 && b < T && off <= band && -off <= band;
    const F c = inside ? crow[b] : (F)0;
    const F low = u1 < p1 ? u1 : p1, best = u2 < low ? u2 : low;
    const F g = inside ? (s == 0 ? c : c + best) : inf;
    p2 = p1;
    p1 = g;
  }
  return p1;
}

template <int TP>
__global__ __launch_bounds__(kSelLanes, 2) void dtw_select_kernel(DtwArgs a) {
  constexpr int BK = 16, LD = kDtwTile + 4, TJ = 2, S = kDtwTile / TP;
  static_assert(2 * 2 * BK * LD <= kDtwTile * kDtwCostLd, "the slabs lie inside the costs");
  __shared__ float sbuf[kDtwTile * kDtwCostLd];          // the slabs of the channel loop, then the tile's costs
  __shared__ float sxn[kDtwTile];
  __shared__ float sres[S * S];
  __shared__ unsigned long long lists[S * kDtwMaxL];
  float (*const sQ)[BK][LD] = reinterpret_cast<float (*)[BK][LD]>(sbuf);
  float (*const sX)[BK][LD] = reinterpret_cast<float (*)[BK][LD]>(sbuf + 2 * BK * LD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int fi = lane & 31, fk = lane >> 5;
  const int lcol = tid & (kDtwTile - 1), lk = tid >> 7;  // global loads: column lcol of both operands, channels lk, lk + 4, lk + 8, lk + 12 of a slab
  const int lseq = lcol / TP, lt = lcol % TP;
  const int C = a.C, T = a.T, L = a.L, nk = (C + BK - 1) / BK;
  const long long D = (long long)C * T;
  const int lrow = wm * 32 + fi;                         // the query column of this lane's 32 values, inside the tile
  // the sweep: a lane per row of a pair; with TP = 64 the pairs are those of the first four waves
  const int pair = tid / TP, pa = tid % TP;
  const bool sweeps = pair < S * S;
  const int pq = sweeps ? pair / S : 0, px = sweeps ? pair % S : 0;
  const float* const crow = sbuf + (pq * TP + pa) * kDtwCostLd + px * TP;
  auto load = [&](const float* __restrict__ p, int ch0, float (&v)[4]) {      // p: the column's first channel, null where there is none
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = ch0 + lk + 4 * i;
      v[i] = p && ch < C ? p[ch * T] : 0.0f;
    }
  };
  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const long long qt = item / a.splits;
    const int split = (int)(item - qt * a.splits);
    const long long m0 = qt * S;
    for (int idx = tid; idx < S * L; idx += kSelLanes) lists[idx] = kSelNone;
    const int rseq = lrow / TP, rt = lrow % TP;
    const float qn = m0 + rseq < a.m && rt < T ? a.qnorm[(m0 + rseq) * T + rt] : 0.0f;
    const float* __restrict__ const qp = m0 + lseq < a.m && lt < T ? a.q + (m0 + lseq) * D + lt : nullptr;
    const long long t0 = (long long)split * a.tiles_per_split;
    const long long t1 = t0 + a.tiles_per_split < a.n_tiles ? t0 + a.tiles_per_split : a.n_tiles;
    for (long long t = t0; t < t1; ++t) {
      const long long n0 = t * S;
      if (tid < kDtwTile) sxn[tid] = n0 + lseq < a.n && lt < T ? a.xnorm[(n0 + lseq) * T + lt] : 0.0f;
      const float* __restrict__ const xp = n0 + lseq < a.n && lt < T ? a.x + (n0 + lseq) * D + lt : nullptr;
      float rq[4], rx[4];
      load(qp, 0, rq);
      load(xp, 0, rx);
      auto stage = [&](int b) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sQ[b][lk + 4 * i][lcol] = rq[i];
          sX[b][lk + 4 * i][lcol] = rx[i];
        }
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
        if (kt + 1 < nk) { load(qp, (kt + 1) * BK, rq); load(xp, (kt + 1) * BK, rx); }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {             // lanes 0-31 carry channel kk, lanes 32-63 kk + 1: ascending channels
          const float qf = sQ[b][kk + fk][lrow];
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(sX[b][kk + fk][wn * 64 + j * 32 + fi], qf, acc[j], 0, 0, 0);
        }
        if (kt + 1 < nk) stage(b ^ 1);
        __syncthreads();
      }
      // Register r of acc[j]: query column lrow, candidate column sel_candidate(wn, fk, j, r) of the tile.  The
      // slabs were read for the last time before the barrier above: the costs go over them.
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = sel_candidate(wn, fk, j, r);
          sbuf[lrow * kDtwCostLd + c] = fmaf(-2.0f, acc[j][r], qn + sxn[c]);
        }
      __syncthreads();
      if (wave * 64 < S * S * TP) {                      // (whole waves: every lane of a sweeping wave takes part in the shifts)
        const float g = dtw_sweep<float, TP>(crow, pa, T, a.band);
        if (pa == T - 1) sres[pq * S + px] = g + 0.0f;   // (+ 0: no negative zero among the keys)
      }
      __syncthreads();
      if (tid < S && m0 + tid < a.m) {                   // a lane per query sequence: its S candidates of the tile
        for (int c = 0; c < S; ++c) {
          const long long j = n0 + c;
          if (j < a.n && !(a.exclude && j == m0 + tid))
            sel_insert(lists + tid * L, L, ((unsigned long long)f2ord(sres[tid * S + c]) << 32) | (unsigned)j);
        }
      }
      __syncthreads();                                   // the costs are read, the lists written: the next tile stages its first slab
    }
    if (t1 <= t0) __syncthreads();                       // (no tile: the cleared lists are written out)
    for (int idx = tid; idx < S * L; idx += kSelLanes) {
      const int row = idx / L, e = idx - row * L;
      a.keys[((m0 + row) * a.splits + split) * L + e] = lists[idx];
    }
    __syncthreads();                                     // the lists are cleared for the next item
  }
}

// THE DEFINITION on one pair, by one wave: the costs of the band's cells into `sc` [T][T] (a lane per cell, the chain sequential in
// ch: difference, square and addition each rounded once, in float64), then the sweep in float64 -> dtw(q, x) in every lane.
__device__ __forceinline__ double dtw_pair_f64(const float* __restrict__ q, const float* __restrict__ x, int C, int T, int band, double* sc,
                                               int lane) {
  const int W = 2 * band + 1;
  for (int e = lane; e < T * W; e += 64) {
    const int ca = e / W, cb = ca - band + (e - ca * W);
    if (cb < 0 || cb >= T) continue;
    double acc = 0.0;
    for (int ch = 0; ch < C; ++ch) {
      const double df = (double)q[ch * T + ca] - (double)x[ch * T + cb];
      const double sq = df * df;
      acc = acc + sq;
    }
    sc[ca * T + cb] = acc;
  }
  __syncthreads();                                       // (a single-wave workgroup: the costs are written)
  const double g = dtw_sweep<double, 64>(sc + (lane < T ? lane : 0) * T, lane, T, band);
  const double out = __shfl(g, T - 1);
  __syncthreads();                                       // sc is laid down anew by the next pair
  return out;
}

__global__ __launch_bounds__(64) void dtw_finish_kernel(DtwArgs a) {
  __shared__ double sc[kDtwMaxSteps * kDtwMaxSteps];
  __shared__ unsigned sj[kDtwMaxL];
  __shared__ unsigned long long sk[kDtwMaxL];
  const int lane = threadIdx.x, L = a.L;
  const long long D = (long long)a.C * a.T;
  const long long total = (long long)a.splits * L;
  for (long long row = blockIdx.x; row < a.m; row += gridDim.x) {
    const int cnt = sel_merge_split_lists(a.keys + row * total, total, L, lane, sj);
    __syncthreads();
    const float* __restrict__ q = a.q + row * D;
    for (int t = 0; t < cnt; ++t) {
      const unsigned j = sj[t];
      const double g = dtw_pair_f64(q, a.x + (long long)j * D, a.C, a.T, a.band, sc, lane);
      if (lane == 0) sk[t] = sel_key((float)g, j);
    }
    __syncthreads();
    sel_rank_and_write(sk, cnt, a.k, lane, a.index_out + row * a.k, a.distance_out + row * a.k);
    __syncthreads();                                     // sj and sk are laid down anew
  }
}

// out[p] = float32(dtw(q[pairs[p][0]], x[pairs[p][1]])); NaN, and nothing read, where an index is outside its rows
__global__ __launch_bounds__(64) void dtw_pairs_kernel(DtwArgs a, const int* __restrict__ pairs, long long count, float* __restrict__ out) {
  __shared__ double sc[kDtwMaxSteps * kDtwMaxSteps];
  const int lane = threadIdx.x;
  const long long D = (long long)a.C * a.T;
  for (long long p = blockIdx.x; p < count; p += gridDim.x) {
    const long long i = pairs[2 * p], j = pairs[2 * p + 1];
    if (i < 0 || i >= a.m || j < 0 || j >= a.n) {        // (the same for every lane)
      if (lane == 0) out[p] = __uint_as_float(0x7fc00000u);
      continue;
    }
    const double g = dtw_pair_f64(a.q + i * D, a.x + j * D, a.C, a.T, a.band, sc, lane);
    if (lane == 0) out[p] = (float)g;
  }
}

}  // namespace wseg

using namespace wseg;

extern "C" size_t wseg_dtw_scratch_bytes(int64_t m, int64_t n, int32_t channels, int32_t steps, int32_t k) {
  DtwPlan plan;
  char msg[200];
  if (dtw_plan(m, n, channels, steps, k, kDtwGridCap, &plan, msg, sizeof(msg))) {
    set_error("wseg_dtw_scratch_bytes: %s", msg);
    return 0;
  }
  return (size_t)plan.scratch_bytes;
}

extern "C" int wseg_dtw_knn_f32(const float* queries, int64_t m, const float* corpus, int64_t n, int32_t channels, int32_t steps, int32_t band,
                                int32_t k, int32_t exclude_same_index, void* scratch, size_t scratch_bytes, int32_t* index_out,
                                float* distance_out, void* stream_) {
  const char* fn = "wseg_dtw_knn_f32";
  hipStream_t stream = (hipStream_t)stream_;
  DtwPlan plan;
  char msg[200];
  // (the grid cap — and with it the candidate splits — is a test knob)
  if (dtw_plan(m, n, channels, steps, k, grid_cap_env("WSEG_DTW_GRID", kDtwGridCap, kDtwGridCap), &plan, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (band < 0 || dtw_check_shape(channels, steps, band, msg, sizeof(msg))) {
    if (band < 0) snprintf(msg, sizeof(msg), "band must be 0 .. steps - 1 = %d (got %d)", (int)steps - 1, (int)band);
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (exclude_same_index != 0 && exclude_same_index != 1) { set_error("%s: exclude_same_index must be 0 or 1", fn); return WSEG_ERR_INVALID; }
  if (m == 0) return WSEG_OK;
  if (sel_bad_pointer(fn, queries, true, "queries", "a float32") || sel_bad_pointer(fn, corpus, n > 0, "corpus", "a float32") ||
      sel_bad_pointer(fn, index_out, true, "index_out", "an int32") || sel_bad_pointer(fn, distance_out, true, "distance_out", "a float32"))
    return WSEG_ERR_INVALID;
  if (n == 0) {
    sel_launch_fill((int*)index_out, distance_out, (long long)m * k, stream);
    WSEG_LAUNCH_CHECK();
    return WSEG_OK;
  }
  if (sel_bad_scratch(fn, scratch, scratch_bytes, plan.scratch_bytes)) return WSEG_ERR_INVALID;
  DtwArgs a;
  a.q = queries;
  a.x = corpus;
  a.m = m;
  a.n = n;
  a.C = channels;
  a.T = steps;
  a.band = band;
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
  hipLaunchKernelGGL(dtw_norms_kernel, dim3((unsigned)plan.norm_grid), dim3(256), 0, stream, a);
  WSEG_LAUNCH_CHECK();
  const dim3 grid((unsigned)plan.grid), block(kSelLanes);
  if (plan.padded == kDtwBlock) hipLaunchKernelGGL(dtw_select_kernel<kDtwBlock>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(dtw_select_kernel<2 * kDtwBlock>, grid, block, 0, stream, a);
  WSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(dtw_finish_kernel, dim3((unsigned)plan.finish_grid), dim3(64), 0, stream, a);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}

extern "C" int wseg_dtw_pairs_f64(const float* queries, int64_t m, const float* corpus, int64_t n, int32_t channels, int32_t steps, int32_t band,
                                  const int32_t* pairs, int64_t count, float* out, void* stream_) {
  const char* fn = "wseg_dtw_pairs_f64";
  hipStream_t stream = (hipStream_t)stream_;
  char msg[200];
  if (band < 0 || dtw_check_shape(channels, steps, band, msg, sizeof(msg))) {
    if (band < 0) snprintf(msg, sizeof(msg), "band must be 0 .. steps - 1 = %d (got %d)", (int)steps - 1, (int)band);
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (sel_check_rows("m", m, msg, sizeof(msg)) || sel_check_rows("n", n, msg, sizeof(msg))) { set_error("%s: %s", fn, msg); return WSEG_ERR_INVALID; }
  if (count < 0 || count > kDtwMaxRows) { set_error("%s: the pair count must be 0 .. 2^31 - 1 (got %lld)", fn, (long long)count); return WSEG_ERR_INVALID; }
  if (count == 0) return WSEG_OK;
  if (m == 0 || n == 0) { set_error("%s: pairs need rows on both sides (m %lld, n %lld)", fn, (long long)m, (long long)n); return WSEG_ERR_INVALID; }
  if (sel_bad_pointer(fn, queries, true, "queries", "a float32") || sel_bad_pointer(fn, corpus, true, "corpus", "a float32") ||
      sel_bad_pointer(fn, pairs, true, "pairs", "an int32") || sel_bad_pointer(fn, out, true, "out", "a float32"))
    return WSEG_ERR_INVALID;
  DtwArgs a = {};
  a.q = queries;
  a.x = corpus;
  a.m = m;
  a.n = n;
  a.C = channels;
  a.T = steps;
  a.band = band;
  const int32_t grid = dtw_wave_grid(count, grid_cap_env("WSEG_DTW_GRID", kDtwGridCap, kDtwGridCap));
  hipLaunchKernelGGL(dtw_pairs_kernel, dim3((unsigned)grid), dim3(64), 0, stream, a, (const int*)pairs, (long long)count, out);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}
