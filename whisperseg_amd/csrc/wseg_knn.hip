// k nearest neighbours of every query row among the corpus rows under the squared Euclidean distance (wseg_knn_f32): the graph that
// clustering, embedding and "calls like this one" start from, over the per-segment patches or any float32 rows.  The m x n matrix of
// distances never exists.  whisperseg_amd/neighbors.py::neighbors_host is the definition (numpy, float64, direct form, total order
// (distance, index)); the host arithmetic — tiles, splits, grids, scratch — is wseg_knn_plan.h.  The device pattern — norms, the
// 128 x 128 tile of dot products, keys, sorted lists in LDS, per-(row, split) lists in scratch, the wave-per-row finish — is
// wseg_select.h; this file states what is kNN's own.  No inline assembly, no atomics.
//
// select_norms_kernel            |row|^2 of every query and corpus row, one launch over the m + n rows.
// select_kernel<.., KnnScore>    ranks by d^(i, j) = fmaf(-2, q_i . x_j, |q_i|^2 + |x_j|^2) and keeps the L = k + 8 smallest keys of every
//   query row; with exclude the row's own index is none.  LDS: 33.0 KiB of slabs + 128 norms + the lists: 128 x 24 keys (24.0 KiB;
//   k <= 16) = 57.5 KiB, two workgroups a CU at 128 registers — or 128 x 72 keys (72.0 KiB) = 105.5 KiB, one workgroup a CU.
// knn_finish_kernel              a wave per query row: the L smallest keys of the splits' lists, the DIRECT form sum (q - x)^2 of those
//   candidates with fp64 accumulation, ordered by (float32 of that sum, j), the first k written.
#include "wseg_knn_plan.h"
#include "wseg_select.h"

namespace wseg {

// the squared Euclidean distance; the candidate j == query row i is none where asked
struct KnnScore {
  int exclude;
  struct Tile { __attribute__((aligned(16))) float xn[kSelTile]; };
  struct Row { float qn; int selfc; };                   // selfc: the row's own column in the current tile, -1 where it has none
  __device__ __forceinline__ void stage(const SelectArgs& a, Tile& t, int c, long long j, bool in) const { t.xn[c] = in ? a.xnorm[j] : 0.0f; }
  __device__ __forceinline__ Row row(const SelectArgs& a, long long i, bool ok) const { return {ok ? a.qnorm[i] : 0.0f, -1}; }
  // (one int per tile: a 64-bit compare per value does not fit 128 registers beside the accumulators)
  __device__ __forceinline__ void enter(Row& r, long long i, long long n0) const { r.selfc = exclude && i >= n0 && i - n0 < kSelTile ? (int)(i - n0) : -1; }
  __device__ __forceinline__ float value(const Row& r, const Tile& t, int c, float dot) const { return fmaf(-2.0f, dot, r.qn + t.xn[c]); }
  __device__ __forceinline__ bool masked(const Row& r, const Tile&, int c) const { return c == r.selfc; }
};

struct KnnFinishArgs {
  const float* q;                  // [m][d]
  const float* x;                  // [n][d]
  long long m;
  int d, k, L, splits;
  const unsigned long long* keys;  // [m_tiles * 128][splits][L]
  int* index_out;                  // [m][k]
  float* distance_out;             // [m][k]
};

__global__ __launch_bounds__(64) void knn_finish_kernel(KnnFinishArgs a, int vec) {
  __shared__ unsigned sj[kKnnMaxL];
  __shared__ unsigned long long sk[kKnnMaxL];
  const int lane = threadIdx.x;
  const long long total = (long long)a.splits * a.L;
  for (long long row = blockIdx.x; row < a.m; row += gridDim.x) {
    const int cnt = sel_merge_split_lists(a.keys + row * total, total, a.L, lane, sj);
    __syncthreads();
    // the direct form with fp64 accumulation, reported as float32
    for (int t = 0; t < cnt; ++t) {
      const unsigned j = sj[t];
      const double s = sel_direct_sq_f64(a.q + row * a.d, a.x + (long long)j * a.d, a.d, vec, lane);
      if (lane == 0) sk[t] = sel_key((float)s, j);
    }
    __syncthreads();
    sel_rank_and_write(sk, cnt, a.k, lane, a.index_out + row * a.k, a.distance_out + row * a.k);
    __syncthreads();                                     // sj and sk are laid down anew
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
  if (sel_bad_pointer(fn, queries, true, "queries", "a float32") || sel_bad_pointer(fn, corpus, n > 0, "corpus", "a float32") ||
      sel_bad_pointer(fn, index_out, true, "index_out", "an int32") || sel_bad_pointer(fn, distance_out, true, "distance_out", "a float32"))
    return WSEG_ERR_INVALID;
  if (n == 0) {
    sel_launch_fill((int*)index_out, distance_out, (long long)m * k, stream);
    WSEG_LAUNCH_CHECK();
    return WSEG_OK;
  }
  if (sel_bad_scratch(fn, scratch, scratch_bytes, plan.scratch_bytes)) return WSEG_ERR_INVALID;
  float* const qnorm = reinterpret_cast<float*>(static_cast<char*>(scratch) + plan.qnorm_offset);
  float* const xnorm = reinterpret_cast<float*>(static_cast<char*>(scratch) + plan.xnorm_offset);
  unsigned long long* const keys = reinterpret_cast<unsigned long long*>(static_cast<char*>(scratch) + plan.keys_offset);
  const SelectArgs a = {queries, corpus, m, n, d, plan.L, plan.splits, plan.tiles_per_split, plan.n_tiles, plan.items, qnorm, xnorm, keys};
  const KnnScore score = {exclude_same_index};
  const KnnFinishArgs f = {queries, corpus, m, d, k, plan.L, plan.splits, keys, (int*)index_out, distance_out};
  // 16-byte loads where every row starts on 16 bytes
  const bool vec = d % 4 == 0 && !((uintptr_t)queries & 15) && !((uintptr_t)corpus & 15);
  const dim3 ngrid((unsigned)plan.norm_grid), nblock(256);
  if (vec) hipLaunchKernelGGL(select_norms_kernel<true>, ngrid, nblock, 0, stream, queries, (long long)m, corpus, (long long)n, (int)d, qnorm, xnorm);
  else hipLaunchKernelGGL(select_norms_kernel<false>, ngrid, nblock, 0, stream, queries, (long long)m, corpus, (long long)n, (int)d, qnorm, xnorm);
  WSEG_LAUNCH_CHECK();
  // lists of up to kKnnSmallL entries leave room for two workgroups a CU
  const dim3 grid((unsigned)plan.grid), block(kSelLanes);
  if (plan.L <= kKnnSmallL) {
    if (vec) hipLaunchKernelGGL((select_kernel<true, kKnnSmallL, KnnScore>), grid, block, 0, stream, a, score);
    else hipLaunchKernelGGL((select_kernel<false, kKnnSmallL, KnnScore>), grid, block, 0, stream, a, score);
  } else {
    if (vec) hipLaunchKernelGGL((select_kernel<true, kKnnMaxL, KnnScore>), grid, block, 0, stream, a, score);
    else hipLaunchKernelGGL((select_kernel<false, kKnnMaxL, KnnScore>), grid, block, 0, stream, a, score);
  }
  WSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_finish_kernel, dim3((unsigned)plan.finish_grid), dim3(64), 0, stream, f, vec ? 1 : 0);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}
