// The layout epochs of the 2-D / 3-D embedding of the calls (wseg_embed_epochs_f64): a SYNCHRONOUS variant of UMAP's optimiser over
// the fuzzy graph whisperseg_amd/embed.py builds on the host from the nearest-neighbour lists.  embed.py::layout_host is the
// definition (numpy, float64) and spells out the schedule, the negative samples and a term; this file restates it operation for
// operation: float64 + - * / are correctly rounded on both sides and the build has -ffp-contract=off, so with b == 1 the positions
// are the definition's in every bit, and with another b they differ by what the two pow functions differ by.  The host arithmetic —
// validation, grid, which buffer an epoch reads and writes, the scratch — is wseg_embed_plan.h.  No inline assembly, no atomics.
//
// embed_epoch_kernel<POW>   one epoch t: a lane per vertex i, the grid striding over the vertices.  The lane walks the entries of
//   row i of the CSR IN ORDER; an entry that the schedule makes active in epoch t adds its attraction term and then the repulsion
//   terms of its n_neg negative samples (counter-based: splitmix64's finaliser of seed * golden + ((t * nnz + e) * n_neg + s)) to
//   the lane's G — ONE sequential chain per vertex, whatever the grid — and y_out[i] = y_in[i] + alpha_t * G.  Every epoch reads only
//   the positions the previous epoch wrote (another buffer: the plan's ping-pong), so there is no race and nothing depends on
//   scheduling.  POW = false is the instance for b == 1 (x^b is x: no pow); POW = true calls pow(d2, b).
//   An entry whose index is outside 0 .. n - 1 and the part of a row outside 0 .. nnz contribute nothing: the kernel reads no byte
//   outside its inputs whatever the arrays hold.
//
// embed_place_kernel<POW>   ALL the epochs t0 .. t1 - 1 of placing new rows on a frozen map (wseg_embed_place_f64; the definition is
//   embed.py::place_host): a lane per NEW row, the grid striding over them.  A new row's terms read only the corpus positions, which
//   never move, and its own position, so the lane keeps that in registers and runs every epoch itself — one launch, no ping-pong, no
//   scratch — walking its entries in order as above: ONE sequential chain per row and epoch, whatever the grid and whichever other
//   rows came in the call.  The negative samples of entry q (its position in the row, < 64) in epoch t are counter-based on the
//   row's own key: splitmix64's finaliser of key + ((t * 64 + q) * 16 + s); none is skipped (a corpus vertex is never the row).
//   The same memory safety: an entry outside 0 .. n - 1 contributes nothing but keeps its q, a row reaches no further than
//   0 .. nnz, and its entries past the 64th contribute nothing.
//
// Both kernels form a term with the one embed_term below.
#include "wseg_common.h"
#include "wseg_embed_plan.h"

namespace wseg {

struct EmbedArgs {
  const long long* indptr;         // [n + 1]
  const int* indices;              // [nnz]
  const unsigned* rate;            // [nnz]
  long long n, nnz;
  int dim, n_neg;
  const double* y_in;              // [n][dim]
  double* y_out;                   // [n][dim]
  unsigned long long t;            // the epoch
  unsigned long long seed_mul;     // seed * 0x9E3779B97F4A7C15
  double alpha, a, b, gamma;
};

__device__ __forceinline__ unsigned long long embed_mix(unsigned long long x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// fmin / fmax drop a NaN operand (a NaN v becomes -4) where numpy's minimum / maximum of the definition keep it: the two differ only
// once d2 or P overflowed (coef * delta = 0 * inf), which the definition's conventions exclude
__device__ __forceinline__ double embed_clip(double v) { return fmin(4.0, fmax(-4.0, v)); }

// A term of the definition, written ONCE for both kernels: G += the clipped attraction (PULL) or repulsion term of the point
// (x0, x1, x2) towards / away from the position y.  pull_ab = (-2 a) b and push_gb = (2 gamma) b are the products the definition
// forms first; every other operation stands here in the definition's order.
struct EmbedTerm {
  double a, b, pull_ab, push_gb;
  bool three;
};

template <bool POW, bool PULL>
__device__ __forceinline__ void embed_term(const EmbedTerm& c, double x0, double x1, double x2, const double* y, double& g0, double& g1,
                                           double& g2) {
  const double d0 = x0 - y[0], d1 = x1 - y[1], d2c = c.three ? x2 - y[2] : 0.0;
  double d2 = d0 * d0 + d1 * d1;
  if (c.three) d2 = d2 + d2c * d2c;
  if (PULL && d2 == 0.0) return;       // coef is 0 and the term +0 or -0, which leaves G (never -0: it began as +0) as it is
  const double P = POW ? pow(d2, c.b) : d2;
  const double coef = PULL ? (c.pull_ab * P) / (d2 * (1.0 + c.a * P)) : c.push_gb / ((0.001 + d2) * (1.0 + c.a * P));
  g0 += embed_clip(coef * d0);
  g1 += embed_clip(coef * d1);
  if (c.three) g2 += embed_clip(coef * d2c);
}

template <bool POW>
__global__ __launch_bounds__(kEmbedLanes) void embed_epoch_kernel(EmbedArgs p) {
  const bool three = p.dim == 3;
  const EmbedTerm term = {p.a, p.b, (-2.0 * p.a) * p.b, (2.0 * p.gamma) * p.b, three};
  for (long long i = (long long)blockIdx.x * kEmbedLanes + threadIdx.x; i < p.n; i += (long long)gridDim.x * kEmbedLanes) {
    const double* yi = p.y_in + i * p.dim;
    const double x0 = yi[0], x1 = yi[1], x2 = three ? yi[2] : 0.0;
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    long long e = p.indptr[i], e_end = p.indptr[i + 1];
    if (e < 0) e = 0;
    if (e_end > p.nnz) e_end = p.nnz;
    for (; e < e_end; ++e) {
      const unsigned long long r = p.rate[e];
      if ((((p.t + 1) * r) >> 16) == ((p.t * r) >> 16)) continue;                    // not this epoch
      const long long j = p.indices[e];
      if (j < 0 || j >= p.n) continue;
      embed_term<POW, true>(term, x0, x1, x2, p.y_in + j * p.dim, g0, g1, g2);
      const unsigned long long c0 = (p.t * (unsigned long long)p.nnz + (unsigned long long)e) * (unsigned long long)p.n_neg;
      for (int s = 0; s < p.n_neg; ++s) {
        const unsigned long long h = embed_mix(p.seed_mul + (c0 + (unsigned long long)s));
        const long long m = (long long)(((h >> 32) * (unsigned long long)p.n) >> 32);
        if (m == i) continue;
        embed_term<POW, false>(term, x0, x1, x2, p.y_in + m * p.dim, g0, g1, g2);
      }
    }
    double* yo = p.y_out + i * p.dim;
    yo[0] = x0 + p.alpha * g0;
    yo[1] = x1 + p.alpha * g1;
    if (three) yo[2] = x2 + p.alpha * g2;
  }
}

struct PlaceArgs {
  const long long* indptr;         // [m + 1]
  const int* indices;              // [nnz]: corpus vertices
  const unsigned* rate;            // [nnz]
  const unsigned long long* key;   // [m]
  long long m, nnz, n;
  int dim, n_neg;
  const double* corpus;            // [n][dim]: never written
  const double* y_in;              // [m][dim]
  double* y_out;                   // [m][dim]
  long long t0, t1;                // the epochs of this call
  double total, lr, a, b, gamma;   // total: T as a double
};

template <bool POW>
__global__ __launch_bounds__(kEmbedLanes) void embed_place_kernel(PlaceArgs p) {
  const bool three = p.dim == 3;
  const EmbedTerm term = {p.a, p.b, (-2.0 * p.a) * p.b, (2.0 * p.gamma) * p.b, three};
  for (long long i = (long long)blockIdx.x * kEmbedLanes + threadIdx.x; i < p.m; i += (long long)gridDim.x * kEmbedLanes) {
    const double* yi = p.y_in + i * p.dim;
    double x0 = yi[0], x1 = yi[1], x2 = three ? yi[2] : 0.0;
    // entry q of the row is e0 + q; only 0 <= e0 + q < min(e1, nnz) with q < kEmbedPlaceRow is ever read
    const long long e0 = p.indptr[i];
    long long e1 = p.indptr[i + 1];
    if (e1 > p.nnz) e1 = p.nnz;
    if (e1 < 0) e1 = 0;                                   // (e1 - first below stays inside int64 whatever indptr holds)
    const long long first = e0 < 0 ? 0 : e0;
    const long long q_first = e0 < 0 ? (e0 < -(long long)kEmbedPlaceRow ? (long long)kEmbedPlaceRow : -e0) : 0;
    long long q_end = q_first + (e1 - first);
    if (q_end > kEmbedPlaceRow) q_end = kEmbedPlaceRow;
    const unsigned long long key = p.key[i];
    for (long long t = p.t0; t < p.t1; ++t) {
      const unsigned long long tu = (unsigned long long)t;
      double g0 = 0.0, g1 = 0.0, g2 = 0.0;
      for (long long q = q_first; q < q_end; ++q) {
        const long long e = first + (q - q_first);
        const unsigned long long r = p.rate[e];
        if ((((tu + 1) * r) >> 16) == ((tu * r) >> 16)) continue;                    // not this epoch
        const long long j = p.indices[e];
        if (j < 0 || j >= p.n) continue;
        embed_term<POW, true>(term, x0, x1, x2, p.corpus + j * p.dim, g0, g1, g2);
        const unsigned long long c0 = key + (tu * (unsigned long long)kEmbedPlaceRow + (unsigned long long)q) * (unsigned long long)kEmbedMaxNeg;
        for (int s = 0; s < p.n_neg; ++s) {
          const unsigned long long h = embed_mix(c0 + (unsigned long long)s);
          const long long v = (long long)(((h >> 32) * (unsigned long long)p.n) >> 32);
          embed_term<POW, false>(term, x0, x1, x2, p.corpus + v * p.dim, g0, g1, g2);
        }
      }
      const double alpha = p.lr * (1.0 - (double)t / p.total);
      x0 = x0 + alpha * g0;
      x1 = x1 + alpha * g1;
      if (three) x2 = x2 + alpha * g2;
    }
    double* yo = p.y_out + i * p.dim;
    yo[0] = x0;
    yo[1] = x1;
    if (three) yo[2] = x2;
  }
}

static bool embed_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

}  // namespace wseg

using namespace wseg;

extern "C" size_t wseg_embed_scratch_bytes(int64_t n, int32_t dim) {
  EmbedPlan plan;
  char msg[200];
  if (embed_sizes(n, dim, &plan, msg, sizeof(msg))) {
    set_error("wseg_embed_scratch_bytes: %s", msg);
    return 0;
  }
  return (size_t)plan.scratch_bytes;
}

extern "C" int wseg_embed_epochs_f64(const int64_t* indptr, const int32_t* indices, const uint32_t* rate, int64_t n, int64_t nnz, int32_t dim,
                                     const double* y_in, double* y_out, void* scratch, size_t scratch_bytes, int64_t t0, int64_t t1,
                                     int64_t total_epochs, double lr, double a, double b, double gamma, int32_t n_neg, uint64_t seed,
                                     void* stream_) {
  const char* fn = "wseg_embed_epochs_f64";
  hipStream_t stream = (hipStream_t)stream_;
  EmbedPlan plan;
  char msg[200];
  if (embed_plan(n, nnz, dim, t0, t1, total_epochs, lr, a, b, gamma, n_neg, &plan, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (n == 0) return WSEG_OK;
  if (!indptr || ((uintptr_t)indptr & 7)) { set_error("%s: indptr must be an int64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (nnz && (!indices || ((uintptr_t)indices & 3))) { set_error("%s: indices must be an int32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (nnz && (!rate || ((uintptr_t)rate & 3))) { set_error("%s: rate must be a uint32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!y_in || ((uintptr_t)y_in & 7)) { set_error("%s: y_in must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!y_out || ((uintptr_t)y_out & 7)) { set_error("%s: y_out must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < (size_t)plan.scratch_bytes) {
    set_error("%s: scratch must be an 8-byte aligned device buffer of at least %lld bytes (got %zu)", fn, (long long)plan.scratch_bytes, scratch_bytes);
    return WSEG_ERR_INVALID;
  }
  const size_t y_bytes = (size_t)n * (size_t)dim * 8;
  if (embed_overlap(y_in, y_bytes, y_out, y_bytes) || embed_overlap(y_in, y_bytes, scratch, y_bytes) || embed_overlap(y_out, y_bytes, scratch, y_bytes)) {
    set_error("%s: y_in, y_out and scratch must not overlap (an epoch reads only what the one before it wrote)", fn);
    return WSEG_ERR_INVALID;
  }
  EmbedArgs args;
  args.indptr = (const long long*)indptr;
  args.indices = (const int*)indices;
  args.rate = (const unsigned*)rate;
  args.n = n;
  args.nnz = nnz;
  args.dim = dim;
  args.n_neg = n_neg;
  args.seed_mul = (unsigned long long)seed * 0x9E3779B97F4A7C15ull;
  args.a = a;
  args.b = b;
  args.gamma = gamma;
  const bool general = b != 1.0;
  const double* from = y_in;
  for (int64_t t = t0; t < t1; ++t) {
    double* to = embed_writes(plan, t) ? y_out : static_cast<double*>(scratch);
    args.y_in = from;
    args.y_out = to;
    args.t = (unsigned long long)t;
    args.alpha = lr * (1.0 - (double)t / (double)total_epochs);
    if (general) hipLaunchKernelGGL(embed_epoch_kernel<true>, dim3((unsigned)plan.grid), dim3(kEmbedLanes), 0, stream, args);
    else hipLaunchKernelGGL(embed_epoch_kernel<false>, dim3((unsigned)plan.grid), dim3(kEmbedLanes), 0, stream, args);
    WSEG_LAUNCH_CHECK();
    from = to;
  }
  return WSEG_OK;
}

extern "C" int wseg_embed_place_f64(const int64_t* indptr, const int32_t* indices, const uint32_t* rate, const uint64_t* key, int64_t m,
                                    int64_t nnz, const double* corpus, int64_t n, int32_t dim, const double* y_in, double* y_out, int64_t t0,
                                    int64_t t1, int64_t total_epochs, double lr, double a, double b, double gamma, int32_t n_neg,
                                    void* stream_) {
  const char* fn = "wseg_embed_place_f64";
  hipStream_t stream = (hipStream_t)stream_;
  EmbedPlacePlan plan;
  char msg[200];
  if (embed_place_plan(m, nnz, n, dim, t0, t1, total_epochs, lr, a, b, gamma, n_neg, &plan, msg, sizeof(msg))) {
    set_error("%s: %s", fn, msg);
    return WSEG_ERR_INVALID;
  }
  if (m == 0) return WSEG_OK;
  if (!indptr || ((uintptr_t)indptr & 7)) { set_error("%s: indptr must be an int64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (nnz && (!indices || ((uintptr_t)indices & 3))) { set_error("%s: indices must be an int32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (nnz && (!rate || ((uintptr_t)rate & 3))) { set_error("%s: rate must be a uint32 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!key || ((uintptr_t)key & 7)) { set_error("%s: key must be a uint64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!corpus || ((uintptr_t)corpus & 7)) { set_error("%s: corpus must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!y_in || ((uintptr_t)y_in & 7)) { set_error("%s: y_in must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  if (!y_out || ((uintptr_t)y_out & 7)) { set_error("%s: y_out must be a float64 device pointer", fn); return WSEG_ERR_INVALID; }
  const size_t y_bytes = (size_t)m * (size_t)dim * 8;
  if (embed_overlap(y_out, y_bytes, y_in, y_bytes) || embed_overlap(y_out, y_bytes, corpus, (size_t)n * (size_t)dim * 8) ||
      embed_overlap(y_out, y_bytes, indptr, ((size_t)m + 1) * 8) || embed_overlap(y_out, y_bytes, key, (size_t)m * 8) ||
      embed_overlap(y_out, y_bytes, indices, (size_t)nnz * 4) || embed_overlap(y_out, y_bytes, rate, (size_t)nnz * 4)) {
    set_error("%s: y_out must not overlap y_in, corpus, indptr, indices, rate or key (lanes write it while others still read those)", fn);
    return WSEG_ERR_INVALID;
  }
  PlaceArgs args;
  args.indptr = (const long long*)indptr;
  args.indices = (const int*)indices;
  args.rate = (const unsigned*)rate;
  args.key = (const unsigned long long*)key;
  args.m = m;
  args.nnz = nnz;
  args.n = n;
  args.dim = dim;
  args.n_neg = n_neg;
  args.corpus = corpus;
  args.y_in = y_in;
  args.y_out = y_out;
  args.t0 = t0;
  args.t1 = t1;
  args.total = (double)total_epochs;
  args.lr = lr;
  args.a = a;
  args.b = b;
  args.gamma = gamma;
  if (b != 1.0) hipLaunchKernelGGL(embed_place_kernel<true>, dim3((unsigned)plan.grid), dim3(kEmbedLanes), 0, stream, args);
  else hipLaunchKernelGGL(embed_place_kernel<false>, dim3((unsigned)plan.grid), dim3(kEmbedLanes), 0, stream, args);
  WSEG_LAUNCH_CHECK();
  return WSEG_OK;
}
