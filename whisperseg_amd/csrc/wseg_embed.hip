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

template <bool POW>
__global__ __launch_bounds__(kEmbedLanes) void embed_epoch_kernel(EmbedArgs p) {
  const bool three = p.dim == 3;
  const double two_a = -2.0 * p.a, two_gamma = 2.0 * p.gamma;
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
      {
        const double* yj = p.y_in + j * p.dim;
        const double d0 = x0 - yj[0], d1 = x1 - yj[1], d2c = three ? x2 - yj[2] : 0.0;
        double d2 = d0 * d0 + d1 * d1;
        if (three) d2 = d2 + d2c * d2c;
        if (d2 != 0.0) {               // d2 == 0: coef is 0 and the term +0 or -0, which leaves G (never -0: it began as +0) as it is
          const double P = POW ? pow(d2, p.b) : d2;
          const double coef = ((two_a * p.b) * P) / (d2 * (1.0 + p.a * P));
          g0 += embed_clip(coef * d0);
          g1 += embed_clip(coef * d1);
          if (three) g2 += embed_clip(coef * d2c);
        }
      }
      const unsigned long long c0 = (p.t * (unsigned long long)p.nnz + (unsigned long long)e) * (unsigned long long)p.n_neg;
      for (int s = 0; s < p.n_neg; ++s) {
        const unsigned long long h = embed_mix(p.seed_mul + (c0 + (unsigned long long)s));
        const long long m = (long long)(((h >> 32) * (unsigned long long)p.n) >> 32);
        if (m == i) continue;
        const double* ym = p.y_in + m * p.dim;
        const double d0 = x0 - ym[0], d1 = x1 - ym[1], d2c = three ? x2 - ym[2] : 0.0;
        double d2 = d0 * d0 + d1 * d1;
        if (three) d2 = d2 + d2c * d2c;
        const double P = POW ? pow(d2, p.b) : d2;
        const double coef = (two_gamma * p.b) / ((0.001 + d2) * (1.0 + p.a * P));
        g0 += embed_clip(coef * d0);
        g1 += embed_clip(coef * d1);
        if (three) g2 += embed_clip(coef * d2c);
      }
    }
    double* yo = p.y_out + i * p.dim;
    yo[0] = x0 + p.alpha * g0;
    yo[1] = x1 + p.alpha * g1;
    if (three) yo[2] = x2 + p.alpha * g2;
  }
}

static bool embed_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
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
  if (embed_overlap(y_in, y_out, y_bytes) || embed_overlap(y_in, scratch, y_bytes) || embed_overlap(y_out, scratch, y_bytes)) {
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
