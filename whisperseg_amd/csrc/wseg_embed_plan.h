// The host arithmetic of the layout epochs of the 2-D / 3-D embedding (wseg_embed_scratch_bytes / wseg_embed_epochs_f64), in one
// place: the validation of a call, the grid, which buffer each epoch reads and writes, and the size of the scratch.  Plain C++ with
// no HIP dependency, so that a host-only program can run it under a sanitizer (tools/embed_plan_check.cpp, and
// tools/embed_place_plan_check.cpp for the placement of new rows at the end of this file).
//
// An epoch is ONE launch of embed_epoch_kernel: a lane per vertex, kEmbedLanes lanes a workgroup, the grid striding over the
// vertices.  Epoch t reads the positions epoch t - 1 wrote and writes others, so the epochs t0 .. t1 - 1 of a call ping-pong between
// y_out and the scratch (one more array of n * dim doubles) such that the LAST one writes y_out: epoch t0 + j writes y_out where
// t1 - 1 - (t0 + j) is even, the scratch where it is odd, and reads what epoch t0 + j - 1 wrote (j == 0: y_in).  y_in is only read,
// and never by an epoch that writes it: it must not overlap y_out or the scratch.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace wseg {

constexpr int kEmbedLanes = 64;                        // vertices of a workgroup: one wave
constexpr int kEmbedGridCap = 16384;                   // workgroups: 16 waves a SIMD; more vertices take the grid stride
constexpr int kEmbedMaxNeg = 16;                       // negative samples of an active entry
constexpr int kEmbedAlign = 256;                       // bytes
constexpr int64_t kEmbedMaxRows = INT32_MAX;           // indices are int32
constexpr int64_t kEmbedMaxNnz = (int64_t)1 << 38;     // 2 * 64 entries a row of 2^31 rows
constexpr int64_t kEmbedMaxEpochs = INT32_MAX;         // (t + 1) * rate stays below 2^48

struct EmbedPlan {
  int64_t n, nnz;
  int32_t dim;
  int64_t t0, t1, total;
  int32_t grid;                    // workgroups of an epoch, min(ceil(n / 64), cap); 0 without a vertex
  int32_t first_to_out;            // 1: epoch t0 writes y_out, 0: the scratch; then alternating, the last one y_out
  int64_t scratch_bytes;           // n * dim doubles, padded
};

inline int64_t embed_pad(int64_t bytes) { return bytes <= 0 ? kEmbedAlign : (bytes + kEmbedAlign - 1) / kEmbedAlign * kEmbedAlign; }

// finite: not NaN, not an infinity (no <cmath>: x - x is 0 exactly for finite x)
inline bool embed_finite(double x) { return x - x == 0.0; }

// Validates the sizes (wseg_embed_scratch_bytes needs no more) -> 0, or -1 with the argument's name in msg.  n == 0 is valid.
inline int embed_sizes(int64_t n, int32_t dim, EmbedPlan* plan, char* msg, size_t msg_len) {
  if (dim != 2 && dim != 3) { snprintf(msg, msg_len, "dim must be 2 or 3 (got %d)", (int)dim); return -1; }
  if (n < 0 || n > kEmbedMaxRows) { snprintf(msg, msg_len, "n must be 0 .. 2^31 - 1 (got %lld)", (long long)n); return -1; }
  plan->n = n;
  plan->dim = dim;
  plan->scratch_bytes = embed_pad(n * dim * 8);
  const int64_t groups = (n + kEmbedLanes - 1) / kEmbedLanes;
  plan->grid = (int32_t)(groups < kEmbedGridCap ? groups : kEmbedGridCap);
  return 0;
}

// Validates what a run has besides its sizes: nnz, the epochs and the parameters -> 0, or -1 with the argument's name in msg.
inline int embed_run(int64_t nnz, int64_t t0, int64_t t1, int64_t total, double lr, double a, double b, double gamma, int32_t n_neg, char* msg,
                     size_t msg_len) {
  if (nnz < 0 || nnz > kEmbedMaxNnz) { snprintf(msg, msg_len, "nnz must be 0 .. 2^38 (got %lld)", (long long)nnz); return -1; }
  if (total < 1 || total > kEmbedMaxEpochs) { snprintf(msg, msg_len, "total_epochs must be 1 .. 2^31 - 1 (got %lld)", (long long)total); return -1; }
  if (t0 < 0 || t0 >= t1 || t1 > total) {
    snprintf(msg, msg_len, "t0 < t1 must lie in 0 .. total_epochs = %lld (got %lld and %lld)", (long long)total, (long long)t0, (long long)t1);
    return -1;
  }
  if (n_neg < 0 || n_neg > kEmbedMaxNeg) { snprintf(msg, msg_len, "n_neg must be 0 .. %d (got %d)", kEmbedMaxNeg, (int)n_neg); return -1; }
  if (!embed_finite(lr)) { snprintf(msg, msg_len, "lr must be finite"); return -1; }
  if (!embed_finite(a) || a < 0) { snprintf(msg, msg_len, "a must be finite and not negative"); return -1; }
  if (!embed_finite(b) || b <= 0) { snprintf(msg, msg_len, "b must be finite and positive"); return -1; }
  if (!embed_finite(gamma)) { snprintf(msg, msg_len, "gamma must be finite"); return -1; }
  return 0;
}

// Validates a whole call and fills the plan -> 0, or -1 with the argument's name in msg.
inline int embed_plan(int64_t n, int64_t nnz, int32_t dim, int64_t t0, int64_t t1, int64_t total, double lr, double a, double b,
                      double gamma, int32_t n_neg, EmbedPlan* plan, char* msg, size_t msg_len) {
  EmbedPlan p = {};
  if (embed_sizes(n, dim, &p, msg, msg_len)) return -1;
  if (embed_run(nnz, t0, t1, total, lr, a, b, gamma, n_neg, msg, msg_len)) return -1;
  p.nnz = nnz;
  p.t0 = t0;
  p.t1 = t1;
  p.total = total;
  p.first_to_out = (int32_t)(((t1 - 1 - t0) & 1) == 0);
  *plan = p;
  return 0;
}

// where epoch t of the plan writes (1: y_out, 0: the scratch) and reads (2: y_in, 1: y_out, 0: the scratch)
inline int embed_writes(const EmbedPlan& p, int64_t t) { return (int)(((p.t1 - 1 - t) & 1) == 0); }
inline int embed_reads(const EmbedPlan& p, int64_t t) { return t == p.t0 ? 2 : embed_writes(p, t - 1); }

// ---- placing new rows on a frozen map (wseg_embed_place_f64) -----------------------------------------------------------------------
// ONE launch of embed_place_kernel runs all the epochs t0 .. t1 - 1: a lane per new row, kEmbedLanes lanes a workgroup, the grid
// striding over the m new rows.  A lane keeps its row's position in registers from y_in to y_out, so there is no ping-pong and no
// scratch.  A row holds at most kEmbedPlaceRow entries (the k of a nearest-neighbour list); entry q of a row in epoch t draws its
// negatives from the counters key + ((t * kEmbedPlaceRow + q) * kEmbedMaxNeg + s), which wrap in uint64 by design.
constexpr int kEmbedPlaceRow = 64;                     // entries of a new row that count: neighbors' largest k

struct EmbedPlacePlan {
  int64_t m, nnz, n;
  int32_t dim;
  int64_t t0, t1, total;
  int32_t grid;                    // workgroups of the launch, min(ceil(m / 64), cap); 0 without a new row: nothing is launched
};

// Validates a whole call and fills the plan -> 0, or -1 with the argument's name in msg.  The limits are embed_plan's; m == 0 is
// valid and launches nothing (n may then be 0 too), and with m > 0 the corpus holds at least one vertex: n >= 1.
inline int embed_place_plan(int64_t m, int64_t nnz, int64_t n, int32_t dim, int64_t t0, int64_t t1, int64_t total, double lr, double a,
                            double b, double gamma, int32_t n_neg, EmbedPlacePlan* plan, char* msg, size_t msg_len) {
  EmbedPlacePlan p = {};
  if (dim != 2 && dim != 3) { snprintf(msg, msg_len, "dim must be 2 or 3 (got %d)", (int)dim); return -1; }
  if (m < 0 || m > kEmbedMaxRows) { snprintf(msg, msg_len, "m must be 0 .. 2^31 - 1 (got %lld)", (long long)m); return -1; }
  if (n < (m > 0 ? 1 : 0) || n > kEmbedMaxRows) {
    snprintf(msg, msg_len, "n must be %d .. 2^31 - 1: new rows need a corpus (got %lld)", m > 0 ? 1 : 0, (long long)n);
    return -1;
  }
  if (embed_run(nnz, t0, t1, total, lr, a, b, gamma, n_neg, msg, msg_len)) return -1;
  p.m = m;
  p.nnz = nnz;
  p.n = n;
  p.dim = dim;
  p.t0 = t0;
  p.t1 = t1;
  p.total = total;
  const int64_t groups = (m + kEmbedLanes - 1) / kEmbedLanes;
  p.grid = (int32_t)(groups < kEmbedGridCap ? groups : kEmbedGridCap);
  *plan = p;
  return 0;
}

}  // namespace wseg
