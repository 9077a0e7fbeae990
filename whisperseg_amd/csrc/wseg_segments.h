// The segment table of the analyses that read a recording's resident PCM (wseg_measure.hip, wseg_patch.hip, wseg_pitch.hip), in one
// place: the validation of bounds[n_seg][2], the exclusive prefix of a per-segment item count, the table's layout on the device and
// the bisection that maps a work item to its segment.  Plain C++ with no HIP dependency (the bisection alone is __host__ __device__
// where hipcc compiles it), so that the host-only check programs (tools/*_plan_check.cpp) run all of it under a sanitizer.
// Device layout, int64:   table[n_seg][2] = (s0, s1) of every segment, then — where work items are counted per segment (measure's
// chunks, pitch's frames) — prefix[n_seg + 1], the exclusive prefix of the counts.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if defined(__HIPCC__)
#define WSEG_SEGMENTS_HD __host__ __device__ __forceinline__
#else
#define WSEG_SEGMENTS_HD inline
#endif

namespace wseg {

constexpr int64_t kSegmentMaxSamples = (int64_t)1 << 52;      // of a recording: every product and sum the three plans form stays inside int64

// bounds[n_seg][2] as the library gets them; any callable (i, &s0, &s1) is a bounds source (tools/patch_plan_check.cpp: 2^31 - 1 synthetic ones)
struct SegmentBoundsArray {
  const int64_t* p;
  void operator()(int32_t i, int64_t* s0, int64_t* s1) const { *s0 = p[2 * (int64_t)i]; *s1 = p[2 * (int64_t)i + 1]; }
};
inline bool segment_bounds_missing(const SegmentBoundsArray& b) { return !b.p; }
template <class Bounds> inline bool segment_bounds_missing(const Bounds&) { return false; }

// Validates the bounds — n_seg >= 0, an array where n_seg > 0, n <= 2^52, every segment 0 <= s0 <= s1 <= n (n < 0: no recording
// length is known, s1 <= 2^52) — and sums count(s1 - s0), the work items of a segment, which may not pass max_items (`items` is
// the caller's word for them in the message).  Where `prefix` is given (n_seg + 1 entries) it receives the exclusive prefix of
// the counts; *total their sum -> 0, or -1 with the offending argument's name in msg.
template <class Bounds, class Count>
inline int segment_prefix(Bounds bounds, int32_t n_seg, int64_t n, Count count, int64_t max_items, const char* items, int64_t* prefix,
                          int64_t* total, char* msg, size_t msg_len) {
  if (n_seg < 0) { snprintf(msg, msg_len, "n_seg is negative (%d)", (int)n_seg); return -1; }
  if (n_seg > 0 && segment_bounds_missing(bounds)) { snprintf(msg, msg_len, "bounds is null for n_seg = %d", (int)n_seg); return -1; }
  if (n > kSegmentMaxSamples) { snprintf(msg, msg_len, "n must be at most 2^52 samples (got %lld)", (long long)n); return -1; }
  const int64_t limit = n < 0 ? kSegmentMaxSamples : n;
  int64_t sum = 0;
  for (int32_t i = 0; i < n_seg; ++i) {
    int64_t s0, s1;
    bounds(i, &s0, &s1);
    if (s0 < 0 || s1 < s0 || s1 > limit) {
      snprintf(msg, msg_len, "bounds of segment %d must satisfy 0 <= s0 <= s1 <= %lld (got %lld, %lld)", (int)i, (long long)limit,
               (long long)s0, (long long)s1);
      return -1;
    }
    if (prefix) prefix[i] = sum;
    sum += count(s1 - s0);                           // at most 2^52 a segment; checked before it can pass 2^53
    if (sum > max_items) {
      snprintf(msg, msg_len, "bounds hold more than 2^40 %s up to segment %d", items, (int)i);
      return -1;
    }
  }
  if (prefix) prefix[n_seg] = sum;
  *total = sum;
  return 0;
}
// The validation alone, for an analysis whose items are not counted per segment (the patches).
template <class Bounds>
inline int segment_check(Bounds bounds, int32_t n_seg, int64_t n, char* msg, size_t msg_len) {
  int64_t none;
  return segment_prefix(bounds, n_seg, n, [](int64_t) { return (int64_t)0; }, 0, "", nullptr, &none, msg, msg_len);
}

// The device layout: entries and the writer of the host copy (n_seg >= 1; `prefix` null: the pairs alone).
inline int64_t segment_table_entries(int32_t n_seg, bool with_prefix) { return 2 * (int64_t)n_seg + (with_prefix ? (int64_t)n_seg + 1 : 0); }
inline void segment_table_fill(void* table, const int64_t* bounds, int32_t n_seg, const int64_t* prefix) {
  memcpy(table, bounds, (size_t)n_seg * 16);
  if (prefix) memcpy(static_cast<int64_t*>(table) + 2 * (size_t)n_seg, prefix, ((size_t)n_seg + 1) * 8);
}

// The segment of work item `item`, 0 <= item < prefix[n_seg] (n_seg >= 1): prefix[lo] <= item < prefix[lo + 1] — the LAST segment
// that starts at or before the item, so segments without an item (equal neighbours in the prefix) are passed over.
template <class I>
WSEG_SEGMENTS_HD int segment_of_item(const I* prefix, int n_seg, I item) {
  int lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (prefix[mid] <= item) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace wseg
