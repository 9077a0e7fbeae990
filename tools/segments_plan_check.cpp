// Host-only check of segment_of_item (whisperseg_amd/csrc/wseg_segments.h: the bisection that maps a work item of
// measure_chunk_kernel and pitch_frame_kernel to its segment) against a linear walk of the prefix.  Build it under the host
// sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/segments_plan_check.cpp \
//       -o segments_plan_check && ./segments_plan_check
//
// Prefixes are built by segment_prefix from per-segment item counts with runs of empty segments at the start, in the middle and
// at the end, a single segment, and totals around 2^31 and 2^40; asked are item 0, the last item, both sides of every segment
// seam and, for small totals, every item.  The answer must be the one segment with prefix[s] <= item < prefix[s + 1].
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../whisperseg_amd/csrc/wseg_segments.h"

using namespace wseg;

static int64_t linear_walk(const std::vector<int64_t>& prefix, int64_t item) {
  for (size_t s = 0; s + 1 < prefix.size(); ++s)
    if (prefix[s] <= item && item < prefix[s + 1]) return (int64_t)s;
  return -1;
}

int main() {
  const int64_t two31 = (int64_t)1 << 31, two40 = (int64_t)1 << 40;
  const std::vector<std::vector<int64_t>> cases = {
      {1}, {7}, {two31 - 1}, {two31 + 1}, {two40},                                   // a single segment
      {0, 0, 0, 5, 1, 2},                                                           // empty ones at the start
      {3, 0, 0, 0, 0, 4, 0, 1},                                                     // in the middle
      {2, 9, 0, 0, 0},                                                              // at the end
      {0, 0, 1, 0, 0, 1, 0, 0},                                                     // everywhere, one item between them
      {0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0},                       // one item a segment
      {two31 - 2, 1, 0, 1, 1, 0, 5},                                                // seams around 2^31
      {0, two31, 0, two31, 3},
      {two40 - two31 - 3, 0, two31, 1, 0, 1, 1, 0},                                 // the last items at 2^40 - 1, the total 2^40
      {1, 0, two40 - 2, 0, 1, 0},
  };
  int bad = 0;
  for (size_t c = 0; c < cases.size(); ++c) {
    const std::vector<int64_t>& counts = cases[c];
    const int32_t n_seg = (int32_t)counts.size();
    std::vector<int64_t> bounds, prefix(counts.size() + 1);
    for (int64_t v : counts) { bounds.push_back(0); bounds.push_back(v); }          // a segment of v samples counts v items
    int64_t total = 0;
    char msg[256];
    int fails = 0;
    if (segment_prefix(SegmentBoundsArray{bounds.data()}, n_seg, -1, [](int64_t len) { return len; }, two40, "items", prefix.data(), &total, msg,
                       sizeof(msg)) || total != prefix.back() || prefix[0] != 0) {
      std::printf("  case %zu: %s\n", c, msg);
      ++fails;
    }
    std::vector<int64_t> items = {0, total - 1};
    for (int64_t p : prefix)
      for (int64_t d = -2; d <= 2; ++d)
        if (p + d >= 0 && p + d < total) items.push_back(p + d);
    if (total <= 4096)
      for (int64_t i = 0; i < total; ++i) items.push_back(i);
    for (int64_t item : items) {
      const int64_t want = linear_walk(prefix, item), got = segment_of_item(prefix.data(), n_seg, item);
      if (want < 0 || got != want || counts[got] == 0) {
        std::printf("  case %zu, item %lld: segment %lld, expected %lld\n", c, (long long)item, (long long)got, (long long)want);
        ++fails;
      }
    }
    std::printf("case %2zu: %d segments, %lld items, %zu asked: %s\n", c, (int)n_seg, (long long)total, items.size(), fails ? "FAILED" : "ok");
    bad += fails;
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
