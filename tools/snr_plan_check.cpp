// Host-only check of the validation and launch plans of wseg_frame_energy_f32 and wseg_snr_rows_scratch_bytes / wseg_snr_rows_f64
// (whisperseg_amd/csrc/wseg_snr_plan.h: plain C++, no HIP), over the five transform sizes, recordings from nothing to 2^40 frames
// and tables up to 2^31 - 1 rows: the arithmetic must stay inside int64 and int32, and the plans must keep what the kernels rely on.
// Build it under the host sanitizer and run it — no GPU, no library:
//
//   c++ -O1 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined tools/snr_plan_check.cpp \
//       -o snr_plan_check && ./snr_plan_check
//
// Per n_fft it fails unless: the frame count agrees with a count made another way (bisection over the frames' ends); the last
// frame ends inside the recording (read_end <= n) and one more would not; a group's span fits the staging array; the groups cover
// the frames; the grid is 1 .. cap and never more than the groups.  For rows at every structural position it compares the signal
// frames and the noise window with a second statement that looks at the frames one by one.  For tables with repeated, nested and
// overlapping windows around the split constant it checks the dedup (equal triples share a unique window, different ones do
// not, every row keeps its triple), the short / long lists, the chunk prefix, the upload's size and the scratch layout (sections
// in order, aligned, inside scratch_bytes); the layout alone at 2^31 - 1 rows, as many windows and 2^40 frames.  Every rejected
// argument must be rejected with its name.  Prints one line per n_fft.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../whisperseg_amd/csrc/wseg_snr_plan.h"

using namespace wseg;

static char msg[256];

static bool rejected(int rc, const char* word) { return rc == -1 && std::strstr(msg, word) != nullptr; }

// Whole frames of n samples: the largest J with (J - 1) hop + n_fft <= n, by bisection (another route than the header's division).
static int64_t frames_by_definition(int64_t n, int64_t n_fft) {
  const int64_t hop = n_fft / 4;
  if (n < n_fft) return 0;
  int64_t lo = 1, hi = n / hop + 2;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((__int128)(mid - 1) * hop + n_fft <= n) lo = mid; else hi = mid;
  }
  return lo;
}

// The signal frames and the window of a row, by looking at every frame (J small).
static void ranges_by_definition(int64_t s0, int64_t s1, int64_t n_fft, int64_t J, int64_t c, int64_t out[4]) {
  const int64_t hop = n_fft / 4;
  int64_t j0 = -1, j1 = -1;
  for (int64_t j = 0; j < J; ++j)
    if (s0 <= j * hop && j * hop + n_fft <= s1) { if (j0 < 0) j0 = j; j1 = j + 1; }
  if (j0 < 0) {
    const int64_t centre = (s0 + s1) / 2;
    int64_t best = -1, jb = 0;
    for (int64_t j = 0; j < J; ++j) {
      int64_t d = j * hop + n_fft / 2 - centre;
      if (d < 0) d = -d;
      if (best < 0 || d <= best) { best = d; jb = j; }
    }
    j0 = jb;
    j1 = jb + 1;
  }
  int64_t w0 = J, w1 = 0;
  for (int64_t j = 0; j < J; ++j)
    if (c < 0 || (j0 - c <= j && j < j1 + c)) { if (j < w0) w0 = j; w1 = j + 1; }
  out[0] = j0; out[1] = j1; out[2] = w0; out[3] = w1;
}

int main() {
  int bad = 0;
  for (const int32_t n_fft : {512, 1024, 2048, 4096, 8192}) {
    int fails = 0;
    const int64_t hop = n_fft / 4;
    // ---- the track
    std::vector<int64_t> lengths = {0, 1, n_fft - 1, n_fft, n_fft + 1, n_fft + hop - 1, n_fft + hop, n_fft + 15 * hop, n_fft + 16 * hop,
                                    ((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 40) - 1, (int64_t)1 << 40,
                                    (kSnrMaxFrames - 1) * hop + n_fft, (kSnrMaxFrames - 1) * hop + n_fft + hop - 1};
    for (const int64_t n : lengths) {
      for (const int64_t cap : {(int64_t)kSnrGridCap, (int64_t)1, (int64_t)3, (int64_t)1 << 40, (int64_t)0, (int64_t)-5}) {
        SnrTrackPlan p;
        if (snr_track_plan(n, n_fft, 1, n_fft / 2, cap, &p, msg, sizeof(msg))) { std::printf("  n %lld rejected: %s\n", (long long)n, msg); ++fails; continue; }
        const int64_t J = frames_by_definition(n, n_fft), top = cap < 1 ? 1 : cap > kSnrGridCap ? kSnrGridCap : cap;
        bool ok = p.frames == J && snr_frames(n, n_fft) == J && p.hop == hop && (1 << p.log2_half) == n_fft / 2 && p.group * (n_fft / 2) == kSnrFrameSlots &&
                  (1 << p.log2_group) == p.group && p.group >= 1 && p.group <= kSnrMaxGroup && kSnrLanes % p.group == 0;
        ok = ok && (p.group == 1 || (p.group - 1) * hop + n_fft <= kSnrStageFloats);
        ok = ok && p.groups * p.group >= J && (p.groups - 1) * p.group < J + (J == 0);
        ok = ok && p.read_end <= n && (J == 0 ? p.read_end == 0 : p.read_end + hop > n && p.read_end == (J - 1) * hop + n_fft);
        ok = ok && (J == 0 ? p.grid == 0 : p.grid >= 1 && p.grid <= top && p.grid <= p.groups && (p.grid == top || p.grid == p.groups));
        if (!ok) { std::printf("  a broken track plan at n %lld cap %lld\n", (long long)n, (long long)cap); ++fails; }
      }
    }
    SnrTrackPlan tp;
    if (!rejected(snr_track_plan(-1, n_fft, 1, 2, 1, &tp, msg, sizeof(msg)), "n must") ||
        !rejected(snr_track_plan(INT64_MAX, n_fft, 1, 2, 1, &tp, msg, sizeof(msg)), "n must") ||
        !rejected(snr_track_plan(kSnrMaxFrames * hop + n_fft, n_fft, 1, 2, 1, &tp, msg, sizeof(msg)), "frames") ||
        !rejected(snr_track_plan(100, n_fft - 1, 1, 2, 1, &tp, msg, sizeof(msg)), "n_fft") ||
        !rejected(snr_track_plan(100, 0, 1, 2, 1, &tp, msg, sizeof(msg)), "n_fft") ||
        !rejected(snr_track_plan(100, INT32_MIN, 1, 2, 1, &tp, msg, sizeof(msg)), "n_fft") ||
        !rejected(snr_track_plan(100, n_fft, -1, 2, 1, &tp, msg, sizeof(msg)), "k_lo") ||
        !rejected(snr_track_plan(100, n_fft, 3, 2, 1, &tp, msg, sizeof(msg)), "k_lo") ||
        !rejected(snr_track_plan(100, n_fft, 1, n_fft / 2 + 1, 1, &tp, msg, sizeof(msg)), "k_lo") ||
        !rejected(snr_track_plan(100, n_fft, INT32_MIN, INT32_MAX, 1, &tp, msg, sizeof(msg)), "k_lo") ||
        snr_track_plan(100, n_fft, 0, n_fft / 2, 1, &tp, msg, sizeof(msg)) || snr_track_plan(100, n_fft, n_fft / 2, n_fft / 2, 1, &tp, msg, sizeof(msg))) {
      std::printf("  the track's arguments are misjudged (%s)\n", msg); ++fails;
    }
    // ---- the frame ranges
    int64_t checked = 0;
    for (const int64_t n : {(int64_t)n_fft, n_fft + hop - 1, n_fft + hop, n_fft + 11 * hop + 7}) {
      const int64_t J = snr_frames(n, n_fft);
      std::vector<int64_t> marks = {0, 1, hop - 1, hop, hop + 1, n_fft - 1, (int64_t)n_fft, n_fft + 1, n / 2, n / 2 + 1, n - n_fft, n - hop, n - 1, n};
      for (const int64_t a : marks)
        for (const int64_t b : marks) {
          if (a < 0 || b < a || b > n) continue;
          for (const int64_t c : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)3, (int64_t)1 << 50}) {
            int64_t want[4], j0, j1, w0, w1;
            ranges_by_definition(a, b, n_fft, J, c, want);
            snr_signal_frames(a, b, n_fft, J, &j0, &j1);
            snr_noise_window(j0, j1, J, c, &w0, &w1);
            ++checked;
            if (j0 != want[0] || j1 != want[1] || w0 != want[2] || w1 != want[3] || !(0 <= j0 && j0 < j1 && j1 <= J && w0 <= j0 && j1 <= w1)) {
              std::printf("  n %lld row (%lld, %lld) context %lld: frames (%lld, %lld) window (%lld, %lld)\n", (long long)n, (long long)a, (long long)b,
                          (long long)c, (long long)j0, (long long)j1, (long long)w0, (long long)w1);
              ++fails;
            }
          }
        }
    }
    {                                                  // the largest recording: nothing overflows, the ranges stay inside
      const int64_t n = (kSnrMaxFrames - 1) * hop + n_fft, J = kSnrMaxFrames;
      for (const int64_t a : {(int64_t)0, n / 2, n - n_fft, n - 1, n})
        for (const int64_t b : {a, a + 1 <= n ? a + 1 : n, n}) {
          int64_t j0, j1, w0, w1;
          snr_signal_frames(a, b, n_fft, J, &j0, &j1);
          snr_noise_window(j0, j1, J, (int64_t)1 << 39, &w0, &w1);
          if (!(0 <= j0 && j0 < j1 && j1 <= J && 0 <= w0 && w0 <= j0 && j1 <= w1 && w1 <= J)) { std::printf("  a range outside 2^40 frames\n"); ++fails; }
        }
      if (snr_rank(1.0, J) != J - 1 || snr_rank(0.0, J) != 0 || snr_rank(0.5, 1) != 0 || snr_rank(0.1, 11) != 1) { std::printf("  a wrong rank\n"); ++fails; }
    }
    // ---- the rows: dedup, split and layout
    const int64_t J = 5 * (int64_t)kSnrSplit;
    const std::vector<int64_t> windows = {0, J, 7,                         // 0 long, 5 chunks
                                          0, kSnrSplit, 0,                 // 1 short: exactly the split constant
                                          0, kSnrSplit + 1, 0,             // 2 long, 2 chunks
                                          0, J, 7,                         // 3 = 0
                                          10, 20, 9,                       // 4 short, nested in 1
                                          10, 20, 8,                       // 5 another rank: another window
                                          0, kSnrSplit, 0,                 // 6 = 1
                                          15, kSnrSplit + 30, 3,           // 7 long, overlaps 1 and 2
                                          10, 20, 9};                      // 8 = 4
    const int32_t n_win = (int32_t)(windows.size() / 3);
    std::vector<int64_t> rows;
    for (int32_t i = 0; i < 40; ++i) { rows.push_back(i); rows.push_back(i + 1 + i % 3); rows.push_back(i % n_win); }
    rows.push_back(5); rows.push_back(5); rows.push_back(0);               // a row without a frame
    const int32_t n_seg = (int32_t)(rows.size() / 3);
    for (const int64_t cap : {(int64_t)kSnrGridCap, (int64_t)1, (int64_t)3, (int64_t)0}) {
      SnrRowsPlan p;
      std::vector<int64_t> table;
      if (snr_rows_plan(J, rows.data(), n_seg, windows.data(), n_win, cap, &p, &table, msg, sizeof(msg))) { std::printf("  rows rejected: %s\n", msg); ++fails; continue; }
      const int64_t top = cap < 1 ? 1 : cap;
      bool ok = p.n_unique == 6 && p.n_short == 3 && p.n_long == 3 && p.long_chunks == 5 + 2 + 2 && (int64_t)table.size() == p.table_entries &&
                p.table_entries == 3 * (int64_t)n_seg + 3 * 6 + 3 + 3 + 4 && p.table_bytes == 8 * p.table_entries;
      ok = ok && p.hist_offset >= p.table_bytes && p.hist_offset % kSnrAlign == 0 && p.hist_bytes == 3 * 4 * 256 * 8 && p.key_offset == p.hist_offset + p.hist_bytes &&
           p.key_offset % 8 == 0 && p.key_bytes == 4 * 6 && p.scratch_bytes >= p.key_offset + p.key_bytes && p.scratch_bytes % kSnrAlign == 0;
      ok = ok && p.short_grid == (3 < top ? 3 : top) && p.long_grid == (9 < top ? 9 : top) && p.finish_grid == (3 < top ? 3 : top) &&
           p.rows_grid == (n_seg < top ? n_seg : top);
      if (ok) {
        const int64_t* uwin = table.data() + 3 * (int64_t)n_seg;
        const int64_t* short_list = uwin + 3 * 6;
        const int64_t* long_list = short_list + 3;
        const int64_t* long_prefix = long_list + 3;
        for (int32_t i = 0; i < n_seg && ok; ++i) {                        // every row keeps its frames and its window's triple
          const int64_t u = table[3 * (size_t)i + 2], w = rows[3 * (size_t)i + 2];
          ok = table[3 * (size_t)i] == rows[3 * (size_t)i] && table[3 * (size_t)i + 1] == rows[3 * (size_t)i + 1] && u >= 0 && u < 6 &&
               uwin[3 * u] == windows[3 * (size_t)w] && uwin[3 * u + 1] == windows[3 * (size_t)w + 1] && uwin[3 * u + 2] == windows[3 * (size_t)w + 2];
        }
        for (int32_t u = 0; u + 1 < 6 && ok; ++u)                          // no two unique windows share a triple
          for (int32_t v = u + 1; v < 6; ++v)
            ok = ok && !(uwin[3 * u] == uwin[3 * v] && uwin[3 * u + 1] == uwin[3 * v + 1] && uwin[3 * u + 2] == uwin[3 * v + 2]);
        int seen[6] = {0, 0, 0, 0, 0, 0};
        for (int32_t s = 0; s < 3 && ok; ++s) { const int64_t u = short_list[s]; ok = u >= 0 && u < 6 && !seen[u]++ && uwin[3 * u + 1] - uwin[3 * u] <= kSnrSplit; }
        int64_t run = 0;
        for (int32_t l = 0; l < 3 && ok; ++l) {
          const int64_t u = long_list[l];
          ok = u >= 0 && u < 6 && !seen[u]++ && uwin[3 * u + 1] - uwin[3 * u] > kSnrSplit && long_prefix[l] == run;
          if (ok) {
            const int64_t len = uwin[3 * u + 1] - uwin[3 * u], chunks = (len + kSnrSplit - 1) / kSnrSplit;
            ok = (chunks - 1) * kSnrSplit < len && chunks * (int64_t)kSnrSplit >= len;      // the last chunk holds a frame, the chunks cover the window
            run += chunks;
          }
        }
        ok = ok && long_prefix[3] == run && run == p.long_chunks;
      }
      if (!ok) { std::printf("  a broken rows plan at grid cap %lld\n", (long long)cap); ++fails; }
    }
    SnrRowsPlan p;
    if (snr_rows_plan(J, nullptr, 0, nullptr, 0, kSnrGridCap, &p, nullptr, msg, sizeof(msg)) || p.rows_grid != 0 || p.n_unique != 0 ||
        p.scratch_bytes % kSnrAlign || snr_rows_plan(0, nullptr, 0, nullptr, 0, kSnrGridCap, &p, nullptr, msg, sizeof(msg))) {
      std::printf("  no rows: %s\n", msg); ++fails;
    }
    snr_rows_layout(INT32_MAX, INT32_MAX, INT32_MAX - 1000, 1000, 1000 * (kSnrMaxFrames / kSnrSplit), kSnrGridCap, &p);
    if (p.table_entries != 3 * (int64_t)INT32_MAX + 3 * (int64_t)INT32_MAX + INT32_MAX + 1001 || p.table_bytes != 8 * p.table_entries ||
        p.hist_offset < p.table_bytes || p.key_offset != p.hist_offset + (int64_t)1000 * 8192 || p.key_bytes != 4 * (int64_t)INT32_MAX ||
        p.scratch_bytes < p.key_offset + p.key_bytes || p.scratch_bytes > INT64_MAX / 2 || p.short_grid != kSnrGridCap || p.long_grid != kSnrGridCap ||
        p.finish_grid != 1000 || p.rows_grid != kSnrGridCap) {
      std::printf("  a broken layout at 2^31 - 1 rows\n"); ++fails;
    }
    {                                                  // one window over 2^40 frames: 2^27 chunks, ranks up to 2^40 - 1
      const int64_t big[3] = {0, kSnrMaxFrames, kSnrMaxFrames - 1}, row[3] = {kSnrMaxFrames - 1, kSnrMaxFrames, 0};
      if (snr_rows_plan(kSnrMaxFrames, row, 1, big, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)) || p.n_long != 1 ||
          p.long_chunks != kSnrMaxFrames / kSnrSplit || p.long_grid != kSnrGridCap) { std::printf("  2^40 frames: %s\n", msg); ++fails; }
    }
    const int64_t row[3] = {0, 2, 0}, win[3] = {0, 5, 2};
    const int64_t row_rev[3] = {2, 1, 0}, row_far[3] = {0, 6, 0}, row_neg[3] = {-1, 2, 0}, row_w[3] = {0, 2, 1}, row_wneg[3] = {0, 2, -1};
    const int64_t win_far[3] = {0, 6, 0}, win_rev[3] = {3, 2, 0}, win_r[3] = {0, 5, 5}, win_rneg[3] = {0, 5, -1}, win_empty[3] = {3, 3, 0};
    if (snr_rows_plan(5, row, 1, win, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)) ||
        !rejected(snr_rows_plan(-1, row, 1, win, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "J must") ||
        !rejected(snr_rows_plan(kSnrMaxFrames + 1, row, 1, win, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "J must") ||
        !rejected(snr_rows_plan(5, row, -1, win, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "n_seg") ||
        !rejected(snr_rows_plan(5, row, 1, win, -1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "n_win") ||
        !rejected(snr_rows_plan(5, nullptr, 1, win, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "table") ||
        !rejected(snr_rows_plan(5, row, 1, nullptr, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "windows") ||
        !rejected(snr_rows_plan(5, row_rev, 1, win, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
        !rejected(snr_rows_plan(5, row_far, 1, win, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
        !rejected(snr_rows_plan(5, row_neg, 1, win, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "bounds") ||
        !rejected(snr_rows_plan(5, row_w, 1, win, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "window of row") ||
        !rejected(snr_rows_plan(5, row_wneg, 1, win, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "window of row") ||
        !rejected(snr_rows_plan(5, row, 1, nullptr, 0, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "window of row") ||
        !rejected(snr_rows_plan(5, row, 1, win_far, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "windows") ||
        !rejected(snr_rows_plan(5, row, 1, win_rev, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "windows") ||
        !rejected(snr_rows_plan(5, row, 1, win_r, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "rank") ||
        !rejected(snr_rows_plan(5, row, 1, win_rneg, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "rank") ||
        !rejected(snr_rows_plan(5, row, 1, win_empty, 1, kSnrGridCap, &p, nullptr, msg, sizeof(msg)), "rank")) {
      std::printf("  the rows' arguments are misjudged (%s)\n", msg); ++fails;
    }
    std::printf("n_fft %4d: %zu recordings up to 2^40 frames, %lld rows' ranges, %d windows of %d rows: %s\n", (int)n_fft, lengths.size(), (long long)checked,
                (int)n_win, (int)n_seg, fails ? "FAILED" : "ok");
    bad += fails;
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
