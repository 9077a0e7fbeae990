// Slot scheduler of wseg_generate: the continuous-batching POLICY, host-only (C++ standard library, no HIP).
//
// The reference decodes batch by batch (model.py:653): a batch runs until its slowest window has finished.  Here a
// finished window's slot is retired and handed to the next queued window while the other slots keep decoding: every
// slot has its own position, every per-step kernel skips idle slots (so they cost no K/V traffic), and the captured
// step graph never changes.  Windows are independent, so the tokens of a window do not depend on which slot it ran in
// or on what ran beside it (row-independent kernels, fixed row count => fixed tile / split-K plan).
// The host runs at most `lookahead` steps ahead of the device: the per-step status mirror (done flag of every slot)
// is read behind an event, which both bounds the wasted steps after the last window finishes and tells the scheduler
// which slots to retire / refill.  The status of step u is consumed exactly when step u + lookahead has been launched,
// never "when it happens to be ready": the schedule is a deterministic function of the geometry and of the done flags.
//
// Self-attention K / V are PAGED (wseg_kernels.h): the host knows the position every occupied slot feeds at step t (t minus the
// step it was admitted at), so it hands out a pool unit whenever a slot crosses a page boundary — before the step is launched,
// through a small page-table update kernel — and takes the slot's units back when it retires.  The pool is sized for the
// expected length; when it runs short the YOUNGEST slot is preempted (aborted on the device, its window re-queued and later
// decoded again from scratch: the same tokens), so the oldest window always makes progress, and admissions keep a one-page
// cushion per window in flight and pause after a preemption until a slot retires.
//
// SlotScheduler decides; generate_windows (wseg_model.hip) enqueues what it decided.  One iteration of the driver:
//   plan_admission()  -> encoder + cross K/V + admit kernel + first pages + prompt pass for the admitted windows
//   more_steps()      -> stop?
//   plan_pages()      -> aborts of the preempted slots, then ONE page-table update
//   (the step, its status mirror)  step_launched()
//   status_due() / retire(u, flags) -> finalize the slots that step u left finished
// and after the loop status_due(true) / retire for the statuses still outstanding, then finish().
// wseg_debug_sched_trace drives the same object with a scripted device (tests/test_scheduler_cpu.py).
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <vector>

namespace wseg {

constexpr int SCHED_KV_PAGE = 8;     // positions per K/V page (== KV_PAGE of wseg_kernels.h)
constexpr int SCHED_RING = 8;        // step statuses the driver can keep in flight (entries of its pinned status ring)

// the scheduler's half of wseg_generate_stats (include/wseg.h)
struct SchedStats {
  int32_t n_steps = 0, n_admissions = 0, kv_units_peak = 0, n_preemptions = 0;
  int64_t slot_steps_active = 0, slot_steps_total = 0, queued_slot_steps_active = 0, queued_slot_steps_total = 0;
};

class SlotScheduler {
 public:
  struct Admission {
    std::vector<int> slots, wins;      // window wins[i] enters slot slots[i]
    std::vector<int> runs;             // (first i, count) of every run of consecutive window indices (a re-queued window breaks a run)
    std::vector<int> first_pages;      // NPF > 0: (page-table index, unit) of every admitted slot's first page
  };
  struct Pages {
    std::vector<int> preempt;          // slots to abort, in order
    std::vector<int> pairs;            // (page-table index, unit) pairs to write
  };

  // NPF: positions the admission's prompt pass covers (0: none, the slots step through the prompt); POS0: the position a slot is
  // at when the decode loop first steps it.  refill_min: admit once this many slots are free (0: S / 8, min 1); lookahead: steps
  // the host may run ahead of the device (0: 1; at most SCHED_RING - 2).
  SlotScheduler(int n_windows, int S, int kv_units, int L, int NPF, int POS0, int refill_min, int lookahead)
      : n_windows_(n_windows), S_(S), kv_units_(kv_units), L_(L), NPF_(NPF), POS0_(POS0),
        npg_((L + SCHED_KV_PAGE - 1) / SCHED_KV_PAGE),
        G_(refill_min > 0 ? refill_min : (S >= 16 ? S / 8 : 1)),
        K_(lookahead > 0 ? std::min(lookahead, SCHED_RING - 2) : 1),
        slot_win_(S, -1), slot_from_(S, 0), slot_units_(S) {
    for (int i = S - 1; i >= 0; --i) free_slots_.push_back(i);      // popped from the back: lowest slot first
    for (int i = kv_units - 1; i >= 0; --i) free_units_.push_back(i);
    for (int i = 0; i < n_windows; ++i) queue_.push_back(i);
  }

  bool ok() const { return err_[0] == 0; }
  const char* error() const { return err_; }
  const SchedStats& stats() const { return stats_; }
  int t() const { return t_; }                                    // steps launched so far = index of the next step
  bool started_together() const { return started_together_; }    // did the first admission take every window of the call?

  // Refill rule: enough free slots, or the rest of the queue, or nothing else is running — and a pool unit for every admitted
  // window on top of one spare unit per window in flight (16+ steps without a preemption).  nullptr: nothing to admit now.
  const Admission* plan_admission() {
    const int rem = (int)queue_.size();
    if (rem == 0 || (hold_admission_ && in_flight_ > 0)) return nullptr;
    int n = std::min(rem, (int)free_slots_.size());
    const int spare = (int)free_units_.size() - in_flight_;
    n = std::min(n, in_flight_ == 0 ? (int)free_units_.size() : std::max(spare, 0));
    if (n <= 0 || !(n >= G_ || n == rem || in_flight_ == 0)) return nullptr;
    if (stats_.n_admissions == 0) started_together_ = n == n_windows_;
    Admission& a = adm_;
    a.slots.clear(); a.wins.clear(); a.runs.clear(); a.first_pages.clear();
    for (int i = 0; i < n; ++i) {      // the first n windows of the queue into the n lowest free slots
      const int sl = free_slots_.back(); free_slots_.pop_back();
      const int w = queue_.front(); queue_.pop_front();
      a.slots.push_back(sl); a.wins.push_back(w);
      slot_win_[sl] = w; slot_from_[sl] = t_;
    }
    for (int i = 0; i < n;) {
      int j = i + 1;
      while (j < n && a.wins[j] == a.wins[j - 1] + 1) ++j;
      a.runs.push_back(i); a.runs.push_back(j - i);
      i = j;
    }
    if (NPF_ > 0) {      // the first page of every admitted slot now (the refill rule left a pool unit for each)
      for (int sl : a.slots) {
        if (free_units_.empty()) { fail("admission without a pool unit per window"); return nullptr; }
        take_unit(sl, 0, a.first_pages);
      }
      note_peak();
    }
    in_flight_ += n;
    stats_.n_admissions += 1;
    return &a;
  }

  // Is there another step to launch?  false: every window has been retired, or (nothing left to admit later) every window in flight
  // must have ended — a window admitted before step f feeds its last position, L - 2, at step f + L - 2 - POS0.
  bool more_steps() {
    drained_ = queue_.empty();
    if (in_flight_ == 0) {
      if (!drained_) fail("scheduler stalled with %d windows queued", (int)queue_.size());
      return false;
    }
    if (!drained_) return true;
    for (int sl = 0; sl < S_; ++sl)
      if (slot_win_[sl] >= 0 && t_ < slot_from_[sl] + L_ - 1 - POS0_) return true;
    return false;
  }

  // Pool units for every occupied slot that enters a new page at the step about to be launched (position t - slot_from + POS0:
  // the host's upper bound — a slot that finished inside the look-ahead window is idle on the device and simply does not use the
  // page).  When the pool is empty the youngest slot that holds pages (never the requester; among equals the highest slot) is
  // preempted: out of flight without output, its window back to the head of the queue, admissions on hold until a slot retires.
  const Pages& plan_pages() {
    Pages& p = pages_;
    p.preempt.clear(); p.pairs.clear();
    for (int sl = 0; sl < S_; ++sl) {
      if (slot_win_[sl] < 0) continue;
      const int pos = t_ - slot_from_[sl] + POS0_;
      if (pos >= L_ || pos % SCHED_KV_PAGE) continue;
      while (free_units_.empty()) {
        int victim = -1;
        for (int v = 0; v < S_; ++v)
          if (v != sl && slot_win_[v] >= 0 && !slot_units_[v].empty() && (victim < 0 || slot_from_[v] >= slot_from_[victim])) victim = v;
        if (victim < 0) { fail("self-attention K/V pool exhausted by one window (pool of %d units)", kv_units_); return p; }
        // an assignment already queued for the victim in this pass is void: drop it
        for (size_t i = 0; i + 1 < p.pairs.size();) { if (p.pairs[i] / npg_ == victim) p.pairs.erase(p.pairs.begin() + i, p.pairs.begin() + i + 2); else i += 2; }
        p.preempt.push_back(victim);
        queue_.push_front(slot_win_[victim]);
        release(victim);
        stats_.n_preemptions += 1;
        hold_admission_ = true;
      }
      take_unit(sl, pos / SCHED_KV_PAGE, p.pairs);
    }
    note_peak();
    return p;
  }

  void step_launched() {
    step_queued_[t_ % SCHED_RING] = !drained_;
    ++t_;
    stats_.slot_steps_total += S_;
  }

  // The next step whose status must be consumed now (the host stays at most `lookahead` steps ahead of the device; drain: every
  // step launched), or -1.  The caller hands that step's done flags to retire().
  int status_due(bool drain = false) { return consumed_ < (drain ? t_ : t_ - K_) ? consumed_++ : -1; }

  // done[S]: the slots' idle flags as step u left them.  Returns the slots to finalize (their windows are complete).
  const std::vector<int>& retire(int u, const int* done) {
    retired_.clear();
    int active = 0;
    for (int sl = 0; sl < S_; ++sl) {
      if (slot_win_[sl] < 0 || u < slot_from_[sl]) continue;
      if (done[sl]) retired_.push_back(sl);
      else ++active;
    }
    stats_.slot_steps_active += active + (int64_t)retired_.size();
    if (step_queued_[u % SCHED_RING]) {      // were windows still waiting in the queue when the step was launched?
      stats_.queued_slot_steps_active += active + (int64_t)retired_.size();
      stats_.queued_slot_steps_total += S_;
    }
    for (int sl : retired_) release(sl);
    if (!retired_.empty()) hold_admission_ = false;
    return retired_;
  }

  bool finish() {
    if (in_flight_ != 0 || !queue_.empty()) fail("scheduler ended with %d windows in flight, %d queued", in_flight_, (int)queue_.size());
    stats_.n_steps = t_;
    return ok();
  }

 private:
  // the slot's units back to the pool, the slot back to the free list (kept descending: the lowest slot is handed out first)
  void release(int sl) {
    slot_win_[sl] = -1;
    for (int u : slot_units_[sl]) free_units_.push_back(u);
    units_in_use_ -= (int)slot_units_[sl].size();
    slot_units_[sl].clear();
    free_slots_.insert(std::upper_bound(free_slots_.begin(), free_slots_.end(), sl, [](int a, int b) { return a > b; }), sl);
    --in_flight_;
  }
  // a free unit becomes page `page` of the slot; the (page-table index, unit) pair is queued for the device
  void take_unit(int sl, int page, std::vector<int>& pairs) {
    const int u = free_units_.back(); free_units_.pop_back();
    slot_units_[sl].push_back(u);
    ++units_in_use_;
    pairs.push_back(sl * npg_ + page); pairs.push_back(u);
  }
  // the peak counts units in use when device work is enqueued (after an admission / before a step), not inside a plan
  void note_peak() { if (units_in_use_ > stats_.kv_units_peak) stats_.kv_units_peak = units_in_use_; }
  void fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_, sizeof(err_), fmt, ap);
    va_end(ap);
  }

  const int n_windows_, S_, kv_units_, L_, NPF_, POS0_, npg_, G_, K_;
  std::vector<int> slot_win_, slot_from_;        // window in the slot (-1 = free), first step whose status counts for it (at which
                                                 // the slot is at position POS0)
  std::vector<std::vector<int>> slot_units_;     // pool units the slot holds, in page order
  std::vector<int> free_slots_, free_units_;
  std::deque<int> queue_;                        // windows waiting for a slot (preempted windows return to the front)
  int in_flight_ = 0, t_ = 0, units_in_use_ = 0, consumed_ = 0;      // statuses of steps [0, consumed) have been processed
  bool hold_admission_ = false;                  // set by a preemption, cleared by the next retirement
  bool started_together_ = false, drained_ = false;
  bool step_queued_[SCHED_RING] = {};
  SchedStats stats_;
  Admission adm_;
  Pages pages_;
  std::vector<int> retired_;
  char err_[160] = {0};
};

}  // namespace wseg
