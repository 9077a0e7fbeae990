"""The slot scheduler's policy (whisperseg_amd/csrc/wseg_sched.h) without a GPU.

wseg_debug_sched_trace runs the scheduler object wseg_generate drives against a scripted device (window i's slot reports done after
done_after[i] decode-loop steps) and returns the statistics of the call and a trace of what would be enqueued.  `replay` walks the
trace with its own model of the slots, the queue, the pool and the scripted device and asserts the conditions the scheduler promises:
every window retired once, preempted windows first in line, one owner per pool unit, the page of every assumed position in place
before a step, the victim rule, the refill rule with its cushion, the look-ahead bound, the stop rule, and the statistics."""
import ctypes as C
from collections import deque

import numpy as np
import pytest

ADMIT, ASSIGN, PREEMPT, STEP, RETIRE = 1, 2, 3, 4, 5
PAGE, RING = 8, 8
STATS = ("n_windows", "n_slots", "n_steps", "n_admissions", "slot_steps_active", "slot_steps_total", "queued_slot_steps_active",
         "queued_slot_steps_total", "kv_units_total", "kv_units_peak", "n_preemptions")


@pytest.fixture(scope="module")
def lib():
    from whisperseg_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def run_tap(lib, case):
    """-> (status, stats dict, trace [events][4])"""
    from whisperseg_amd import _lib
    n, S, units, L, npf, pos0, refill, la, done_after = case
    d = np.ascontiguousarray(done_after, dtype=np.int32)
    assert len(d) == n
    st = _lib.GenerateStats()
    n_trace = C.c_int64(0)
    args = (n, S, units, L, npf, pos0, refill, la, d.ctypes.data, C.byref(st))
    rc = lib.wseg_debug_sched_trace(*args, None, 0, C.byref(n_trace))
    if rc != 0:
        return rc, None, None
    trace = np.zeros(n_trace.value, dtype=np.int32)
    assert lib.wseg_debug_sched_trace(*args, trace.ctypes.data, trace.size, C.byref(n_trace)) == 0 and n_trace.value == trace.size
    return 0, {k: int(getattr(st, k)) for k in STATS}, trace.reshape(-1, 4).tolist()


def replay(case, stats, trace):
    """Asserts conditions 1-6 of the module docstring on one trace; returns what the case exercised."""
    n, S, units, L, npf, pos0, refill, la, done_after = case
    npg = -(-L // PAGE)
    G = refill if refill > 0 else (S // 8 if S >= 16 else 1)
    K = min(la, RING - 2) if la > 0 else 1
    win, since = [-1] * S, [0] * S              # the replay's slots: window (-1 free), first step that counts for it
    pages = [[] for _ in range(S)]              # units a slot owns, in page order
    owner = {}                                  # unit -> slot
    queue = deque(range(n))
    left, done = [0] * S, [1] * S               # the scripted device
    status, queued_at = {}, {}                  # per step: done flags it left, were windows queued when it was launched
    retired, admitted_before, preempted = [], set(), set()
    seen = dict(preemptions=0, dropped=0, hold_released=0, ended_in_pass=0, readmitted=0, oldest_preempted=0)
    hold = held_back = False
    t = consumed = peak = admissions = active_sum = q_active = q_total = 0
    ev = 0

    def take(kind, b=None):
        nonlocal ev
        out = []
        while ev < len(trace) and trace[ev][0] == kind and b in (None, trace[ev][2]):
            out.append(trace[ev][1:])
            ev += 1
        return out

    def in_flight():
        return sum(w >= 0 for w in win)

    def release(sl):
        for u in pages[sl]:
            assert owner.pop(u) == sl
        pages[sl] = []
        win[sl] = -1

    def own(pairs):
        for sl, page, u in pairs:
            assert 0 <= u < units and u not in owner, ("unit with two owners", sl, page, u)       # condition 2
            assert win[sl] >= 0 and page == len(pages[sl]) < npg
            owner[u] = sl
            pages[sl].append(u)

    def consume(u):
        nonlocal active_sum, q_active, q_total, hold
        counted = [sl for sl in range(S) if win[sl] >= 0 and u >= since[sl]]
        want = [sl for sl in counted if status[u][sl]]
        assert [(sl, uu) for sl, uu, _ in take(RETIRE, u)] == [(sl, u) for sl in want], ("retirements of step", u)
        active_sum += len(counted)
        if queued_at[u]:
            q_active += len(counted)
            q_total += S
        for sl in want:
            retired.append(win[sl])
            release(sl)
        if want:
            hold = False

    while True:
        # ---- admission: condition 5
        free_slots = [sl for sl in range(S) if win[sl] < 0]
        free_units, fl, rem = units - len(owner), in_flight(), len(queue)
        n_adm = min(rem, len(free_slots), free_units if fl == 0 else max(free_units - fl, 0))      # a unit per window + one per window in flight
        allowed = n_adm > 0 and (n_adm >= G or n_adm == rem or fl == 0)
        if allowed and hold and fl > 0:
            allowed, held_back = False, True
        adm = take(ADMIT)
        assert bool(adm) == allowed, ("admission", t, n_adm, G, rem, fl, hold)
        if adm:
            assert [a[0] for a in adm] == free_slots[:n_adm], "lowest free slots"
            assert [a[1] for a in adm] == [queue.popleft() for _ in range(n_adm)], "queue order, preempted windows first"      # condition 1
            for sl, w, _ in adm:
                seen["readmitted"] += w in preempted
                admitted_before.add(w)
                win[sl], since[sl], left[sl], done[sl] = w, t, done_after[w], int(done_after[w] <= 0)
                seen["ended_in_pass"] += done_after[w] <= 0
            if npf > 0:
                first = [trace[ev + i] for i in range(n_adm)]
                ev += n_adm
                assert [f[:3] for f in first] == [[ASSIGN, a[0], 0] for a in adm]
                own([f[1:] for f in first])
            admissions += 1
            seen["hold_released"] += held_back
            held_back = False
            peak = max(peak, len(owner))
        # ---- stop rule: condition 6
        drained = not queue
        if in_flight() == 0:
            assert drained
            break
        if drained and not any(win[sl] >= 0 and t < since[sl] + L - 1 - pos0 for sl in range(S)):
            break                                # every window in flight must have ended: no step may follow (checked after the loop)
        # ---- pages of step t: conditions 2, 3, 4
        victims, pairs = [v[0] for v in take(PREEMPT)], take(ASSIGN)
        free, tentative, vi = units - len(owner), {}, 0
        for sl in range(S):
            if win[sl] < 0:
                continue
            pos = t - since[sl] + pos0
            if pos >= L or pos % PAGE:
                continue
            while free == 0:
                assert vi < len(victims), ("a preemption is missing", t, sl)
                v = victims[vi]
                vi += 1
                holders = [x for x in range(S) if x != sl and win[x] >= 0 and (pages[x] or x in tentative)]
                assert v != sl and v in holders
                assert (since[v], v) == max((since[x], x) for x in holders), "youngest page holder, highest slot among equals"
                # never the oldest slot in flight: some other slot was admitted no later than the victim.  TODAY that has one exception
                # (a policy defect, reported with test_oldest_slot_is_preempted_when_it_is_the_only_other_page_holder and left for
                # its own change): the requester is never a candidate, so when every other page holder is older than the requester
                # the youngest of THEM goes, and when there is just one, that is the oldest slot in flight
                if not any(since[x] <= since[v] for x in range(S) if x != v and win[x] >= 0):
                    assert holders == [v]
                    seen["oldest_preempted"] += 1
                if v in tentative:               # the assignment queued for it in this pass is void
                    del tentative[v]
                    free += 1
                    seen["dropped"] += 1
                free += len(pages[v])
                queue.appendleft(win[v])
                preempted.add(win[v])
                release(v)
                done[v] = 1
                hold = True
                seen["preemptions"] += 1
            tentative[sl] = pos // PAGE
            free -= 1
        assert vi == len(victims), "a preemption nobody asked for"
        assert [p[:2] for p in pairs] == [[sl, tentative[sl]] for sl in sorted(tentative)], ("assignments of step", t)
        own(pairs)
        assert len(owner) <= units
        peak = max(peak, len(owner))
        for sl in range(S):
            pos = t - since[sl] + pos0
            if win[sl] >= 0 and pos < L:
                assert len(pages[sl]) > pos // PAGE, ("no page under the assumed position", t, sl, pos)      # condition 3
        # ---- the step
        assert ev < len(trace) and trace[ev] == [STEP, t, 0, 0]
        ev += 1
        assert t - consumed <= K, "more than `lookahead` statuses outstanding at a launch"      # condition 6
        for sl in range(S):
            if not done[sl]:
                left[sl] -= 1
                done[sl] = int(left[sl] <= 0)
        status[t], queued_at[t] = list(done), not drained
        t += 1
        while consumed < t - K:
            consume(consumed)
            consumed += 1
    while consumed < t:
        consume(consumed)
        consumed += 1
    assert ev == len(trace), "events after the end"
    assert sorted(retired) == list(range(n)), "every window retired exactly once"      # condition 1
    assert not owner and in_flight() == 0 and not queue
    want = dict(n_windows=n, n_slots=S, n_steps=t, n_admissions=admissions, slot_steps_active=active_sum, slot_steps_total=t * S,
                queued_slot_steps_active=q_active, queued_slot_steps_total=q_total, kv_units_total=units, kv_units_peak=peak,
                n_preemptions=seen["preemptions"])
    assert stats == want
    return seen


def shapes(P, L):
    """(NPF, POS0) as generate_windows resolves them: no prompt pass; the pass with the first generated step merged; the pass alone."""
    out = [(0, 0), (min(P - 1, 4),) * 2]
    if P <= 4 and L >= P + 2:
        out.append((P, P))
    return out


def random_cases():
    rng = np.random.default_rng(20240607)
    cases = []
    for i in range(160):
        L = (12, 64, 448)[i % 3]
        n = int(rng.integers(1, 301)) if i % 4 else int(rng.integers(1, 12))
        S = min(n, int(rng.integers(1, 65)))
        P = int(rng.integers(1, min(8, L - 1) + 1))
        sh = shapes(P, L)
        npf, pos0 = sh[int(rng.integers(len(sh)))]
        npg = -(-L // PAGE)
        units = (npg, S * npg, int(rng.integers(npg, S * npg + 1)), min(S * npg, npg + S))[int(rng.integers(4))]
        refill = (0, 1, S)[int(rng.integers(3))]
        la = int(rng.integers(1, 7))
        lo, hi = (0 if pos0 == P and npf == P else 1), L - 1 - pos0       # a slot ends inside the pass only if the pass runs the first step
        kind = rng.integers(0, 10, size=n)
        typical = np.minimum(rng.integers(lo, min(hi, 40) + 1, size=n), hi)
        d = np.where(kind == 0, hi, np.where(kind == 1, lo, typical))      # some run to max_length, some end at once
        if i % 7 == 0:
            d[:] = hi
        cases.append((n, S, units, L, npf, pos0, refill, la, d.astype(np.int32)))
    return cases


def hand_cases():
    c = []
    # minimum pool, several slots, every window runs to max_length: preemptions, and the victims had assignments queued (no prompt
    # pass: the first page of all slots is handed out in the same pass that runs out of units)
    c.append((12, 6, 8, 64, 0, 0, 1, 2, np.full(12, 63, np.int32)))
    # the same with the merged pass; windows ending inside the pass, at once and at max_length mixed
    c.append((20, 6, 8, 64, 3, 3, 1, 3, np.array([0, 60, 1, 0, 60, 5] * 3 + [60, 0], np.int32)))
    # a preemption holds the admissions back although slots are free, until a retirement releases them
    c.append((10, 4, 4, 28, 0, 0, 1, 1, np.array([27, 3, 27, 2, 27, 27, 1, 27, 27, 5], np.int32)))
    # look-ahead beyond the status ring and the default look-ahead / refill threshold
    c.append((40, 16, 40, 64, 2, 2, 0, 50, (np.arange(40) % 50 + 1).astype(np.int32)))
    c.append((40, 16, 40, 64, 2, 2, 0, 0, (np.arange(40) % 50 + 1).astype(np.int32)))
    # one window, one slot, the least pool, to max_length; and the prompt of 8 with the 4-position pass
    c.append((1, 1, 56, 448, 0, 0, 0, 2, np.array([447], np.int32)))
    c.append((9, 3, 9, 64, 4, 4, 3, 6, np.array([59, 1, 59, 30, 2, 59, 59, 8, 1], np.int32)))
    return c


def test_scheduler_invariants_over_scripted_cases(lib):
    total = dict(preemptions=0, dropped=0, hold_released=0, ended_in_pass=0, readmitted=0, oldest_preempted=0)
    min_pool_multi_slot = 0
    for case in hand_cases() + random_cases():
        n, S, units, L = case[:4]
        npg = -(-L // PAGE)
        assert units >= npg
        rc, stats, trace = run_tap(lib, case)
        assert rc == 0, (case[:8], lib.wseg_last_error())      # condition 8: no scheduler error with a pool of one slot's worth or more
        seen = replay(case, stats, trace)
        if units == S * npg:
            assert seen["preemptions"] == 0, case[:8]           # condition 7: a full pool never preempts
        min_pool_multi_slot += units == npg and S > 2           # ... and the least pool still completes (rc == 0 above)
        assert seen["readmitted"] >= seen["preemptions"] > -1 and (seen["preemptions"] == 0) == (seen["readmitted"] == 0)
        for k in total:
            total[k] += seen[k]
    # the case set exercises every branch
    assert total["preemptions"] > 0 and total["dropped"] > 0 and total["hold_released"] > 0 and total["ended_in_pass"] > 0, total
    assert min_pool_multi_slot > 3


def test_oldest_slot_is_preempted_when_it_is_the_only_other_page_holder(lib):
    """TODAY'S behaviour, a policy defect kept as it is by the refactor that made it visible: 2 slots, a pool of 8 units = one window
    of 64 positions.  Window 0 (slot 0, admitted at step 0) runs to max_length; window 1 ends after 7 steps and window 2 takes its
    slot at step 8.  When slot 1 later needs a page with the pool empty, the only other page holder is slot 0 — the OLDEST slot in
    flight loses its progress (the requester is never a candidate), although the header says
    the oldest window always makes progress.  The call still completes: window 0 is decoded again once window 2 has retired."""
    case = (3, 2, 8, 64, 0, 0, 1, 1, np.array([63, 7, 40], np.int32))
    rc, stats, trace = run_tap(lib, case)
    assert rc == 0 and stats["n_preemptions"] == 1
    seen = replay(case, stats, trace)
    assert seen["oldest_preempted"] == 1
    admits = [e[1:3] for e in trace if e[0] == ADMIT]
    assert [e[1] for e in trace if e[0] == PREEMPT] == [0] and admits == [[0, 0], [1, 1], [1, 2], [0, 0]]


def test_pool_smaller_than_one_window_is_an_error(lib):
    """wseg_generate never gives the scheduler less than one slot's worth of pages; handed to the tap directly, a lone window that
    runs to max_length exhausts the pool: the scheduler's own error, nothing on a device."""
    for L, units, shape in ((448, 55, (0, 0)), (64, 7, (3, 3)), (64, 1, (2, 2))):
        rc, _, _ = run_tap(lib, (1, 1, units, L) + shape + (0, 2, np.array([L - 1 - shape[1]], np.int32)))
        assert rc == -3
        assert lib.wseg_last_error() == b"self-attention K/V pool exhausted by one window (pool of %d units)" % units
    rc, stats, _ = run_tap(lib, (1, 1, 7, 64, 3, 3, 0, 2, np.array([50], np.int32)))      # ... unless it ends before the last page
    assert rc == 0 and stats["kv_units_peak"] == 7 and stats["n_preemptions"] == 0
    assert lib.wseg_debug_sched_trace(0, 1, 8, 64, 0, 0, 0, 0, None, None, None, 0, None) == -1      # bad arguments are refused


def test_sched_header_is_host_only():
    """wseg_sched.h compiles on its own with a plain C++17 compiler: standard library only, no HIP."""
    import os
    import subprocess
    from conftest import ROOT
    hdr = os.path.join(ROOT, "whisperseg_amd", "csrc", "wseg_sched.h")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", hdr])
    with open(hdr) as f:
        includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
