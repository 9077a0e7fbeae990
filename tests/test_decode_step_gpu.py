"""The decode step's token selection on the device — log-softmax / suppression / top-Kc over the sliced vocabulary, HF's beam
bookkeeping, the greedy choice and the sampler, the retirement of finished slots — through wseg_debug_decode_step, one call per
case, against the reference's step (oracle/whisper_ref.py beam_step / greedy_step) started from the very state the device started from.

What must be EQUAL: every token, index, flag, length and position (cand_tok, tokens_in, pos, done, unsat, wmax, fin_flag, fin_len,
anc; run_seq up to the new position; fin_seq of flagged entries; the retired tokens and lengths), the state of slots that were not
stepped and every guard word bit for bit.  For a slot that the step finished only the finished side and its retired output count.

What may differ, and by how much (no figure here comes from the kernels' output): the scores.  One candidate score is
((x - max) - log(sum exp(x - max))) + running score.  The reference sums in float64 and rounds once; the kernels make one
subtraction, a sum of up to ceil(V / (256 nseg)) sequential fp32 additions per thread plus the wave (6 levels) and slice merges
(<= 10), expf and logf at 2 ulp each, one addition of the running score, and for finished scores one division:
    bound = (ceil(V / (256 nseg)) + 16) * 2^-24 + 4 * 2^-24 * max(1, |largest term|)          (decode_step_cases.score_bound)
about 2e-5 at these shapes; a finished score c / denom: bound(terms of c) / denom + 3 * 2^-24 |c / denom| (fin_bound: the error of c
divided like c itself, the division, and the float32 denominator of two pow() implementations); a stored finished score that keeps
its place is a copy and must be bit-equal.  The cases keep every decision of the
reference 8 x that bound away from flipping or make it an exact tie (decode_step_cases.settle), which leaves room for the
second-order terms; a -1e9 in the reference must be exactly -1e9 on the device.  Greedy candidates are raw logits: equal.
(Observed on an MI355X, for the record and not as a source of any tolerance: the largest difference is 0.44 of the bound for
candidate scores, 0.39 for running scores, 0.47 for finished scores — 0.18 at length_penalty -1, where the bound grows with the
length —; every test prints its own ratios.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_step_cases as D
from oracle import whisper_ref as W

pytestmark = pytest.mark.gpu

GUARD = 256           # bytes before and after every array
GUARD_BYTE = 0x5A
DTYPES = dict(pos=np.int32, done=np.int32, win=np.int32, wmax=np.int32, unsat=np.int32, tokens_in=np.int32, run_score=np.float32,
              fin_score=np.float32, fin_flag=np.int32, fin_len=np.int32, run_seq=np.int32, fin_seq=np.int32, anc=np.uint8,
              cand_val=np.float32, cand_tok=np.int32)


class Guarded:
    """A device array between guard words."""

    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        n = self.host.nbytes
        self.pad = (-n) % 256
        buf = np.full(GUARD + n + self.pad + GUARD, GUARD_BYTE, np.uint8)
        buf[GUARD:GUARD + n] = self.host.view(np.uint8).reshape(-1)
        self.dev = torch.from_numpy(buf).cuda()
        self.ptr = self.dev.data_ptr() + GUARD
        assert self.ptr % 256 == 0

    def read(self):
        """(array, guards intact)"""
        raw = self.dev.cpu().numpy()
        n = self.host.nbytes
        ok = bool((raw[:GUARD] == GUARD_BYTE).all() and (raw[GUARD + n:] == GUARD_BYTE).all())
        return raw[GUARD:GUARD + n].copy().view(self.host.dtype).reshape(self.host.shape), ok


def run_tap(lib, case, state=None, logits=None, slot_list="case", want_out=True, n_out_rows=None, expect_error=None):
    """One call of the tap.  Returns (state after, out_tokens, out_lengths, raw): raw holds what the checks on untouched memory need."""
    from whisperseg_amd import _lib
    gp, S, nb, V, kc = case.gp, case.S, case.nb, case.V, case.kc
    state = case.state if state is None else state
    slot_list = case.slot_list if slot_list == "case" else slot_list
    R, L = S * nb, gp.max_length
    arrays = {}
    for f in W.StepState.FIELDS:
        if f in ("cand_val", "cand_tok"):
            host = np.full(R * W.MAX_CAND * 4, GUARD_BYTE, np.uint8).view(DTYPES[f])
        else:
            host = getattr(state, f).astype(DTYPES[f])
        arrays[f] = Guarded(host)
    lg = Guarded(case.padded_logits() if logits is None else logits)
    sup = Guarded(np.asarray(gp.suppress_tokens or [0], np.int32))
    bsup = Guarded(np.asarray(gp.begin_suppress_tokens or [0], np.int32))
    n_out_rows = int(state.win.max()) + 1 if n_out_rows is None else n_out_rows
    out_t = Guarded(np.full((n_out_rows, L), -7, np.int32))
    out_l = Guarded(np.full(n_out_rows, -7, np.int32))
    lst = Guarded(np.asarray(slot_list if slot_list is not None else [0], np.int32))
    nbytes = lib.wseg_debug_decode_step_scratch_bytes(S, nb, V)
    assert nbytes > 0
    scratch = Guarded(np.zeros(nbytes, np.uint8))
    p = D.tap_params(gp, S, V, case.ldv, sup.ptr if gp.suppress_tokens else None, bsup.ptr if gp.begin_suppress_tokens else None)
    st = _lib.DecodeStepState(**{f: arrays[f].ptr for f in W.StepState.FIELDS})
    torch.cuda.synchronize()
    rc = lib.wseg_debug_decode_step(C.byref(p), C.byref(st), lg.ptr, lst.ptr if slot_list is not None else None,
                                    len(slot_list) if slot_list is not None else 0, scratch.ptr, nbytes,
                                    out_t.ptr if want_out else None, out_l.ptr if want_out else None, n_out_rows if want_out else 0,
                                    _lib.stream_ptr())
    if expect_error is not None:
        msg = lib.wseg_last_error().decode()
        assert rc == -1 and msg.startswith("wseg_debug_decode_step:") and expect_error in msg, (rc, msg)
    else:
        assert rc == 0, lib.wseg_last_error().decode()
    torch.cuda.synchronize()
    got, raw, guards = {}, {}, True
    for f in W.StepState.FIELDS:
        a, ok = arrays[f].read()
        guards = guards and ok
        raw[f] = a
        if f in ("cand_val", "cand_tok"):
            full = np.zeros((R, W.MAX_CAND), DTYPES[f])
            full[:, :kc] = a[:R * kc].reshape(R, kc)
            assert (a[R * kc:].view(np.uint8) == GUARD_BYTE).all(), f
            got[f] = full
        else:
            got[f] = a
    for g in (lg, sup, bsup, out_t, out_l, lst, scratch):
        guards = guards and g.read()[1]
    assert guards, "a guard word changed"
    assert np.array_equal(lg.read()[0].view(np.uint32), lg.host.view(np.uint32))
    return W.StepState(**got), out_t.read()[0], out_l.read()[0], raw


def slot_rows(nb, w):
    return slice(w * nb, (w + 1) * nb)


def close(got, want, tol):
    if np.isinf(want) or want == np.float32(-1.0e9):
        return got == want
    return abs(float(got) - float(want)) <= tol


def check_step(case, before, got, out_t, out_l, slot_list, want_out=True):
    """Steps the reference from `before` and compares the device's result with it under the rules of the module docstring."""
    gp, S, nb, V, kc, nseg = case.gp, case.S, case.nb, case.V, case.kc, case.nseg
    L = gp.max_length
    ref = before.copy()
    tr = W.StepTrace()
    fn = W.greedy_step if nb == 1 else W.beam_step
    fn(ref, case.logits, gp, slots=slot_list, trace=tr, list_form=slot_list is not None)
    stepped = [w for w in (range(S) if slot_list is None else slot_list) if not before.done[w]]
    worst = {"cand_val": 0.0, "run_score": 0.0, "fin_score": 0.0}
    for w in range(S):
        rows = slot_rows(nb, w)
        if w not in stepped:          # idle or not listed: bit-unchanged
            for f in W.StepState.FIELDS:
                a, b = getattr(got, f), getattr(before, f)
                if f in ("cand_val", "cand_tok"):
                    continue              # compared raw by the caller (the device buffer started as guard pattern)
                sel = slice(w, w + 1) if f in ("pos", "done", "win", "wmax", "unsat") else rows
                assert np.array_equal(np.asarray(a[sel]).view(np.uint8), np.asarray(b[sel]).view(np.uint8)), (case.name, w, f)
            continue
        cur_len = int(before.pos[w]) + 1
        for f in ("done", "unsat", "wmax", "win"):
            assert getattr(got, f)[w] == getattr(ref, f)[w], (case.name, w, f, getattr(got, f)[w], getattr(ref, f)[w])
        if cur_len < D.P:               # prompt phase: the forced token, nothing else
            assert got.pos[w] == ref.pos[w] and np.array_equal(got.tokens_in[rows], ref.tokens_in[rows]), (case.name, w)
            for f in ("run_score", "fin_score", "fin_flag", "fin_len", "run_seq", "fin_seq", "anc"):
                assert np.array_equal(getattr(got, f)[rows].view(np.uint8), getattr(before, f)[rows].view(np.uint8)), (case.name, w, f)
            continue
        # the finished side
        assert np.array_equal(got.fin_flag[rows], ref.fin_flag[rows]), (case.name, w, got.fin_flag[rows], ref.fin_flag[rows])
        if nb > 1 or ref.done[w]:
            assert np.array_equal(got.fin_len[rows], ref.fin_len[rows]), (case.name, w, got.fin_len[rows], ref.fin_len[rows])
        if nb > 1:
            for r in range(rows.start, rows.stop):
                if ref.fin_flag[r]:
                    n = D.P + int(ref.fin_len[r])
                    assert np.array_equal(got.fin_seq[r, :n], ref.fin_seq[r, :n]), (case.name, r)
                    scale, denom, carried = tr.largest[("fin_score", r)]
                    if carried:           # a stored score that kept a place: copied, so bit-equal
                        assert got.fin_score[r] == ref.fin_score[r], (case.name, r, got.fin_score[r], ref.fin_score[r])
                        continue
                    tol = D.fin_bound(V, nseg, scale, denom, float(ref.fin_score[r]))
                    ratio = abs(float(got.fin_score[r]) - float(ref.fin_score[r])) / tol
                    if ratio > worst["fin_score"]:
                        worst["fin_score"], worst["fin_at"] = ratio, (gp.length_penalty, float(denom), float(ref.fin_score[r]), float(got.fin_score[r]), tol)
                    assert close(got.fin_score[r], ref.fin_score[r], tol), (case.name, r, got.fin_score[r], ref.fin_score[r], tol)
                elif ref.fin_score[r] == np.float32(-1.0e9):
                    assert got.fin_score[r] == ref.fin_score[r], (case.name, r, got.fin_score[r])
        if ref.done[w]:
            if want_out:
                row = int(before.win[w])
                toks, lens = W.finalize(ref, gp, slots=[w])
                assert out_l[row] == lens[0] and np.array_equal(out_t[row], toks[0]), (case.name, w, out_t[row], toks[0])
            continue
        # the running side of a slot that goes on
        assert got.pos[w] == ref.pos[w] and np.array_equal(got.tokens_in[rows], ref.tokens_in[rows]), (case.name, w, got.tokens_in[rows], ref.tokens_in[rows])
        assert np.array_equal(got.cand_tok[rows, :kc], ref.cand_tok[rows, :kc]), (case.name, w, got.cand_tok[rows, :kc], ref.cand_tok[rows, :kc])
        assert np.array_equal(got.run_seq[rows, :cur_len + 1], ref.run_seq[rows, :cur_len + 1]), (case.name, w)
        assert np.array_equal(got.anc[rows], ref.anc[rows]), (case.name, w)
        for r in range(rows.start, rows.stop):
            for k in range(kc):
                if nb == 1:
                    assert got.cand_val[r, k] == ref.cand_val[r, k], (case.name, r, k)
                    continue
                tol = D.score_bound(V, nseg, tr.largest[("cand", r, k)])
                if np.isfinite(ref.cand_val[r, k]) and ref.cand_val[r, k] != np.float32(-1.0e9):
                    worst["cand_val"] = max(worst["cand_val"], abs(float(got.cand_val[r, k]) - float(ref.cand_val[r, k])) / tol)
                assert close(got.cand_val[r, k], ref.cand_val[r, k], tol), (case.name, r, k, got.cand_val[r, k], ref.cand_val[r, k], tol)
            if nb > 1:
                tol = D.score_bound(V, nseg, tr.largest[("run_score", r)])
                if ref.run_score[r] != np.float32(-1.0e9):
                    worst["run_score"] = max(worst["run_score"], abs(float(got.run_score[r]) - float(ref.run_score[r])) / tol)
                assert close(got.run_score[r], ref.run_score[r], tol), (case.name, r, got.run_score[r], ref.run_score[r], tol)
    if want_out:          # written only for the slots this step finished
        rows_written = {int(before.win[w]) for w in stepped if ref.done[w]}
        for row in range(out_t.shape[0]):
            if row not in rows_written:
                assert out_l[row] == -7 and (out_t[row] == -7).all(), (case.name, row)
    print("%s: largest score difference / bound: %s" % (case.name, {k: round(v, 3) if isinstance(v, float) else v for k, v in worst.items()}))
    return ref, tr


def check_untouched_candidates(case, before, raw, slot_list):
    """Candidate rows of slots that were not stepped still hold the pattern they were filled with."""
    kc = case.kc
    stepped = [w for w in (range(case.S) if slot_list is None else slot_list) if not before.done[w]]
    for w in range(case.S):
        if w not in stepped:
            for f in ("cand_val", "cand_tok"):
                a = raw[f][w * case.nb * kc:(w + 1) * case.nb * kc]
                assert (a.view(np.uint8) == GUARD_BYTE).all(), (case.name, w, f)


@pytest.mark.parametrize("name", D.CASE_NAMES)
def test_single_step(gpu_lib, name):
    case = D.get_case(name)
    got, out_t, out_l, raw = run_tap(gpu_lib, case)
    check_step(case, case.state, got, out_t, out_l, case.slot_list)
    check_untouched_candidates(case, case.state, raw, case.slot_list)


@pytest.mark.parametrize("nb,L,lp", D.LOOP_CASES)
def test_closed_loop(gpu_lib, nb, L, lp):
    """A scripted language model stepped through the tap until every slot is done; at every step the reference is stepped from the
    device's own previous state.  The retired tokens and lengths are those of the free-running reference."""
    gp, lm, caps = D.loop_params(nb, L, lp, D.LOOP_CASES.index((nb, L, lp)))
    want_t, want_l, _ = W.run_loop(lambda st, src: lm.logits(st, gp), D.LOOP_SLOTS, gp, window_max_length=caps, max_steps=32)
    state = W.new_state(D.LOOP_SLOTS, gp, window_max_length=caps)
    out_t = np.full((D.LOOP_SLOTS, L), -7, np.int32)
    out_l = np.full(D.LOOP_SLOTS, -7, np.int32)
    calls = 0
    while not state.done.all():
        case = D.Case("loop_nb%d_L%d_lp%g_step%d" % (nb, L, lp, calls), gp, D.LOOP_SLOTS, lm.V, D.align_up(lm.V, 128), lm.logits(state, gp), state)
        got, t, l, raw = run_tap(gpu_lib, case, n_out_rows=D.LOOP_SLOTS)
        check_step(case, state, got, t, l, None)
        check_untouched_candidates(case, state, raw, None)
        for row in np.flatnonzero(l != -7):
            assert out_l[row] == -7          # a slot retires once
            out_t[row], out_l[row] = t[row], l[row]
        state = got
        calls += 1
        assert calls <= 32
    assert np.array_equal(out_l, want_l) and np.array_equal(out_t, want_t), (nb, L, lp, out_l, want_l)


@pytest.mark.parametrize("nb,top_k", [(4, 1), (8, 1), (1, 1), (1, 5)])
def test_list_form_equals_full_form(gpu_lib, nb, top_k):
    """A slot stepped through `list` with its one logits row = the same slot stepped in the full form with its beam rows being copies,
    bit for bit, whether one slot is listed or all of them (in any order)."""
    S, V = 5, 1283
    for listed in ([3], [4, 0, 2, 1, 3]):
        case = D.list_case("list_nb%d_k%d_n%d" % (nb, top_k, len(listed)), S, nb, V, 1700 + nb + top_k + len(listed), listed, top_k=top_k)
        got, out_t, out_l, raw = run_tap(gpu_lib, case)
        check_step(case, case.state, got, out_t, out_l, case.slot_list)
        check_untouched_candidates(case, case.state, raw, case.slot_list)
        full = D.full_form_of(case)
        got2, out_t2, out_l2, raw2 = run_tap(gpu_lib, full, n_out_rows=out_t.shape[0])
        kc = case.kc
        for w in listed:
            for f in W.StepState.FIELDS:
                a, b = getattr(got, f), getattr(got2, f)
                sel = slice(w, w + 1) if f in ("pos", "done", "win", "wmax", "unsat") else slot_rows(nb, w)
                assert np.array_equal(np.asarray(a[sel]).view(np.uint8), np.asarray(b[sel]).view(np.uint8)), (case.name, w, f)
        assert np.array_equal(out_t, out_t2) and np.array_equal(out_l, out_l2)


@pytest.mark.parametrize("name", ["mixed_5x8_v1283", "mixed_33x4_v5003", "mixed_3x1_k16_v1283", "ties_2x3_v1283"])
def test_same_call_twice_same_bits(gpu_lib, name):
    case = D.get_case(name)
    a = run_tap(gpu_lib, case)
    b = run_tap(gpu_lib, case)
    for f in W.StepState.FIELDS:
        assert np.array_equal(a[3][f].view(np.uint8), b[3][f].view(np.uint8)), f
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def sampler_case(top_k, top_p, dead):
    """3 windows, one row each; `dead`: so many ids suppressed that the last candidates of every row have weight 0."""
    rng = np.random.default_rng(1800 + top_k)
    V = 61
    keep = [int(t) for t in rng.permutation(np.arange(D.FIRST_TOKEN, V))[:top_k - 2]]
    sup = [t for t in range(V) if t not in keep] if dead else []
    case = D.blank_case("sampler_k%d_p%g%s" % (top_k, top_p, "_dead" if dead else ""), 3, 1, V, 0, top_k=top_k, top_p=top_p, sup=sup)
    case.state = D.random_state(rng, 3, case.gp, V, t_range=(0, 6))
    case.state.win[:] = [0, 7, 1000]
    for r in range(3):
        row = D.grid(rng, V, -256, 0)
        ids = [int(t) for t in rng.permutation(np.arange(D.FIRST_TOKEN, V)) if int(t) not in sup][:top_k]
        for k, i in enumerate(ids):
            row[i] = 4.0 - k / (4.0 if top_k > 8 else 2.0) - float(rng.integers(0, 8)) / 64.0
        case.logits[r] = row
    return case


def safe_seeds(case, n):
    """The first n seeds, on the reference alone, at which no window's uniform lies within 2^-20 of a cumulative boundary."""
    seeds, s = [], 0xC0FFEE
    while len(seeds) < n:
        case.gp.seed = s
        tr = W.StepTrace()
        case.step(trace=tr)
        if not D.unsafe_decisions(tr, case.V, case.nseg):
            seeds.append(s)
        s += 0x9E3779B97F4A7C15 >> 13
        assert s < 0xC0FFEE + 4 * n * (0x9E3779B97F4A7C15 >> 13)
    return seeds


@pytest.mark.parametrize("top_k,top_p,dead", [(2, 1.0, False), (5, 0.9, False), (16, 0.5, False), (6, 0.0, False), (6, 1.0, True), (16, 2.0, True)])
def test_sampler_draws_the_reference_token(gpu_lib, top_k, top_p, dead):
    """The generator is counter-based: every draw is predictable.  64 seeds x 3 windows per setting; top_p <= 0 or >= 1 disables the
    nucleus cut; a candidate of weight 0 (a suppressed id that reached the candidate list) is never drawn."""
    case = sampler_case(top_k, top_p, dead)
    drawn, cut = set(), 0
    for seed in safe_seeds(case, 64):
        case.gp.seed = seed
        got, out_t, out_l, raw = run_tap(gpu_lib, case, want_out=False)
        tr = W.StepTrace()
        ref = case.step(trace=tr)
        cut += tr.events["sample_cut"]
        assert np.array_equal(got.tokens_in, ref.tokens_in), (seed, got.tokens_in, ref.tokens_in)
        assert np.array_equal(got.cand_tok[:, :top_k], ref.cand_tok[:, :top_k]) and np.array_equal(got.done, ref.done)
        for w in range(3):
            assert got.run_seq[w, int(case.state.pos[w]) + 1] == ref.tokens_in[w]
            assert ref.tokens_in[w] not in case.gp.suppress_tokens
            drawn.add((w, int(np.flatnonzero(ref.cand_tok[w, :top_k] == ref.tokens_in[w])[0])))
    if dead:
        assert np.isinf(ref.cand_val[:, top_k - 1]).all()
    assert len({k for _, k in drawn}) >= 2 and ((cut > 0) == (0.0 < top_p < 1.0) or dead)
    if not (0.0 < top_p < 1.0) and not dead:
        assert max(k for _, k in drawn) >= min(top_k - 1, 3)          # no cut: the tail is reachable


REFUSED_STATES = {
    "pos_at_the_end": (lambda st, L: st.pos.__setitem__(1, L - 1), None, "pos[1]"),
    "pos_negative": (lambda st, L: st.pos.__setitem__(0, -1), None, "pos[0]"),
    "win_negative": (lambda st, L: st.win.__setitem__(1, -1), None, "win[1]"),
    "win_past_the_output_rows": (lambda st, L: st.win.__setitem__(0, 4), None, "win[0]"),
    "list_entry_is_no_slot": (lambda st, L: None, [0, 2], "list[1]"),
    "list_entry_negative": (lambda st, L: None, [-1], "list[0]"),
    "list_entry_repeats": (lambda st, L: None, [1, 1], "twice"),
}


@pytest.mark.parametrize("name", sorted(REFUSED_STATES))
def test_tap_refuses_state_it_cannot_index_with(gpu_lib, name):
    """What the tap reads back before it launches anything: a position with no room left, a window outside the output rows, a list
    entry that is no slot or repeats.  The call is refused on the host and every array keeps its bits."""
    mutate, slot_list, word = REFUSED_STATES[name]
    rng = np.random.default_rng(1900)
    case = D.blank_case("refused_" + name, 2, 2, 61, 1900)
    case.state = D.random_state(rng, 2, case.gp, 61, t_range=(1, 5))
    case.state.win[:] = [0, 3]
    for r in range(4):
        case.logits[r] = D.make_row(rng, 61, case.nseg, case.kc, "one_per_slice")
    mutate(case.state, case.gp.max_length)
    got, out_t, out_l, raw = run_tap(gpu_lib, case, slot_list=slot_list, n_out_rows=4, expect_error=word)
    for f in W.StepState.FIELDS:
        if f in ("cand_val", "cand_tok"):
            assert (raw[f].view(np.uint8) == GUARD_BYTE).all(), f
        else:
            assert np.array_equal(raw[f].view(np.uint8), getattr(case.state, f).astype(DTYPES[f]).view(np.uint8)), f
    assert (out_t == -7).all() and (out_l == -7).all()
