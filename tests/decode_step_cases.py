"""Deterministic cases for the decode step's token selection (tests/test_decode_step_cpu.py, tests/test_decode_step_gpu.py): logits,
a starting state and parameters, built on the reference alone (oracle/whisper_ref.py beam_step / greedy_step).

Logits are multiples of 2^-6 inside [-8, 8] unless a case says otherwise: distinct values are far apart, equal values exactly equal.
Every case is SETTLED: each decision the reference takes in it is either determined bit for bit whatever the summation order (an
exact tie by construction, a value that rounds to -1e9, a row whose log-sum-exp is exactly its maximum), or separated by at least
MARGIN_FACTOR x the score bound.  Unconstrained random inputs miss that in about 1 comparison in 1 000, so the generators redraw a
slot's running scores (seeded) until the reference's own trace passes; a case that cannot be settled is an error when the module
builds it, never a skip.

The score bound (score_bound) follows from the operations of the kernels, not from their output: one subtraction x - max; a sum of up
to ceil(V / (256 nseg)) sequential fp32 additions per thread plus the wave (6) and slice (<= 4 + 4 + 2) merges, each 2^-24 relative
on a sum whose relative error moves log() by as much absolutely; expf and logf at 2 ulp each; one addition of the running score;
for finished scores one division:
    bound = (ceil(V / (256 nseg)) + 16) 2^-24 + 4 * 2^-24 * max(1, |largest term|)
A finished score c / denom (and the early-stop comparison's best running score / denom) carries c's error divided by denom — smaller
for a long sequence under a positive length penalty, LARGER for a negative one (denom < 1) — plus the division's rounding and an
ulp or two of the float32 denominator, on which two pow() implementations may differ:
    fin_bound = bound(largest term of c) / denom + 3 * 2^-24 |c / denom|
(where a margin is checked before c / denom is at hand, |c| <= its largest term stands in for it: a larger margin, never a smaller).
For denom >= 1 this is at most the bound above; for length_penalty -1 at 29 generated tokens it is 29 x the bound of c.
"""
import math
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import whisper_ref as W  # noqa: E402

PROMPT = [1, 2, 3]
P = 3
EOS = 5
FIRST_TOKEN = 6          # ordinary tokens are FIRST_TOKEN .. V - 1
MARGIN_FACTOR = 8.0
U = 2.0 ** -24
LENGTH_PENALTIES = (0.0, 0.6, 1.0, 2.0, -1.0)
# slots x beams, top_k: the smallest populations that reach each slice count and each candidate-list template
GEOMETRIES = ((1, 1, 1), (1, 2, 1), (2, 3, 1), (5, 8, 1), (33, 4, 1), (130, 4, 1), (600, 1, 1), (3, 1, 5), (3, 1, 16))
VOCABS = (61, 1283, 5003)
REAL_VOCAB = 51865
PLACEMENTS = ("one_stride", "one_wave", "one_per_wave", "slice_edges", "a4b4", "ends", "one_slice", "one_per_slice")


def n_slices(rows):
    return max(1, min(16, (512 + rows - 1) // rows))


def kc_of(nb, top_k):
    return (top_k if top_k > 1 else 1) if nb == 1 else 2 * nb


def kc_template(kc):
    return 1 if kc == 1 else 4 if kc <= 4 else 8 if kc <= 8 else 16


def align_up(v, a):
    return (v + a - 1) // a * a


def slice_bounds(V, nseg, s):
    """(lo, a4, b4, hi) of slice s: scalar head [lo, a4), 16-byte body [a4, b4), scalar tail [b4, hi)."""
    per = (V + nseg - 1) // nseg
    lo = s * per
    hi = min(V, lo + per)
    if hi <= lo:
        return lo, lo, lo, lo
    a4 = min(hi, (lo + 3) & ~3)
    b4 = max(a4, hi & ~3)
    return lo, a4, b4, hi


def score_bound(V, nseg, largest):
    return (math.ceil(V / (256 * nseg)) + 16) * U + 4 * U * max(1.0, abs(largest))


def fin_bound(V, nseg, largest, denom, value=None):
    """largest: the largest term of the UNDIVIDED score c; value: c / denom where it is known (else |c| <= largest stands in)."""
    d = abs(denom)
    return score_bound(V, nseg, largest) / d + 3 * U * (abs(largest) / d if value is None else abs(value))


def decision_bound(V, nseg, kind, scale, denom):
    if kind in ("finished", "early_stop"):
        return fin_bound(V, nseg, scale, min(denom, 1.0e29) if denom < 1.0e29 else 1.0)
    return score_bound(V, nseg, scale)


def unsafe_decisions(trace, V, nseg):
    """The decisions of a reference trace that are neither bit-determined nor separated by MARGIN_FACTOR x the bound."""
    bad = []
    for kind, gap, scale, denom, safe in trace.decisions:
        if safe:
            continue
        if kind == "sample":
            if gap < 2.0 ** -20:
                bad.append((kind, gap))
            continue
        if not gap >= MARGIN_FACTOR * decision_bound(V, nseg, kind, scale, denom):
            bad.append((kind, gap, scale, denom))
    return bad


def placement_kinds(V, nseg, ids):
    """Which of PLACEMENTS (and single edge positions) the winners `ids` of one row realise, from the slicing alone."""
    per = (V + nseg - 1) // nseg
    out = set()
    seg = [i // per for i in ids]
    info = []
    for i, s in zip(ids, seg):
        lo, a4, b4, hi = slice_bounds(V, nseg, s)
        if a4 <= i < b4:
            tid = ((i - a4) // 4) % 256
        elif i < a4:
            tid = (i - lo) % 256
        else:
            tid = (i - b4) % 256
        info.append((s, tid, lo, a4, b4, hi))
        for name, at in (("at_lo", lo), ("at_hi_1", hi - 1), ("at_a4_1", a4 - 1), ("at_a4", a4), ("at_b4_1", b4 - 1), ("at_b4", b4)):
            if i == at and lo <= at < hi:
                out.add(name)
        if i == 0:
            out.add("at_0")
        if i == V - 1:
            out.add("at_V_1")
    if len(ids) >= 2:
        if len(set(seg)) == 1:
            out.add("one_slice")
            if len({t for _, t, *_ in info}) == 1:
                out.add("one_stride")
                lo, a4, b4, hi = info[0][2:]
                if all(a4 <= i < b4 for i in ids):
                    out.add("one_stride_%d_groups" % len({(i - a4) // 1024 for i in ids}))
            if len({t // 64 for _, t, *_ in info}) == 1:
                out.add("one_wave")
            if len({t // 64 for _, t, *_ in info}) == min(4, len(ids)):
                out.add("one_per_wave")
        if len(set(seg)) == len(ids):
            out.add("one_per_slice")
    return out


def tie_kinds(V, nseg, ids, vals):
    """Ties among a row's winners (ids best first with their processed logits): between two slices, between two threads of a wave."""
    per = (V + nseg - 1) // nseg
    out = set()
    for k in range(len(ids) - 1):
        if vals[k] == vals[k + 1] and not np.isinf(vals[k]):
            a, b = ids[k], ids[k + 1]
            if a // per != b // per:
                out.add("tie_two_slices")
            else:
                lo, a4, b4, hi = slice_bounds(V, nseg, a // per)
                if a4 <= a < b4 and a4 <= b < b4:
                    ta, tb = ((a - a4) // 4) % 256, ((b - a4) // 4) % 256
                    if ta != tb and ta // 64 == tb // 64:
                        out.add("tie_two_threads_of_a_wave")
    return out


@dataclass
class Case:
    name: str
    gp: object
    S: int
    V: int
    ldv: int
    logits: np.ndarray            # [rows][V] float32
    state: object                 # W.StepState before the step
    slot_list: list = None        # the list form: logits hold one row per listed slot
    notes: dict = field(default_factory=dict)

    @property
    def nb(self):
        return self.gp.num_beams

    @property
    def kc(self):
        return kc_of(self.gp.num_beams, self.gp.top_k)

    @property
    def nseg(self):
        return n_slices(self.S * self.gp.num_beams)

    def step(self, state=None, trace=None):
        """The reference's step on a copy of the case's (or the given) state."""
        st = (self.state if state is None else state).copy()
        fn = W.greedy_step if self.nb == 1 else W.beam_step
        fn(st, self.logits, self.gp, slots=self.slot_list, trace=trace, list_form=self.slot_list is not None)
        return st

    def padded_logits(self):
        """[rows][ldv]: columns past the vocabulary hold 3e38, rows of idle slots NaN (neither may ever be read)."""
        out = np.full((self.logits.shape[0], self.ldv), 3.0e38, np.float32)
        out[:, :self.V] = self.logits
        if self.slot_list is None:
            for w in np.flatnonzero(self.state.done):
                out[w * self.nb:(w + 1) * self.nb] = np.nan
        return out


def grid(rng, n, lo=-512, hi=256):
    """n multiples of 2^-6 in [lo / 64, hi / 64)."""
    return (rng.integers(lo, hi, size=n) / 64.0).astype(np.float32)


def winner_positions(rng, V, nseg, kind, n):
    """n distinct ids (best first) that realise placement `kind` as far as the slicing allows; the rest are random."""
    per = (V + nseg - 1) // nseg
    live = [s for s in range(nseg) if slice_bounds(V, nseg, s)[3] > slice_bounds(V, nseg, s)[0]]
    s = int(rng.choice(live))
    lo, a4, b4, hi = slice_bounds(V, nseg, s)
    ids = []
    if kind == "one_stride":
        t = int(rng.integers(0, 256))
        ids = [a4 + 4 * t + 1024 * k + int(rng.integers(0, 4)) for k in range(n)] + [a4 + 4 * t + k for k in range(4)]
    elif kind == "one_wave":
        wv = int(rng.integers(0, 4))
        ids = [a4 + 256 * wv + int(x) for x in rng.permutation(256)[:n]]
    elif kind == "one_per_wave":
        ids = [a4 + 256 * (k % 4) + 1024 * (k // 4) + int(rng.integers(0, 256)) for k in range(n)]
    elif kind == "slice_edges":
        for q in rng.permutation(live):
            l2, _, _, h2 = slice_bounds(V, nseg, int(q))
            ids += [l2, h2 - 1]
    elif kind == "a4b4":
        ids = [a4 - 1, a4, b4 - 1, b4]
        for q in rng.permutation(live):
            l2, x4, y4, h2 = slice_bounds(V, nseg, int(q))
            ids += [x4 - 1, x4, y4 - 1, y4]
    elif kind == "ends":
        ids = [0, V - 1, 1, V - 2]
    elif kind == "one_slice":
        ids = [lo + int(x) for x in rng.permutation(hi - lo)[:n]]
    elif kind == "one_per_slice":
        ids = [slice_bounds(V, nseg, int(q))[0] + int(rng.integers(0, slice_bounds(V, nseg, int(q))[3] - slice_bounds(V, nseg, int(q))[0]))
               for q in rng.permutation(live)]
    if kind in ("one_stride", "one_wave", "one_per_wave", "one_slice"):
        ids = [i for i in ids if lo <= i < hi]
    out = []
    for i in ids:
        if 0 <= i < V and i != EOS and i not in out:
            out.append(int(i))
    while len(out) < n:
        i = int(rng.integers(FIRST_TOKEN, V))
        if i not in out:
            out.append(i)
    return out[:n]


def make_row(rng, V, nseg, kc, kind):
    """A row whose kc + 1 best are the designated winners: 8, 8 - 1/8, ... (distinct), background below 4."""
    row = grid(rng, V)
    ids = winner_positions(rng, V, nseg, kind, kc + 1)
    for k, i in enumerate(ids):
        row[i] = 8.0 - k / 8.0
    row[EOS] = min(row[EOS], 0.0)
    return row


def random_state(rng, S, gp, V, t_range=None):
    """Slots in the middle of decoding: random histories, ancestry, running and finished scores (finished lists sorted as a merge
    leaves them)."""
    nb, L = gp.num_beams, gp.max_length
    st = W.new_state(S, gp)
    for w in range(S):
        lo_t, hi_t = t_range if t_range is not None else (0, L - P - 2)
        t = int(rng.integers(lo_t, hi_t + 1))
        cur_len = P + t
        st.pos[w] = cur_len - 1
        st.win[w] = int(rng.integers(0, 3 * S))
        rows = slice(w * nb, (w + 1) * nb)
        st.run_seq[rows, P:cur_len] = rng.integers(FIRST_TOKEN, V, size=(nb, t))
        st.anc[rows, :cur_len] = rng.integers(0, nb, size=(nb, cur_len))
        st.tokens_in[rows] = st.run_seq[rows, cur_len - 1]
        if nb > 1 and t > 0:
            st.run_score[rows] = -np.sort(rng.uniform(0.2, 6.0, nb)).astype(np.float32)
            n_f = int(rng.integers(0, nb + 1))
            fs = np.full(nb, -1.0e9, np.float32)
            fs[:n_f] = -np.sort(rng.uniform(0.05, 3.0, n_f)).astype(np.float32)
            st.fin_score[rows] = fs
            st.fin_flag[rows] = (np.arange(nb) < n_f)
            for j in range(n_f):
                fl = int(rng.integers(1, t + 1))
                st.fin_len[w * nb + j] = fl
                st.fin_seq[w * nb + j, P:P + fl] = rng.integers(FIRST_TOKEN, V, size=fl)
                st.fin_seq[w * nb + j, P + fl - 1] = EOS
    st.win[:] = rng.permutation(3 * S)[:S]
    return st


FLAVOURS = ("plain", "eos_best_beam", "eos_all_rows", "eos_last_beam", "cap", "finished_strong", "finished_weak", "first_step",
            "cap_first_step", "prompt_phase", "unsat_0", "twins")


def dress_slot(rng, case, w, flavour, kind=None):
    """Draws the logits rows and the state of slot w for a flavour (what makes each beam event likely; the reference's trace says
    whether it happened)."""
    gp, V, nb, st = case.gp, case.V, case.nb, case.state
    L = gp.max_length
    rows = range(w * nb, (w + 1) * nb)
    one = random_state(rng, 1, gp, V, t_range=(1, L - P - 2))
    if flavour in ("first_step", "cap_first_step"):
        one = W.new_state(1, gp)
    if flavour == "prompt_phase":
        one = W.new_state(1, gp, pos=P - 2)
    for f in W.StepState.FIELDS:
        if f in ("cand_val", "cand_tok", "win"):
            continue
        a, b = getattr(st, f), getattr(one, f)
        if a.shape[0] == case.S:
            a[w] = b[0]
        else:
            a[w * nb:(w + 1) * nb] = b
    cur_len = int(st.pos[w]) + 1
    for j, r in enumerate(rows):
        case.logits[r] = make_row(rng, V, case.nseg, case.kc, kind or PLACEMENTS[int(rng.integers(0, len(PLACEMENTS)))])
    if nb > 1 and flavour not in ("first_step", "cap_first_step", "prompt_phase"):
        redraw_scores(rng, case, w, spread={"eos_all_rows": 0.3, "eos_last_beam": 1.0}.get(flavour, 6.0))
    if flavour == "eos_best_beam":
        case.logits[w * nb, EOS] = 8.5
    elif flavour == "eos_all_rows":
        for r in rows:
            case.logits[r, EOS] = 12.0
    elif flavour == "eos_last_beam":
        case.logits[w * nb + int(rng.integers(0, nb)), EOS] = 8.0 - float(rng.integers(0, 4)) / 8.0 - 1.0 / 16.0
    elif flavour in ("cap", "cap_first_step"):
        st.wmax[w] = cur_len + 1
    elif flavour == "finished_strong":          # every finished slot taken by a good score, the running beams poor
        st.fin_score[w * nb:(w + 1) * nb] = -np.sort(rng.uniform(0.01, 0.05, nb)).astype(np.float32)
        st.fin_flag[w * nb:(w + 1) * nb] = 1
        st.fin_len[w * nb:(w + 1) * nb] = 1
        st.run_score[w * nb:(w + 1) * nb] = -np.sort(rng.uniform(20.0, 25.0, nb)).astype(np.float32)
    elif flavour == "finished_weak":            # a poor finished score that a running beam can still beat
        st.fin_score[w * nb] = np.float32(-rng.uniform(30.0, 40.0))
        st.fin_score[w * nb + 1:(w + 1) * nb] = -1.0e9
        st.fin_flag[w * nb:(w + 1) * nb] = np.arange(nb) < 1
        st.fin_len[w * nb] = 1
    elif flavour == "unsat_0":
        st.unsat[w] = 0
        case.logits[w * nb, EOS] = 8.5
    elif flavour == "twins" and nb > 1:         # bit-equal rows and bit-equal running scores: broken by the beam index alone
        case.logits[w * nb + 1] = case.logits[w * nb]
        st.run_score[w * nb + 1] = st.run_score[w * nb]


def redraw_scores(rng, case, w, spread=6.0):
    nb, st = case.nb, case.state
    if nb > 1 and int(st.pos[w]) + 1 > P:
        s = -np.sort(rng.uniform(0.2, 0.2 + spread, nb)).astype(np.float32)
        twin = st.run_score[w * nb + 1] == st.run_score[w * nb] and np.array_equal(case.logits[w * nb + 1], case.logits[w * nb])
        st.run_score[w * nb:(w + 1) * nb] = s
        if twin:
            st.run_score[w * nb + 1] = s[0]


def slot_trace(case, w):
    tr = W.StepTrace()
    st = case.state.copy()
    fn = W.greedy_step if case.nb == 1 else W.beam_step
    if case.slot_list is None:
        fn(st, case.logits, case.gp, slots=[w], trace=tr)
    else:
        li = case.slot_list.index(w)
        fn(st, case.logits[li:li + 1], case.gp, slots=[w], trace=tr, list_form=True)
    return tr


def settle(rng, case, slots=None, want=None, flavour=None, fixed=()):
    """Redraws (seeded) what is free in each slot until the reference's trace of the slot is safe and, with `want`, shows the event.
    Slots in `fixed` are constructions that must be safe as they stand."""
    for w in (range(case.S) if slots is None else slots):
        if case.state.done[w]:
            continue
        for attempt in range(400):
            tr = slot_trace(case, w)
            ok = not unsafe_decisions(tr, case.V, case.nseg) and (want is None or tr.events[want] > 0)
            if ok:
                break
            assert w not in fixed, (case.name, w, unsafe_decisions(tr, case.V, case.nseg), dict(tr.events))
            if want is not None:
                dress_slot(rng, case, w, flavour)
            else:
                redraw_scores(rng, case, w)
        else:
            raise AssertionError("case %s: slot %d cannot be settled (%s)" % (case.name, w, want))


def make_gp(nb, L, lp=1.0, top_k=1, top_p=1.0, seed=0, sup=(), bsup=()):
    return W.GenParams(prompt=list(PROMPT), eos_token_id=EOS, pad_token_id=EOS, max_length=L, num_beams=nb, length_penalty=lp,
                       suppress_tokens=list(sup), begin_suppress_tokens=list(bsup), top_k=top_k, top_p=top_p, seed=seed)


def settle_seed(case):
    """Sampling: the first seed from the case's own at which no slot's uniform lies within 2^-20 of a cumulative boundary."""
    if case.nb != 1 or case.gp.top_k <= 1:
        return
    for k in range(1000):
        tr = W.StepTrace()
        case.step(trace=tr)
        if not unsafe_decisions(tr, case.V, case.nseg):
            return
        case.gp.seed += 1
    raise AssertionError("case %s: no seed clears the boundaries" % case.name)


def blank_case(name, S, nb, V, seed, L=24, lp=1.0, top_k=1, top_p=1.0, ldv=None, sup=(), bsup=()):
    gp = make_gp(nb, L, lp, top_k, top_p, seed=0x5EED0000 + seed, sup=sup, bsup=bsup)
    return Case(name, gp, S, V, ldv or align_up(V, 128), np.zeros((S * nb, V), np.float32), W.new_state(S, gp))


def mixed_case(name, S, nb, V, seed, top_k=1, top_p=1.0, lp=1.0, L=24, ldv=None, sup=(), bsup=(), idle=True):
    """Every slot draws a flavour and every row a placement; the last slot of a population of several is idle."""
    rng = np.random.default_rng(seed)
    case = blank_case(name, S, nb, V, seed, L, lp, top_k, top_p, ldv, sup, bsup)
    case.state = random_state(rng, S, case.gp, V)
    flavours = ("plain", "plain", "eos_best_beam", "eos_all_rows", "eos_last_beam", "cap", "finished_strong", "finished_weak",
                "first_step", "twins")
    for w in range(S):
        dress_slot(rng, case, w, flavours[(w + seed) % len(flavours)], kind=None if S * nb > 4 else PLACEMENTS[(seed + w) % len(PLACEMENTS)])
    if idle and S > 1:
        case.state.done[S - 1] = 1
    settle(rng, case)
    settle_seed(case)
    return case


def event_case(name, nb, V, seed, lp):
    """One crafted slot per beam event; the reference's trace confirms each."""
    rng = np.random.default_rng(seed)
    plan = (("eos_rank_ge_nb_only", "eos_last_beam"), ("eos_rank_0", "eos_best_beam"), ("eos_in_nb_rows", "eos_all_rows"),
            ("several_finish", "eos_all_rows"), ("cap_hit", "cap"), ("cap_at_first_step", "cap_first_step"),
            ("prompt_phase", "prompt_phase"), ("unsat_already_0", "unsat_0"), ("early_stop_improves", "finished_weak"),
            ("early_stop_stops", "finished_strong"), ("tie_two_beams", "twins"))
    case = blank_case(name, len(plan), nb, V, seed, lp=lp)
    for w, (want, flavour) in enumerate(plan):
        dress_slot(rng, case, w, flavour)
        settle(rng, case, slots=[w], want=want, flavour=flavour)
    case.notes["events"] = [p[0] for p in plan]
    return case


def tie_case(name, S, nb, V, seed, top_k=1):
    """Equal maxima in two slices (rows 0 mod 3), in two threads of one wave (1 mod 3), three equal values around a slice edge (2 mod 3);
    with beams, slot 0's beams are twins."""
    rng = np.random.default_rng(seed)
    case = blank_case(name, S, nb, V, seed, top_k=top_k)
    case.state = random_state(rng, S, case.gp, V, t_range=(1, 10))
    nseg, kc = case.nseg, case.kc
    per = (V + nseg - 1) // nseg
    for r in range(S * nb):
        row = grid(rng, V)
        row[EOS] = -8.0
        if r % 3 == 0 and nseg > 1:
            a, b = FIRST_TOKEN + int(rng.integers(0, per - FIRST_TOKEN)), per * (nseg // 2) + int(rng.integers(0, per // 2))
        elif r % 3 == 1:
            _, a4, _, _ = slice_bounds(V, nseg, 0)
            a = max(FIRST_TOKEN, a4 + 4 * int(rng.integers(2, 30)))
            b = a + 4 * int(rng.integers(1, 20))
        else:
            a, b = per - 1 if nseg > 1 and per > FIRST_TOKEN else V - 2, per if nseg > 1 and per > FIRST_TOKEN else V - 1
        # the tied pair at every rank down the list: the first, the kc-th | (kc + 1)-th boundary, and in between
        vals = [8.0 - k / 8.0 for k in range(kc + 2)]
        tie_at = r % max(1, kc)
        ids = winner_positions(rng, V, nseg, "one_per_slice", kc + 2)
        ids = [i for i in ids if i not in (a, b)][:kc]
        row[a] = row[b] = vals[tie_at]
        others = [v for k, v in enumerate(vals) if k != tie_at]
        for i, v in zip(ids, others):
            row[i] = v
        case.logits[r] = row
    if nb > 1:
        case.logits[1] = case.logits[0]
        case.state.run_score[1] = case.state.run_score[0]
    settle(rng, case)
    settle_seed(case)
    return case


def finished_tie_case(name, nb, V, seed):
    """A new finished candidate whose score equals a stored one bit for bit: beam 0's row is dominated by EOS (everything else 60
    below, so its log-softmax is exactly 0 in any summation order), length_penalty 0 (denominator 1), and the stored score is
    beam 0's running score.  The stored one keeps its place ("already finished before new")."""
    rng = np.random.default_rng(seed)
    case = blank_case(name, 2, nb, V, seed, lp=0.0)
    case.state = random_state(rng, 2, case.gp, V, t_range=(2, 10))
    for w in range(2):
        for r in range(w * nb, (w + 1) * nb):
            case.logits[r] = make_row(rng, V, case.nseg, case.kc, "one_per_slice")
        redraw_scores(rng, case, w)
        case.logits[w * nb] = grid(rng, V) - 60.0
        case.logits[w * nb, EOS] = 8.0
        st = case.state
        st.fin_score[w * nb:(w + 1) * nb] = -1.0e9
        st.fin_flag[w * nb:(w + 1) * nb] = 0
        st.fin_score[w * nb] = st.run_score[w * nb]
        st.fin_flag[w * nb] = 1
        st.fin_len[w * nb] = 2
        st.fin_seq[w * nb, P:] = EOS
        st.fin_seq[w * nb, P] = FIRST_TOKEN + w
    for w in range(2):
        for attempt in range(400):
            if not unsafe_decisions(slot_trace(case, w), case.V, case.nseg):
                break
            redraw_scores(rng, case, w)
            case.state.fin_score[w * nb] = case.state.run_score[w * nb]
        else:
            raise AssertionError("case %s cannot be settled" % name)
    tr = W.StepTrace()
    case.step(trace=tr)
    assert tr.events["tie_finished_scores"] >= 2, dict(tr.events)
    return case


def suppress_case(name, S, nb, V, seed, first_step, top_k=1):
    """The row maximum suppressed; four suppressed ids in one aligned group; an id in both lists; ids outside the vocabulary;
    EOS in the begin list (the row's second best: banned at the first generated step, allowed at the next)."""
    rng = np.random.default_rng(seed)
    g = 4 * int(rng.integers(4, V // 4 - 1))
    sup = [g, g + 1, g + 2, g + 3, FIRST_TOKEN + 1, V, V + 7, -1, -V]
    bsup = [EOS, FIRST_TOKEN + 1, V + 1, -3]
    case = blank_case(name, S, nb, V, seed, top_k=top_k, sup=sup, bsup=bsup)
    case.state = W.new_state(S, case.gp) if first_step else random_state(rng, S, case.gp, V, t_range=(1, 1))
    for w in range(S):
        for r in range(w * nb, (w + 1) * nb):
            row = make_row(rng, V, case.nseg, case.kc + 3, "one_per_slice")
            row[g + r % 4] = 9.0                # the row maximum is suppressed
            row[FIRST_TOKEN + 1] = 8.75
            row[EOS] = 8.5
            case.logits[r] = row
        if not first_step:
            redraw_scores(rng, case, w)
    settle(rng, case)
    settle_seed(case)
    return case


def range_case(name, S, nb, V, seed, top_k=1):
    """Rows shifted by +100 and by -100 (an unshifted exp overflows / flushes to 0), and rows whose maximum sits in one slice
    while every other slice is 60 below it."""
    rng = np.random.default_rng(seed)
    case = blank_case(name, S, nb, V, seed, top_k=top_k)
    case.state = random_state(rng, S, case.gp, V, t_range=(1, 10))
    nseg = case.nseg
    per = (V + nseg - 1) // nseg
    for r in range(S * nb):
        row = make_row(rng, V, nseg, case.kc, PLACEMENTS[r % len(PLACEMENTS)])
        if r % 3 == 0:
            row = row + np.float32(100.0)
        elif r % 3 == 1:
            row = row - np.float32(100.0)
        elif nseg > 1:
            s = int(np.argmax(row)) // per
            keep = np.zeros(V, bool)
            keep[s * per:(s + 1) * per] = True
            row = np.where(keep, row, row - np.float32(60.0))
        case.logits[r] = row
    settle(rng, case)
    settle_seed(case)
    return case


def list_case(name, S, nb, V, seed, listed, top_k=1):
    """The admission's form: freshly admitted slots `listed`, one logits row each; the other slots hold mid-decode state."""
    rng = np.random.default_rng(seed)
    case = blank_case(name, S, nb, V, seed, top_k=top_k)
    case.state = random_state(rng, S, case.gp, V)
    fresh = W.new_state(S, case.gp)
    for f in W.StepState.FIELDS:
        if f in ("win", "cand_val", "cand_tok"):
            continue
        a, b = getattr(case.state, f), getattr(fresh, f)
        for w in listed:
            if a.shape[0] == S:
                a[w] = b[w]
            else:
                a[w * nb:(w + 1) * nb] = b[w * nb:(w + 1) * nb]
    case.slot_list = list(listed)
    case.logits = np.stack([make_row(rng, V, case.nseg, case.kc, PLACEMENTS[(seed + i) % len(PLACEMENTS)]) for i in range(len(listed))])
    settle(rng, case, slots=listed)
    settle_seed(case)
    return case


def full_form_of(case):
    """The same slots stepped in the full form: every beam row of a listed slot is a copy of its one row, the other slots idle."""
    full = Case(case.name + "/full", case.gp, case.S, case.V, case.ldv, np.zeros((case.S * case.nb, case.V), np.float32), case.state.copy())
    full.state.done[:] = 1
    for i, w in enumerate(case.slot_list):
        full.state.done[w] = case.state.done[w]
        full.logits[w * case.nb:(w + 1) * case.nb] = case.logits[i]
    return full


_CACHE = {}


def single_step_cases():
    """name -> builder.  Cases are built on demand and kept: the references are computed once and shared."""
    b = {}
    n = 0
    for S, nb, top_k in GEOMETRIES:
        vocabs = VOCABS + ((REAL_VOCAB,) if S * nb <= 3 else ())
        for V in vocabs:
            if V < kc_of(nb, top_k) + 8:
                continue
            n += 1
            lp = LENGTH_PENALTIES[n % len(LENGTH_PENALTIES)]
            top_p = (1.0, 0.9, 0.5, 0.0)[n % 4]
            tag = "mixed_%dx%d%s_v%d" % (S, nb, "_k%d" % top_k if top_k > 1 else "", V)
            b[tag] = (mixed_case, (tag, S, nb, V, 1000 + n), dict(top_k=top_k, top_p=top_p, lp=lp))
    b["mixed_2x3_v1283_ldv4"] = (mixed_case, ("mixed_2x3_v1283_ldv4", 2, 3, 1283, 1100), dict(ldv=align_up(1283, 4)))
    for i, lp in enumerate(LENGTH_PENALTIES):
        for nb in (2, 4):
            tag = "events_nb%d_lp%g" % (nb, lp)
            b[tag] = (event_case, (tag, nb, 61 if nb == 2 else 1283, 1200 + 10 * i + nb, lp), {})
    b["events_nb8_lp0.6"] = (event_case, ("events_nb8_lp0.6", 8, 1283, 1290, 0.6), {})
    for S, nb, top_k, V in ((2, 3, 1, 1283), (5, 8, 1, 1283), (33, 4, 1, 5003), (1, 1, 1, 1283), (3, 1, 5, 5003), (3, 1, 16, 1283), (130, 4, 1, 1283),
                            (1, 2, 1, REAL_VOCAB)):
        tag = "ties_%dx%d%s_v%d" % (S, nb, "_k%d" % top_k if top_k > 1 else "", V)
        b[tag] = (tie_case, (tag, S, nb, V, 1300 + S + nb + top_k), dict(top_k=top_k))
    for nb in (2, 4):
        b["finished_tie_nb%d" % nb] = (finished_tie_case, ("finished_tie_nb%d" % nb, nb, 1283, 1400 + nb), {})
    for S, nb, top_k, V in ((2, 3, 1, 1283), (5, 8, 1, 61), (3, 1, 1, 5003), (3, 1, 5, 1283)):
        for first in (True, False):
            tag = "suppress_%dx%d%s_v%d_%s" % (S, nb, "_k%d" % top_k if top_k > 1 else "", V, "first" if first else "second")
            b[tag] = (suppress_case, (tag, S, nb, V, 1500 + S + nb + top_k, first), dict(top_k=top_k))
    for S, nb, top_k, V in ((2, 3, 1, 1283), (5, 8, 1, 5003), (130, 4, 1, 1283), (3, 1, 16, 5003), (1, 1, 1, REAL_VOCAB)):
        tag = "range_%dx%d%s_v%d" % (S, nb, "_k%d" % top_k if top_k > 1 else "", V)
        b[tag] = (range_case, (tag, S, nb, V, 1600 + S + nb + top_k), dict(top_k=top_k))
    return b


def get_case(name):
    if name not in _CACHE:
        fn, args, kw = single_step_cases()[name]
        _CACHE[name] = fn(*args, **kw)
    return _CACHE[name]


CASE_NAMES = sorted(single_step_cases())


# ---- closed loops: a scripted "language model" ----------------------------------------------------------------------------------------
class ScriptedLM:
    """(window, last token, position) -> a logits row from a host table; EOS is made likely at a few positions.  `salt` moves the rows
    of one (window, position): loop_params uses it to redraw a slot's step until the reference's decisions in it are safe."""

    def __init__(self, V, seed, n_rows=64):
        rng = np.random.default_rng(seed)
        self.V = V
        self.table = np.stack([grid(rng, V, -512, 513) for _ in range(n_rows)])
        self.table[:, EOS] = -8.0
        self.eos_rows = set(int(x) for x in rng.permutation(n_rows)[:n_rows // 10])
        for r in self.eos_rows:
            self.table[r, EOS] = 8.0 + float(rng.integers(0, 64)) / 64.0
        self.jitter = [int(x) | 1 for x in rng.integers(0, 1 << 30, size=3)]
        self.salt = {}

    def row_index(self, window, token, position):
        return (window * self.jitter[0] + token * self.jitter[1] + position * self.jitter[2]
                + self.salt.get((window, position), 0) * 104729) % self.table.shape[0]

    def logits(self, state, gp):
        nb = gp.num_beams
        out = np.zeros((state.tokens_in.shape[0], self.V), np.float32)
        for r in range(out.shape[0]):
            w = r // nb
            out[r] = self.table[self.row_index(int(state.win[w]), int(state.tokens_in[r]), int(state.pos[w]))]
        return out


LOOP_SLOTS = 4


def loop_params(nb, L, lp, seed):
    """A closed loop whose every reference decision is safe on the free-running reference: wherever a slot's step is not, the
    scripted model's rows for that (window, position) are redrawn.  Returns (gp, lm, window caps)."""
    caps = [L, P + 1, L, max(P + 1, L - 5)]
    gp = make_gp(nb, L, lp)
    gp.window_max_length = caps
    lm = ScriptedLM(61 if nb < 8 else 131, 7000 + seed)
    state = W.new_state(LOOP_SLOTS, gp, window_max_length=caps)
    step = W.greedy_step if nb == 1 else W.beam_step
    nseg = n_slices(LOOP_SLOTS * nb)
    while not state.done.all():
        for w in np.flatnonzero(state.done == 0):
            for salt in range(400):
                lm.salt[(int(state.win[w]), int(state.pos[w]))] = salt
                tr = W.StepTrace()
                step(state.copy(), lm.logits(state, gp), gp, slots=[int(w)], trace=tr)
                if not unsafe_decisions(tr, lm.V, nseg):
                    break
            else:
                raise AssertionError("loop %s: slot %d cannot be settled" % ((nb, L, lp), w))
        step(state, lm.logits(state, gp), gp)
    return gp, lm, caps


LOOP_CASES = [(nb, L, lp) for nb in (1, 2, 4, 8) for L in (12, 32) for lp in LENGTH_PENALTIES]


# ---- the tap's argument block ---------------------------------------------------------------------------------------------------------
def tap_params(gp, S, V, ldv, sup_ptr=None, bsup_ptr=None):
    """wseg_decode_step_params for a case (device pointers of the two lists given by the caller)."""
    from whisperseg_amd import _lib
    p = _lib.DecodeStepParams()
    p.n_slots, p.num_beams, p.max_length, p.vocab, p.ldv = S, gp.num_beams, gp.max_length, V, ldv
    for i, t in enumerate(gp.prompt):
        p.prompt[i] = t
    p.prompt_len = len(gp.prompt)
    p.eos_token_id, p.pad_token_id = gp.eos_token_id, gp.pad_token_id
    p.length_penalty = gp.length_penalty
    p.top_k, p.top_p, p.seed = gp.top_k, gp.top_p, gp.seed
    p.suppress_tokens, p.n_suppress = sup_ptr, len(gp.suppress_tokens) if sup_ptr else 0
    p.begin_suppress_tokens, p.n_begin_suppress = bsup_ptr, len(gp.begin_suppress_tokens) if bsup_ptr else 0
    return p
