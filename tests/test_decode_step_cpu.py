"""The decode step's reference and cases, without a device: every case is settled (tests/decode_step_cases.py), the case list reaches
every beam event, tie kind and slice-edge placement it is meant to, the step functions in a loop are `generate`, and the tap
(wseg_debug_decode_step) rejects each bad argument on the host, before anything is launched."""
import ctypes as C
import json
import os
from collections import Counter

import numpy as np
import pytest
import torch

import decode_step_cases as D
import golden_inputs as GI
from oracle import frontend as F
from oracle import whisper_ref as W
from tools import tiny_model as TM


@pytest.fixture(scope="module")
def traces():
    out = {}
    for name in D.CASE_NAMES:
        case = D.get_case(name)
        tr = W.StepTrace()
        case.step(trace=tr)
        out[name] = (case, tr)
    return out


def test_every_case_is_settled(traces):
    assert len(traces) >= 60
    for name, (case, tr) in traces.items():
        assert tr.decisions or case.nb == 1, name
        assert D.unsafe_decisions(tr, case.V, case.nseg) == [], name
        # the geometry each case claims: slice count and candidate template as the library derives them
        assert case.nseg == max(1, min(16, -(-512 // (case.S * case.nb)))) and case.ldv % 4 == 0 and case.ldv >= case.V


def test_margin_check_rejects_a_close_call():
    """The check itself: the same slot with two running scores 1e-6 apart (and different rows) is refused."""
    case = D.mixed_case("probe", 1, 2, 1283, 4242, idle=False)
    case.state.pos[0], case.state.done[0], case.state.unsat[0], case.state.wmax[0] = D.P + 3, 0, 1, case.gp.max_length
    case.logits[1] = case.logits[0]
    case.logits[1, 100:110] += np.float32(0.25)
    case.state.run_score[0:2] = np.float32([-1.0, -1.0 - 1.0e-6])
    lse = [W._log_softmax64(case.logits[r]).max() for r in (0, 1)]
    case.state.run_score[1] = np.float32(-1.0 + lse[0] - lse[1] + 2.0e-6)      # the two best candidates land 2e-6 apart
    assert D.unsafe_decisions(D.slot_trace(case, 0), case.V, case.nseg)


def test_geometries_cover_every_slice_count_and_template():
    seen = {(D.n_slices(S * nb), D.kc_template(D.kc_of(nb, k))) for S, nb, k in D.GEOMETRIES}
    assert seen == {(16, 1), (16, 4), (16, 8), (13, 16), (4, 8), (1, 8), (1, 1), (16, 16)}
    # 1283 in 13 slices of 99: nine of the twelve later slices start misaligned, with every offset 1..3; 61: slices of 4; 5003 in one
    # slice: 5 groups per stride
    assert sorted(D.slice_bounds(1283, 13, s)[0] % 4 for s in range(1, 13)) == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    assert D.slice_bounds(61, 16, 3) == (12, 12, 16, 16) and -(-5003 // 1024) == 5


def test_case_list_reaches_every_event_tie_and_placement(traces):
    events, places, ties, lps = Counter(), Counter(), Counter(), set()
    for name, (case, tr) in traces.items():
        events.update(tr.events)
        lps.add(case.gp.length_penalty)
        for r, ids, vals in tr.rows:
            for k in D.placement_kinds(case.V, case.nseg, ids[:case.kc]):
                places[(k, case.nseg > 1)] += 1
            for k in D.tie_kinds(case.V, case.nseg, ids, vals):
                ties[k] += 1
    for ev in ("eos_rank_ge_nb_only", "eos_rank_0", "eos_in_nb_rows", "several_finish", "cap_hit", "cap_at_first_step", "prompt_phase",
               "unsat_already_0", "early_stop_improves", "early_stop_stops", "finished_new", "suppressed_row_max", "begin_suppress_step",
               "tie_two_beams", "tie_finished_scores", "tie_running", "sample_cut"):
        assert events[ev] > 0, (ev, dict(events))
    assert ties["tie_two_slices"] > 0 and ties["tie_two_threads_of_a_wave"] > 0, dict(ties)
    for k in ("one_stride", "one_wave", "one_per_wave", "one_slice", "one_per_slice", "at_lo", "at_hi_1", "at_a4_1", "at_a4", "at_b4_1",
              "at_b4", "at_0", "at_V_1"):
        assert places[(k, True)] > 0, (k, dict(places))
    # one slice (520 and 600 rows): the edges again, and at V = 5003 winners in all five 16-byte groups of ONE thread's stride
    for k in ("one_stride", "one_stride_5_groups", "one_wave", "one_per_wave", "at_lo", "at_hi_1", "at_a4", "at_b4_1", "at_b4", "at_0", "at_V_1"):
        assert places[(k, False)] > 0, (k, dict(places))
    assert lps >= set(D.LENGTH_PENALTIES)
    for name in [n for n in traces if n.startswith("events_")]:
        assert all(traces[name][1].events[e] > 0 for e in traces[name][0].notes["events"]), name


def test_suppression_cases_do_what_they_say(traces):
    for name, (case, tr) in traces.items():
        if not name.startswith("suppress_"):
            continue
        after = case.step()
        first = name.endswith("_first")
        for w in range(case.S):
            toks = after.cand_tok[w * case.nb:(w + 1) * case.nb, :case.kc]
            assert not np.isin(toks, [t for t in case.gp.suppress_tokens if 0 <= t < case.V]).any(), name
            assert bool((toks == D.EOS).any()) != first, name          # banned at the first generated step, the best again at the next


def test_sampler_generator_known_values():
    """splitmix64's published first outputs for seed 0 are the finaliser of k * 0x9E3779B97F4A7C15: the generator is that function."""
    assert W.sampler_uniform24(0, 0, 0) == 0xE220A8397B1DCDAF >> 40
    assert W.sampler_uniform24(0, 0, 1) == 0x6E789E6AA1B965F4 >> 40
    assert W.sampler_uniform24(0x9E3779B97F4A7C15, 0, 0) == 0x6E789E6AA1B965F4 >> 40
    assert W.sampler_uniform24(0, 1, -1) == W.sampler_uniform24(0, 0, 4095)
    vals = [np.float32(2.0), np.float32(1.0), np.float32(-np.inf)]
    assert W.sample_candidate(vals, 1.0, 0) == 0 and W.sample_candidate(vals, 1.0, (1 << 24) - 1) == 1      # weight 0 is never drawn
    assert W.sample_candidate(vals, 0.5, (1 << 24) - 1) == 0 and W.sample_candidate(vals, 0.0, (1 << 24) - 1) == 1


@pytest.mark.parametrize("nb,L,lp", [(1, 12, 1.0), (2, 12, 2.0), (4, 32, -1.0), (8, 12, 0.6)])
def test_closed_loops_run_on_the_reference(nb, L, lp):
    gp, lm, caps = D.loop_params(nb, L, lp, D.LOOP_CASES.index((nb, L, lp)))
    toks, lens, state = W.run_loop(lambda st, src: lm.logits(st, gp), D.LOOP_SLOTS, gp, window_max_length=caps, max_steps=32)
    assert state.done.all() and (lens <= np.asarray(caps)).all() and lens[1] == D.P + 1 and (lens > D.P).all()
    for i in range(D.LOOP_SLOTS):
        assert (toks[i, lens[i]:] == gp.pad_token_id).all() and list(toks[i, :D.P]) == D.PROMPT


@pytest.mark.parametrize("nb", [1, 2, 4])
def test_the_loop_over_step_functions_is_generate(golden_dir, nb):
    """run_loop with the tiny model's logits in place of scripted ones gives generate's tokens.  `generate` IS that loop now, so this
    half only keeps the two from drifting apart; that the step functions reproduce HF is shown by the unchanged recorded rows of
    tests/test_oracle_model.py.  What this test adds is the per-window cap: the capped window stops at its cap, the others are
    unchanged."""
    from safetensors.torch import load_file
    mdir = os.path.join(golden_dir, "tiny_model")
    sd = {k: v.float() for k, v in load_file(os.path.join(mdir, "model.safetensors")).items()}
    with open(os.path.join(mdir, "config.json")) as f:
        rc = W.RefConfig.from_hf_dict(json.load(f))
    audio = GI.tiny_recording(102, 4)
    feats = torch.from_numpy(np.stack([s[2] for s in F.sliced_audio_features(audio, TM.SR, 0, TM.STS, 1)]))
    gp = W.GenParams(prompt=TM.PROMPT, eos_token_id=TM.EOT, pad_token_id=TM.EOT, max_length=40, num_beams=nb,
                     suppress_tokens=TM.SUPPRESS, begin_suppress_tokens=TM.BEGIN_SUPPRESS)
    want = W.generate(sd, rc, feats, gp)
    enc = W.encoder_forward(sd, rc, feats)
    dec = W.Decoder(sd, rc, enc.repeat_interleave(nb, dim=0))

    def logits_fn(state, src):
        if src is None:
            return dec.step(torch.from_numpy(state.run_seq[:, :3].astype(np.int64))).numpy()
        dec.reorder(torch.from_numpy(src.astype(np.int64)))
        return dec.step(torch.from_numpy(state.tokens_in.astype(np.int64))[:, None]).numpy()

    toks, lens, _ = W.run_loop(logits_fn, feats.shape[0], gp)
    assert torch.equal(torch.from_numpy(toks[:, :int(lens.max())].astype(np.int64)), want)
    # per-window caps: window 1 capped at 8 tokens in all
    gp.window_max_length = [40, 8, 40, 40]
    capped = W.generate(sd, rc, feats, gp)
    for i in (0, 2, 3):
        assert W.canonical(capped[i].tolist(), 3, TM.EOT, TM.PROMPT) == W.canonical(want[i].tolist(), 3, TM.EOT, TM.PROMPT)
    assert bool((capped[1, 8:] == TM.EOT).all()) and bool((want[1, :9] != TM.EOT).all())


# ---- the tap's host-side validation (nothing is launched: every pointer here is a fake, never dereferenced) ----------------------------
FAKE = 0x10000


def tap_call(lib, mutate=None, **over):
    from whisperseg_amd import _lib
    gp = D.make_gp(over.pop("nb", 2), 24, top_k=over.pop("top_k", 1))
    S, V = 2, 61
    p = D.tap_params(gp, S, V, 64)
    st = _lib.DecodeStepState(**{n: FAKE for n, _ in _lib.DecodeStepState._fields_})
    args = dict(p=C.byref(p), st=C.byref(st), logits=FAKE, list=None, n_list=0, scratch=FAKE,
                scratch_bytes=lib.wseg_debug_decode_step_scratch_bytes(S, gp.num_beams, V), out_tokens=None, out_lengths=None, n_out=0)
    if mutate:
        mutate(p, st, args)
    args.update(over)
    rc = lib.wseg_debug_decode_step(args["p"], args["st"], args["logits"], args["list"], args["n_list"], args["scratch"],
                                    args["scratch_bytes"], args["out_tokens"], args["out_lengths"], args["n_out"], None)
    return rc, lib.wseg_last_error().decode()


BAD_ARGUMENTS = {
    "num_beams_0": (lambda p, st, a: setattr(p, "num_beams", 0), "num_beams"),
    "num_beams_9": (lambda p, st, a: setattr(p, "num_beams", 9), "num_beams"),
    "top_k_negative": (lambda p, st, a: setattr(p, "top_k", -1), "top_k"),
    "top_k_17": (lambda p, st, a: setattr(p, "top_k", 17), "top_k"),
    "ldv_below_vocab": (lambda p, st, a: setattr(p, "ldv", 60), "ldv"),
    "ldv_not_multiple_of_4": (lambda p, st, a: setattr(p, "ldv", 62), "ldv"),
    "vocab_below_candidates": (lambda p, st, a: (setattr(p, "vocab", 3), setattr(p, "ldv", 4)), "vocab"),
    "prompt_len_0": (lambda p, st, a: setattr(p, "prompt_len", 0), "prompt_len"),
    "prompt_len_9": (lambda p, st, a: setattr(p, "prompt_len", 9), "prompt_len"),
    "max_length_is_prompt_len": (lambda p, st, a: setattr(p, "max_length", 3), "max_length"),
    "n_slots_0": (lambda p, st, a: setattr(p, "n_slots", 0), "n_slots"),
    "null_params": (lambda p, st, a: a.update(p=None), "params"),
    "null_state": (lambda p, st, a: a.update(st=None), "state"),
    "null_state_array": (lambda p, st, a: setattr(st, "fin_len", None), "fin_len"),
    "null_logits": (lambda p, st, a: a.update(logits=None), "logits"),
    "null_scratch": (lambda p, st, a: a.update(scratch=None), "scratch"),
    "short_scratch": (lambda p, st, a: a.update(scratch_bytes=a["scratch_bytes"] - 1), "scratch"),
    "null_suppress_list": (lambda p, st, a: setattr(p, "n_suppress", 2), "suppress_tokens"),
    "null_begin_suppress_list": (lambda p, st, a: setattr(p, "n_begin_suppress", 1), "begin_suppress_tokens"),
    "list_without_count": (lambda p, st, a: a.update(list=FAKE, n_list=0), "n_list"),
    "count_without_list": (lambda p, st, a: a.update(n_list=1), "n_list"),
    "list_longer_than_slots": (lambda p, st, a: a.update(list=FAKE, n_list=3), "n_list"),
    "out_tokens_without_lengths": (lambda p, st, a: a.update(out_tokens=FAKE, n_out=2), "out_lengths"),
    "out_rows_0": (lambda p, st, a: a.update(out_tokens=FAKE, out_lengths=FAKE, n_out=0), "n_out_rows"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGUMENTS))
def test_tap_rejects_bad_argument_on_the_host(name):
    from whisperseg_amd import _lib
    lib = _lib.load()
    mutate, word = BAD_ARGUMENTS[name]
    rc, msg = tap_call(lib, mutate)
    assert rc == -1 and msg.startswith("wseg_debug_decode_step:") and word in msg, (rc, msg)


def test_tap_scratch_size_is_host_arithmetic():
    from whisperseg_amd import _lib
    lib = _lib.load()
    f = lib.wseg_debug_decode_step_scratch_bytes
    assert f(0, 1, 61) == 0 and f(1, 9, 61) == 0 and f(1, 1, 0) == 0
    assert f(600, 1, 5003) > f(130, 4, 1283) > f(1, 1, 61) > 0 and f(2, 2, 61) % 256 == 0
    assert f(4, 8, 51865) >= 4 * 8 * 16 * (16 * 4 + 16 * 4 + 2 * 4) + 51868 + 8 + 4 * 4


def test_closed_loops_meet_the_beam_events_on_their_own():
    """The crafted single steps are not the only place an event occurs: the scripted loops reach them unprompted."""
    events = Counter()
    for i, (nb, L, lp) in enumerate(D.LOOP_CASES):
        if nb == 1:
            continue
        gp, lm, caps = D.loop_params(nb, L, lp, i)
        state = W.new_state(D.LOOP_SLOTS, gp, window_max_length=caps)
        while not state.done.all():
            tr = W.StepTrace()
            W.beam_step(state, lm.logits(state, gp), gp, trace=tr)
            events.update(tr.events)
    for ev in ("eos_rank_ge_nb_only", "eos_rank_0", "several_finish", "cap_hit", "cap_at_first_step", "early_stop_improves",
               "early_stop_stops", "finished_new"):
        assert events[ev] > 0, (ev, dict(events))
