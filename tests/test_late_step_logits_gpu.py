"""Decoder logits at LATE steps against a float64 oracle.

The rest of the suite compares numbers with an independent reference at the first generated step only; later steps are covered by token
equality over short sequences and by self-consistency.  The decoder's self-attention changes behaviour with the position
(csrc/wseg_dec.hip::dec_self_attn_kernel): ancestry bytes and page-table units of the keys come from lane-held registers for positions
< 64 and from memory behind them, the first 32 V rows are prefetched (16-bit storage), the key loop runs in clamped blocks of 32, K / V
live in pages of 8 positions written by one of two writers, and with beams every row's history is scattered over other beams' cache rows.

Each case decodes >= 3 windows of a trained fixture model with EOS suppressed (no row ever finishes), takes the logits and the decode
state of chosen steps through the step-snapshot tap (Engine.generate(snapshot_steps=...), include/wseg.h), feeds THE ENGINE'S OWN row
histories through oracle/whisper_ref.py::TeacherForcer in float64 and compares the logits of every row.  Using the engine's histories
keeps the comparison valid where the engine and an oracle decode would have broken a near-tie differently earlier on.

Steps, as the number of keys n = position + 1 the self-attention sees: 8, 9 (page boundary), 32, 33 (V prefetch / second key block),
64, 65, 66 (register-held -> memory-held ancestry and page table), 96, 97, 128, 129, 257 and 447 (the last step of max_length 448).

Bounds.  The reference is always the float64 oracle.
  ceiling (every mode, every step; taken from the suite): f32 and the split-precision modes 1e-3 * max(1, |logits|_max)
      (test_first_logits_f32); bf16 cosine > 0.999 per row and 0.1 * scale, f16 cosine > 0.999 and 1.5e-2 * scale
      (test_two_layer_256_windows_1024_rows_vs_oracle / test_two_layer_8_windows_vs_oracle).
  tight (f32 and f16x3): 3 x the largest max |error| measured for the mode over all models, beam counts and steps
      (profiles/late_step_logit_error.txt; the factor covers other seeds and accumulation orders) — see TIGHT below.

MEASURED (MI355X, profiles/late_step_logit_error.txt holds every row): largest max |error| over the steps n < 32 | n >= 64, logit scale 14 .. 24
    f32     1.8e-5 | 4.3e-5        f16x3   1.8e-5 | 6.3e-5 (1.12e-4 on ONE row, below)
    bf16x3  1.4e-4 | 3.1e-4 (4.6e-4 at n = 32)      f16m6   8.1e-4 | 1.5e-3
    bf16    0.16   | 0.77 (min cosine 0.99971)      f16     1.3e-2 | 0.10
No mode is an order of magnitude worse behind position 64 than in front of 32.  The tight bounds, 1.3e-4 (f32) and 3.4e-4 (f16x3), are
above the 4.8e-5 class of the first-step comparison of f16x3 with the f32 MODE because the reference here is float64: fp32 arithmetic
alone is 2.6e-5 .. 4.0e-5 away from it on these models (the fp32 CPU oracle against the float64 one).  The f16x3 maximum is one
ill-conditioned row of the large-tile case (window 933, beam row 2, n = 66): both K / V writers give it (they differ by 3.8e-5 there,
3e-6 elsewhere), all 116 copies of the window agree bit for bit, and the steps around it are at 1e-5.  In the plain f16 mode that row is
0.987 off (cosine 0.9933, either writer) — outside the f16 class of 1.5e-2 x scale, while every other f16 row of that case is within
0.022; the large-tile case therefore runs the default mode only, and the f16 figure is recorded in the profile and DESIGN.md section 3.
"""
import json
import os

import numpy as np
import pytest
import torch

import golden_inputs as GI
from conftest import GOLDEN
from oracle import frontend as OF
from oracle import whisper_ref as R
from tools import tiny_model as TM

pytestmark = pytest.mark.gpu

P = len(TM.PROMPT)
SUP = TM.SUPPRESS + [TM.EOT]                  # EOS suppressed: every row runs to max_length
STEPS_N = [8, 9, 32, 33, 64, 65, 66, 96, 97, 128, 129, 257, 447]
MODELS = {"tiny2": ("tiny_model2", "tiny2", 100), "tiny3": ("tiny_model3", "tiny3", 100)}      # directory, signal family, recording seed

# max |logit error| against the float64 oracle allowed for the two modes with a tight bound = 3 x the largest value measured over every
# case of this file (profiles/late_step_logit_error.txt).
TIGHT = {"f32": 3 * 4.32e-5, "f16x3": 3 * 1.12e-4}


def ceiling_ok(mode, got, want):
    """The suite's own bound of the mode -> (ok, figures)."""
    scale = max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    cos = torch.nn.functional.cosine_similarity(got, want, dim=1).min().item()
    if mode == "bf16":
        return cos > 0.999 and err <= 0.1 * scale, (err, cos, scale)
    if mode == "f16":
        return cos > 0.999 and err <= 1.5e-2 * scale, (err, cos, scale)
    return err <= 1e-3 * scale, (err, cos, scale)


_models, _engines, _forcers = {}, {}, {}


def model(name):
    if name not in _models:
        from safetensors.torch import load_file
        mdir = os.path.join(GOLDEN, MODELS[name][0])
        sd = {k: v.float() for k, v in load_file(os.path.join(mdir, "model.safetensors")).items()}
        with open(os.path.join(mdir, "config.json")) as f:
            cfg = json.load(f)
        _models[name] = (sd, cfg, R.RefConfig.from_hf_dict(cfg))
    return _models[name]


def engine(name, mode):
    if (name, mode) not in _engines:
        from whisperseg_amd.engine import Engine
        sd, cfg, _ = model(name)
        _engines[(name, mode)] = Engine.from_state_dict(sd, cfg, "cuda:0", mode)
    return _engines[(name, mode)]


def windows(name, n_windows=3, seed=None):
    """log-mel windows of a recording of the model's own signal family (as test_full_length_decode_matches_oracle builds them)"""
    _, variant, s0 = MODELS[name]
    audio = GI.tiny_recording(s0 if seed is None else seed, n_windows, tail=1.0, variant=variant)
    x = torch.from_numpy(np.stack([s[2] for s in OF.sliced_audio_features(audio, TM.SR, 0, TM.STS, 1)]))
    assert x.shape[0] == n_windows
    return x


def forcer(name, key, x_i):
    """float64 encoder output + cross K / V of one window, shared by all cases that decode it"""
    if (name, key) not in _forcers:
        sd, _, rc = model(name)
        _forcers[(name, key)] = R.TeacherForcer(sd, rc, x_i)
    return _forcers[(name, key)]


def decode(eng, x, nb, max_length, steps_n=None, **kw):
    """every window in a slot of its own from the first step on, the K / V pool provisioned for max_length in every slot (no preemption)"""
    kw.setdefault("kv_positions", max_length)
    return eng.generate(x.cuda(), TM.PROMPT, TM.EOT, TM.EOT, max_length=max_length, num_beams=nb, suppress_tokens=SUP,
                        begin_suppress_tokens=TM.BEGIN_SUPPRESS, n_slots=x.shape[0],
                        snapshot_steps=None if steps_n is None else [n - 1 for n in steps_n], **kw)


def check_case(name, mode, nb, steps_n, x, keys, pick=None, max_length=448, want_split=None):
    """One decode with snapshots at `steps_n`; logits of every row of the windows `pick` (default: all) against the float64 oracle.
    Returns the table rows (mode, model, beams, n, max, mean, scale); asserts the coverage conditions and the bounds."""
    W = x.shape[0]
    pick = list(range(W)) if pick is None else pick
    toks, lens, snap = decode(engine(name, mode), x, nb, max_length, steps_n)
    assert lens.cpu().tolist() == [max_length] * W
    if want_split is not None:
        assert snap["qkv_split"] == want_split, (mode, W * nb, snap["qkv_split"])
    logits, seq, anc = snap["logits"].cpu().double(), snap["run_seq"].cpu().long(), snap["anc"].cpu().long()
    pos, idle = snap["pos"].cpu(), snap["idle"].cpu()
    assert logits.shape[0] == len(steps_n)
    rows_out, failures = [], []
    for si, n in enumerate(sorted(steps_n)):
        # coverage: every row is live and at the requested step
        assert idle[si].tolist() == [0] * W and pos[si].tolist() == [n - 1] * W, (n, idle[si].tolist()[:8], pos[si].tolist()[:8])
        got, want = [], []
        for w in pick:
            rows = slice(w * nb, (w + 1) * nb)
            hist = seq[si, rows, :n]
            assert hist[:, :P].tolist() == [list(TM.PROMPT)] * nb and not (set(hist[:, P:].flatten().tolist()) & set(SUP))
            got.append(logits[si, rows])
            want.append(forcer(name, keys[w], x[w]).logits(hist))
        got, want = torch.cat(got), torch.cat(want)
        if nb > 1 and n >= 65:
            # coverage: memory-held ancestry is live and the beams are different hypotheses.  anc[r][t]: the beam whose cache rows hold
            # position t of row r; the kernel reads it for t < n - 1 (t = n - 1 is the row's own, just appended)
            a = anc[si].view(W, nb, -1)
            assert (a[:, :, 64:] != 0).any(), n
            if n >= 66:      # ... and some key at a position >= 64 really lives in ANOTHER beam's cache rows
                own = torch.arange(nb).view(1, nb, 1)
                assert (a[:, :, 64:n - 1] != own).any(), n
            h = seq[si].view(W, nb, -1)[:, :, :n]
            assert any((h[w, 0] != h[w, j]).any() for w in range(W) for j in range(1, nb)), n
        ok, (err, cos, scale) = ceiling_ok(mode, got, want)
        mean = (got - want).abs().mean().item()
        rows_out.append(dict(mode=mode, model=name, beams=nb, n=n, rows=got.shape[0], max=err, mean=mean, scale=scale, cos=cos))
        print("LATE_STEP " + json.dumps(rows_out[-1]))
        if not ok:
            failures.append(("ceiling", n, err, cos, scale))
        if TIGHT.get(mode) is not None and err > TIGHT[mode]:
            failures.append(("tight", n, err, TIGHT[mode]))
    assert not failures, (name, mode, nb, failures)
    return rows_out


CASES = [(m, nb) for m in ("f32", "f16x3", "bf16x3", "f16m6") for nb in (1, 2, 3, 4)] + [(m, nb) for m in ("bf16", "f16") for nb in (1, 4)]


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("mode,nb", CASES)
def test_late_step_logits_vs_fp64_oracle(gpu_lib, name, mode, nb):
    """Every listed step of a 448-position decode of 3 windows.  Which K / V writer runs at these row counts is asserted, not assumed:
    the exact mode never splits K (the q | k | v GEMM's EPI_QKV_DEC epilogue writes the cache rows), the other modes hand split-K partials
    to the attention kernel, which finishes the reduction and appends K / V itself."""
    x = windows(name)
    check_case(name, mode, nb, STEPS_N, x, keys=[("rec", i) for i in range(3)], want_split=0 if mode == "f32" else 1)


@pytest.mark.parametrize("name", list(MODELS))
def test_late_step_logits_8_beams(gpu_lib, name):
    """5..8 beams run the general cross-attention kernel; the default mode at a few of the steps."""
    x = windows(name)
    check_case(name, "f16x3", 8, [9, 33, 65, 66, 129, 447], x, keys=[("rec", i) for i in range(3)], want_split=1)


def test_late_step_logits_large_tile_writer(gpu_lib, mode="f16x3"):
    """The other K / V writer of the MFMA modes: at 1 856 windows x 4 beams = 7 424 rows the q | k | v GEMM of tiny_model2 (N = 768:
    58 x 6 tiles of 128 x 128 >= 340) runs on the large-tile kernels and its EPI_QKV_DEC epilogue writes q and the paged cache rows
    (qkv_split == 0, asserted).  16 distinct windows repeated 116 times; the oracle checks the first, an interior and the last one."""
    base = windows("tiny2", 16, seed=104)
    x = base.repeat(116, 1, 1)
    pick = [0, 933, 1855]
    steps = [9, 33, 64, 65, 66, 97, 99]
    check_case("tiny2", mode, 4, steps, x, keys={w: ("big", w % 16) for w in pick}, pick=pick, max_length=100, want_split=0)


def test_small_rows_use_the_fused_writer_in_f16(gpu_lib):
    """... and the plain 16-bit modes at 12 rows take the fused writer (asserted inside check_case for every mode of the main test);
    this case pins the page-table path of the fused writer's own row beyond position 64 (`own_unit` is loaded, not lane-held) at a
    page boundary: n = 73 is the first position of page 9."""
    x = windows("tiny3")
    check_case("tiny3", "f16x3", 4, [72, 73, 74], x, keys=[("rec", i) for i in range(3)], want_split=1)


# ---- the tap itself ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("nb", [1, 4])
def test_snapshot_does_not_change_the_decode(gpu_lib, mode, nb):
    """Tokens and lengths of a call with snapshots are bit-identical to the same call without; the snapshot of the first generated step is
    bit-identical to wseg_debug_first_logits of that call; histories in the records are prefixes of nothing else than what was fed."""
    x = windows("tiny2")
    eng = engine("tiny2", mode)
    t0, l0 = decode(eng, x, nb, 448)
    steps = [P, 8, 9, 64, 65, 66, 257, 447]
    t1, l1, fl, snap = decode(eng, x, nb, 448, steps, return_first_logits=True)
    t2, l2 = decode(eng, x, nb, 448)
    assert torch.equal(t0, t1) and torch.equal(l0, l1) and torch.equal(t0, t2) and torch.equal(l0, l2)
    assert snap["positions"].tolist() == [n - 1 for n in steps]
    assert torch.equal(snap["logits"][0], fl)
    assert snap["pos"].cpu().tolist() == [[n - 1] * 3 for n in steps] and not snap["idle"].any()
    if nb == 1:      # greedy: a row's history at any step is the prefix of the final sequence
        for si, n in enumerate(steps):
            assert torch.equal(snap["run_seq"][si, :, :n], t0[:, :n])
    # the same records when asked for one step at a time
    for si in (3, 5):
        _, _, one = decode(eng, x, nb, 448, [steps[si]])
        for k in ("logits", "run_seq", "pos", "idle", "anc"):
            assert torch.equal(one[k][0], snap[k][si]), (k, steps[si])


def test_snapshot_needs_all_windows_to_start_together(gpu_lib):
    import ctypes as C
    from whisperseg_amd import _lib
    x = windows("tiny3")
    eng = engine("tiny3", "f16x3")
    with pytest.raises(ValueError):
        eng.generate(x.cuda(), TM.PROMPT, TM.EOT, TM.EOT, max_length=12, num_beams=1, n_slots=2, snapshot_steps=[4])
    taken = C.c_int32(0)
    eng.generate(x.cuda(), TM.PROMPT, TM.EOT, TM.EOT, max_length=12, num_beams=1)      # not armed
    assert eng.lib.wseg_debug_step_snapshot_result(eng.handle, C.byref(taken), None) == -3
    # armed, but the three windows go through two slots: WSEG_ERR_STATE, and the tokens are those of the plain call
    rec = eng.lib.wseg_debug_step_snapshot_bytes(eng.handle, 2, 1, 12)
    buf = torch.zeros(rec, dtype=torch.uint8, device="cuda:0")
    _lib.check(eng.lib.wseg_debug_step_snapshot_arm(eng.handle, (C.c_int32 * 1)(4), 1, buf.data_ptr(), buf.numel()))
    t_a, l_a = eng.generate(x.cuda(), TM.PROMPT, TM.EOT, TM.EOT, max_length=12, num_beams=1, n_slots=2)
    assert eng.lib.wseg_debug_step_snapshot_result(eng.handle, C.byref(taken), None) == -3
    t_b, l_b = eng.generate(x.cuda(), TM.PROMPT, TM.EOT, TM.EOT, max_length=12, num_beams=1, n_slots=2)
    assert torch.equal(t_a, t_b) and torch.equal(l_a, l_b)
    # bad arguments
    assert eng.lib.wseg_debug_step_snapshot_arm(eng.handle, (C.c_int32 * 2)(5, 4), 2, buf.data_ptr(), buf.numel()) == -1
    assert eng.lib.wseg_debug_step_snapshot_arm(eng.handle, (C.c_int32 * 17)(*range(17)), 17, buf.data_ptr(), buf.numel()) == -1
    # a buffer that cannot hold the records is refused by the call it was armed for, which then stays disarmed
    _lib.check(eng.lib.wseg_debug_step_snapshot_arm(eng.handle, (C.c_int32 * 1)(4), 1, buf.data_ptr(), 16))
    with pytest.raises(_lib.WsegError):
        eng.generate(x.cuda(), TM.PROMPT, TM.EOT, TM.EOT, max_length=12, num_beams=1)
    t_c, l_c = eng.generate(x.cuda(), TM.PROMPT, TM.EOT, TM.EOT, max_length=12, num_beams=1, n_slots=2)
    assert torch.equal(t_a, t_c)
