"""Pins oracle/whisper_ref.py against outputs of HF `generate` driven through the reference's own
WhisperSegmenterForEval on the tiny trained model (tools/make_golden.py -> tests/golden/tiny_generate.*)."""
import json
import os

import numpy as np
import pytest
import torch

import golden_inputs as GI
from oracle import frontend as F
from oracle import whisper_ref as W
from tools import tiny_model as TM


@pytest.fixture(scope="module")
def tiny(golden_dir):
    from safetensors.torch import load_file
    mdir = os.path.join(golden_dir, "tiny_model")
    sd = {k: v.float() for k, v in load_file(os.path.join(mdir, "model.safetensors")).items()}
    with open(os.path.join(mdir, "config.json")) as f:
        cfg = json.load(f)
    with open(os.path.join(golden_dir, "tiny_generate.json")) as f:
        runs = json.load(f)
    return sd, W.RefConfig.from_hf_dict(cfg), runs, np.load(os.path.join(golden_dir, "tiny_generate.npz"))


def content(tokens):
    """generated ids before the first EOS, prompt stripped (HF 4.38.2 returns the prompt, 5.15 does not)."""
    c = W.canonical(tokens, 3, TM.EOT, TM.PROMPT)
    return c[:-1] if c and c[-1] == TM.EOT else c


def test_encoder_and_first_logits(tiny):
    sd, rc, runs, z = tiny
    audio = GI.tiny_recording(100, 3)
    sliced = F.sliced_audio_features(audio, TM.SR, 0, TM.STS, 1)
    feats = torch.from_numpy(np.stack([s[2] for s in sliced]))
    assert np.max(np.abs(feats.numpy()[:, :, ::GI.COL_STRIDE] - z["features_cols"])) <= 1e-4
    enc = W.encoder_forward(sd, rc, feats)
    assert np.max(np.abs(enc.numpy()[:, ::25, :] - z["enc_out_sample"])) <= 2e-4
    gp = W.GenParams(prompt=TM.PROMPT, eos_token_id=TM.EOT, pad_token_id=TM.EOT, max_length=8, num_beams=1)
    _, logits = W.generate(sd, rc, feats, gp, return_first_logits=True)
    assert np.max(np.abs(logits.numpy() - z["first_logits"])) <= 2e-3


def test_token_sequences_match_hf(tiny):
    """Greedy and beam search (beams 1/2/4, default and short max_length, EOS at varied lengths)."""
    sd, rc, runs, _ = tiny
    n_checked = 0
    for run in runs:
        kw = run["kwargs"]
        audio = GI.tiny_recording(run["seed"], run["n_windows"])
        sliced = F.sliced_audio_features(audio, TM.SR, 0, TM.STS, kw.get("num_trials", 1))
        feats = torch.from_numpy(np.stack([s[2] for s in sliced]))
        gp = W.GenParams(prompt=TM.PROMPT, eos_token_id=TM.EOT, pad_token_id=TM.EOT, max_length=kw.get("max_length", 448),
                         num_beams=kw["num_beams"], suppress_tokens=TM.SUPPRESS, begin_suppress_tokens=TM.BEGIN_SUPPRESS)
        pos = 0
        for batch in run["token_batches"]:
            out = W.generate(sd, rc, feats[pos:pos + len(batch)], gp)
            for want, got in zip(batch, out.tolist()):
                assert content(got) == content(want), (kw, pos)
                n_checked += 1
            pos += len(batch)
        assert pos == len(sliced)
    assert n_checked >= 20


@pytest.mark.parametrize("num_beams", [2, 4])
@pytest.mark.parametrize("length_penalty", [0.0, 2.0, -1.0])
def test_length_penalty_matches_installed_transformers(tiny, golden_dir, num_beams, length_penalty):
    """The pow() denominators of the finished-beam scores and of the early-stop comparison against the installed HF `generate` on
    the tiny trained model (every recorded golden has length_penalty 1.0).  HF 5.x counts max_length without the prompt and returns
    no prompt: the oracle's max_length = L is HF's L - 3.  Two recordings: tiny_recording(102, 4), where only (4 beams, 2.0) moves a
    token, and tiny_recording(118, 4), where every one of the six settings gives other tokens than length_penalty 1.0 does — asserted
    below, so that an oracle which ignored the penalty or misread its sign fails each case."""
    transformers = pytest.importorskip("transformers")
    sd, rc, _, _ = tiny
    model = transformers.WhisperForConditionalGeneration.from_pretrained(os.path.join(golden_dir, "tiny_model")).float().eval()
    hf_strips_prompt = int(transformers.__version__.split(".")[0]) >= 5
    lengths = set()
    for rec, Ls in ((102, (40, 12)), (118, (40,))):
        audio = GI.tiny_recording(rec, 4)
        feats = torch.from_numpy(np.stack([s[2] for s in F.sliced_audio_features(audio, TM.SR, 0, TM.STS, 1)]))
        assert feats.shape[0] == 4
        for L in Ls:
            gp = W.GenParams(prompt=TM.PROMPT, eos_token_id=TM.EOT, pad_token_id=TM.EOT, max_length=L, num_beams=num_beams,
                             length_penalty=length_penalty, suppress_tokens=TM.SUPPRESS, begin_suppress_tokens=TM.BEGIN_SUPPRESS)
            got = W.generate(sd, rc, feats, gp)
            with torch.no_grad():
                want = model.generate(input_features=feats, decoder_input_ids=torch.tensor([TM.PROMPT] * feats.shape[0]), pad_token_id=TM.EOT,
                                      eos_token_id=TM.EOT, max_length=L - 3 if hf_strips_prompt else L, num_beams=num_beams,
                                      do_sample=False, length_penalty=length_penalty, suppress_tokens=TM.SUPPRESS,
                                      begin_suppress_tokens=TM.BEGIN_SUPPRESS)
            for i in range(feats.shape[0]):
                assert content(got[i].tolist()) == content(want[i].tolist()), (rec, L, i)
                lengths.add(len(content(got[i].tolist())))
            if rec == 118:          # the penalty is live here: length_penalty 1.0 decodes something else
                gp.length_penalty = 1.0
                neutral = W.generate(sd, rc, feats, gp)
                assert [content(r.tolist()) for r in neutral] != [content(r.tolist()) for r in got], (num_beams, length_penalty)
    assert len(lengths) >= 3


def test_eos_fires_at_varied_lengths(tiny):
    _, _, runs, _ = tiny
    lengths = {len(content(row)) for run in runs for b in run["token_batches"] for row in b}
    assert len(lengths) >= 5


# ---- the second (held-out) fixture model: another geometry (d 256, 4 heads, 3 + 3 layers), full-mantissa fp32 weights -----------------
@pytest.fixture(scope="module")
def tiny2(golden_dir):
    from safetensors.torch import load_file
    mdir = os.path.join(golden_dir, "tiny_model2")
    sd = {k: v.float() for k, v in load_file(os.path.join(mdir, "model.safetensors")).items()}
    with open(os.path.join(mdir, "config.json")) as f:
        cfg = json.load(f)
    with open(os.path.join(golden_dir, "tiny2_sweep.json")) as f:
        sweep = json.load(f)
    return sd, W.RefConfig.from_hf_dict(cfg), sweep, np.load(os.path.join(golden_dir, "tiny2_generate.npz"))


def test_second_fixture_model_is_another_model(tiny, tiny2):
    sd1, rc1 = tiny[0], tiny[1]
    sd2, rc2, sweep, _ = tiny2
    assert (rc2.d_model, rc2.encoder_layers, rc2.decoder_layers) == (256, 3, 3) and rc1.d_model == 128
    w = sd2["model.decoder.layers.0.fc1.weight"]
    assert not torch.equal(w, w.half().float()) and not torch.equal(w, w.bfloat16().float())      # full-mantissa weights: lo halves are live
    assert len(sweep) == 1000 and {r["seed"] for r in sweep} == set(range(5000, 5250))


def test_second_fixture_encoder_and_first_logits(tiny2):
    """oracle vs HF (recorded by tools/make_golden.py --only sweep2) on the held-out model's geometry"""
    sd, rc, _, z = tiny2
    audio = GI.tiny_recording(5000, 3, variant="tiny2")
    sliced = F.sliced_audio_features(audio, TM.SR, 0, TM.STS, 1)
    feats = torch.from_numpy(np.stack([s[2] for s in sliced]))
    enc = W.encoder_forward(sd, rc, feats)
    assert np.max(np.abs(enc.numpy()[:, ::25, :] - z["enc_out_sample"])) <= 5e-4
    gp = W.GenParams(prompt=TM.PROMPT, eos_token_id=TM.EOT, pad_token_id=TM.EOT, max_length=8, num_beams=1)
    _, logits = W.generate(sd, rc, feats, gp, return_first_logits=True)
    assert np.max(np.abs(logits.numpy() - z["first_logits"])) <= 3e-3


def test_oracle_reproduces_heldout_rows(tiny2, golden_dir):
    """the CPU oracle + the product's host epilogue through 12 of the 1 000 held-out recordings (all four (trials, beams) combinations)"""
    from tools.precision_study import OracleSegmenter, Policy
    _, _, sweep, _ = tiny2
    seg = OracleSegmenter(Policy(""), model_dir=os.path.join(golden_dir, "tiny_model2"))
    for run in sweep[0:8] + sweep[500:504]:
        got = seg.segment(GI.tiny_recording(run["seed"], run["n_windows"], variant="tiny2"), TM.SR, **run["kwargs"])
        assert got == run["expected"], (run["seed"], run["kwargs"])


# ---- the third fixture model (d 128, 2 heads, 4 + 4 layers, ffn 640, fp32 weights) ---------------------------------------------------
def test_third_fixture_encoder_logits_and_rows(golden_dir):
    """oracle vs HF on the third model's geometry (tools/make_golden.py --only sweep5): encoder output, first-step logits, and 8 of its
    1 000 sweep recordings end to end through the oracle + the product's host epilogue"""
    from safetensors.torch import load_file
    from tools.precision_study import OracleSegmenter, Policy
    mdir = os.path.join(golden_dir, "tiny_model3")
    sd = {k: v.float() for k, v in load_file(os.path.join(mdir, "model.safetensors")).items()}
    with open(os.path.join(mdir, "config.json")) as f:
        rc = W.RefConfig.from_hf_dict(json.load(f))
    assert (rc.d_model, rc.encoder_layers, rc.decoder_layers) == (128, 4, 4)
    z = np.load(os.path.join(golden_dir, "tiny3_generate.npz"))
    with open(os.path.join(golden_dir, "tiny3_sweep.json")) as f:
        sweep = json.load(f)
    assert len(sweep) == 1000 and {r["seed"] for r in sweep} == set(range(11000, 11250))
    audio = GI.tiny_recording(11000, 3, variant="tiny3")
    sliced = F.sliced_audio_features(audio, TM.SR, 0, TM.STS, 1)
    feats = torch.from_numpy(np.stack([s[2] for s in sliced]))
    enc = W.encoder_forward(sd, rc, feats)
    assert np.max(np.abs(enc.numpy()[:, ::25, :] - z["enc_out_sample"])) <= 5e-4
    gp = W.GenParams(prompt=TM.PROMPT, eos_token_id=TM.EOT, pad_token_id=TM.EOT, max_length=8, num_beams=1)
    _, logits = W.generate(sd, rc, feats, gp, return_first_logits=True)
    assert np.max(np.abs(logits.numpy() - z["first_logits"])) <= 3e-3
    seg = OracleSegmenter(Policy(""), model_dir=mdir)
    with open(os.path.join(golden_dir, "tiny3_sweep6.json")) as f:      # sweep 6: 1 000 more of the same model (tools/record_sweep.sh sweep6)
        sweep6 = json.load(f)
    assert len(sweep6) == 1000 and {r["seed"] for r in sweep6} == set(range(13000, 13250))
    with open(os.path.join(golden_dir, "tiny3_sweep7.json")) as f:      # sweep 7: and 1 000 more (tools/record_sweep.sh sweep7)
        sweep7 = json.load(f)
    assert len(sweep7) == 1000 and {r["seed"] for r in sweep7} == set(range(15000, 15250))
    for run in sweep[0:4] + sweep[600:604] + sweep6[0:4] + sweep6[700:702] + sweep7[300:302]:
        got = seg.segment(GI.tiny_recording(run["seed"], run["n_windows"], variant="tiny3"), TM.SR, **run["kwargs"])
        assert got == run["expected"], (run["seed"], run["kwargs"])


# ---- the float64 teacher-forced reference (tests/test_late_step_logits_gpu.py) ---------------------------------------------------------
def test_teacher_forced_logits_match_the_incremental_oracle(tiny2):
    """teacher_forced_logits runs given histories as ONE causal pass; in fp32 it must agree with what the pinned incremental decoder
    gives where the two overlap: the first-step logits of generate(), and the per-token log-probabilities score_sequence() sums up at
    later positions.  Bound: two fp32 summation orders of the same network — each is at most 4.0e-5 away from the float64 result on this
    model (logit scale 19) — so 1e-4; the float64 result itself lies within the same distance of both."""
    sd, rc, _, _ = tiny2
    audio = GI.tiny_recording(5000, 3, variant="tiny2")
    feats = torch.from_numpy(np.stack([s[2] for s in F.sliced_audio_features(audio, TM.SR, 0, TM.STS, 1)]))
    gp = W.GenParams(prompt=TM.PROMPT, eos_token_id=TM.EOT, pad_token_id=TM.EOT, max_length=24, num_beams=1,
                     suppress_tokens=TM.SUPPRESS, begin_suppress_tokens=TM.BEGIN_SUPPRESS)
    seqs, first = W.generate(sd, rc, feats, gp, return_first_logits=True)
    P = len(TM.PROMPT)
    for i in range(feats.shape[0]):
        got32 = W.teacher_forced_logits(sd, rc, feats[i], [TM.PROMPT], dtype=torch.float32)
        got64 = W.teacher_forced_logits(sd, rc, feats[i], [TM.PROMPT])
        assert got32.dtype == torch.float32 and got64.dtype == torch.float64 and got64.shape == (1, rc.vocab_size)
        assert (got32[0] - first[i]).abs().max().item() <= 1e-4
        assert (got64[0] - first[i].double()).abs().max().item() <= 1e-4
    # later positions: score_sequence == mean of log_softmax(teacher-forced logits)[next token] over the generated tokens
    toks = W.canonical(seqs[0].tolist(), P, TM.EOT, TM.PROMPT)
    full = list(TM.PROMPT) + toks
    assert len(toks) >= 6
    want = W.score_sequence(sd, rc, feats[0:1], gp, full)
    for dtype in (torch.float32, torch.float64):
        total = 0.0
        for k in range(len(toks)):
            # two rows per call: rows are independent, the second one is a shorter history padded by repeating itself
            lg = W.teacher_forced_logits(sd, rc, feats[0:1], [full[:P + k], full[:P + k]], dtype=dtype)
            assert torch.equal(lg[0], lg[1])
            total += float(torch.log_softmax(lg[0].double(), dim=-1)[toks[k]])
        assert abs(total / len(toks) - want) <= 1e-4, (dtype, total / len(toks), want)
    # the decoder's fp32 behaviour is unchanged: keep_dtype only matters for non-fp32 weights
    dec = W.Decoder(sd, rc, W.encoder_forward(sd, rc, feats[0:1]))
    assert dec.step(torch.tensor([TM.PROMPT])).dtype == torch.float32
    sd64 = {k: v.double() for k, v in sd.items()}
    enc64 = W.encoder_forward(sd64, rc, feats[0:1].double())
    assert W.Decoder(sd64, rc, enc64).step(torch.tensor([TM.PROMPT])).dtype == torch.float32
    assert W.Decoder(sd64, rc, enc64, keep_dtype=True).step(torch.tensor([TM.PROMPT])).dtype == torch.float64
