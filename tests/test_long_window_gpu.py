"""Windows of more than 512 encoder positions (checkpoints trained with `--total_spec_columns` up to 3000: 1500 rows of Whisper's position
table), through the C-ABI against the oracle on seeded random weights.

Up to 512 positions the cross-attention kernels are the instantiations they always were; above, the same bodies run with LDS arrays for 1504
keys (wseg_dec.hip, CROSS_TK_LONG) and the encoder runs over fewer windows per pass.  Geometry, inputs and tolerances are those of
tests/test_model_gpu.py::test_other_window_lengths: a softmax-weighted average does not accumulate error with the key count beyond fp32
summation noise, so a mode that passes at 576 positions and fails at 1500 is a finding, not a tolerance to widen."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import whisper_ref as R
from test_model_gpu import EOS, PROMPT, hf_cfg, make

pytestmark = pytest.mark.gpu

MODES = ["f32", "f16x3", "bf16x3", "f16m6", "bf16", "f16"]
ENC_TOL = {"f32": 5e-4, "f16x3": 5e-4, "bf16x3": 5e-4, "f16m6": 5e-4, "bf16": 6e-2, "f16": 6e-2}
SUP, BSUP = [5, 6, 7, 200], [220, EOS]
_ORACLE = {}


def inputs(positions, n):
    g = torch.Generator().manual_seed(positions)
    return torch.randn(n, 80, 2 * positions, generator=g) * 0.5


def oracle(positions, n, nb, dtype):
    """Encoder output, tokens and first-step logits of the oracle, computed once per (geometry, weight rounding, beams)."""
    rounded = dtype in ("bf16", "f16")
    key = (positions, n, nb, rounded)
    if key not in _ORACLE:
        cfg = dict(hf_cfg(), max_source_positions=positions)
        rc = R.RefConfig.from_hf_dict(cfg)
        sd = R.random_state_dict(rc, seed=23)
        if rounded:
            sd = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}
        x = inputs(positions, n)
        gp = R.GenParams(prompt=PROMPT, eos_token_id=EOS, pad_token_id=EOS, max_length=10, num_beams=nb, suppress_tokens=SUP,
                         begin_suppress_tokens=BSUP)
        toks, logits = R.generate(sd, rc, x, gp, return_first_logits=True)
        _ORACLE[key] = (R.encoder_forward(sd, rc, x), toks, logits)
    return _ORACLE[key]


def engine(positions, dtype):
    return make(dict(hf_cfg(), max_source_positions=positions), dtype, seed=23)[2]


def gen(eng, x, nb, **kw):
    return eng.generate(x.cuda(), PROMPT, EOS, EOS, max_length=10, num_beams=nb, suppress_tokens=SUP, begin_suppress_tokens=BSUP, **kw)


def same_tokens(toks, lens, want, where):
    toks, lens = toks.cpu(), lens.cpu()
    for i in range(len(want)):
        assert R.canonical(toks[i, :lens[i]].tolist(), 3, EOS, PROMPT) == R.canonical(want[i].tolist(), 3, EOS, PROMPT), (where, i)


@pytest.mark.parametrize("positions", [576, 750, 1500])      # 512 + one key tile | the 1500-column checkpoint (no multiple of 4 or 64) | the maximum
@pytest.mark.parametrize("dtype", MODES)
def test_encoder_and_greedy_decode_match_the_oracle(gpu_lib, dtype, positions):
    eng = engine(positions, dtype)
    x = inputs(positions, 3)
    want, want_t, _ = oracle(positions, 3, 1, dtype)
    got = eng.encode(x.cuda()).float().cpu()
    assert got.shape == want.shape == (3, positions, 128)
    err, scale = (got - want).abs().max().item(), max(1.0, want.abs().max().item())
    print(dtype, positions, "encoder error", err, "of scale", scale)
    assert err <= ENC_TOL[dtype] * scale, (err, scale)
    if dtype not in ("bf16", "f16"):
        toks, lens = gen(eng, x, 1)
        same_tokens(toks, lens, want_t, (dtype, positions))


# first-step logits of the modes whose beam tokens are not pinned: the bounds of the existing first-logit checks of each mode —
# tests/test_model_gpu.py::test_first_logits_f32 (1e-3 absolute: the split modes on this geometry) and ::test_real_vocab_logits_bf16
# (8e-2 of the logit scale), tests/test_large_geometry_gpu.py::test_two_layer_8_windows_vs_oracle (f16: 0.015 of the logit scale)
def logit_bound(dtype, want):
    scale = max(1.0, want.abs().max().item())
    return {"bf16x3": 1e-3, "f16m6": 1e-3, "bf16": 8e-2 * scale, "f16": 0.015 * scale}[dtype]


@pytest.mark.parametrize("nb", [2, 4, 5])      # the 2- and 4-beam tiles of every row format; 5 beams: the general kernel (f16m6: hi | lo output, converted)
@pytest.mark.parametrize("dtype", MODES)
def test_every_beam_tile_at_750_positions(gpu_lib, dtype, nb):
    eng = engine(750, dtype)
    x = inputs(750, 3)
    _, want_t, want_l = oracle(750, 3, nb, dtype)
    toks, lens, got_l = gen(eng, x, nb, return_first_logits=True)
    err = (got_l.cpu() - want_l).abs().max().item()
    print(dtype, nb, "first-step logit error", err)
    if dtype in ("f32", "f16x3"):
        same_tokens(toks, lens, want_t, (dtype, nb))
    else:
        assert err <= logit_bound(dtype, want_l), (dtype, nb, err)


@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("dtype", ["f32", "f16x3"])
def test_refill_through_two_slots_gives_the_same_tokens(gpu_lib, dtype, nb):
    """5 windows through 2 slots: the slot map of the long-key kernels (prompt pass and decode step), and a window's tokens do not depend on
    how many windows were admitted with it."""
    eng = engine(750, dtype)
    x = inputs(750, 5)
    t_all, l_all = gen(eng, x, nb, n_slots=5)
    assert eng.last_stats()["n_admissions"] == 1
    t_two, l_two = gen(eng, x, nb, n_slots=2)
    st = eng.last_stats()
    assert st["n_slots"] == 2 and st["n_admissions"] > 1, st
    assert torch.equal(l_two.cpu(), l_all.cpu()) and torch.equal(t_two.cpu(), t_all.cpu())


def test_geometry_limits():
    from whisperseg_amd import _lib
    lib = _lib.load()

    def create(positions, cols):
        cfg = _lib.ModelConfig(d_model=128, n_heads=2, enc_layers=2, dec_layers=2, ffn=512, vocab=1280, n_mels=80, spec_cols=cols,
                               enc_positions=positions, dec_positions=448, dtype=1)
        h = C.c_void_p()
        st = lib.wseg_model_create(C.byref(cfg), C.byref(h))
        if st == 0:
            lib.wseg_model_destroy(h)
        return st, lib.wseg_last_error().decode()

    assert create(1500, 3000)[0] == 0
    for positions, cols in ((1501, 3002), (1500, 2999)):
        st, msg = create(positions, cols)
        assert st == -1 and "spec_cols" in msg, (positions, cols, st, msg)


def test_segment_with_a_1500_column_checkpoint(gpu_lib, tmp_path):
    """A random-weight model directory with total_spec_columns = 1500 (tools/tiny_model.py) through WhisperSegmenter.segment: one window longer
    than the 5-s clip, three trials.  f32: the rows of the oracle pipeline (oracle front-end, oracle generate, the product's parse_generation).
    f16x3 (the default mode): the same texts, or a differing window is a hypothesis the oracle scores like its own choice (flat random-weight
    distributions tie: tests/test_large_geometry_gpu.py::assert_equally_scored)."""
    from oracle import frontend as OF
    from test_large_geometry_gpu import assert_equally_scored
    from tools import tiny_model as TM
    from whisperseg_amd import postprocess
    from whisperseg_amd.model import WhisperSegmenter, get_n_fft_given_sr
    from whisperseg_amd.wavio import load_wav
    cols, sts, trials, ml = 1500, 0.005, 3, 16
    cfg = TM.hf_config_dict("tiny", cols)
    rc = R.RefConfig.from_hf_dict(cfg)
    sd = R.random_state_dict(rc, seed=31)
    mdir = str(tmp_path / "tiny1500")
    TM.write_model_dir(mdir, sd, "tiny", cols)
    audio, sr = load_wav(os.path.join(GOLDEN, "meerkat_5s.wav"))
    audio = np.asarray(audio, dtype=np.float32)
    assert cols * sts > len(audio) / sr
    kw = dict(spec_time_step=sts, num_trials=trials, max_length=ml, min_frequency=0)

    sliced = OF.sliced_audio_features(audio, sr, 0, sts, trials, total_spec_columns=cols)
    feats = torch.from_numpy(np.stack([s[2] for s in sliced]))
    assert feats.shape[1:] == (80, cols)
    gp = R.GenParams(prompt=TM.PROMPT, eos_token_id=TM.EOT, pad_token_id=TM.EOT, max_length=ml, num_beams=4, suppress_tokens=TM.SUPPRESS,
                     begin_suppress_tokens=TM.BEGIN_SUPPRESS)
    want_tokens = R.generate(sd, rc, feats, gp)

    seg = WhisperSegmenter(mdir, device="cuda", device_ids=[0], dtype="f32")
    assert seg.total_spec_columns == cols and seg.model_list[0].geo["enc_positions"] == cols // 2
    want_texts = seg.tokenizer_list[0].batch_decode([R.canonical(t.tolist(), 3, TM.EOT, TM.PROMPT) for t in want_tokens], skip_special_tokens=False)
    mine = seg.get_sliced_audios_features(audio, sr, 0, sts, trials)
    assert [(m[0], m[1], m[3]) for m in mine] == [(s[0], s[1], s[3]) for s in sliced]
    _, sts_, msl, eps, tpf = seg.resolve_segmentation_params(0, sts, None, None, None)
    want = seg.parse_generation(want_texts, sliced, msl, len(audio) / sr, sts_, trials, eps, tpf, "clustering")
    want = postprocess.drop_consecutive_duplicates(postprocess.correct_fft_blur(want, get_n_fft_given_sr(sr), sr))
    got = seg.segment(audio, sr, **kw)
    assert got == want
    t32, l32 = (t.cpu() for t in seg.decode_shard_tokens(mine, max_length=ml))
    for i, w in enumerate(want_tokens):
        assert R.canonical(t32[i, :l32[i]].tolist(), 3, TM.EOT, TM.PROMPT) == R.canonical(w.tolist(), 3, TM.EOT, TM.PROMPT), i

    seg3 = WhisperSegmenter(mdir, device="cuda", device_ids=[0])
    assert seg3.model_list[0].dtype_name == "f16x3"
    t3, l3 = (t.cpu() for t in seg3.decode_shard_tokens(seg3.get_sliced_audios_features(audio, sr, 0, sts, trials), max_length=ml))
    for i, w in enumerate(want_tokens):
        a, b = R.canonical(t3[i, :l3[i]].tolist(), 3, TM.EOT, TM.PROMPT), R.canonical(w.tolist(), 3, TM.EOT, TM.PROMPT)
        if a != b:
            assert_equally_scored(sd, rc, feats[i:i + 1], gp, t3[i, :l3[i]].tolist(), w.tolist(), ("1500 columns, f16x3", i))
