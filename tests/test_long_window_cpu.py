"""Host side of windows longer than 1000 spectrogram columns (checkpoints trained with `--total_spec_columns` up to 3000): the window table,
time tokens above <|1000|>, and the model directory tools/tiny_model.py writes for another column count."""
import json
import os

import pytest
import torch

import golden_inputs as GI
from oracle import frontend as OF
from oracle import whisper_ref as R
from tools import tiny_model as TM


@pytest.mark.parametrize("cols", [1500, 3000])
def test_window_table_equals_the_oracle(cols):
    from whisperseg_amd.windows import clip_length_samples, window_table
    for sr, sts, n, trials in GI.WINDOW_TABLE_CASES:
        want = OF.window_table(n, sr, sts, trials, cols)
        got = window_table(n, sr, sts, trials, cols)
        assert len(got) == len(want) >= trials
        for w, (trial_id, pos, n_pad, _, offset_time, clip_len) in zip(got, want):
            assert (w.trial_id, w.start, w.offset_time, w.clip_seconds) == (trial_id, pos - n_pad, offset_time, clip_len / sr), (cols, sr, sts, n, trials)
        assert clip_length_samples(cols, sts, sr) == int(cols * sts * sr)


def test_time_tokens_above_1000_are_parsed():
    from whisperseg_amd import postprocess
    sts = 0.005
    text = "<|startoftranscript|><|en|><|notimestamps|><|unknown|><|12|>0<|998|><|1002|>1<|1499|><|1500|>2<|1500|><|endoftext|>"
    rows = postprocess.extract_segments(text, sts, TM.CLUSTER_CODEBOOK)
    assert rows == [[12 * sts * 2, 998 * sts * 2, "a"], [1002 * sts * 2, 1499 * sts * 2, "b"]]      # (the empty segment is dropped)
    windows = [(0, 0.0, None, 15.0), (0, 15.0, None, 3.0)]
    pred = postprocess.parse_generation([text, "<|2900|>2<|3000|>"], windows, TM.CLUSTER_CODEBOOK, 2 * sts, 18.0, sts, 1, 8 * sts, sts, "clustering")
    assert pred["cluster"] == ["a", "b"] and pred["offset"][1] == pytest.approx(14.99)      # the second window's segment lies past the recording's end


def test_the_default_column_count_writes_the_committed_fixture(golden_dir):
    with open(os.path.join(golden_dir, "tiny_model", "config.json")) as f:
        assert TM.hf_config_dict() == json.load(f)
    with open(os.path.join(golden_dir, "tiny_model", "added_tokens.json")) as f:
        assert TM.added_tokens() == json.load(f)
    assert (TM.vocab_size(), TM.species0()) == (TM.VOCAB_SIZE, TM.SPECIES0)
    for bad in (1501, 254, 3002):
        with pytest.raises(ValueError):
            TM.hf_config_dict("tiny", bad)


@pytest.mark.parametrize("cols", [1500, 3000])
def test_model_directory_for_another_column_count_round_trips(tmp_path, cols):
    from whisperseg_amd.checkpoint import LazyCheckpoint
    from whisperseg_amd.engine import geometry_from_config
    from whisperseg_amd.tokenizer import WhisperSegTokenizer
    cfg = TM.hf_config_dict("tiny", cols)
    assert cfg["total_spec_columns"] == cols and cfg["max_source_positions"] == cols // 2
    assert cfg["vocab_size"] % 128 == 0 and cfg["vocab_size"] >= TM.species0(cols) + len(TM.SPECIES)
    sd = R.random_state_dict(R.RefConfig.from_hf_dict(cfg), seed=3)
    mdir = str(tmp_path / "m")
    TM.write_model_dir(mdir, sd, "tiny", cols)
    with open(os.path.join(mdir, "config.json")) as f:
        on_disk = json.load(f)
    geo = geometry_from_config(on_disk)
    assert (geo["spec_cols"], geo["enc_positions"], geo["vocab"]) == (cols, cols // 2, cfg["vocab_size"])
    ckpt = LazyCheckpoint(mdir)
    try:
        assert set(ckpt.keys()) == set(sd)
        pos = ckpt["model.encoder.embed_positions.weight"]
        assert tuple(pos.shape) == (cols // 2, cfg["d_model"]) and torch.equal(pos.float(), sd["model.encoder.embed_positions.weight"])
        assert tuple(ckpt["model.decoder.embed_tokens.weight"].shape) == (cfg["vocab_size"], cfg["d_model"])
    finally:
        ckpt.close()
    tok = WhisperSegTokenizer.from_pretrained(mdir, language="english")
    last = "<|%d|>" % cols
    ids = tok.convert_tokens_to_ids([last, "<|1001|>", "<|0|>", "<|unknown|>"])
    assert ids == [TM.TIME0 + cols, TM.TIME0 + 1001, TM.TIME0, TM.species0(cols) + TM.SPECIES.index("<|unknown|>")]
    assert len(set(ids)) == 4 and max(ids) < cfg["vocab_size"]
    assert tok.decode([ids[0], 15, ids[1]]) == last + "0<|1001|>"
