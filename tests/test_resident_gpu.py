"""The pictures in every form the `patch_*` functions take — what segment* returned, a numpy array, a device tensor that is searched
where it lies — give one result; the command line with every analysis at once writes what it writes with one at a time; and an
`out` that is no tensor, or lies on another device, is refused by the per-segment launch functions."""
import os
import sys

import numpy as np
import pytest
import torch

import golden_inputs as GI
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import _lib, dtw as DW, embed as EM, linkage as LK, measure as M, neighbors as NB, patches as P, pca as PC, pitch as PT

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
GUARD = 3                              # NaN pictures in front of and behind the resident ones


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_pictures_in_three_forms_give_one_result(gpu_lib):
    n, mels, width = 37, 80, 8
    p = np.random.default_rng(37).standard_normal((n, mels, width)).astype(np.float32)
    preds = [{"patch": p[:20]}, [{"patch": p[20:21]}, {"patch": p[21:]}]]
    whole = torch.full((n + 2 * GUARD, mels, width), float("nan"), dtype=torch.float32, device="cuda")
    whole[GUARD:GUARD + n] = torch.from_numpy(p).cuda()
    before = whole.view(torch.int32).cpu().numpy().copy()
    held = whole[GUARD:GUARD + n]
    calls = (("neighbors", lambda x: NB.patch_neighbors(x, 5)), ("dtw", lambda x: DW.patch_dtw_neighbors(x, 5)),
             ("clusters", lambda x: LK.patch_clusters(x, 3)), ("embedding", lambda x: EM.patch_embedding(x, k=5, epochs=20, seed=2, init="pca")),
             ("pca", lambda x: PC.patch_pca(x, 4)))
    for what, call in calls:
        first = call(preds)
        assert all(isinstance(v, np.ndarray) and len(v) for v in first.values()), what
        for form in (p, held):
            got = call(form)
            assert list(got) == list(first), what
            for name in first:
                assert same_bits(got[name], first[name]), (what, name)
    assert np.array_equal(whole.view(torch.int32).cpu().numpy(), before)               # the pictures' bits and their guards: untouched
    assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + n:]).all() and held.data_ptr() == whole[GUARD].data_ptr()


def test_an_out_that_is_no_tensor_or_lies_elsewhere_is_refused(gpu_lib):
    sr = 16000
    pcm = torch.zeros(4000, dtype=torch.float32, device="cuda")
    tables = P.device_tables(sr, 0, None, pcm.device)
    n_frames = int(PT.frame_offsets_of([(10, 3000)], 256, 128)[-1])
    launches = ((lambda out: M.measure_rows(pcm, [(10, 3000)], 512, 1, 256, out=out), (1, 8)),
                (lambda out: P.patch_rows(pcm, [(10, 3000)], tables, 8, out=out), (1, 80, 8)),
                (lambda out: PT.pitch_rows(pcm, [(10, 3000)], 8, 256, 128, out=out), (n_frames, 3)))
    for launch, shape in launches:
        good = torch.empty(shape, dtype=torch.float32, device="cuda")
        got = launch(good)
        assert (got[0] if isinstance(got, tuple) else got).data_ptr() == good.data_ptr()      # a good one is used
        for bad in (np.zeros(shape, np.float32), [0.0], torch.empty(shape, dtype=torch.float32), torch.empty(shape, dtype=torch.float64, device="cuda")):
            with pytest.raises(_lib.WsegError, match="^out must"):
                launch(bad)
        if torch.cuda.device_count() > 1:
            with pytest.raises(_lib.WsegError, match="^out must"):
                launch(torch.empty(shape, dtype=torch.float32, device="cuda:1"))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def s16(v):
    return np.clip(np.round(np.asarray(v, np.float64) * 32768), -32768, 32767).astype(np.int64)


def test_cli_with_every_analysis_at_once(gpu_lib, tmp_path, monkeypatch):
    """One run with --neighbors, --clusters, --embed (PCA start) and --pca against the runs with one of them each: every array of the
    archive is the same-named array of the single-flag run, bit for bit."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    monkeypatch.setenv("WHISPERSEG_AMD_DTYPE", "f32")
    tiny = tmp_path / "tiny.wav"
    tiny.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", s16(GI.tiny_recording(3, 2)))))
    base = ["--model_path", MODEL_DIR, "--audio_path", str(tiny), "--spec_time_step", str(TM.STS)]
    single = {"neighbors": ["--neighbors", "3"], "clusters": ["--clusters", "2"],
              "embed": ["--embed", "2", "--embed_neighbors", "3", "--embed_init", "pca"], "pca": ["--pca", "2"]}

    def run(name, flags):
        csv, npz = tmp_path / (name + ".csv"), tmp_path / (name + ".npz")
        segment.main(base + ["--csv_save_path", str(csv), "--patches", "8", "--patches_save_path", str(npz)] + flags)
        with np.load(npz) as arch:
            return csv.read_bytes(), {name: arch[name] for name in arch.files}

    csv, full = run("full", [flag for flags in single.values() for flag in flags])
    assert list(full) == ["patch", "onset", "offset", "cluster", "neighbor_index", "neighbor_distance", "patch_cluster", "mst_edges", "mst_weight",
                          "embedding", "pca_mean", "pca_components", "pca_variance", "pca_variance_ratio", "pca_scores"]
    rows = len(full["patch"])
    assert rows >= 3 and full["embedding"].shape == (rows, 2) and full["pca_scores"].shape == (rows, 2) and full["neighbor_index"].shape == (rows, 3)
    seen = set()
    for name, flags in single.items():
        one_csv, one = run(name, flags)
        assert one_csv == csv and set(one) <= set(full) and len(one) > 4, name
        for key, value in one.items():
            assert same_bits(full[key], value), (name, key)
        seen |= set(one)
    assert seen == set(full)
