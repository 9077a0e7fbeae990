"""What the analyses share on the Python side (whisperseg_amd/resident.py), the one statement of the pictures' row order
(neighbors.patch_pictures_of) and the command line's analysis function (scripts/segment.py::analyses), as far as they can be held to
their word without a GPU: every refusal that happens before a device is touched, and the uploads of the command line counted with
the device steps replaced by the host definitions."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from whisperseg_amd import _lib, dtw as DW, embed as EM, linkage as LK, neighbors as NB, pca as PC, resident as RS


class OnDevice(torch.Tensor):
    """A host tensor that says it lies on a device: check_tensor then goes on to its other conditions, one at a time.  Nothing is
    ever launched on it."""
    is_cuda = property(lambda self: True)


def on_device(t):
    return t.as_subclass(OnDevice)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_check_tensor_refuses_each_defect_with_the_callers_words():
    cpu = torch.device("cpu")
    good = on_device(torch.zeros((4, 6)))
    RS.check_tensor(good, "the rows of a_launch", "[N, D]")
    RS.check_tensor(good, "the rows of a_launch", "[N, D]", torch.float32, (4, 6), cpu, ndim=2)
    RS.check_tensor(on_device(torch.zeros(4, dtype=torch.int32)), "component", "[N]", torch.int32, (4,), cpu)
    # the defects, each alone
    for bad in (torch.zeros((4, 6)),                                   # a CPU tensor
                on_device(torch.zeros((4, 6), dtype=torch.float64)),   # a float64 tensor
                on_device(torch.zeros((6, 4))).t(),                    # a transposed view
                on_device(torch.zeros((4, 12)))[:, ::2],               # a strided view
                np.zeros((4, 6), np.float32), None, [[0.0] * 6] * 4):  # no tensor at all
        with pytest.raises(_lib.WsegError, match=r"the rows of a_launch must be a contiguous float32 device tensor \[N, D\] \(no CPU path\)"):
            RS.check_tensor(bad, "the rows of a_launch", "[N, D]")
    assert isinstance(on_device(torch.zeros((6, 4))).t(), OnDevice)                    # (the views above are still "on the device")
    with pytest.raises(_lib.WsegError, match="the recording of x_rows must be a contiguous.*no CPU path"):
        RS.check_tensor(good, "the recording of x_rows", "[n]", ndim=1)                # a wrong rank
    RS.check_tensor(on_device(torch.zeros(5)), "the recording of x_rows", "[n]", ndim=1)
    for shape in ((4, 5), (3, 6), (4,), (4, 6, 1)):                                    # a wrong shape
        with pytest.raises(_lib.WsegError, match="core must be a contiguous float32"):
            RS.check_tensor(good, "core", "[N]", torch.float32, shape, cpu)
    with pytest.raises(_lib.WsegError, match="component must be a contiguous int32 device tensor .* on meta"):
        RS.check_tensor(on_device(torch.zeros(4, dtype=torch.int32)), "component", "[N]", torch.int32, (4,), torch.device("meta"))      # another device


def test_out_tensor_checks_what_it_is_given_and_allocates_what_it_is_not():
    cpu = torch.device("cpu")
    new = RS.out_tensor(None, "out_index", "[M, k]", torch.int32, (5, 3), cpu)
    assert new.shape == (5, 3) and new.dtype == torch.int32 and new.device == cpu and new.is_contiguous()
    assert RS.out_tensor(None, "out", "[n_seg, 8]", torch.float32, [0, 8], cpu).shape == (0, 8)
    held = on_device(torch.zeros((5, 3), dtype=torch.int32))
    assert RS.out_tensor(held, "out_index", "[M, k]", torch.int32, (5, 3), cpu) is held
    for name, dtype in (("out_index", torch.int32), ("out_distance", torch.float32), ("out_weight", torch.float32), ("out", torch.float32)):
        wrong = torch.float64 if dtype == torch.float32 else torch.int64
        for bad in (np.zeros((5, 3), np.float32), [0] * 15, 0,                         # no tensor
                    on_device(torch.zeros((5, 3), dtype=wrong)),                       # the wrong dtype
                    on_device(torch.zeros((5, 4), dtype=dtype)), on_device(torch.zeros((3, 5), dtype=dtype)).t(),
                    torch.zeros((5, 3), dtype=dtype)):                                 # on the host
            with pytest.raises(_lib.WsegError, match=rf"^{name} must be a contiguous {str(dtype)[6:]} device tensor \[M, k\] on cpu"):
                RS.out_tensor(bad, name, "[M, k]", dtype, (5, 3), cpu)
    with pytest.raises(_lib.WsegError, match="^out must .* on meta"):
        RS.out_tensor(on_device(torch.zeros((5, 3))), "out", "[M, k]", torch.float32, (5, 3), torch.device("meta"))


def test_check_int():
    for bad in (True, False, 2.5, 3.0, "3", None, np.float32(3), np.bool_(True)):
        with pytest.raises(ValueError, match=r"k must be an integer in 1 \.\. 64"):
            RS.check_int(bad, "k", 1, 64)
    got = RS.check_int(np.int64(3), "k", 1, 64)
    assert got == 3 and type(got) is int and type(RS.check_int(np.uint8(7), "k", 1, 64)) is int
    for lo, hi in ((1, 64), (0, 0), (-3, 5), (2, 3)):
        assert RS.check_int(lo, "r", lo, hi) == lo and RS.check_int(hi, "r", lo, hi) == hi
        for past in (lo - 1, hi + 1):
            with pytest.raises(ValueError, match="r must"):
                RS.check_int(past, "r", lo, hi)
    with pytest.raises(ValueError, match=r"band must be an integer in 0 \.\. T - 1 = 7 \(got 8\)"):
        RS.check_int(8, "band", 0, 7, "in 0 .. T - 1 = 7")
    # the analyses' own checks are this one: their words survive
    for call, word in ((lambda: NB.check_k(65), "k must"), (lambda: NB.check_k(True), "k must"), (lambda: DW.check_band(8, 8), "band must"),
                       (lambda: DW.check_channels(129), "channels must"), (lambda: LK.check_samples(7, 7), "min_samples must"),
                       (lambda: LK.check_size(1, 2), "min_cluster_size must"), (lambda: PC.check_r(5, 5, 16), "r must"),
                       (lambda: EM.check_dim(4), "dim must"), (lambda: EM.check_embed(15, 2, 0.1, 1.0, 0), "epochs must"),
                       (lambda: EM.check_embed(15, 2.0, 0.1, 1.0, 5), "dim must")):
        with pytest.raises(ValueError, match=word):
            call()
    assert LK.check_size(10 ** 12, 2) == 10 ** 12 and DW.check_band(None, 64) == 8


def test_resident_and_shape_of_on_the_host():
    a = np.arange(24, dtype=np.float64).reshape(4, 6)[:, ::2]
    got = RS.resident(a, "cpu")
    assert got.dtype == torch.float32 and got.is_contiguous() and np.array_equal(got.numpy(), a.astype(np.float32))
    got = RS.resident(torch.from_numpy(a), "cpu")
    assert got.dtype == torch.float32 and got.is_contiguous() and np.array_equal(got.numpy(), a.astype(np.float32))
    lies = on_device(torch.zeros((4, 6)))
    assert RS.resident(lies, "meta").data_ptr() == lies.data_ptr()                     # a device tensor stays where it lies: no copy
    assert RS.shape_of(a) == (4, 3) and RS.shape_of(torch.zeros((2, 5))) == (2, 5) and RS.shape_of([[1, 2], [3, 4], [5, 6]]) == (3, 2)


def test_the_pictures_in_every_form_are_one_matrix():
    rng = np.random.default_rng(5)
    p = rng.standard_normal((7, 3, 2)).astype(np.float32)
    preds = [{"patch": p[:4]}, [{"patch": p[4:6]}, {"patch": p[6:]}]]
    for form in (preds, p, p.astype(np.float64), torch.from_numpy(p)):
        got = NB.patch_pictures_of(form)
        assert tuple(got.shape) == (7, 3, 2) and same_bits(np.asarray(got), p)
        rows = NB.patch_rows_of(form)
        assert tuple(rows.shape) == (7, 6) and same_bits(np.asarray(rows), p.reshape(7, 6))
    held = torch.from_numpy(p)
    assert NB.patch_pictures_of(held) is held and NB.patch_rows_of(held).data_ptr() == held.data_ptr()      # a tensor is used where it lies
    assert np.shares_memory(NB.patch_rows_of(p), p)
    assert NB.patch_pictures_of([]).shape == (0, 0, 0) and NB.patch_rows_of([]).shape == (0, 0)
    assert NB.patch_pictures_of([], none=(80, 8)).shape == (0, 80, 8) and NB.patch_pictures_of([], none=(80, 8)).dtype == np.float32
    for bad in (p.reshape(7, 6), torch.zeros((7, 6)), np.zeros((7, 3, 2, 1), np.float32)):
        with pytest.raises(ValueError, match="n_mels"):
            NB.patch_pictures_of(bad)
    # the empty and the single-row results, from pictures as from predictions
    for none in ([], p[:0], torch.from_numpy(p[:0])):
        d = 0 if isinstance(none, list) else 6
        assert NB.patch_neighbors(none, 3)["neighbor_index"].shape == (0, 3) and DW.patch_dtw_neighbors(none, 3)["neighbor_distance"].shape == (0, 3)
        found = LK.patch_clusters(none, 2)
        assert found["cluster"].shape == (0,) and found["mst_edges"].shape == (0, 2) and found["mst_weight"].shape == (0,)
        assert EM.patch_embedding(none, dim=3)["embedding"].shape == (0, 3)
        assert PC.patch_pca(none, 3)["pca_components"].shape == (0, d) and PC.patch_pca(none, 3)["pca_scores"].shape == (0, 3)
    for one in (p[:1], torch.from_numpy(p[:1])):
        found = LK.patch_clusters(one, 2)
        assert found["cluster"].tolist() == [-1] and found["cluster"].dtype == np.int32 and found["mst_edges"].shape == (0, 2)
        assert PC.patch_pca(one, 3)["pca_components"].shape == (0, 6) and PC.patch_pca(one, 3)["pca_mean"].dtype == np.float64
    with pytest.raises(ValueError, match="up to 64 columns"):
        DW.patch_dtw_neighbors(np.zeros((2, 3, 65), np.float32), 1)


# ---- the command line's analysis function ------------------------------------------------------------------------------------------
@pytest.fixture()
def segment():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    return segment


@pytest.fixture()
def host_steps(monkeypatch):
    """Every device step of the five analyses replaced by its host definition, and the one way to the device by a counter that
    leaves the array on the host.  -> the counts."""
    seen = {"resident": 0, "neighbors": 0}

    def counted(a, device):
        seen["resident"] += 1
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))

    def host_neighbors(queries, corpus=None, k=15, device="cuda"):
        seen["neighbors"] += 1
        return NB.neighbors_host(queries, corpus, k)

    monkeypatch.setattr(RS, "resident", counted)
    monkeypatch.setattr(NB, "neighbors", host_neighbors)
    monkeypatch.setattr(DW, "dtw_neighbors", lambda q, x=None, k=15, channels=80, band=None, device="cuda": DW.dtw_neighbors_host(q, x, k, channels, band))
    monkeypatch.setattr(LK, "mst", lambda rows, min_samples=5, device="cuda", stats=None: LK.mst_host(rows, min_samples))
    monkeypatch.setattr(PC, "pca", lambda rows, r, device="cuda", scores=True: PC.pca_host(rows, r))
    monkeypatch.setattr(EM, "layout_epochs", lambda run, device="cuda": torch.from_numpy(EM.host_epochs(run)))
    return seen


@pytest.mark.parametrize("metric", ("euclidean", "dtw"))
def test_the_command_line_uploads_the_pictures_once(segment, host_steps, metric):
    p = np.random.default_rng(11).standard_normal((7, 3, 2)).astype(np.float32)
    preds = [{"patch": p[:4]}, [{"patch": p[4:6]}, {"patch": p[6:]}]]
    flags = ["--neighbors", "2", "--clusters", "2", "--embed", "2", "--embed_neighbors", "3", "--embed_init", "pca", "--pca", "2"]
    dtw = metric == "dtw"
    args = segment.parse_args(["--model_path", "m", "--csv_save_path", "o.csv", "--patches", "2", "--patches_save_path", "p.npz"] + flags
                              + (["--neighbors_metric", "dtw"] if dtw else []))
    got = segment.analyses(p, args)
    assert host_steps["resident"] == 1
    # what the five calls return one by one
    want = dict(DW.patch_dtw_neighbors(preds, 2, None) if dtw else NB.patch_neighbors(preds, 2))
    if dtw:
        want.update(neighbor_metric=np.array("dtw"), neighbor_band=np.array(1, dtype=np.int64))
    found = LK.patch_clusters(preds, 2, 5)
    want.update(patch_cluster=found["cluster"], mst_edges=found["mst_edges"], mst_weight=found["mst_weight"])
    lists = DW.patch_dtw_neighbors(preds, 3, None) if dtw else None
    want.update(EM.patch_embedding(preds, 3, 2, 0.1, seed=0, init="pca", lists=lists and (lists["neighbor_index"], lists["neighbor_distance"])))
    want.update(PC.patch_pca(preds, 2))
    assert host_steps["resident"] == 1                                 # (the host definitions never look for a device)
    assert list(got) == list(want) and len(got) == (13 if dtw else 11)
    for name in want:
        assert same_bits(np.asarray(got[name]), np.asarray(want[name])), name
    assert got["embedding"].shape == (7, 2) and got["pca_scores"].shape == (7, 2) and got["neighbor_index"].shape == (7, 2)
    assert len(set(got["patch_cluster"].tolist())) >= 1 and got["mst_edges"].shape == (6, 2)


def test_the_command_line_shares_lists_of_one_k_and_asks_for_nothing_it_was_not_told(segment, host_steps):
    p = np.random.default_rng(12).standard_normal((7, 3, 2)).astype(np.float32)
    base = ["--model_path", "m", "--csv_save_path", "o.csv", "--patches", "2", "--patches_save_path", "p.npz"]
    assert segment.analyses(p, segment.parse_args(base)) == {} and host_steps["resident"] == 0        # no analysis: no upload
    got = segment.analyses(p, segment.parse_args(base + ["--neighbors", "3", "--embed", "2", "--embed_neighbors", "3"]))
    assert host_steps["resident"] == 1 and host_steps["neighbors"] == 1                                # the same K: the lists are computed once
    assert list(got) == ["neighbor_index", "neighbor_distance", "embedding"]
    lists = NB.neighbors_host(p.reshape(7, 6), None, 3)
    assert same_bits(got["embedding"], EM.patch_embedding(p, 3, 2, 0.1, seed=0, lists=lists)["embedding"])
    segment.analyses(p, segment.parse_args(base + ["--neighbors", "2", "--embed", "2", "--embed_neighbors", "3"]))
    assert host_steps["resident"] == 2 and host_steps["neighbors"] == 3                                # another K: the map's own lists
    # the archives' identifying columns come from one helper
    a = {"onset": [0.1, 0.2], "offset": [0.15, 0.3], "cluster": ["a", 1], "patch": p[:2]}
    c = {"onset": [0.5], "offset": [0.6], "cluster": ["c"], "patch": p[2:3]}
    arch = segment.patch_archive([[a, c], [c, a]], ["x.wav", "y.wav"], True, width=2)
    assert list(arch) == ["patch", "onset", "offset", "cluster", "filename", "channel"]
    assert arch["filename"].tolist() == ["x.wav"] * 3 + ["y.wav"] * 3 and arch["channel"].tolist() == [0, 0, 1, 0, 1, 1] and arch["channel"].dtype == np.int64
    assert arch["cluster"].tolist() == ["a", "1", "c", "c", "a", "1"] and arch["onset"].dtype == np.float64
    assert same_bits(arch["patch"], np.concatenate([p[:2], p[2:3], p[2:3], p[:2]]))
    none = segment.patch_archive([], None, False, width=8)
    assert list(none) == ["patch", "onset", "offset", "cluster"] and none["patch"].shape == (0, 80, 8) and none["patch"].dtype == np.float32
