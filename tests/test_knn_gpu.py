"""Nearest neighbours on the GPU (wseg_knn_f32, whisperseg_amd/csrc/wseg_knn.hip) against the host definition
whisperseg_amd.neighbors.neighbors_host, from the kernels up to patch_neighbors and the CLI's --neighbors.

What may differ from the definition, and by how much, is derived in tests/knn_cases.py: nothing on integer inputs (every quantity is
exact in float32, the ties at the k-th boundary included), and on float inputs only candidates within 2 tau of the k-th distance,
with every reported distance the direct form's to one float32 ulp.  The shapes are the smallest at which the kernels can go wrong:
ragged query and candidate tiles, D = 1, 3, 17 and 2 562 (the zero-filled tail, the scalar loads), the longest row, every k class,
several candidate splits.  Every device run reads its rows between NaN rows and writes between guard rows."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import golden_inputs as GI
import knn_cases as KC
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import neighbors as NB

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
GUARD_BITS = 0x7fc12345               # float guards: a NaN no kernel writes
GUARD_INDEX = -0x12345                # int32 guards


def guarded_rows(rows):
    """-> the rows as a device tensor inside a larger one, a NaN row in front and behind."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    whole = torch.full((len(rows) + 2, rows.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
    whole[1:len(rows) + 1] = torch.from_numpy(rows).cuda()
    return whole[1:len(rows) + 1]


def device_knn(queries, corpus, k):
    """knn_rows on guarded inputs into guarded outputs -> (index, distance) as numpy; the guards must survive and every entry must be
    a row of the corpus with a finite distance, or -1 / +inf."""
    q = guarded_rows(queries)
    x = None if corpus is None else guarded_rows(corpus)
    m, n = len(queries), len(queries if corpus is None else corpus)
    held_i = torch.full((m + 2, k), GUARD_INDEX, dtype=torch.int32, device="cuda")
    held_d = torch.from_numpy(np.full((m + 2, k), GUARD_BITS, np.uint32).view(np.float32)).cuda()
    got_i, got_d = NB.knn_rows(q, x, k, out_index=held_i[1:m + 1], out_distance=held_d[1:m + 1])
    assert got_i.data_ptr() == held_i[1:m + 1].data_ptr() and got_d.data_ptr() == held_d[1:m + 1].data_ptr()
    index, distance = held_i.cpu().numpy(), held_d.cpu().numpy()
    for edge in (0, -1):
        assert (index[edge] == GUARD_INDEX).all() and (distance[edge].view(np.uint32) == GUARD_BITS).all(), "a guard row was written"
    index, distance = index[1:-1], distance[1:-1]
    found = index >= 0
    assert (index[found] < n).all() and np.isfinite(distance[found]).all() and (index[~found] == -1).all() and np.isposinf(distance[~found]).all()
    return np.ascontiguousarray(index), np.ascontiguousarray(distance)


@functools.lru_cache(maxsize=None)
def device_case(kind, *shape):
    """The device's lists of a case of knn_cases.reference: computed once, shared, never modified."""
    ref = KC.reference(kind, *shape)
    index, distance = device_knn(ref.q, None if ref.own else ref.x, ref.k)
    index.setflags(write=False)
    distance.setflags(write=False)
    return index, distance


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("shape", KC.INTEGER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_self_search_is_exact(gpu_lib, shape):
    """Every quantity is an exact integer in float32: the definition entry for entry, the ties at the k-th boundary included."""
    KC.check_exact(KC.reference("integer", *shape), *device_case("integer", *shape), what=shape)


def test_integer_queries_against_a_corpus(gpu_lib):
    """M = 37 queries, N = 500, D = 81, a row's own index a candidate like any other; ten queries are corpus rows and find them at 0."""
    ref = KC.reference("cross")
    index, distance = device_case("cross")
    KC.check_exact(ref, index, distance, what="cross")
    for i, j in KC.cross_case()[2].items():
        assert distance[i, 0] == 0 and (index[i, 0] == j or np.array_equal(ref.x[index[i, 0]], ref.x[j])), (i, j)
        assert index[i, 0] == ref.index[i, 0]


@pytest.mark.parametrize("shape", KC.CLUSTERED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float_rows_within_the_slack(gpu_lib, shape):
    """Clustered float rows: the slack contract on every row, the definition's set on the decided ones — at least 90 % of them."""
    share = KC.check_contract(KC.reference("clustered", *shape), *device_case("clustered", *shape), what=shape)
    print(f"(D, N, k) = {shape}: {100 * share:.1f} % of the rows decided")
    assert share >= KC.MIN_DECIDED


def test_float_rows_at_the_patch_size(gpu_lib):
    """D = 2 560: uniform rows (about half decided: the contract alone), and real pictures with five duplicates, which find each other
    at distance exactly 0 in first place."""
    share = KC.check_contract(KC.reference("uniform"), *device_case("uniform"), what="uniform")
    print(f"uniform D = 2560: {100 * share:.1f} % of the rows decided")
    rows = KC.picture_rows()
    ref = KC.reference("pictures", 3)
    index, distance = device_case("pictures", 3)
    share = KC.check_contract(ref, index, distance, what="pictures")
    print(f"{len(rows)} pictures: {100 * share:.1f} % of the rows decided")
    n = len(rows) - 5
    for i in range(5):
        for a, b in ((i, n + i), (n + i, i)):
            assert distance[a, 0] == 0 and np.array_equal(rows[index[a, 0]], rows[a]) and index[a, 0] != a, (a, b, index[a].tolist())
            assert index[a, 0] == ref.index[a, 0]


def test_same_bits_on_every_run_and_for_every_grid(gpu_lib, monkeypatch):
    cases = (("integer", 1000, 80, 15), ("clustered", 80, 1500, 15))
    for case in cases:
        ref = KC.reference(*case)
        assert same_bits(device_knn(ref.q, None, ref.k), device_case(*case)), case
    for cap in ("1", "2", "7"):
        monkeypatch.setenv("WSEG_KNN_GRID", cap)
        for case in cases:
            ref = KC.reference(*case)
            assert same_bits(device_knn(ref.q, None, ref.k), device_case(*case)), (case, cap)
    monkeypatch.delenv("WSEG_KNN_GRID")
    ref = KC.reference(*cases[1])
    assert same_bits(device_knn(ref.q, None, ref.k), device_case(*cases[1]))


def test_invalid_calls_are_refused_before_a_launch(gpu_lib):
    from whisperseg_amd import _lib
    x = torch.from_numpy(KC.integer_rows(64, 16)).cuda()
    for k in (0, 65):
        with pytest.raises(ValueError, match="k must"):
            NB.knn_rows(x, None, k)
        with pytest.raises(ValueError, match="k must"):
            NB.neighbors(x, None, k)
    for d in (0, 20481):
        with pytest.raises(ValueError, match="D must"):
            NB.knn_rows(torch.zeros((3, d), device="cuda"), None, 2)
    with pytest.raises(ValueError, match="same D"):
        NB.knn_rows(x, x[:, :8].contiguous(), 2)
    with pytest.raises(ValueError, match="2-D"):
        NB.knn_rows(x[0], None, 2)
    with pytest.raises(_lib.WsegError, match="no CPU path"):
        NB.knn_rows(x.cpu(), None, 2)
    with pytest.raises(_lib.WsegError, match="no CPU path"):
        NB.knn_rows(x, x.cpu(), 2)
    with pytest.raises(_lib.WsegError, match="contiguous"):
        NB.knn_rows(x.t(), None, 2)
    with pytest.raises(_lib.WsegError, match="contiguous"):
        NB.knn_rows(x, x[:, ::2], 2)
    with pytest.raises(_lib.WsegError, match="contiguous"):
        NB.knn_rows(x.double(), None, 2)
    if torch.cuda.device_count() > 1:
        with pytest.raises(_lib.WsegError, match="corpus is on"):
            NB.knn_rows(x, x.to("cuda:1"), 2)
        with pytest.raises(_lib.WsegError, match="out_index"):
            NB.knn_rows(x, None, 2, out_index=torch.empty((64, 2), dtype=torch.int32, device="cuda:1"))
    for bad in (torch.empty((64, 3), dtype=torch.int32, device="cuda"), torch.empty((63, 2), dtype=torch.int32, device="cuda"),
                torch.empty((64, 2), dtype=torch.int64, device="cuda"), torch.empty((64, 2), dtype=torch.int32), torch.empty((64, 4), dtype=torch.int32, device="cuda")[:, ::2]):
        with pytest.raises(_lib.WsegError, match="out_index"):
            NB.knn_rows(x, None, 2, out_index=bad)
    for bad in (torch.empty((64, 3), device="cuda"), torch.empty((64, 2), dtype=torch.float64, device="cuda"), torch.empty((64, 2))):
        with pytest.raises(_lib.WsegError, match="out_distance"):
            NB.knn_rows(x, None, 2, out_distance=bad)
    # no queries: an empty result; no corpus rows: -1 / +inf everywhere (between intact guards)
    for corpus in (None, x):
        index, distance = NB.knn_rows(x[:0], corpus, 4)
        assert index.shape == distance.shape == (0, 4) and index.dtype == torch.int32 and distance.dtype == torch.float32 and index.is_cuda
    index, distance = device_knn(KC.integer_rows(64, 16), np.zeros((0, 16), np.float32), 4)
    assert index.shape == (64, 4) and (index == -1).all() and np.isposinf(distance).all()
    index, distance = NB.neighbors(KC.integer_rows(5, 7), np.zeros((0, 7), np.float32), 3)
    assert (index == -1).all() and np.isposinf(distance).all()
    index, distance = NB.neighbors(np.zeros((0, 7), np.float32), None, 3)
    assert index.shape == distance.shape == (0, 3)


def test_public_call_gives_the_kernels_bits(gpu_lib):
    """neighbors() from numpy and from a resident tensor, self-search and against a corpus."""
    for case in (("integer", 65, 17, 15), ("clustered", 16, 1500, 10), ("cross",)):
        ref = KC.reference(*case)
        corpus = None if ref.own else ref.x
        for q, x in ((ref.q, corpus), (guarded_rows(ref.q), None if ref.own else guarded_rows(ref.x)), (torch.from_numpy(ref.q), corpus)):
            got = NB.neighbors(q, x, ref.k)
            assert isinstance(got[0], np.ndarray) and got[0].dtype == np.int32 and got[1].dtype == np.float32
            assert same_bits(got, device_case(*case)), case


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seg():
    from whisperseg_amd.model import WhisperSegmenter
    return WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")


def s16(v):
    return np.clip(np.round(np.asarray(v, np.float64) * 32768), -32768, 32767).astype(np.int64)


@pytest.fixture(scope="module")
def tiny_wav(tmp_path_factory):
    """A recording of the fixture model's own signal family as an s16 file: the model finds rows in it."""
    tiny = tmp_path_factory.mktemp("knn") / "tiny.wav"
    tiny.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", s16(GI.tiny_recording(3, 2)))))
    return str(tiny)


KW = dict(spec_time_step=TM.STS)


def check_archive_lists(patch, index, distance, k, what):
    rows = np.ascontiguousarray(patch.reshape(len(patch), patch.shape[1] * patch.shape[2]))
    assert index.shape == distance.shape == (len(rows), k) and index.dtype == np.int32 and distance.dtype == np.float32, what
    if len(rows):
        KC.check_contract(KC.Reference(rows, None, k), index, distance, what=what)


def test_patch_neighbors_of_a_segmentation(gpu_lib, seg, tiny_wav):
    from whisperseg_amd.wavio import load_wav
    total = 0
    for path in (os.path.join(GOLDEN, "meerkat_5s.wav"), tiny_wav):
        pred = seg.segment(*load_wav(path), patches=8, **KW)
        got = NB.patch_neighbors([pred], 3)
        assert list(got) == ["neighbor_index", "neighbor_distance"]
        check_archive_lists(pred["patch"], got["neighbor_index"], got["neighbor_distance"], 3, os.path.basename(path))
        total += len(pred["onset"])
    assert total >= 3                                  # not vacuous: the fixture model finds rows in its own signal family
    # per-channel lists, as segment_files(channel_id="all") returns them: rows in file, channel, row order
    preds = seg.segment_files([tiny_wav, tiny_wav], channel_id="all", patches=8, **KW)
    got = NB.patch_neighbors(preds, 2)
    flat = np.concatenate([r["patch"] for res in preds for r in res], axis=0)
    check_archive_lists(flat, got["neighbor_index"], got["neighbor_distance"], 2, "two files, every channel")
    twin = got["neighbor_index"][:, 0]
    assert len(flat) >= 2 and (got["neighbor_distance"][:, 0] == 0).all()       # the same file twice: every row has a twin
    assert (twin != np.arange(len(flat))).all() and np.array_equal(flat[twin], flat)


def test_cli_neighbors(gpu_lib, seg, tiny_wav, tmp_path, monkeypatch):
    from whisperseg_amd.wavio import load_wav
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    monkeypatch.setenv("WHISPERSEG_AMD_DTYPE", "f32")
    base = ["--model_path", MODEL_DIR, "--audio_path", tiny_wav, "--spec_time_step", str(TM.STS)]
    plain_csv, full_csv, plain_npz, full_npz = tmp_path / "plain.csv", tmp_path / "full.csv", tmp_path / "plain.npz", tmp_path / "full.npz"
    segment.main(base + ["--csv_save_path", str(plain_csv), "--patches", "8", "--patches_save_path", str(plain_npz)])
    segment.main(base + ["--csv_save_path", str(full_csv), "--patches", "8", "--patches_save_path", str(full_npz), "--neighbors", "3"])
    assert full_csv.read_bytes() == plain_csv.read_bytes() and len(plain_csv.read_text().splitlines()) > 3
    with np.load(plain_npz) as plain, np.load(full_npz) as full:
        assert set(plain.files) == {"patch", "onset", "offset", "cluster"}                       # without the flag: exactly the keys there were
        assert set(full.files) == set(plain.files) | {"neighbor_index", "neighbor_distance"}
        assert all(np.array_equal(plain[name], full[name]) for name in plain.files)
        rows = len(plain_csv.read_text().splitlines()) - 1
        assert full["patch"].shape == (rows, 80, 8) and full["neighbor_index"].shape == full["neighbor_distance"].shape == (rows, 3)
        check_archive_lists(full["patch"], full["neighbor_index"], full["neighbor_distance"], 3, "the archive")
        want = seg.segment(*load_wav(tiny_wav), patches=8, **KW)
        got = NB.patch_neighbors([want], 3)
        assert np.array_equal(full["neighbor_index"], got["neighbor_index"])
        assert np.array_equal(full["neighbor_distance"].view(np.uint32), got["neighbor_distance"].view(np.uint32))
    # folder mode with every channel: the indices count the archive's rows, which are the CSV's
    folder = tmp_path / "wavs"
    folder.mkdir()
    for name in ("a.wav", "b.wav"):
        (folder / name).write_bytes(open(tiny_wav, "rb").read())
    out_csv, out_npz = tmp_path / "folder.csv", tmp_path / "folder.npz"
    segment.main(["--model_path", MODEL_DIR, "--audio_folder", str(folder), "--spec_time_step", str(TM.STS), "--channel_id", "all",
                  "--csv_save_path", str(out_csv), "--patches", "8", "--patches_save_path", str(out_npz), "--neighbors", "2"])
    with np.load(out_npz) as arch:
        lines = out_csv.read_text().splitlines()
        assert arch["neighbor_index"].shape == (len(lines) - 1, 2) and len(lines) - 1 == 2 * rows
        check_archive_lists(arch["patch"], arch["neighbor_index"], arch["neighbor_distance"], 2, "folder mode")
        twin = arch["neighbor_index"][:, 0]
        assert (arch["neighbor_distance"][:, 0] == 0).all() and (twin != np.arange(len(twin))).all()      # two copies of one file: a twin each
        assert np.array_equal(arch["patch"][twin], arch["patch"])
