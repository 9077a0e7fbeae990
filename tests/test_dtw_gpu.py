"""Nearest neighbours under dynamic time warping on the GPU (wseg_dtw_knn_f32 / wseg_dtw_pairs_f64, whisperseg_amd/csrc/wseg_dtw.hip)
against the host definition whisperseg_amd.dtw.dtw_neighbors_host, from the kernels up to patch_dtw_neighbors and the CLI's
--neighbors_metric dtw.

What may differ from the definition, and by how much, is derived in tests/dtw_cases.py: nothing on integer inputs (every quantity is
exact in float32, the ties at the k-th boundary included), and on float inputs only candidates within 2 tau of the k-th distance,
with every reported distance the definition's float32 bits.  The shapes are the smallest at which the kernels can go wrong: ragged
query and candidate tiles, C = 1, 3, 17 (the zero-filled channel tail), T below, at and one past a 32-block and at 64, band 0, narrow
and full, every k class, several candidate splits.  Every device run reads its rows between NaN rows and writes between guard
rows."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import dtw_cases as DC
import golden_inputs as GI
import knn_cases as KC
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import dtw as DW
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


def device_dtw(queries, corpus, k, channels, band):
    """dtw_knn_rows on guarded inputs into guarded outputs -> (index, distance) as numpy; the guards must survive and every entry must
    be a row of the corpus with a finite distance, or -1 / +inf."""
    q = guarded_rows(queries)
    x = None if corpus is None else guarded_rows(corpus)
    m, n = len(queries), len(queries if corpus is None else corpus)
    held_i = torch.full((m + 2, k), GUARD_INDEX, dtype=torch.int32, device="cuda")
    held_d = torch.from_numpy(np.full((m + 2, k), GUARD_BITS, np.uint32).view(np.float32)).cuda()
    got_i, got_d = DW.dtw_knn_rows(q, x, k, channels, band, out_index=held_i[1:m + 1], out_distance=held_d[1:m + 1])
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
    """The device's lists of a case of dtw_cases.reference: computed once, shared, never modified."""
    ref = DC.reference(kind, *shape)
    index, distance = device_dtw(ref.q, None if ref.own else ref.x, ref.k, ref.channels, ref.band)
    index.setflags(write=False)
    distance.setflags(write=False)
    return index, distance


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("shape", DC.INTEGER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_self_search_is_exact(gpu_lib, shape):
    """Every quantity is an exact integer in float32: the definition entry for entry, the ties at the k-th boundary included."""
    DC.check_exact(DC.reference("integer", *shape), *device_case("integer", *shape), what=shape)
    n, c, t, band, k = shape
    if band == 0 and n > 1:            # the Euclidean device lists of the same rows
        index, distance = NB.knn_rows(torch.from_numpy(DC.integer_rows(n, c * t)).cuda(), None, k)
        assert same_bits((index.cpu().numpy(), distance.cpu().numpy()), device_case("integer", *shape))


def test_integer_queries_against_a_corpus(gpu_lib):
    """M = 37 queries, N = 500, C = T = 9, band 2, a row's own index a candidate like any other; ten queries are corpus rows and find
    them at 0."""
    ref = DC.reference("cross")
    index, distance = device_case("cross")
    DC.check_exact(ref, index, distance, what="cross")
    for i, j in DC.cross_case()[2].items():
        assert distance[i, 0] == 0 and (index[i, 0] == j or ref.dist[i, index[i, 0]] == 0), (i, j)
        assert index[i, 0] == ref.index[i, 0]


def test_warped_twins(gpu_lib):
    """Rows one step late: with a band every row finds its twin first, at distance exactly 0; with band 0 it does not, and the device
    agrees with the definition's Euclidean distance."""
    n = DC.TWINS["n"]
    twin = np.concatenate([n + np.arange(n), np.arange(n)])
    for band in (1, 3):
        ref = DC.reference("twins", band)
        index, distance = device_case("twins", band)
        DC.check_exact(ref, index, distance, what=("twins", band))
        assert np.array_equal(index[:, 0], twin) and (distance[:, 0] == 0).all()
    ref = DC.reference("twins", 0)
    index, distance = device_case("twins", 0)
    DC.check_exact(ref, index, distance, what=("twins", 0))
    assert (distance[:, 0] > 0).all() and (ref.dist[np.arange(2 * n), twin] > 0).all()
    knn = NB.knn_rows(torch.from_numpy(DC.twin_rows()).cuda(), None, DC.TWINS["k"])
    assert same_bits((knn[0].cpu().numpy(), knn[1].cpu().numpy()), (index, distance))


@pytest.mark.parametrize("shape", DC.FLOAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float_rows_within_the_slack(gpu_lib, shape):
    """Clustered float rows: the slack contract on every row, the definition's set on the decided ones — at least 90 % of them."""
    share = DC.check_contract(DC.reference("float", *shape), *device_case("float", *shape), what=shape)
    print(f"(C, T, N, band, k) = {shape}: {100 * share:.1f} % of the rows decided")
    assert share >= DC.MIN_DECIDED


def test_float_rows_at_the_largest_k(gpu_lib):
    """(7, 20, 400, 3, 64): about 0.907 of the rows decided — the contract alone, no floor on the share."""
    share = DC.check_contract(DC.reference("float", *DC.FLOAT_LOOSE), *device_case("float", *DC.FLOAT_LOOSE), what=DC.FLOAT_LOOSE)
    print(f"(C, T, N, band, k) = {DC.FLOAT_LOOSE}: {100 * share:.1f} % of the rows decided")


def test_real_pictures(gpu_lib):
    """Real pictures (C = 80, T = 32) with five duplicates, which find each other at distance exactly 0 in first place."""
    rows = KC.picture_rows()
    ref = DC.reference("pictures", 4, 3)
    index, distance = device_case("pictures", 4, 3)
    share = DC.check_contract(ref, index, distance, what="pictures")
    print(f"{len(rows)} pictures: {100 * share:.1f} % of the rows decided")
    n = len(rows) - 5
    for i in range(5):
        for a, b in ((i, n + i), (n + i, i)):
            assert distance[a, 0] == 0 and np.array_equal(rows[index[a, 0]], rows[a]) and index[a, 0] != a, (a, b, index[a].tolist())
            assert index[a, 0] == ref.index[a, 0]


@pytest.mark.parametrize("shape", ((80, 32, 150, 4), (5, 64, 120, 8)), ids=lambda s: "x".join(map(str, s)))
def test_pairs_have_the_definitions_bits(gpu_lib, shape):
    c, t, n, band = shape
    rows = DC.float_rows(c, t, n)
    rng = np.random.default_rng([DC.SEED, c, t, 11])
    pairs = rng.integers(0, n, (1000, 2))
    pairs[:10, 1] = pairs[:10, 0]                        # i == j among them
    want = DW.dtw_pairs_host(rows, rows, pairs, c, band)
    assert (want[:10] == 0).all() and (want[10:] > 0).any()
    for count in (0, 1, 1000):
        for q, x in ((rows, rows), (guarded_rows(rows), None)):
            got = DW.dtw_pairs(q, x, pairs[:count], c, band)
            assert got.dtype == np.float32 and got.shape == (count,)
            assert np.array_equal(got.view(np.uint32), want[:count].view(np.uint32)), (shape, count)
    got = DW.dtw_pairs(rows[:7], rows[100:], torch.from_numpy(pairs[:50] % 7), c, band)          # queries != corpus, pairs as a tensor
    assert np.array_equal(got.view(np.uint32), DW.dtw_pairs_host(rows[:7], rows[100:], pairs[:50] % 7, c, band).view(np.uint32))


def test_same_bits_on_every_run_and_for_every_grid(gpu_lib, monkeypatch):
    cases = (("integer", 130, 80, 32, 4, 15), ("float", 16, 8, 600, 2, 10))
    pairs = np.random.default_rng(DC.SEED).integers(0, 600, (300, 2))
    rows = DC.float_rows(16, 8, 600)
    want_pairs = DW.dtw_pairs(rows, None, pairs, 16, 2)

    def runs(tag):
        for case in cases:
            ref = DC.reference(*case)
            assert same_bits(device_dtw(ref.q, None, ref.k, ref.channels, ref.band), device_case(*case)), (case, tag)
        assert np.array_equal(DW.dtw_pairs(rows, None, pairs, 16, 2).view(np.uint32), want_pairs.view(np.uint32)), tag

    runs("again")
    for cap in ("1", "2", "7"):
        monkeypatch.setenv("WSEG_DTW_GRID", cap)
        runs(cap)
    monkeypatch.delenv("WSEG_DTW_GRID")
    runs("default")


def test_invalid_calls_are_refused_before_a_launch(gpu_lib):
    from whisperseg_amd import _lib
    x = torch.from_numpy(DC.integer_rows(64, 16)).cuda()          # C = 4, T = 4
    for k in (0, 65):
        with pytest.raises(ValueError, match="k must"):
            DW.dtw_knn_rows(x, None, k, 4, 1)
        with pytest.raises(ValueError, match="k must"):
            DW.dtw_neighbors(x, None, k, 4, 1)
    for band in (-1, 4, 1.5):
        with pytest.raises(ValueError, match="band must"):
            DW.dtw_knn_rows(x, None, 2, 4, band)
        with pytest.raises(ValueError, match="band must"):
            DW.dtw_neighbors(x, None, 2, 4, band)
        with pytest.raises(ValueError, match="band must"):
            DW.dtw_pairs(x, None, np.zeros((1, 2), np.int64), 4, band)
    for channels in (0, 129):
        with pytest.raises(ValueError, match="channels must"):
            DW.dtw_knn_rows(x, None, 2, channels, 0)
    with pytest.raises(ValueError, match="multiple of channels"):
        DW.dtw_knn_rows(x, None, 2, 5, 0)
    with pytest.raises(ValueError, match="multiple of channels"):
        DW.dtw_knn_rows(torch.zeros((3, 0), device="cuda"), None, 2, 1, 0)
    with pytest.raises(ValueError, match="T = D / channels must"):
        DW.dtw_knn_rows(torch.zeros((3, 130), device="cuda"), None, 2, 2, 0)
    with pytest.raises(ValueError, match="T = D / channels must"):
        DW.dtw_pairs(np.zeros((3, 130), np.float32), None, np.zeros((1, 2), np.int64), 2, 0)
    with pytest.raises(ValueError, match="same D"):
        DW.dtw_knn_rows(x, x[:, :8].contiguous(), 2, 4, 1)
    with pytest.raises(ValueError, match="2-D"):
        DW.dtw_knn_rows(x[0], None, 2, 4, 1)
    with pytest.raises(_lib.WsegError, match="no CPU path"):
        DW.dtw_knn_rows(x.cpu(), None, 2, 4, 1)
    with pytest.raises(_lib.WsegError, match="no CPU path"):
        DW.dtw_knn_rows(x, x.cpu(), 2, 4, 1)
    with pytest.raises(_lib.WsegError, match="contiguous"):
        DW.dtw_knn_rows(x.t(), None, 2, 4, 1)
    with pytest.raises(_lib.WsegError, match="contiguous"):
        DW.dtw_knn_rows(x, x[:, ::2], 2, 4, 1)
    with pytest.raises(_lib.WsegError, match="contiguous"):
        DW.dtw_knn_rows(x.double(), None, 2, 4, 1)
    if torch.cuda.device_count() > 1:
        with pytest.raises(_lib.WsegError, match="corpus is on"):
            DW.dtw_knn_rows(x, x.to("cuda:1"), 2, 4, 1)
        with pytest.raises(_lib.WsegError, match="out_index"):
            DW.dtw_knn_rows(x, None, 2, 4, 1, out_index=torch.empty((64, 2), dtype=torch.int32, device="cuda:1"))
    for bad in (torch.empty((64, 3), dtype=torch.int32, device="cuda"), torch.empty((63, 2), dtype=torch.int32, device="cuda"),
                torch.empty((64, 2), dtype=torch.int64, device="cuda"), torch.empty((64, 2), dtype=torch.int32), torch.empty((64, 4), dtype=torch.int32, device="cuda")[:, ::2]):
        with pytest.raises(_lib.WsegError, match="out_index"):
            DW.dtw_knn_rows(x, None, 2, 4, 1, out_index=bad)
    for bad in (torch.empty((64, 3), device="cuda"), torch.empty((64, 2), dtype=torch.float64, device="cuda"), torch.empty((64, 2))):
        with pytest.raises(_lib.WsegError, match="out_distance"):
            DW.dtw_knn_rows(x, None, 2, 4, 1, out_distance=bad)
    for pairs in ([[0, 64]], [[64, 0]], [[-1, 0]], [[0, 1, 2]], [[0.5, 1.0]]):
        with pytest.raises(ValueError, match="pairs must"):
            DW.dtw_pairs(x, None, np.array(pairs), 4, 1)
    with pytest.raises(ValueError, match="pairs must"):
        DW.dtw_pairs(x, x[:5].contiguous(), torch.tensor([[0, 5]]), 4, 1)
    # no queries: an empty result; no corpus rows: -1 / +inf everywhere (between intact guards)
    for corpus in (None, x):
        index, distance = DW.dtw_knn_rows(x[:0], corpus, 4, 4, 1)
        assert index.shape == distance.shape == (0, 4) and index.dtype == torch.int32 and distance.dtype == torch.float32 and index.is_cuda
    index, distance = device_dtw(DC.integer_rows(64, 16), np.zeros((0, 16), np.float32), 4, 4, 1)
    assert index.shape == (64, 4) and (index == -1).all() and np.isposinf(distance).all()
    index, distance = DW.dtw_neighbors(DC.integer_rows(5, 12), np.zeros((0, 12), np.float32), 3, 3, 1)
    assert (index == -1).all() and np.isposinf(distance).all()
    index, distance = DW.dtw_neighbors(np.zeros((0, 12), np.float32), None, 3, 3, 1)
    assert index.shape == distance.shape == (0, 3)


def test_public_call_gives_the_kernels_bits(gpu_lib):
    """dtw_neighbors() from numpy and from a resident tensor, self-search and against a corpus."""
    for case in (("integer", 65, 17, 8, 2, 15), ("float", 16, 8, 600, 2, 10), ("cross",)):
        ref = DC.reference(*case)
        corpus = None if ref.own else ref.x
        for q, x in ((ref.q, corpus), (guarded_rows(ref.q), None if ref.own else guarded_rows(ref.x)), (torch.from_numpy(ref.q), corpus)):
            got = DW.dtw_neighbors(q, x, ref.k, ref.channels, ref.band)
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
    tiny = tmp_path_factory.mktemp("dtw") / "tiny.wav"
    tiny.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", s16(GI.tiny_recording(3, 2)))))
    return str(tiny)


KW = dict(spec_time_step=TM.STS)


def check_archive_lists(patch, index, distance, k, band, what):
    rows = np.ascontiguousarray(patch.reshape(len(patch), patch.shape[1] * patch.shape[2]))
    assert index.shape == distance.shape == (len(rows), k) and index.dtype == np.int32 and distance.dtype == np.float32, what
    if len(rows):
        DC.check_contract(DC.Reference(rows, None, k, patch.shape[1], band), index, distance, what=what)


def test_patch_dtw_neighbors_of_a_segmentation(gpu_lib, seg, tiny_wav):
    from whisperseg_amd.wavio import load_wav
    total = 0
    for path in (os.path.join(GOLDEN, "meerkat_5s.wav"), tiny_wav):
        pred = seg.segment(*load_wav(path), patches=8, **KW)
        got = DW.patch_dtw_neighbors([pred], 3)
        assert list(got) == ["neighbor_index", "neighbor_distance"]
        check_archive_lists(pred["patch"], got["neighbor_index"], got["neighbor_distance"], 3, None, os.path.basename(path))
        total += len(pred["onset"])
    assert total >= 3                                  # not vacuous: the fixture model finds rows in its own signal family
    # per-channel lists, as segment_files(channel_id="all") returns them: rows in file, channel, row order
    preds = seg.segment_files([tiny_wav, tiny_wav], channel_id="all", patches=8, **KW)
    got = DW.patch_dtw_neighbors(preds, 2, band=2)
    flat = np.concatenate([r["patch"] for res in preds for r in res], axis=0)
    check_archive_lists(flat, got["neighbor_index"], got["neighbor_distance"], 2, 2, "two files, every channel")
    twin = got["neighbor_index"][:, 0]
    assert len(flat) >= 2 and (got["neighbor_distance"][:, 0] == 0).all()       # the same file twice: every row has a twin
    assert (twin != np.arange(len(flat))).all() and np.array_equal(flat[twin], flat)


def cli(tmp_path, monkeypatch, tiny_wav):
    """-> run(tag, *flags): scripts/segment.py on the tiny recording with --patches 8 -> (csv path, npz path)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    monkeypatch.setenv("WHISPERSEG_AMD_DTYPE", "f32")
    base = ["--model_path", MODEL_DIR, "--audio_path", tiny_wav, "--spec_time_step", str(TM.STS)]

    def run(tag, *extra):
        out_csv, out_npz = tmp_path / (tag + ".csv"), tmp_path / (tag + ".npz")
        segment.main(base + ["--csv_save_path", str(out_csv), "--patches", "8", "--patches_save_path", str(out_npz)] + list(extra))
        return out_csv, out_npz

    return run


def test_cli_neighbors_metric(gpu_lib, seg, tiny_wav, tmp_path, monkeypatch):
    """--neighbors 3 --neighbors_metric dtw writes the API's bits plus the two new keys (and, with --embed at the same K, the map of
    those lists); the same command without the metric flag writes what it always wrote."""
    from whisperseg_amd.embed import patch_embedding
    from whisperseg_amd.wavio import load_wav
    run = cli(tmp_path, monkeypatch, tiny_wav)
    plain_csv, plain_npz = run("plain", "--neighbors", "3")
    dtw_csv, dtw_npz = run("dtw", "--neighbors", "3", "--neighbors_metric", "dtw", "--embed", "2", "--embed_neighbors", "3")
    assert plain_csv.read_bytes() == dtw_csv.read_bytes() and len(plain_csv.read_text().splitlines()) > 3
    want = seg.segment(*load_wav(tiny_wav), patches=8, **KW)
    with np.load(plain_npz) as plain, np.load(dtw_npz) as full:
        # without the flag: exactly the keys, the order and the bits there were
        assert list(plain.files) == ["patch", "onset", "offset", "cluster", "neighbor_index", "neighbor_distance"]
        euclid = NB.patch_neighbors([want], 3)
        assert plain["neighbor_index"].dtype == np.int32 and np.array_equal(plain["neighbor_index"], euclid["neighbor_index"])
        assert np.array_equal(plain["neighbor_distance"].view(np.uint32), euclid["neighbor_distance"].view(np.uint32))
        assert set(full.files) == set(plain.files) | {"neighbor_metric", "neighbor_band", "embedding"}
        assert all(np.array_equal(plain[name], full[name]) for name in ("patch", "onset", "offset", "cluster"))
        assert str(full["neighbor_metric"]) == "dtw" and int(full["neighbor_band"]) == 1
        rows = len(plain_csv.read_text().splitlines()) - 1
        assert full["patch"].shape == (rows, 80, 8) and full["neighbor_index"].shape == full["neighbor_distance"].shape == (rows, 3)
        check_archive_lists(full["patch"], full["neighbor_index"], full["neighbor_distance"], 3, None, "the archive")
        got = DW.patch_dtw_neighbors([want], 3)
        assert np.array_equal(full["neighbor_index"], got["neighbor_index"])
        assert np.array_equal(full["neighbor_distance"].view(np.uint32), got["neighbor_distance"].view(np.uint32))
        layout = patch_embedding([want], 3, 2, lists=(got["neighbor_index"], got["neighbor_distance"]))["embedding"]
        assert np.array_equal(full["embedding"].view(np.uint32), layout.view(np.uint32))


def test_cli_embed_from_dtw_lists(gpu_lib, seg, tiny_wav, tmp_path, monkeypatch):
    """--embed 2 --neighbors_metric dtw equals patch_embedding(..., lists=<dtw lists>) bit for bit — without --neighbors, and with a
    --neighbors of another K and a band, where the lists are computed a second time."""
    from whisperseg_amd.embed import patch_embedding
    from whisperseg_amd.wavio import load_wav
    run = cli(tmp_path, monkeypatch, tiny_wav)
    want = seg.segment(*load_wav(tiny_wav), patches=8, **KW)
    for tag, extra, k, band in (("alone", ["--embed", "2", "--neighbors_metric", "dtw"], 15, None),
                                ("second", ["--embed", "2", "--embed_neighbors", "2", "--neighbors", "3", "--neighbors_metric", "dtw",
                                            "--neighbors_band", "2"], 2, 2)):
        _, out_npz = run(tag, *extra)
        lists = DW.patch_dtw_neighbors([want], k, band)
        layout = patch_embedding([want], k, 2, lists=(lists["neighbor_index"], lists["neighbor_distance"]))["embedding"]
        with np.load(out_npz) as arch:
            assert np.array_equal(arch["embedding"].view(np.uint32), layout.view(np.uint32)), tag
            assert ("neighbor_metric" in arch.files) == ("neighbor_index" in arch.files) == (tag == "second")
            if tag == "second":
                three = DW.patch_dtw_neighbors([want], 3, 2)
                assert np.array_equal(arch["neighbor_index"], three["neighbor_index"]) and int(arch["neighbor_band"]) == 2
