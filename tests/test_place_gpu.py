"""Placing new rows on a frozen map on the GPU (wseg_embed_place_f64, whisperseg_amd/csrc/wseg_embed.hip) against the host definition
whisperseg_amd.embed.place_host, from the kernel up to transform, linkage.assign, library.patch_onto and the CLI's --onto.

With b == 1 nothing may differ: every coordinate has the definition's bits after all 50 epochs, on the smallest cases at which the
kernel can go wrong (tests/place_cases.py::exact_case).  With a general b one epoch from the same positions stays inside the bound
derived in tests/embed_cases.py, and a continued run is compared device against device, bit for bit.  Every raw call writes between
guard rows and reads arrays that lie inside larger ones."""
import os
import sys

import numpy as np
import pytest
import torch

import embed_cases as EC
import golden_inputs as GI
import place_cases as PL
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import embed as EM
from whisperseg_amd import library as LB
from whisperseg_amd import linkage as LK
from whisperseg_amd import neighbors as NB

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
GUARD_BITS = 0x7ff8000000012345          # float64 guards: a NaN no kernel writes


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def inside(array, fill, pad=8):
    """-> the array as a device tensor inside a larger one, `pad` entries (rows) of `fill` in front and behind."""
    array = np.ascontiguousarray(array)
    whole = torch.full((len(array) + 2 * pad,) + array.shape[1:], fill, dtype=torch.from_numpy(array).dtype, device="cuda")
    whole[pad:pad + len(array)] = torch.from_numpy(array).cuda()
    return whole[pad:pad + len(array)]


def device_place(run):
    """wseg_embed_place_f64 of a checked Place with y_out between guard rows and every input inside a larger array -> the positions as
    numpy; the guards must survive and y_in, the corpus and the CSR must be left as they were."""
    from whisperseg_amd import _lib
    lib = _lib.load(require_device=True)
    m, dim = run.m, run.dim
    guard = torch.from_numpy(np.array([GUARD_BITS], np.uint64).view(np.float64)).cuda()
    held = guard.repeat((m + 2) * dim).reshape(m + 2, dim).contiguous()
    indptr, indices = inside(run.indptr, 0), inside(run.indices, 0)
    rate = inside(run.rate.view(np.int32), 65536)                 # (around the CSR: entries that would be active, of vertex 0)
    key = inside(run.key.view(np.int64), 0)
    corpus, y_in = inside(run.y, float("nan")), inside(run.y0, float("nan"))
    _lib.check(lib.wseg_embed_place_f64(indptr.data_ptr(), indices.data_ptr() if run.nnz else None, rate.data_ptr() if run.nnz else None, key.data_ptr(),
                                        m, run.nnz, corpus.data_ptr(), run.n, dim, y_in.data_ptr(), held[1:m + 1].data_ptr(), run.t0, run.t1, run.total,
                                        run.lr, run.a, run.b, run.gamma, run.n_neg, _lib.stream_ptr()))
    out = held.cpu().numpy()
    assert (out[[0, -1]].view(np.uint64) == GUARD_BITS).all(), "a guard was written"
    assert same_bits(y_in.cpu().numpy(), run.y0) and same_bits(corpus.cpu().numpy(), run.y), "y_in or the corpus was written"
    assert np.array_equal(indptr.cpu().numpy(), run.indptr) and np.array_equal(indices.cpu().numpy(), run.indices), "the CSR was written"
    assert np.array_equal(rate.cpu().numpy(), run.rate.view(np.int32)) and np.array_equal(key.cpu().numpy(), run.key.view(np.int64)), "the CSR was written"
    return np.ascontiguousarray(out[1:-1])


def run_of(graph, y, keys, epochs, total=None, n_neg=5, a=None, b=None, init=None):
    return EM.Place(graph, y, keys, epochs, total, n_neg, 1.0, 1.0, a, b, init)


@pytest.mark.parametrize("n_neg", (0, 1, 5))
@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("name", PL.EXACT_CASES)
def test_b1_gives_the_definitions_bits(gpu_lib, name, dim, n_neg):
    graph, y, keys, init = PL.exact_args(name, dim)
    want = PL.exact_reference(name, dim, n_neg)
    got = device_place(run_of(graph, y, keys, PL.EXACT_EPOCHS, n_neg=n_neg, a=1.0, b=1.0, init=init))
    differ = got.view(np.uint64) != want.view(np.uint64)
    assert not differ.any(), (int(differ.sum()), float(np.abs(got - want).max()))


def test_public_call_gives_the_kernels_bits(gpu_lib):
    for name, dim in (("m65", 2), ("on_top", 3), ("n1", 2), ("empty_row", 3)):
        graph, y, keys, init = PL.exact_args(name, dim)
        got = EM.place(graph, y, keys, PL.EXACT_EPOCHS, n_neg=5, a=1.0, b=1.0, init=init)
        assert isinstance(got, np.ndarray) and same_bits(got, PL.exact_reference(name, dim, 5)), name
    graph, y, keys, init = PL.exact_args("m65", 2)
    for epochs in (1, 2, 3):
        assert same_bits(EM.place(graph, y, keys, epochs, a=1.0, b=1.0), EM.place_host(graph, y, keys, epochs, a=1.0, b=1.0)), epochs
    # no new row, and rows without an entry
    nothing = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    assert EM.place(nothing, y, np.zeros(0, np.uint64), 5).shape == (0, 2)
    lone = (np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0))
    start = np.arange(6.0).reshape(3, 2)
    assert same_bits(EM.place(lone, y, keys[:3], 5, init=start), start) and not EM.place(lone, y, keys[:3], 5).any()


@pytest.mark.parametrize("dim", (2, 3))
def test_entries_outside_the_inputs_contribute_nothing(gpu_lib, dim):
    """An entry whose index is outside 0 .. n - 1 adds neither its attraction nor its negatives but keeps its position q, a row
    reaches no further than 0 .. nnz, and its entries past the 64th contribute nothing: the result is the definition's with those
    entries switched off (rate 0: never active, the numbering of the others kept).  The arrays lie inside larger ones (NaN rows
    around the corpus and y_in), so nothing here reads outside a buffer."""
    graph, y, keys, init = PL.exact_args("m65", dim)
    plain = EM.place_host(graph, y, keys, 10, a=1.0, b=1.0)
    want, got = (run_of(graph, y, keys, 10, a=1.0, b=1.0) for _ in range(2))
    bad = np.arange(3, got.nnz, 7)
    got.indices[bad] = np.resize(np.array([-1, got.n, got.n + 5, -7], np.int32), len(bad))
    want.rate[bad] = 0
    assert len(bad) > 20 and not same_bits(EM.place_epochs_host(want), plain)
    assert same_bits(device_place(got), EM.place_epochs_host(want))
    # the last row claims entries behind the CSR: clipped to nnz
    wide = run_of(graph, y, keys, 10, a=1.0, b=1.0)
    wide.indptr[-1] = wide.nnz + 4
    assert same_bits(device_place(wide), plain)
    # the first row claims three entries in front of the CSR: they are not read, and its own entries keep the positions 3, 4, ...
    # — the definition's result for a row with three more entries of rate 0 in front
    front, shifted = (run_of(graph, y, keys, 10, a=1.0, b=1.0) for _ in range(2))
    front.indptr[0] = -3
    shifted.indptr[1:] += 3
    shifted.indices = np.concatenate([np.zeros(3, np.int32), shifted.indices])
    shifted.rate = np.concatenate([np.zeros(3, np.uint32), shifted.rate])
    shifted.nnz += 3
    moved = EM.place_epochs_host(shifted)
    assert same_bits(device_place(front), moved) and same_bits(moved[1:], plain[1:]) and not same_bits(moved[:1], plain[:1])
    # a row of 70 entries: those past the 64th contribute nothing
    rng = np.random.default_rng(dim)
    long_graph = PL.bipartite(rng, [2, 64, 1], 80)
    corpus = np.ascontiguousarray(rng.uniform(-10, 10, (80, dim)))
    some = EM.draw(1, np.arange(3, dtype=np.uint64))
    want, got = (run_of(long_graph, corpus, some, 10, a=1.0, b=1.0) for _ in range(2))
    extra = 6
    got.indices = np.concatenate([got.indices[:66], rng.integers(0, 80, extra).astype(np.int32), got.indices[66:]])
    got.rate = np.concatenate([got.rate[:66], np.full(extra, 65536, np.uint32), got.rate[66:]])
    got.indptr[2:] += extra
    got.nnz += extra
    assert same_bits(device_place(got), EM.place_epochs_host(want))


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("general", (False, True), ids=("b1", "b"))
def test_a_continued_run_gives_the_whole_runs_bits(gpu_lib, general, dim):
    """Epochs (0, 20) then (20, 50) against (0, 50), device against device: a lane's epochs in one launch are the epochs of two."""
    a, b = EM.curve_ab(0.1) if general else (1.0, 1.0)
    for name in ("m65", "row64"):
        graph, y, keys, init = PL.exact_args(name, dim)
        whole = device_place(run_of(graph, y, keys, 50, a=a, b=b, init=init))
        part = device_place(run_of(graph, y, keys, (0, 20), 50, a=a, b=b, init=init))
        rest = device_place(run_of(graph, y, keys, (20, 50), 50, a=a, b=b, init=part))
        assert same_bits(rest, whole) and not same_bits(part, whole), name
        odd = device_place(run_of(graph, y, keys, (0, 21), 50, a=a, b=b, init=init))
        assert same_bits(device_place(run_of(graph, y, keys, (21, 50), 50, a=a, b=b, init=odd)), whole), name
        assert same_bits(EM.place(graph, y, keys, (20, 50), 50, a=a, b=b, init=part), whole), name


@pytest.mark.parametrize("dim", (2, 3))
def test_one_epoch_with_a_general_b_stays_inside_the_bound(gpu_lib, dim):
    """The 60 held-out blob rows on the library's map (3-D: the same lists on a random cloud), a, b = curve_ab(0.1), T = 100: from the
    same float64 y_in at several t, the device and the plain statement differ per coordinate by at most
    alpha_t u sum|g| (64 + n_terms) + 1 ulp(y) (tests/embed_cases.py::one_epoch_bound).
    Measured on an MI355X: the largest share of the bound used is 0.098 (dim 2) and 0.187 (dim 3), up to 8 % of the coordinates differ."""
    lib = PL.blob_library()
    index, distance = lib["lists"]
    graph, keys = EM.membership_host(index, distance, 240), EM.row_keys(index, distance, 1)
    y = np.array(lib["positions"]) if dim == 2 else np.random.default_rng(2).uniform(-10, 10, (240, 3))
    a, b = EM.curve_ab(0.1)
    worst = 0.0
    for t in (0, 1, 37, 99):
        y_in = EM.place_host(graph, y, keys, (0, t), 100, a=a, b=b) if t else EM.start_host(graph, y)
        stats = {}
        want = PL.plain_place(graph, y, keys, t, t + 1, 100, 5, 1.0, 1.0, a, b, y_in, stats)
        assert same_bits(EM.place_host(graph, y, keys, (t, t + 1), 100, a=a, b=b, init=y_in), want)
        got = device_place(run_of(graph, y, keys, (t, t + 1), 100, a=a, b=b, init=y_in))
        bound = EC.one_epoch_bound(want, 1.0 - t / 100, stats)
        share = float((np.abs(got - want) / bound).max())
        print(f"dim {dim}, t {t}: {int(stats['terms'].sum())} terms, largest share of the bound used {share:.3f}, "
              f"{int((got != want).sum())} of {got.size} coordinates differ")
        worst = max(worst, share)
        assert (np.abs(got - want) <= bound).all(), (t, share)
    print(f"dim {dim}: largest share of the bound used {worst:.3f}")


@pytest.mark.parametrize("general", (False, True), ids=("b1", "b"))
def test_a_rows_result_does_not_depend_on_its_batch(gpu_lib, general):
    """place of rows A u B in shuffled order equals, row by row and bit for bit, place of A alone and of B alone (the same host
    lists): another grid, other lanes, other neighbours in the wave."""
    a, b = EM.curve_ab(0.1) if general else (1.0, 1.0)
    lib = PL.blob_library()
    index, distance = lib["lists"]

    def placed(rows):
        i, d = index[rows], distance[rows]
        return EM.place(EM.membership_host(i, d, 240), lib["positions"], EM.row_keys(i, d, 4), 60, a=a, b=b)

    order = np.random.default_rng(7).permutation(60)
    both = placed(order)
    first, second, where = np.sort(order[:23]), np.sort(order[23:]), np.argsort(order)
    assert same_bits(both[where[first]], placed(first)) and same_bits(both[where[second]], placed(second))
    assert same_bits(both[where[[17]]], placed(np.array([17]))) and not same_bits(both[:23], placed(first))
    # a batch of several workgroups: every row three times, 180 rows
    many = placed(np.tile(order, 3))
    assert same_bits(many[:60], both) and same_bits(many[60:120], both) and same_bits(many[120:], both)


def test_transform_is_a_placement(gpu_lib):
    """The blobs' hold-out on their library's map, with the device's lists: purity >= 0.99; the result is place of the same lists
    cast to float32; assign gives assign_host of the device lists and every held-out row the cluster of its blob."""
    lib = PL.blob_library()
    got = EM.transform(lib["new_rows"], lib["rows"], lib["positions"], k=10)
    purity = PL.placed_purity(got, lib["new_labels"], lib["positions"], lib["labels"])
    print(f"purity of the placed rows among the library's points: {purity:.4f}")
    assert got.shape == (60, 2) and got.dtype == np.float32 and np.isfinite(got).all() and purity >= 0.99
    index, distance = NB.neighbors(lib["new_rows"], lib["rows"], 10)
    a, b = EM.curve_ab(0.1)
    same = EM.place(EM.membership_host(index, distance, 240), lib["positions"], EM.row_keys(index, distance, 0), 100, a=a, b=b)
    assert np.array_equal(got, same.astype(np.float32))
    assert np.array_equal(got, EM.transform(lib["new_rows"], lib["rows"], lib["positions"], k=10, lists=(index, distance)))
    assert np.array_equal(got[5:9], EM.transform(lib["new_rows"][5:9], lib["rows"], lib["positions"], k=10))       # a row alone in another batch
    assert not np.array_equal(got, EM.transform(lib["new_rows"], lib["rows"], lib["positions"], k=10, seed=3))
    cloud = np.random.default_rng(4).uniform(-10, 10, (240, 3))
    assert EM.transform(lib["new_rows"], torch.from_numpy(lib["rows"]).cuda(), cloud, k=10, epochs=20).shape == (60, 3)
    # call types
    edges, weight = LK.mst_host(lib["rows"], 5)
    labels = LK.hdbscan_labels(edges, weight, 240, 15)
    assert np.bincount(labels + 1).tolist() == [0, 79, 85, 76]
    types = LK.assign(lib["new_rows"], lib["rows"], labels, edges, weight, min_samples=5, k=10)
    core = NB.neighbors(lib["rows"], None, 5)[1][:, 4]
    assert types.dtype == np.int32 and np.array_equal(types, LK.assign_host(index, distance, core, labels, LK.reach_of(edges, weight, labels), 5))
    assert np.array_equal(types, LK.assign(lib["new_rows"], lib["rows"], labels, edges, weight, min_samples=5, k=10, lists=(index, distance)))
    blob_of = np.array([np.bincount(lib["labels"][labels == c]).argmax() for c in range(3)])
    assert (types >= 0).all() and np.array_equal(blob_of[types], lib["new_labels"])
    far = np.random.default_rng(5).normal(40.0, 1.0, (5, 16)).astype(np.float32)
    assert LK.assign(far, lib["rows"], labels, edges, weight, min_samples=5, k=10).tolist() == [-1] * 5


def test_public_edges(gpu_lib):
    lib = PL.blob_library()
    none = EM.transform(lib["new_rows"][:0], lib["rows"], np.zeros((240, 3)))
    assert none.shape == (0, 3) and none.dtype == np.float32
    with pytest.raises(ValueError):
        EM.transform(lib["new_rows"], lib["rows"][:0], np.zeros((0, 2)))
    with pytest.raises(ValueError):
        EM.place((np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0)), np.zeros((0, 2)), np.zeros(1, np.uint64))
    one = EM.transform(lib["new_rows"][:3], lib["rows"][:1], np.array([[1.5, -2.0]]), k=4)         # a library of one call: every row lands on it
    assert np.array_equal(one, np.tile(np.array([[1.5, -2.0]], np.float32), (3, 1)))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def s16(v):
    return np.clip(np.round(np.asarray(v, np.float64) * 32768), -32768, 32767).astype(np.int64)


def test_cli_onto(gpu_lib, tmp_path, monkeypatch):
    """The tiny recording as its own library: segmented once with --clusters, --embed and --pca into lib.npz, then again --onto it."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    monkeypatch.setenv("WHISPERSEG_AMD_DTYPE", "f32")
    tiny = tmp_path / "tiny.wav"
    tiny.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", s16(GI.tiny_recording(3, 2)))))
    base = ["--model_path", MODEL_DIR, "--audio_path", str(tiny), "--spec_time_step", str(TM.STS)]
    plain_csv, lib_csv, onto_csv = tmp_path / "plain.csv", tmp_path / "lib.csv", tmp_path / "onto.csv"
    plain_npz, lib_npz, onto_npz = tmp_path / "plain.npz", tmp_path / "lib.npz", tmp_path / "onto.npz"
    segment.main(base + ["--csv_save_path", str(plain_csv), "--patches", "8", "--patches_save_path", str(plain_npz)])
    segment.main(base + ["--csv_save_path", str(lib_csv), "--patches", "8", "--patches_save_path", str(lib_npz), "--clusters", "2", "--embed", "2", "--pca", "2"])
    segment.main(base + ["--csv_save_path", str(onto_csv), "--patches", "8", "--patches_save_path", str(onto_npz), "--onto", str(lib_npz)])
    assert onto_csv.read_bytes() == plain_csv.read_bytes() == lib_csv.read_bytes()
    rows = len(plain_csv.read_text().splitlines()) - 1
    with np.load(plain_npz) as plain, np.load(lib_npz) as lib, np.load(onto_npz) as onto:
        assert set(plain.files) == {"patch", "onset", "offset", "cluster"}                       # without the flag: exactly the keys there were
        assert set(lib.files) == set(plain.files) | {"patch_cluster", "mst_edges", "mst_weight", "embedding", "pca_mean", "pca_components", "pca_variance",
                                                     "pca_variance_ratio", "pca_scores"}
        assert set(onto.files) == set(plain.files) | {"library_index", "library_distance", "patch_cluster", "embedding", "pca_scores"}
        assert all(np.array_equal(plain[name], onto[name]) for name in plain.files)
        assert rows >= 3 and onto["library_index"].shape == (rows, 15) and onto["library_index"].dtype == np.int32 and onto["library_distance"].dtype == np.float32
        # every placed call is its own nearest library row (or an identical twin), at distance 0
        nearest = onto["library_index"][:, 0]
        assert (onto["library_distance"][:, 0] == 0).all() and all(np.array_equal(lib["patch"][j], plain["patch"][i]) for i, j in enumerate(nearest))
        assert (onto["library_index"][:, rows:] == -1).all() and (onto["library_index"][:, :rows] >= 0).all()
        assert onto["pca_scores"].dtype == np.float32 and np.array_equal(onto["pca_scores"], lib["pca_scores"])
        assert onto["embedding"].shape == (rows, 2) and onto["embedding"].dtype == np.float32 and np.isfinite(onto["embedding"]).all()
        typed = lib["patch_cluster"] >= 0
        print(f"{rows} rows; the library's call types {lib['patch_cluster'].tolist()}, the placed rows' {onto['patch_cluster'].tolist()}")
        assert onto["patch_cluster"].dtype == np.int32 and np.array_equal(onto["patch_cluster"][typed], lib["patch_cluster"][typed])
        # the same through the public call, and a library that holds the pictures alone
        again = LB.patch_onto(plain["patch"], str(lib_npz))
        assert list(again) == ["library_index", "library_distance", "patch_cluster", "embedding", "pca_scores"] and all(np.array_equal(again[key], onto[key]) for key in again)
        alone = LB.patch_onto(plain["patch"][::-1], {"patch": lib["patch"]}, k=2)
        assert list(alone) == ["library_index", "library_distance"] and np.array_equal(alone["library_distance"][::-1], onto["library_distance"][:, :2])
    # a 3-D library, its own K, min_dist and seed; the placed rows of a batch in another order are the same rows
    lib3_npz, onto3_npz = tmp_path / "lib3.npz", tmp_path / "onto3.npz"
    flags = ["--embed_neighbors", "3", "--embed_min_dist", "0.5", "--embed_seed", "7"]
    segment.main(base + ["--csv_save_path", str(lib_csv), "--patches", "8", "--patches_save_path", str(lib3_npz), "--embed", "3"] + flags)
    segment.main(base + ["--csv_save_path", str(onto_csv), "--patches", "8", "--patches_save_path", str(onto3_npz), "--onto", str(lib3_npz)] + flags)
    with np.load(plain_npz) as plain, np.load(onto3_npz) as onto:
        assert set(onto.files) == set(plain.files) | {"library_index", "library_distance", "embedding"}
        assert onto["embedding"].shape == (rows, 3) and onto["library_index"].shape == (rows, 3) and np.isfinite(onto["embedding"]).all()
        turned = LB.patch_onto(plain["patch"][::-1], str(lib3_npz), k=3, min_dist=0.5, seed=7)
        assert np.array_equal(turned["embedding"][::-1], onto["embedding"])
