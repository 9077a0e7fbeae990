"""The layout epochs on the GPU (wseg_embed_epochs_f64, whisperseg_amd/csrc/wseg_embed.hip) against the host definition
whisperseg_amd.embed.layout_host, from the kernel up to patch_embedding and the CLI's --embed.

With b == 1 nothing may differ: every coordinate has the definition's bits after all 50 epochs, on the smallest graphs at which the
kernel can go wrong (tests/embed_cases.py::exact_case).  With a general b one epoch from the same positions stays inside the bound
derived in tests/embed_cases.py, and a continued run is compared device against device, bit for bit.  Every raw call writes between
guard rows."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import embed_cases as EC
import golden_inputs as GI
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import embed as EM
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


def device_epochs(run):
    """wseg_embed_epochs_f64 of a checked Run with y_out and the scratch between guard rows -> the positions as numpy; the guards must
    survive and y_in must be left as it was."""
    from whisperseg_amd import _lib
    lib = _lib.load(require_device=True)
    n, dim = run.n, run.dim
    guard = torch.from_numpy(np.array([GUARD_BITS], np.uint64).view(np.float64)).cuda()
    held = guard.repeat((n + 2) * dim).reshape(n + 2, dim).contiguous()
    words = EM.scratch_bytes(n, dim) // 8
    scratch = guard.repeat(words + 64).contiguous()
    indptr, indices = torch.from_numpy(run.indptr).cuda(), inside(run.indices, 0)
    rate = inside(run.rate.view(np.int32), 65536)                 # (around the CSR: entries that would be active, of vertex 0)
    y_in = inside(run.y0, float("nan"))
    _lib.check(lib.wseg_embed_epochs_f64(indptr.data_ptr(), indices.data_ptr() if run.nnz else None, rate.data_ptr() if run.nnz else None, n, run.nnz, dim,
                                         y_in.data_ptr(), held[1:n + 1].data_ptr(), scratch[32:].data_ptr(), words * 8, run.t0, run.t1, run.total,
                                         run.lr, run.a, run.b, run.gamma, run.n_neg, run.seed, _lib.stream_ptr()))
    out, pad = held.cpu().numpy(), scratch.cpu().numpy()
    assert (out[[0, -1]].view(np.uint64) == GUARD_BITS).all() and (pad[:32].view(np.uint64) == GUARD_BITS).all() and (pad[32 + words:].view(np.uint64) == GUARD_BITS).all(), "a guard was written"
    assert same_bits(y_in.cpu().numpy(), run.y0), "y_in was written"
    return np.ascontiguousarray(out[1:-1])


def run_of(graph, dim, epochs, total=None, n_neg=5, a=None, b=None, init=None, seed=0):
    return EM.Run(graph, dim, epochs, total, n_neg, 1.0, 1.0, a, b, init, seed)


@pytest.mark.parametrize("n_neg", (0, 1, 5))
@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("name", EC.EXACT_CASES)
def test_b1_gives_the_definitions_bits(gpu_lib, name, dim, n_neg):
    want = EC.exact_reference(name, dim, n_neg)
    got = device_epochs(run_of(EC.exact_case(name)[0], dim, EC.EXACT_EPOCHS, n_neg=n_neg, a=1.0, b=1.0, init=EC.exact_init(name, dim), seed=3))
    differ = got.view(np.uint64) != want.view(np.uint64)
    assert not differ.any(), (int(differ.sum()), float(np.abs(got - want).max()))


def test_public_call_gives_the_kernels_bits(gpu_lib):
    for name, dim in (("n65", 2), ("twins", 3), ("n1", 2)):
        got = EM.layout(EC.exact_case(name)[0], dim, EC.EXACT_EPOCHS, n_neg=5, a=1.0, b=1.0, init=EC.exact_init(name, dim), seed=3)
        assert isinstance(got, np.ndarray) and same_bits(got, EC.exact_reference(name, dim, 5)), name
    # a single epoch (the scratch is not used), and an even and an odd number of them
    graph = EC.exact_case("n65")[0]
    for epochs in (1, 2, 3):
        assert same_bits(EM.layout(graph, 2, epochs, a=1.0, b=1.0, seed=8), EM.layout_host(graph, 2, epochs, a=1.0, b=1.0, seed=8)), epochs
    # no vertex, and a graph without an entry
    assert EM.layout((np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0)), 3, 5).shape == (0, 3)
    lone = (np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0))
    assert same_bits(EM.layout(lone, 2, 5, seed=4), EM.init_positions(3, 2, 4))


@pytest.mark.parametrize("dim", (2, 3))
def test_entries_outside_the_graph_contribute_nothing(gpu_lib, dim):
    """An entry whose index is outside 0 .. n - 1 adds neither its attraction nor its negatives, and a row reaches no further than
    0 .. nnz: the result is the definition's with those entries switched off (rate 0: never active, the numbering of the others kept).
    The arrays lie inside larger ones (NaN rows around y_in), so nothing here reads outside a buffer."""
    graph = EC.exact_case("n65")[0]
    want, got = (run_of(graph, dim, 10, a=1.0, b=1.0, seed=6) for _ in range(2))
    bad = np.arange(3, got.nnz, 7)
    got.indices[bad] = np.resize(np.array([-1, got.n, got.n + 5, -7], np.int32), len(bad))
    want.rate[bad] = 0
    assert len(bad) > 20 and not same_bits(EM.host_epochs(want), EM.layout_host(graph, dim, 10, a=1.0, b=1.0, seed=6))
    assert same_bits(device_epochs(got), EM.host_epochs(want))
    # rows that claim entries in front of the CSR and behind it: clipped to 0 .. nnz
    wide = run_of(graph, dim, 10, a=1.0, b=1.0, seed=6)
    wide.indptr[0], wide.indptr[-1] = -3, wide.nnz + 4
    assert same_bits(device_epochs(wide), EM.layout_host(graph, dim, 10, a=1.0, b=1.0, seed=6))


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("general", (False, True), ids=("b1", "b"))
def test_a_continued_run_gives_the_whole_runs_bits(gpu_lib, general, dim):
    """Epochs (0, 20) then (20, 50) against (0, 50), device against device: t, T and the parity of the ping-pong are carried."""
    a, b = EM.curve_ab(0.1) if general else (1.0, 1.0)
    for name in ("n65", "star257"):
        graph = EC.exact_case(name)[0]
        whole = device_epochs(run_of(graph, dim, 50, a=a, b=b, seed=2))
        part = device_epochs(run_of(graph, dim, (0, 20), 50, a=a, b=b, seed=2))
        rest = device_epochs(run_of(graph, dim, (20, 50), 50, a=a, b=b, init=part, seed=2))
        assert same_bits(rest, whole) and not same_bits(part, whole), name
        odd = device_epochs(run_of(graph, dim, (0, 21), 50, a=a, b=b, seed=2))                     # the other parity of both halves
        assert same_bits(device_epochs(run_of(graph, dim, (21, 50), 50, a=a, b=b, init=odd, seed=2)), whole), name
        assert same_bits(EM.layout(graph, dim, (20, 50), 50, a=a, b=b, init=part, seed=2), whole), name


@pytest.mark.parametrize("dim", (2, 3))
def test_one_epoch_with_a_general_b_stays_inside_the_bound(gpu_lib, dim):
    """N = 300, a, b = curve_ab(0.1), T = 200: from the same float64 y_in at several t, the device and the definition differ per
    coordinate by at most alpha_t u sum|g| (64 + n_terms) + 1 ulp(y) (tests/embed_cases.py).
    Measured on an MI355X: the largest share of the bound used is 0.460 (dim 2) and 0.599 (dim 3), 0.7 to 13 % of the coordinates differ."""
    graph = EC.blob_graph()
    a, b = EM.curve_ab(0.1)
    worst = 0.0
    for t in (0, 1, 37, 150, 199):
        y_in = EM.layout_host(graph, dim, (0, t), 200, a=a, b=b, seed=1) if t else EM.init_positions(300, dim, 1)
        stats = {}
        want = EC.plain_layout(graph, dim, t, t + 1, 200, 5, 1.0, 1.0, a, b, y_in, 1, stats)
        assert same_bits(EM.layout_host(graph, dim, (t, t + 1), 200, a=a, b=b, init=y_in, seed=1), want)
        got = device_epochs(run_of(graph, dim, (t, t + 1), 200, a=a, b=b, init=y_in, seed=1))
        bound = EC.one_epoch_bound(want, 1.0 - t / 200, stats)
        share = float((np.abs(got - want) / bound).max())
        print(f"dim {dim}, t {t}: {int(stats['terms'].sum())} terms, largest share of the bound used {share:.3f}, "
              f"{int((got != want).sum())} of {got.size} coordinates differ")
        worst = max(worst, share)
        assert (np.abs(got - want) <= bound).all(), (t, share)
    print(f"dim {dim}: largest share of the bound used {worst:.3f}")


def test_it_is_a_map(gpu_lib):
    """Three Gaussian blobs of 100 rows (D 16, k 10, T 200, default a and b): the 10 nearest neighbours of a point on the map carry its
    own label — for the device's result and for the definition's."""
    rows, labels = EC.blobs()
    host = EM.layout_host(EC.blob_graph(), 2, 200)
    assert EC.purity(host, labels) >= 0.99, "the input is at fault"
    graph = EM.fuzzy_graph_host(*NB.neighbors(rows, None, 10))
    device = EM.layout(graph, 2, 200)
    print(f"purity: the definition {EC.purity(host, labels):.4f}, the device {EC.purity(device, labels):.4f}; largest difference {np.abs(device - host).max():.3g}")
    assert np.isfinite(device).all() and EC.purity(device, labels) >= 0.99
    got = EM.embed(rows, k=10, epochs=200)
    assert got.dtype == np.float32 and got.shape == (300, 2) and np.array_equal(got, device.astype(np.float32))
    assert EC.purity(EM.embed(rows, k=10, dim=3, epochs=200, seed=5), labels) >= 0.99
    # one row: its start; no rows: an empty map
    assert np.array_equal(EM.embed(rows[:1], dim=3, seed=9), EM.init_positions(1, 3, 9).astype(np.float32))
    assert EM.embed(rows[:0]).shape == (0, 2)
    two = EM.embed(rows[:2], epochs=30)
    assert two.shape == (2, 2) and np.isfinite(two).all()


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
    tiny = tmp_path_factory.mktemp("embed") / "tiny.wav"
    tiny.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", s16(GI.tiny_recording(3, 2)))))
    return str(tiny)


KW = dict(spec_time_step=TM.STS)


def test_patch_embedding_of_a_segmentation(gpu_lib, seg, tiny_wav):
    from whisperseg_amd.wavio import load_wav
    pred = seg.segment(*load_wav(tiny_wav), patches=8, **KW)
    rows = len(pred["onset"])
    assert rows >= 3                                   # not vacuous: the fixture model finds rows in its own signal family
    for dim in (2, 3):
        got = EM.patch_embedding([pred], k=3, dim=dim, epochs=50)
        assert list(got) == ["embedding"]
        y = got["embedding"]
        assert y.shape == (rows, dim) and y.dtype == np.float32 and np.isfinite(y).all()
        assert np.array_equal(y, EM.embed(NB.patch_rows_of([pred]), k=3, dim=dim, epochs=50))
    assert np.array_equal(EM.patch_embedding([pred])["embedding"], EM.embed(NB.patch_rows_of([pred])))      # the defaults: k 15 > rows
    # per-channel lists, as segment_files(channel_id="all") returns them; the caller's lists give the same map
    preds = seg.segment_files([tiny_wav, tiny_wav], channel_id="all", patches=8, **KW)
    flat = NB.patch_rows_of(preds)
    got = EM.patch_embedding(preds, k=2, epochs=50, seed=4)["embedding"]
    assert got.shape == (len(flat), 2) and len(flat) == 2 * rows and np.array_equal(got, EM.embed(flat, k=2, epochs=50, seed=4))
    lists = NB.patch_neighbors(preds, 2)
    assert np.array_equal(got, EM.patch_embedding(preds, k=2, epochs=50, seed=4, lists=(lists["neighbor_index"], lists["neighbor_distance"]))["embedding"])
    assert not np.array_equal(got, EM.patch_embedding(preds, k=2, epochs=50, seed=5)["embedding"])
    # a recording without a call: an empty map
    quiet = seg.segment(*load_wav(os.path.join(GOLDEN, "meerkat_5s.wav")), patches=8, **KW)
    assert EM.patch_embedding([quiet], dim=3)["embedding"].shape == (len(quiet["onset"]), 3)


def test_cli_embed(gpu_lib, seg, tiny_wav, tmp_path, monkeypatch):
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
    segment.main(base + ["--csv_save_path", str(full_csv), "--patches", "8", "--patches_save_path", str(full_npz), "--embed", "2", "--embed_neighbors", "3"])
    assert full_csv.read_bytes() == plain_csv.read_bytes()
    rows = len(plain_csv.read_text().splitlines()) - 1
    want = seg.segment(*load_wav(tiny_wav), patches=8, **KW)
    with np.load(plain_npz) as plain, np.load(full_npz) as full:
        assert set(plain.files) == {"patch", "onset", "offset", "cluster"}                       # without the flag: exactly the keys there were
        assert set(full.files) == set(plain.files) | {"embedding"}
        assert all(np.array_equal(plain[name], full[name]) for name in plain.files)
        assert rows >= 3 and full["embedding"].shape == (rows, 2) and full["embedding"].dtype == np.float32 and np.isfinite(full["embedding"]).all()
        assert np.array_equal(full["embedding"], EM.patch_embedding([want], k=3)["embedding"])
    # with --neighbors of the same K the lists are shared; another K, min_dist and seed reach the layout
    both_npz, other_npz = tmp_path / "both.npz", tmp_path / "other.npz"
    segment.main(base + ["--csv_save_path", str(full_csv), "--patches", "8", "--patches_save_path", str(both_npz), "--neighbors", "3", "--embed", "2",
                         "--embed_neighbors", "3"])
    segment.main(base + ["--csv_save_path", str(full_csv), "--patches", "8", "--patches_save_path", str(other_npz), "--neighbors", "2", "--embed", "3",
                         "--embed_neighbors", "3", "--embed_min_dist", "0.5", "--embed_seed", "7"])
    with np.load(full_npz) as full, np.load(both_npz) as both, np.load(other_npz) as other:
        assert set(both.files) == set(full.files) | {"neighbor_index", "neighbor_distance"} and both["neighbor_index"].shape == (rows, 3)
        assert np.array_equal(both["embedding"], full["embedding"])
        assert other["neighbor_index"].shape == (rows, 2) and other["embedding"].shape == (rows, 3)
        assert np.array_equal(other["embedding"], EM.patch_embedding([want], k=3, dim=3, min_dist=0.5, seed=7)["embedding"])
    # folder mode with every channel: one row of the map per row of the CSV
    folder = tmp_path / "wavs"
    folder.mkdir()
    for name in ("a.wav", "b.wav"):
        (folder / name).write_bytes(open(tiny_wav, "rb").read())
    out_csv, out_npz = tmp_path / "folder.csv", tmp_path / "folder.npz"
    segment.main(["--model_path", MODEL_DIR, "--audio_folder", str(folder), "--spec_time_step", str(TM.STS), "--channel_id", "all",
                  "--csv_save_path", str(out_csv), "--patches", "8", "--patches_save_path", str(out_npz), "--embed", "3"])
    with np.load(out_npz) as arch:
        lines = out_csv.read_text().splitlines()
        assert arch["embedding"].shape == (len(lines) - 1, 3) and len(lines) - 1 == 2 * rows and np.isfinite(arch["embedding"]).all()
