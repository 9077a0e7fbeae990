"""The mutual-reachability minimum spanning tree on the GPU (wseg_mst_round_f32, whisperseg_amd/csrc/wseg_mst.hip) against the host
definition whisperseg_amd.linkage.mst_host, from one round of the kernels up to patch_clusters and the CLI's --clusters.

What may differ from the definition, and by how much, is derived in tests/mst_cases.py: nothing on exact inputs (integer rows, dyadic
rows: a round is its numpy statement entry for entry, a tree the definition's edge for edge and bit for bit, the mass ties with it),
and on inexact float rows a spanning tree whose weights are the definition's w of their edges to one float32 ulp and whose sorted
weights stay within the derived slack.  The shapes are the smallest at which the kernels can go wrong: ragged tiles, D = 1, 3, 17 and
2 562 (the zero-filled tail, the scalar loads), unaligned rows, several candidate splits.  Every device run of a round reads its
inputs between NaN guards and writes between guards."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import golden_inputs as GI
import mst_cases as MC
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import linkage as LK
from whisperseg_amd import neighbors as NB

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
GUARD_BITS = 0x7fc12345               # float guards: a NaN no kernel writes
GUARD_INDEX = -0x12345                # int32 guards


def guarded(values, unaligned=False):
    """-> the array as a device tensor inside a larger one, NaN (or the int guard) in front and behind; `unaligned`: the first
    element sits 4 bytes past a 16-byte boundary."""
    values = np.ascontiguousarray(values)
    lead = values.size // len(values) if values.ndim == 2 else 4            # one row, or four words: the alignment is kept
    lead += 1 if unaligned else 0
    fill = float("nan") if values.dtype == np.float32 else GUARD_INDEX
    whole = torch.full((lead + values.size + 5,), fill, dtype=torch.from_numpy(values).dtype, device="cuda")
    assert whole.data_ptr() % 16 == 0
    whole[lead:lead + values.size] = torch.from_numpy(values).cuda().reshape(-1)
    inside = whole[lead:lead + values.size].view(values.shape)
    if values.ndim == 2 and values.shape[1] % 4 == 0:
        assert (inside.data_ptr() % 16 != 0) == unaligned
    return inside


def device_round(rows, core, component, unaligned=False):
    """mst_round on guarded inputs into guarded outputs -> (index, weight) as numpy; the guards must survive."""
    n = len(rows)
    held_i = torch.full((n + 8,), GUARD_INDEX, dtype=torch.int32, device="cuda")
    held_w = torch.from_numpy(np.full((n + 8,), GUARD_BITS, np.uint32).view(np.float32)).cuda()
    got_i, got_w = LK.mst_round(guarded(rows, unaligned), guarded(core), guarded(component), out_index=held_i[4:n + 4], out_weight=held_w[4:n + 4])
    assert got_i.data_ptr() == held_i[4:n + 4].data_ptr() and got_w.data_ptr() == held_w[4:n + 4].data_ptr()
    index, weight = held_i.cpu().numpy(), held_w.cpu().numpy()
    for edge in (slice(0, 4), slice(n + 4, n + 8)):
        assert (index[edge] == GUARD_INDEX).all() and (weight[edge].view(np.uint32) == GUARD_BITS).all(), "a guard was written"
    return np.ascontiguousarray(index[4:n + 4]), np.ascontiguousarray(weight[4:n + 4])


@functools.lru_cache(maxsize=None)
def round_reference(n, d):
    """(rows, core, w) of the single-round cases: integer rows, the definition's core at s = min(3, N - 1).  Computed once."""
    rows = MC.rows_of("integer", n, d)
    core, w = LK.weights_host(rows, min(3, n - 1))
    return rows, core, w


@pytest.mark.parametrize("d", MC.ROUND_D)
@pytest.mark.parametrize("n", MC.ROUND_N)
def test_one_round_is_its_numpy_statement(gpu_lib, n, d):
    rows, core, w = round_reference(n, d)
    for pattern in MC.PATTERNS:
        comp = MC.components_of(pattern, n)
        want_i, want_w = MC.round_host(w, comp)
        for unaligned in (False, True):
            index, weight = device_round(rows, core, comp, unaligned)
            wrong = np.flatnonzero((index != want_i) | (weight.view(np.uint32) != want_w.view(np.uint32)))
            assert not len(wrong), (n, d, pattern, unaligned, int(wrong[0]), int(index[wrong[0]]), int(want_i[wrong[0]]),
                                    float(weight[wrong[0]]), float(want_w[wrong[0]]))
        if pattern == "one":
            assert (index == -1).all() and np.isposinf(weight).all()


def test_a_round_with_cores_that_dominate(gpu_lib):
    """core is the caller's: large cores clamp every weight of their row (mass ties at w = core, broken by the lower j), zero cores
    leave the distances."""
    rows, _, _ = round_reference(257, 17)
    d32 = NB.distances_host(rows, rows).astype(np.float32)
    rng = np.random.default_rng(MC.SEED)
    for core in (np.zeros(257, np.float32), rng.integers(0, 400, size=257).astype(np.float32)):
        w = np.maximum(np.maximum(core[:, None], core[None, :]), d32)
        comp = MC.components_of("mod3", 257)
        want = MC.round_host(w, comp)
        got = device_round(rows, core, comp)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@functools.lru_cache(maxsize=None)
def device_tree(kind, n, d, s):
    edges, weight = LK.mst(MC.rows_of(kind, n, d), s)
    edges.setflags(write=False)
    weight.setflags(write=False)
    return edges, weight


@pytest.mark.parametrize("case", MC.EXACT_TREES, ids=lambda c: "-".join(map(str, c)))
def test_exact_inputs_give_the_definitions_tree(gpu_lib, case):
    ref = MC.reference(*case)
    stats = {}
    got = LK.mst(torch.from_numpy(ref.x).cuda(), ref.s, stats=stats)
    MC.check_spanning(*got, ref.n, case)
    wrong = np.flatnonzero((got[0] != ref.edges).any(axis=1) | (got[1].view(np.uint32) != ref.weight.view(np.uint32)))
    assert not len(wrong) and MC.same_tree(got, (ref.edges, ref.weight)), (case, int(wrong[0]), got[0][wrong[0]].tolist(), ref.edges[wrong[0]].tolist(),
                                                                           float(got[1][wrong[0]]), float(ref.weight[wrong[0]]))
    assert MC.same_tree(device_tree(*case), got)                           # from numpy as from a resident tensor
    assert 1 <= stats["rounds"] <= int(np.ceil(np.log2(ref.n)))
    print(f"{case}: {stats['rounds']} rounds")


def test_same_tree_for_every_grid(gpu_lib, monkeypatch):
    cases = (("integer", 1000, 16, 15), ("dyadic", 300, 64, 5), ("clustered", 1000, 64, 5))
    for cap in ("1", "3"):
        monkeypatch.setenv("WSEG_MST_GRID", cap)
        for case in cases:
            assert MC.same_tree(LK.mst(MC.rows_of(*case[:3]), case[3]), device_tree(*case)), (case, cap)
    monkeypatch.delenv("WSEG_MST_GRID")
    assert MC.same_tree(LK.mst(MC.rows_of(*cases[2][:3]), cases[2][3]), device_tree(*cases[2]))
    # one round, too: the knob changes the splits, not a bit of the result
    rows, core, w = round_reference(1000, 17)
    comp = MC.components_of("blocks", 1000)
    whole = device_round(rows, core, comp)
    for cap in ("1", "3"):
        monkeypatch.setenv("WSEG_MST_GRID", cap)
        got = device_round(rows, core, comp)
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1].view(np.uint32), whole[1].view(np.uint32)), cap


@pytest.mark.parametrize("shape", MC.FLOAT_TREES, ids=lambda s: "x".join(map(str, s)))
def test_float_rows_within_the_slack(gpu_lib, shape):
    """Clustered Gaussian rows: a spanning tree, every weight w of its edge to 1 ulp, the sorted weights within the derived slack.
    Measured on an MI355X: D = 64: 0.000 of the slack used at most, 100.0 % of the edges the definition's; D = 2 560: 0.000 and
    100.0 %."""
    d, n, s = shape
    ref = MC.reference("clustered", n, d, s)
    stats = {}
    edges, weight = LK.mst(ref.x, s, stats=stats)
    assert MC.same_tree((edges, weight), device_tree("clustered", n, d, s))                       # the same bits on every run
    used, same = MC.check_contract(ref, edges, weight, what=shape)
    print(f"(D, N, s) = {shape}: {stats['rounds']} rounds; slack {ref.slack:.3g} (median weight {np.median(ref.weight):.3g}), largest share used "
          f"{used:.3f}; {100 * same:.1f} % of the edges are the definition's")


def test_invalid_calls_are_refused_before_a_launch(gpu_lib):
    from whisperseg_amd import _lib
    x = torch.from_numpy(MC.rows_of("integer", 129, 16)).cuda()
    core = torch.zeros(129, device="cuda")
    comp = torch.arange(129, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.WsegError, match="no CPU path"):
        LK.mst_round(x.cpu(), core, comp)
    with pytest.raises(_lib.WsegError, match="no CPU path"):
        LK.mst_round(x.t(), core, comp)
    with pytest.raises(ValueError, match="2-D"):
        LK.mst_round(x[0], core, comp)
    with pytest.raises(ValueError, match="D must"):
        LK.mst_round(torch.zeros((3, 20481), device="cuda"), core[:3], comp[:3])
    for bad in (core.cpu(), core[:128], core.double(), torch.zeros(258, device="cuda")[::2]):
        with pytest.raises(_lib.WsegError, match="core"):
            LK.mst_round(x, bad, comp)
    for bad in (comp.cpu(), comp[:128], comp.long()):
        with pytest.raises(_lib.WsegError, match="component"):
            LK.mst_round(x, core, bad)
    for bad in (torch.empty(128, dtype=torch.int32, device="cuda"), torch.empty(129, dtype=torch.int64, device="cuda"), torch.empty(129, dtype=torch.int32)):
        with pytest.raises(_lib.WsegError, match="out_index"):
            LK.mst_round(x, core, comp, out_index=bad)
    for bad in (torch.empty(130, device="cuda"), torch.empty(129, dtype=torch.float64, device="cuda"), torch.empty(129)):
        with pytest.raises(_lib.WsegError, match="out_weight"):
            LK.mst_round(x, core, comp, out_weight=bad)
    index, weight = LK.mst_round(x[:0], core[:0], comp[:0])
    assert index.shape == weight.shape == (0,) and index.dtype == torch.int32 and weight.dtype == torch.float32 and index.is_cuda
    for s in (0, 65, 129):
        with pytest.raises(ValueError, match="min_samples"):
            LK.mst(x, s)
    edges, weight = LK.mst(x[:2], 1)
    assert edges.tolist() == [[0, 1]] and weight[0] == float(((x[0] - x[1]) ** 2).sum())


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
    tiny = tmp_path_factory.mktemp("mst") / "tiny.wav"
    tiny.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", s16(GI.tiny_recording(3, 2)))))
    return str(tiny)


KW = dict(spec_time_step=TM.STS)


def check_archive_tree(patch, cluster, edges, weight, min_size, s, what):
    """The three arrays of `patch` [rows, 80, W]: the tree within the contract of the definition's, the labels those of that tree."""
    rows = np.ascontiguousarray(patch.reshape(len(patch), patch.shape[1] * patch.shape[2]))
    n = len(rows)
    assert cluster.shape == (n,) and cluster.dtype == np.int32, what
    MC.check_spanning(edges, weight, n, what)
    if n >= 2:
        MC.check_contract(MC.Reference(rows, min(s, n - 1)), edges, weight, what=what)
        assert np.array_equal(cluster, LK.hdbscan_labels(edges, weight, n, min_size)), what
    else:
        assert (cluster == -1).all()


def test_patch_clusters_of_a_segmentation(gpu_lib, seg, tiny_wav):
    from whisperseg_amd.wavio import load_wav
    total = 0
    for path in (os.path.join(GOLDEN, "meerkat_5s.wav"), tiny_wav):
        pred = seg.segment(*load_wav(path), patches=8, **KW)
        got = LK.patch_clusters([pred], 2, min_samples=2)
        assert list(got) == ["cluster", "mst_edges", "mst_weight"]
        check_archive_tree(pred["patch"], got["cluster"], got["mst_edges"], got["mst_weight"], 2, 2, os.path.basename(path))
        total += len(pred["onset"])
    assert total >= 3                                  # not vacuous: the fixture model finds rows in its own signal family
    # per-channel lists, as segment_files(channel_id="all") returns them; the same file twice: every row has a twin at weight 0 with
    # s = 1, and the twins share a cluster
    preds = seg.segment_files([tiny_wav, tiny_wav], channel_id="all", patches=8, **KW)
    got = LK.patch_clusters(preds, 2, min_samples=1)
    flat = np.concatenate([r["patch"] for res in preds for r in res], axis=0)
    check_archive_tree(flat, got["cluster"], got["mst_edges"], got["mst_weight"], 2, 1, "two files, every channel")
    half = len(flat) // 2
    assert half >= 1 and (got["mst_weight"][:half] == 0).all() and np.array_equal(got["cluster"][:half], got["cluster"][half:])


def test_cli_clusters(gpu_lib, seg, tiny_wav, tmp_path, monkeypatch):
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
    segment.main(base + ["--csv_save_path", str(full_csv), "--patches", "8", "--patches_save_path", str(full_npz), "--clusters", "2",
                         "--cluster_min_samples", "2"])
    assert full_csv.read_bytes() == plain_csv.read_bytes() and len(plain_csv.read_text().splitlines()) > 3
    with np.load(plain_npz) as plain, np.load(full_npz) as full:
        assert set(plain.files) == {"patch", "onset", "offset", "cluster"}                       # without the flag: exactly the keys there were
        assert set(full.files) == set(plain.files) | {"patch_cluster", "mst_edges", "mst_weight"}
        assert all(np.array_equal(plain[name], full[name]) for name in plain.files)             # the model's `cluster` among them
        rows = len(plain_csv.read_text().splitlines()) - 1
        assert full["patch"].shape == (rows, 80, 8)
        check_archive_tree(full["patch"], full["patch_cluster"], full["mst_edges"], full["mst_weight"], 2, 2, "the archive")
        want = seg.segment(*load_wav(tiny_wav), patches=8, **KW)
        got = LK.patch_clusters([want], 2, min_samples=2)
        assert np.array_equal(full["patch_cluster"], got["cluster"]) and MC.same_tree((full["mst_edges"], full["mst_weight"]), (got["mst_edges"], got["mst_weight"]))
    # folder mode with every channel, the default S: the tree counts the archive's rows, which are the CSV's
    folder = tmp_path / "wavs"
    folder.mkdir()
    for name in ("a.wav", "b.wav"):
        (folder / name).write_bytes(open(tiny_wav, "rb").read())
    out_csv, out_npz = tmp_path / "folder.csv", tmp_path / "folder.npz"
    segment.main(["--model_path", MODEL_DIR, "--audio_folder", str(folder), "--spec_time_step", str(TM.STS), "--channel_id", "all",
                  "--csv_save_path", str(out_csv), "--patches", "8", "--patches_save_path", str(out_npz), "--clusters", "2"])
    with np.load(out_npz) as arch:
        lines = out_csv.read_text().splitlines()
        assert arch["patch_cluster"].shape == (len(lines) - 1,) and len(lines) - 1 == 2 * rows
        check_archive_tree(arch["patch"], arch["patch_cluster"], arch["mst_edges"], arch["mst_weight"], 2, 5, "folder mode")
