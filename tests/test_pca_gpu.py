"""The principal-component kernels on the GPU (wseg_pca_moments_f64 / wseg_pca_project_f64, whisperseg_amd/csrc/wseg_pca.hip: float64
on the matrix cores) against the host definition whisperseg_amd.pca, from the kernels up to pca(), embed(init="pca"), patch_pca and
the CLI's --pca / --embed_init.

On integer-valued rows every partial sum is exact and nothing may differ: the moments are moments_exact's bits, both triangles of
the Gram matrix alike, on the smallest shapes at which the tiling can go wrong (tests/pca_cases.py).  On float rows the moments and
the scores stay inside the bounds derived there.  Every raw call writes between NaN guard words and reads rows that lie between NaN
rows."""
import os
import sys

import numpy as np
import pytest
import torch

import golden_inputs as GI
import pca_cases as PCS
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import embed as EM
from whisperseg_amd import neighbors as NB
from whisperseg_amd import pca as PC

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
GUARD_BITS = 0x7ff8000000012345          # float64 guards: a NaN no kernel writes
PAD = 32                                 # guard words in front of and behind a buffer
WSEG_ERR_INVALID = -1


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def guarded(words):
    """-> (the whole float64 device buffer of guard words, its inner `words` words)."""
    guard = torch.from_numpy(np.array([GUARD_BITS], np.uint64).view(np.float64)).cuda()
    whole = guard.repeat(words + 2 * PAD).contiguous()
    return whole, whole[PAD:PAD + words]


def guards_intact(whole, words):
    bits = whole.cpu().numpy().view(np.uint64)
    return bool((bits[:PAD] == GUARD_BITS).all() and (bits[PAD + words:] == GUARD_BITS).all())


def untouched(whole):
    return bool((whole.cpu().numpy().view(np.uint64) == GUARD_BITS).all())


def between_nan_rows(rows, pad=3):
    """-> the float32 rows as a device tensor inside a larger one: `pad` rows of NaN in front and behind, which would poison every sum
    that read them."""
    rows = np.array(rows, dtype=np.float32, order="C")
    whole = torch.full((len(rows) + 2 * pad, rows.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
    whole[pad:pad + len(rows)] = torch.from_numpy(rows).cuda()
    return whole[pad:pad + len(rows)]


def device_moments(rows):
    """wseg_pca_moments_f64 with sum, gram and the scratch between guard words -> (s, S) as numpy; the guards must survive and the rows
    must be left as they were."""
    from whisperseg_amd import _lib
    lib = _lib.load(require_device=True)
    n, d = rows.shape
    x = between_nan_rows(rows)
    s_whole, s = guarded(d)
    g_whole, g = guarded(d * d)
    words = PC.scratch_bytes(n, d) // 8
    w_whole, w = guarded(words)
    _lib.check(lib.wseg_pca_moments_f64(x.data_ptr(), n, d, s.data_ptr(), g.data_ptr(), w.data_ptr(), words * 8, _lib.stream_ptr()))
    assert guards_intact(s_whole, d) and guards_intact(g_whole, d * d) and guards_intact(w_whole, words), "a guard was written"
    assert np.array_equal(x.cpu().numpy(), np.asarray(rows, np.float32)), "the rows were written"
    return s.cpu().numpy(), g.cpu().numpy().reshape(d, d)


def device_project(rows, mean, basis):
    """wseg_pca_project_f64 with out between guard words, mean and basis between NaNs -> the scores as numpy."""
    from whisperseg_amd import _lib
    lib = _lib.load(require_device=True)
    n, d = rows.shape
    r = basis.shape[1]
    x = between_nan_rows(rows)
    mean_d = torch.full((d + 16,), float("nan"), dtype=torch.float64, device="cuda")
    mean_d[8:8 + d] = torch.from_numpy(np.ascontiguousarray(mean, dtype=np.float64)).cuda()
    basis_d = torch.full((d + 4, r), float("nan"), dtype=torch.float64, device="cuda")
    basis_d[2:2 + d] = torch.from_numpy(np.ascontiguousarray(basis, dtype=np.float64)).cuda()
    o_whole, o = guarded(n * r)
    _lib.check(lib.wseg_pca_project_f64(x.data_ptr(), n, d, mean_d[8:].data_ptr(), basis_d[2:].data_ptr(), r, o.data_ptr(), _lib.stream_ptr()))
    assert guards_intact(o_whole, n * r), "a guard was written"
    assert np.array_equal(x.cpu().numpy(), np.asarray(rows, np.float32)), "the rows were written"
    return o.cpu().numpy().reshape(n, r)


# ---- the moments -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", PCS.EXACT_PAIRS)
def test_exact_cases_give_the_definitions_bits(gpu_lib, n, d):
    want_s, want_gram = PCS.exact_moments(n, d)
    s, gram = device_moments(PCS.exact_rows(n, d))
    wrong = gram.view(np.uint64) != want_gram.view(np.uint64)
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:8].tolist())
    assert same_bits(s, want_s), np.flatnonzero(s != want_s)[:8].tolist()
    assert same_bits(gram, np.ascontiguousarray(gram.T))
    assert PCS.splits_of(n, d) == PCS.MULTI_SPLIT.get((n, d), 1)


@pytest.mark.parametrize("n,d", PCS.FLOAT_PAIRS)
def test_float_cases_stay_inside_the_bound(gpu_lib, n, d):
    """Measured on an MI355X: the largest share of the bound used is 0.488 for the Gram matrix (N = 5, D = 130; 0.022 at N = 1027) and
    0.000 for the sums; at N = 1027, D = 130 two thirds of the entries differ from the correctly rounded sum, by last bits."""
    want_s, want_gram = PCS.float_moments(n, d)
    bound_s, bound_gram = PCS.moments_bound(PCS.float_rows(n, d))
    s, gram = device_moments(PCS.float_rows(n, d))
    share_s, share_gram = float((np.abs(s - want_s) / bound_s).max()), float((np.abs(gram - want_gram) / bound_gram).max())
    print(f"N {n}, D {d}: largest share of the bound used: sums {share_s:.3f}, Gram matrix {share_gram:.3f}; "
          f"{int((gram != want_gram).sum())} of {gram.size} entries differ from the correctly rounded sum")
    assert (np.abs(s - want_s) <= bound_s).all() and (np.abs(gram - want_gram) <= bound_gram).all(), (share_s, share_gram)
    assert same_bits(gram, np.ascontiguousarray(gram.T))


# ---- the projection ------------------------------------------------------------------------------------------------------------------
PROJECT_SHAPES = ((2, 1, 1), (5, 15, 15), (63, 17, 16), (65, 65, 17), (65, 16, 16), (257, 130, 33), (1027, 130, 64), (3, 33, 2))


@pytest.mark.parametrize("n,d,r", PROJECT_SHAPES)
def test_integer_projection_is_exact(gpu_lib, n, d, r):
    rows, mean, basis = PCS.integer_projection(n, d, r)
    want = (rows.astype(np.float64) - mean) @ basis                      # exact: integers below 2^53 in every order
    got = device_project(rows, mean, basis)
    wrong = got.view(np.uint64) != want.view(np.uint64)
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:8].tolist())
    assert same_bits(PC.project(rows, mean, basis), want)


@pytest.mark.parametrize("n,d,r", PROJECT_SHAPES)
def test_float_projection_stays_inside_the_bound(gpu_lib, n, d, r):
    """Measured on an MI355X: the largest share of the bound used is 0.123 (N = 63, D = 17, r = 16)."""
    rows, mean, basis = PCS.float_projection(n, d, r)
    want, bound = PCS.project_reference(rows, mean, basis)
    got = device_project(rows, mean, basis)
    share = float((np.abs(got - want) / bound).max())
    print(f"N {n}, D {d}, r {r}: largest share of the bound used {share:.3f}")
    assert (np.abs(got - want) <= bound).all(), share


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
def test_the_same_bits_on_every_run_and_under_every_grid_cap(gpu_lib, monkeypatch):
    cases = ((1027, 130), (257, 65), (65, 130))
    base = {}
    for case in cases:
        base[case] = device_moments(PCS.float_rows(*case))
        again = device_moments(PCS.float_rows(*case))
        assert same_bits(base[case][0], again[0]) and same_bits(base[case][1], again[1]), case
    proj = PCS.float_projection(1027, 130, 33)
    z = device_project(*proj)
    assert same_bits(z, device_project(*proj))
    for cap in ("1", "3"):
        monkeypatch.setenv("WSEG_PCA_GRID", cap)
        for case in cases:
            s, gram = device_moments(PCS.float_rows(*case))
            assert same_bits(s, base[case][0]) and same_bits(gram, base[case][1]), (case, cap)
        assert same_bits(device_project(*proj), z), cap
    monkeypatch.delenv("WSEG_PCA_GRID")
    s, gram = device_moments(PCS.float_rows(*cases[0]))
    assert same_bits(s, base[cases[0]][0]) and same_bits(gram, base[cases[0]][1])


# ---- invalid calls -------------------------------------------------------------------------------------------------------------------
def test_invalid_calls_are_refused_and_write_nothing(gpu_lib):
    from whisperseg_amd import _lib
    lib = _lib.load(require_device=True)
    n, d, r = 65, 17, 5
    x = torch.from_numpy(np.array(PCS.exact_rows(n, d))).cuda()
    s_whole, s = guarded(d)
    g_whole, g = guarded(d * d)
    words = PC.scratch_bytes(n, d) // 8
    w_whole, w = guarded(words)
    mean = torch.zeros(d, dtype=torch.float64, device="cuda")
    basis = torch.zeros((d, r), dtype=torch.float64, device="cuda")
    o_whole, o = guarded(n * r)

    def moments(rows=x.data_ptr(), n=n, d=d, sum_=s.data_ptr(), gram=g.data_ptr(), scratch=w.data_ptr(), nbytes=words * 8):
        return lib.wseg_pca_moments_f64(rows, n, d, sum_, gram, scratch, nbytes, _lib.stream_ptr())

    def project(rows=x.data_ptr(), n=n, d=d, mean_=mean.data_ptr(), basis_=basis.data_ptr(), r=r, out=o.data_ptr()):
        return lib.wseg_pca_project_f64(rows, n, d, mean_, basis_, r, out, _lib.stream_ptr())

    for kw, word in ((dict(rows=None), b"rows"), (dict(rows=x.data_ptr() + 2), b"rows"), (dict(sum_=None), b"sum"), (dict(sum_=s.data_ptr() + 4), b"sum"),
                     (dict(gram=None), b"gram"), (dict(gram=g.data_ptr() + 4), b"gram"), (dict(scratch=None), b"scratch"),
                     (dict(scratch=w.data_ptr() + 4), b"scratch"), (dict(nbytes=words * 8 - 8), b"scratch"), (dict(nbytes=0), b"scratch"),
                     (dict(d=0), b"d must"), (dict(d=8193), b"d must"), (dict(n=0), b"n must"), (dict(n=2 ** 31), b"n must"),
                     (dict(gram=s.data_ptr()), b"overlap"), (dict(scratch=g.data_ptr()), b"overlap"), (dict(sum_=x.data_ptr()), b"overlap")):
        assert moments(**kw) == WSEG_ERR_INVALID and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())
    for kw, word in ((dict(rows=None), b"rows"), (dict(rows=x.data_ptr() + 1), b"rows"), (dict(mean_=None), b"mean"), (dict(mean_=mean.data_ptr() + 4), b"mean"),
                     (dict(basis_=None), b"basis"), (dict(basis_=basis.data_ptr() + 4), b"basis"), (dict(out=None), b"out"), (dict(out=o.data_ptr() + 4), b"out"),
                     (dict(d=0), b"d must"), (dict(d=8193), b"d must"), (dict(r=0), b"r must"), (dict(r=65), b"r must"), (dict(n=0), b"n must"),
                     (dict(out=basis.data_ptr()), b"overlap")):
        assert project(**kw) == WSEG_ERR_INVALID and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())
    torch.cuda.synchronize()
    assert untouched(s_whole) and untouched(g_whole) and untouched(w_whole) and untouched(o_whole), "a refused call wrote"
    assert not mean.any() and not basis.any()
    one = np.zeros((1, d), np.float32)
    for call in (lambda: PC.moments(one), lambda: PC.pca(one, 1), lambda: PC.pca(torch.from_numpy(one).cuda(), 1),
                 lambda: PC.pca(PCS.exact_rows(n, d), 0), lambda: PC.pca(PCS.exact_rows(n, d), 18), lambda: PC.pca(PCS.exact_rows(5, 16), 5),
                 lambda: PC.pca(np.zeros((4, 3, 2), np.float32), 1), lambda: PC.pca(np.zeros((3, 8193), np.float32), 1)):
        with pytest.raises(ValueError):
            call()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
ARRAYS = ("mean", "components", "variance", "variance_ratio", "scores")


@pytest.mark.parametrize("n,d", ((65, 130), (257, 17), (1027, 15), (5, 16), (63, 65)))
def test_pca_of_an_exact_case_is_the_definitions(gpu_lib, n, d):
    """The moments have the definition's bits and the host steps behind them are the same calls, so mean, components, variance and
    ratio are equal bit for bit.  The float64 scores of the two sides come from different orders of one sum and may differ in their
    last bits; the float32 they are rounded to once hides that unless a value lies within those bits of a rounding boundary.
    Measured on an MI355X: 0 of 520, 2056, 8216, 20 and 504 float32 scores differ."""
    rows = PCS.exact_rows(n, d)
    r = min(8, d, n - 1)
    want, got = PC.pca_host(rows, r), PC.pca(rows, r)
    assert list(got) == list(ARRAYS) and list(want) == list(ARRAYS)
    for name in ARRAYS[:4]:
        assert same_bits(got[name], want[name]), name
    differ = got["scores"] != want["scores"]
    print(f"N {n}, D {d}, r {r}: {int(differ.sum())} of {differ.size} float32 scores differ")
    assert got["scores"].dtype == np.float32 and got["scores"].shape == (n, r) and np.array_equal(got["scores"], want["scores"])
    resident = PC.pca(torch.from_numpy(np.array(rows)).cuda(), r, scores=False)
    assert list(resident) == list(ARRAYS[:4]) and all(same_bits(resident[name], want[name]) for name in ARRAYS[:4])


def test_pca_of_the_diagonal_case_is_exact_in_every_array(gpu_lib):
    rows = PCS.diagonal_case()
    want, got = PC.pca_host(rows, 5), PC.pca(rows, 5)
    for name in ARRAYS[:4]:
        assert same_bits(got[name], want[name]), name
    assert np.array_equal(got["components"], np.eye(12)[:5]) and np.array_equal(got["mean"], np.arange(12) % 5 - 2.0)
    assert np.array_equal(got["scores"], want["scores"]) and np.array_equal(np.abs(got["scores"]), np.tile(np.arange(12.0, 7.0, -1.0), (64, 1)))


@pytest.mark.parametrize("n,d", ((257, 15), (1027, 130)))
def test_pca_of_a_float_case_stays_inside_the_bounds(gpu_lib, n, d):
    """variance: the two covariance matrices differ by dC — both sides' moments lie within the moments bound of the exact ones, and the
    covariance formula rounds three times on each side — so by Weyl's inequality the eigenvalues differ by at most ||dC||_F, plus
    what each side's eigh adds (HOST_EIG_REL of the largest eigenvalue, measured against a known answer in tests/pca_cases.py).
    scores: the float32 scores against a longdouble evaluation with the device run's OWN mean and components; the rounding to
    float32 (2^-24 |z|) is most of what is allowed, so a share near 1 is that rounding at its worst, not the kernel.
    Measured on an MI355X: the variances differ by 5.8e-15 (tolerance 7.3e-12) and 3.6e-15 (2.9e-10), the scores use 0.982 and 0.989."""
    rows = PCS.float_rows(n, d)
    r = min(8, d)
    want, got = PC.pca_host(rows, r), PC.pca(rows, r)
    s, gram = PCS.float_moments(n, d)
    bound_s, bound_gram = PCS.moments_bound(rows)
    abs_s = np.abs(s) + bound_s
    d_cov = 2 * (bound_gram + (np.outer(abs_s, bound_s) + np.outer(bound_s, abs_s)) / n) / (n - 1)
    d_cov = d_cov + 2 * 4 * PCS.U * (np.abs(gram) + np.outer(abs_s, abs_s) / n) / (n - 1)
    weyl = float(np.sqrt((d_cov ** 2).sum()))
    tolerance = weyl + 2 * PCS.HOST_EIG_REL * float(want["variance"][0])
    worst = float(np.abs(got["variance"] - want["variance"]).max())
    print(f"N {n}, D {d}: variance differs by at most {worst:.3g}; Weyl {weyl:.3g}, tolerance {tolerance:.3g}")
    assert worst <= tolerance
    assert np.allclose(got["mean"], want["mean"], rtol=0, atol=float((2 * bound_s / n + 2 * PCS.U * np.abs(want["mean"])).max()))
    z, bound = PCS.project_reference(rows, got["mean"], got["components"].T)
    err = np.abs(got["scores"].astype(np.float64) - z)
    allowed = bound + 2.0 ** -24 * (np.abs(z) + bound) + 2.0 ** -149
    print(f"N {n}, D {d}: largest share of the score bound used {float((err / allowed).max()):.3f}")
    assert (err <= allowed).all()
    host = PC.project_host(rows, got["mean"], got["components"].T)
    assert (np.abs(host - z) <= bound).all()


def blob_rows():
    rng = np.random.default_rng(77)
    centres = rng.normal(0.0, 4.0, (3, 24))
    rows = (centres[np.arange(90) % 3] + rng.normal(0.0, 1.0, (90, 24))).astype(np.float32)
    rows[11] = rows[10]                                    # two identical rows: the jitter must separate their starts
    return rows


def test_embed_from_the_pca_start(gpu_lib):
    rows = blob_rows()
    lists = NB.neighbors(rows, None, 10)
    graph = EM.fuzzy_graph_host(*lists)
    for dim, seed in ((2, 0), (3, 5)):
        y0 = EM.pca_start(PC.pca(rows, dim)["scores"], seed)
        assert y0.dtype == np.float64 and y0.shape == (90, dim) and np.abs(y0).max() <= 10 + 1e-4 and not np.array_equal(y0[10], y0[11])
        # b == 1: the device's epochs from this start are the definition's, bit for bit
        got = EM.layout(graph, dim, 30, a=1.0, b=1.0, init=y0, seed=seed)
        assert same_bits(got, EM.layout_host(graph, dim, 30, a=1.0, b=1.0, init=y0, seed=seed))
        # embed(init="pca") is the layout from that start
        a, b = EM.curve_ab(0.1)
        want = EM.layout(graph, dim, 30, a=a, b=b, init=y0, seed=seed).astype(np.float32)
        assert np.array_equal(EM.embed(rows, k=10, dim=dim, epochs=30, seed=seed, init="pca"), want)
        assert np.array_equal(EM.embed(rows, k=10, dim=dim, epochs=30, seed=seed, init="pca", lists=lists), want)
        assert not np.array_equal(EM.embed(rows, k=10, dim=dim, epochs=30, seed=seed), want)
    # fewer than dim + 1 rows have no dim components: the hashed start
    assert np.array_equal(EM.embed(rows[:2], epochs=5, init="pca"), EM.embed(rows[:2], epochs=5))
    with pytest.raises(ValueError, match="init"):
        EM.embed(rows, init="spectral")


def test_embed_without_init_is_what_it_was(gpu_lib):
    """The default path: the hashed start.  With a = b = 1 the epochs from it are layout_host's bits; embed() is the device layout of
    the same graph from init_positions."""
    rows = blob_rows()
    graph = EM.fuzzy_graph_host(*NB.neighbors(rows, None, 10))
    assert same_bits(EM.layout(graph, 2, 30, a=1.0, b=1.0, seed=3), EM.layout_host(graph, 2, 30, a=1.0, b=1.0, init=EM.init_positions(90, 2, 3), seed=3))
    a, b = EM.curve_ab(0.1)
    want = EM.layout(graph, 2, 30, a=a, b=b, init=EM.init_positions(90, 2, 3), seed=3).astype(np.float32)
    assert np.array_equal(EM.embed(rows, k=10, epochs=30, seed=3), want) and np.array_equal(EM.embed(rows, k=10, epochs=30, seed=3, init=None), want)


@pytest.fixture(scope="module")
def seg():
    from whisperseg_amd.model import WhisperSegmenter
    return WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")


def s16(v):
    return np.clip(np.round(np.asarray(v, np.float64) * 32768), -32768, 32767).astype(np.int64)


@pytest.fixture(scope="module")
def tiny_wav(tmp_path_factory):
    """A recording of the fixture model's own signal family as an s16 file: the model finds rows in it."""
    tiny = tmp_path_factory.mktemp("pca") / "tiny.wav"
    tiny.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", s16(GI.tiny_recording(3, 2)))))
    return str(tiny)


KW = dict(spec_time_step=TM.STS)
SHAPES = {"pca_mean": ((640,), np.float64), "pca_components": ((2, 640), np.float64), "pca_variance": ((2,), np.float64),
          "pca_variance_ratio": ((2,), np.float64)}


def test_patch_pca_and_the_cli(gpu_lib, seg, tiny_wav, tmp_path, monkeypatch):
    from whisperseg_amd.wavio import load_wav
    pred = seg.segment(*load_wav(tiny_wav), patches=8, **KW)
    rows = len(pred["onset"])
    assert rows >= 3                                   # not vacuous: the fixture model finds rows in its own signal family
    got = PC.patch_pca([pred], 2)
    flat = NB.patch_rows_of([pred])
    want = PC.pca(flat, 2)
    assert list(got) == ["pca_" + name for name in ARRAYS]
    for name in ARRAYS:
        assert np.array_equal(got["pca_" + name], want[name]) and got["pca_" + name].dtype == want[name].dtype, name
    assert got["pca_scores"].shape == (rows, 2) and got["pca_scores"].dtype == np.float32 and 0 < got["pca_variance_ratio"].sum() <= 1 + 1e-12
    # a recording without a call: empty arrays with the trailing shapes, and nothing runs
    quiet = seg.segment(*load_wav(os.path.join(GOLDEN, "meerkat_5s.wav")), patches=8, **KW)
    if len(quiet["onset"]) < 2:
        none = PC.patch_pca([quiet], 2)
        assert none["pca_components"].shape == (0, 640) and none["pca_scores"].shape == (0, 2) and none["pca_scores"].dtype == np.float32
    with pytest.raises(ValueError, match="r must"):
        PC.patch_pca([pred], rows)                     # more components than rows - 1

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    monkeypatch.setenv("WHISPERSEG_AMD_DTYPE", "f32")
    base = ["--model_path", MODEL_DIR, "--audio_path", tiny_wav, "--spec_time_step", str(TM.STS)]
    paths = {name: (tmp_path / (name + ".csv"), tmp_path / (name + ".npz")) for name in ("plain", "pca", "embed", "hash", "start")}

    def run(name, *flags):
        segment.main(base + ["--csv_save_path", str(paths[name][0]), "--patches", "8", "--patches_save_path", str(paths[name][1])] + list(flags))

    run("plain")
    run("pca", "--pca", "2")
    run("embed", "--embed", "2", "--embed_neighbors", "3")
    run("hash", "--embed", "2", "--embed_neighbors", "3", "--embed_init", "hash")
    run("start", "--embed", "2", "--embed_neighbors", "3", "--embed_init", "pca", "--pca", "2")
    assert all(paths[name][0].read_bytes() == paths["plain"][0].read_bytes() for name in paths)
    with np.load(paths["plain"][1]) as plain, np.load(paths["pca"][1]) as full, np.load(paths["embed"][1]) as embed, np.load(paths["hash"][1]) as hashed, \
            np.load(paths["start"][1]) as start:
        assert set(plain.files) == {"patch", "onset", "offset", "cluster"}                       # without the flags: exactly the keys there were
        assert set(full.files) == set(plain.files) | {"pca_" + name for name in ARRAYS}
        assert all(np.array_equal(plain[name], full[name]) for name in plain.files)
        for name, (shape, dtype) in SHAPES.items():
            assert full[name].shape == shape and full[name].dtype == dtype, name
        assert full["pca_scores"].shape == (rows, 2) and full["pca_scores"].dtype == np.float32
        again = PC.pca(full["patch"].reshape(rows, 640), 2)
        assert all(np.array_equal(full["pca_" + name], again[name]) for name in ARRAYS)
        # --embed_init hash is the archive without the flag, array for array
        assert set(embed.files) == set(hashed.files) == set(plain.files) | {"embedding"}
        assert all(np.array_equal(embed[name], hashed[name]) and embed[name].dtype == hashed[name].dtype for name in embed.files)
        assert np.array_equal(embed["embedding"], EM.patch_embedding([pred], k=3)["embedding"])
        assert set(start.files) == set(full.files) | {"embedding"} and all(np.array_equal(start["pca_" + name], full["pca_" + name]) for name in ARRAYS)
        assert np.array_equal(start["embedding"], EM.patch_embedding([pred], k=3, init="pca")["embedding"])
        assert not np.array_equal(start["embedding"], embed["embedding"])
