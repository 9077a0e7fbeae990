"""whisperseg_amd/pca.py on the host: the moments against their correctly rounded values, the conventions of the decomposition against a
construction with a known answer, the projection against longdouble, argument errors, the start of the map from the scores, the
CLI's --pca / --embed_init flags and the host plan of the device path (wseg_pca_scratch_bytes and the validation of the two entry
points: no device needed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pca_cases as PCS
from conftest import ROOT
from whisperseg_amd import embed as EM
from whisperseg_amd import pca as PC


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n,d", PCS.EXACT_PAIRS[:8])
def test_moments_host_is_exact_on_integer_rows(n, d):
    s, gram = PC.moments_host(PCS.exact_rows(n, d))
    want_s, want_gram = PCS.exact_moments(n, d)
    assert same_bits(s, want_s) and same_bits(gram, want_gram) and same_bits(gram, np.ascontiguousarray(gram.T))
    plain = PCS.exact_rows(n, d).astype(np.int64)
    assert np.array_equal(want_gram, plain.T @ plain) and np.array_equal(want_s, plain.sum(axis=0))      # the exact reference is exact
    assert not np.array_equal(want_gram[:, ::-1], want_gram) or d == 1


@pytest.mark.parametrize("n,d", PCS.FLOAT_PAIRS)
def test_moments_host_stays_inside_the_bound(n, d):
    rows = PCS.float_rows(n, d)
    s, gram = PC.moments_host(rows)
    want_s, want_gram = PCS.float_moments(n, d)
    bound_s, bound_gram = PCS.moments_bound(rows)
    assert (np.abs(s - want_s) <= bound_s).all() and (np.abs(gram - want_gram) <= bound_gram).all()
    assert same_bits(gram, np.ascontiguousarray(gram.T))


def test_moments_host_in_blocks(monkeypatch):
    rows = PCS.exact_rows(1027, 15)
    whole = PC.moments_host(rows)
    monkeypatch.setattr(PC, "HOST_BLOCK_BYTES", 8 * 15 * 100)
    parts = PC.moments_host(rows)
    assert same_bits(whole[0], parts[0]) and same_bits(whole[1], parts[1])
    z = PC.project_host(rows, np.ones(15), np.eye(15)[:, :3])
    assert np.array_equal(z, rows[:, :3].astype(np.float64) - 1.0)


def test_splits_and_scratch_mirror_the_plan():
    """pca_cases.splits_of / scratch_bytes_of restate csrc/wseg_pca_plan.h; the library's size agrees, and the shapes the exact cases
    name as split are split."""
    for n, d in PCS.EXACT_PAIRS + PCS.FLOAT_PAIRS:
        assert PC.scratch_bytes(n, d) == PCS.scratch_bytes_of(n, d), (n, d)
        assert PCS.splits_of(n, d) == PCS.MULTI_SPLIT.get((n, d), 1), (n, d)
    assert sum(PCS.splits_of(n, d) > 1 for n, d in PCS.EXACT_PAIRS) >= 4 and max(PCS.MULTI_SPLIT.values()) == 5
    assert PCS.splits_of(10 ** 6, 2560) == 2 and PCS.splits_of(10 ** 6, 80) == 340 and PCS.splits_of(10 ** 6, 8192) == 1


def test_known_answer_and_conventions():
    rows, components, variance = PCS.known_answer()
    got = PC.pca_host(rows, PCS.KNOWN_R)
    eig, vec = PCS.known_answer_errors(got)
    print(f"known answer: eigenvalue error {eig:.3g} of the largest, component entry error {vec:.3g}")
    assert eig <= PCS.HOST_EIG_REL and vec <= PCS.HOST_VEC_ABS
    assert list(got) == ["mean", "components", "variance", "variance_ratio", "scores"]
    assert got["mean"].shape == (16,) and got["components"].shape == (8, 16) and got["variance"].shape == (8,) and got["scores"].shape == (64, 8)
    assert all(got[name].dtype == np.float64 for name in ("mean", "components", "variance", "variance_ratio")) and got["scores"].dtype == np.float32
    assert np.abs(got["mean"]).max() <= 1e-14 and (np.diff(got["variance"]) < 0).all()
    assert 0 < got["variance_ratio"].sum() <= 1 and np.allclose(got["variance_ratio"], variance[:8] / variance.sum(), rtol=1e-12)
    # the scores are U sigma, up to the sign of a component
    truth = (PCS.sylvester(64)[:, 1:9] / 8.0) * PCS.SIGMA[:8]
    assert np.allclose(np.abs(got["scores"]), np.abs(truth), rtol=0, atol=1e-5)
    assert "scores" not in PC.pca_host(rows, 3, scores=False)
    # the sign rule: the entry of largest magnitude is positive, the first one on a tie
    skew = PCS.float_rows(63, 16)
    for v in PC.pca_host(skew, 15)["components"]:
        assert v[np.argmax(np.abs(v))] > 0
    tie = PC.pca_from_moments(np.zeros(2), np.array([[1.0, -1.0], [-1.0, 1.0]]), 3, 1)               # the component is (1, -1) / sqrt 2 or its negative
    assert tie["components"][0, 0] > 0 > tie["components"][0, 1] and tie["variance"][0] == 1.0 and tie["variance_ratio"][0] == 1.0


def test_rank_deficient_and_constant_inputs():
    rows = PCS.float_rows(5, 130)                                # N - 1 = 4 < D
    got = PC.pca_host(rows, 4)
    assert (got["variance"] > 0).all() and (np.diff(got["variance"]) <= 0).all() and abs(got["variance_ratio"].sum() - 1) <= 1e-9
    # eigenvalues that come out below 0 are clamped
    deep = PC.pca_host(np.tile(rows, (14, 1)), 64)               # 70 rows of rank 4: 60 eigenvalues of rounding noise, about half below 0
    assert (deep["variance"] >= 0).all() and (deep["variance"][4:] <= 1e-9).all() and deep["variance_ratio"].sum() <= 1 + 1e-9
    negative = PC.pca_from_moments(np.zeros(2), np.array([[1.0, 0.0], [0.0, -1e-3]]), 3, 2)
    assert negative["variance"].tolist() == [0.5, 0.0] and negative["variance_ratio"].tolist() == [0.5 / (0.5 - 5e-4), 0.0]
    # a zero-variance column takes no part; no variance at all: ratio 0
    flat = np.array(PCS.exact_rows(65, 16))
    flat[:, 3] = 5.0
    got = PC.pca_host(flat, 15)
    assert np.abs(got["components"][:, 3]).max() <= 1e-12 and got["mean"][3] == 5.0
    const = PC.pca_host(np.full((4, 3), 2.0, np.float32), 2)
    assert const["variance"].tolist() == [0.0, 0.0] and const["variance_ratio"].tolist() == [0.0, 0.0] and not const["scores"].any()
    assert np.isfinite(const["components"]).all()


@pytest.mark.parametrize("n,d,r", ((5, 15, 15), (65, 65, 17), (257, 130, 33)))
def test_project_host_against_longdouble(n, d, r):
    rows, mean, basis = PCS.float_projection(n, d, r)
    want, bound = PCS.project_reference(rows, mean, basis)
    assert (np.abs(PC.project_host(rows, mean, basis) - want) <= bound).all()
    rows, mean, basis = PCS.integer_projection(n, d, r)
    want, _ = PCS.project_reference(rows, mean, basis)
    assert same_bits(PC.project_host(rows, mean, basis), want)


def test_argument_errors():
    rows = np.array(PCS.exact_rows(5, 16))
    for fn in (PC.pca_host, PC.pca):                             # refused before a device is looked for
        for r in (0, 5, 17, 65, -1, 2.0, True, None):
            with pytest.raises(ValueError, match="r must"):
                fn(rows, r)
        with pytest.raises(ValueError, match="2-D"):
            fn(rows.reshape(5, 4, 4), 1)
        with pytest.raises(ValueError, match="2-D"):
            fn(rows[0], 1)
        with pytest.raises(ValueError, match="D must"):
            fn(np.zeros((3, 8193), np.float32), 1)
        with pytest.raises(ValueError, match="D must"):
            fn(np.zeros((3, 0), np.float32), 1)
        with pytest.raises(ValueError, match="N must"):
            fn(rows[:1], 1)
        with pytest.raises(ValueError, match="N must"):
            fn(rows[:0], 1)
    for fn in (PC.moments_host, PC.moments, PC.moments_exact):
        with pytest.raises(ValueError, match="N must"):
            fn(rows[:1])
        with pytest.raises(ValueError, match="2-D"):
            fn(rows[0])
    for fn in (PC.project_host, PC.project):
        for mean, basis in ((np.zeros(15), np.zeros((16, 2))), (np.zeros(16), np.zeros((15, 2))), (np.zeros(16), np.zeros(16)),
                            (np.zeros(16), np.zeros((16, 0))), (np.zeros(16), np.zeros((16, 65))), (np.zeros((16, 1)), np.zeros((16, 2)))):
            with pytest.raises(ValueError):
                fn(rows, mean, basis)
    assert PC.pca_host(rows, 4)["scores"].shape == (5, 4)       # r = min(64, D, N - 1) is taken
    with pytest.raises(ValueError):
        PC.pca_from_moments(np.zeros(3), np.zeros((2, 2)), 5, 1)
    good = {"onset": [0.1, 0.2], "offset": [0.15, 0.3], "cluster": ["a", "b"], "patch": np.zeros((2, 80, 4), np.float32)}
    plain = {k: v for k, v in good.items() if k != "patch"}
    with pytest.raises(ValueError, match="patch"):
        PC.patch_pca([good, plain], 1)
    for r in (0, 65, 1.5):
        with pytest.raises(ValueError, match="r must"):
            PC.patch_pca([good], r)
    with pytest.raises(ValueError, match="r must"):
        PC.patch_pca([good], 2)                                  # 2 rows have one component; refused before a device is looked for
    # no rows, or one: empty arrays with the trailing shapes, nothing runs
    one = dict(good, onset=[0.1], offset=[0.2], cluster=["a"], patch=np.zeros((1, 80, 4), np.float32))
    for preds, d in (([], 0), ([one], 320), ([[dict(one, patch=np.zeros((0, 80, 4), np.float32), onset=[], offset=[], cluster=[])]], 320)):
        got = PC.patch_pca(preds, 3)
        assert list(got) == ["pca_mean", "pca_components", "pca_variance", "pca_variance_ratio", "pca_scores"]
        assert got["pca_components"].shape == (0, d) and got["pca_scores"].shape == (0, 3) and got["pca_scores"].dtype == np.float32
        assert got["pca_mean"].shape == got["pca_variance"].shape == got["pca_variance_ratio"].shape == (0,) and got["pca_mean"].dtype == np.float64


def test_pca_start_by_hand():
    """Four rows on a line, the middle two identical: the scores along the first component are -3, 0, 0, 3 times a unit, the second
    component carries nothing.  The start is the scores scaled to 10 plus 1e-5 of the hashed start — which alone keeps the identical
    rows apart."""
    z = np.array([[-3.0, 0.5], [0.0, -0.25], [0.0, -0.25], [3.0, 0.0]])
    hashed = EM.init_positions(4, 2, 7)
    y0 = EM.pca_start(z, 7)
    assert same_bits(y0, z * (10.0 / 3.0) + 1e-5 * hashed)
    assert y0[0, 0] == -10.0 + 1e-5 * hashed[0, 0] and y0[3, 0] == 10.0 + 1e-5 * hashed[3, 0]
    assert same_bits(y0[1], 1e-5 * hashed[1] + np.array([0.0, -0.25 * (10.0 / 3.0)])) and not np.array_equal(y0[1], y0[2])
    assert np.abs(y0[1] - y0[2]).max() <= 2e-4
    # nothing to scale, or too few rows: the hashed start alone
    assert same_bits(EM.pca_start(np.zeros((4, 2)), 7), hashed)
    assert same_bits(EM.pca_start(z[:2], 7), EM.init_positions(2, 2, 7)) and EM.pca_start(np.zeros((0, 3)), 1).shape == (0, 3)
    assert same_bits(EM.pca_start(z.astype(np.float32), 7), y0)              # float32 scores are taken as float64


def test_embed_builds_its_start_from_pca(monkeypatch):
    """embed(init="pca") with the device steps replaced by the host definition: the start handed to the layout is pca_start of the
    host scores, and nothing else about the call changes."""
    rows = np.array([[0, 0, 0], [1, 2, 0], [1, 2, 0], [2, 4, 1], [3, 6, 0]], np.float32)
    seen = {}

    def host_pca(x, r, device="cuda", scores=True):
        seen["r"] = r
        return PC.pca_host(x, r)

    def host_epochs(run, device):
        seen["y0"] = run.y0.copy()
        import torch
        return torch.from_numpy(EM.host_epochs(run))

    from whisperseg_amd import neighbors as NB
    monkeypatch.setattr(PC, "pca", host_pca)
    monkeypatch.setattr(EM, "layout_epochs", host_epochs)
    lists = NB.neighbors_host(rows, None, 2)
    got = EM.embed(rows, k=2, dim=2, epochs=5, seed=3, init="pca", lists=lists)
    z = PC.pca_host(rows, 2)["scores"].astype(np.float64)
    want_y0 = z * (10.0 / np.abs(z).max()) + 1e-5 * EM.init_positions(5, 2, 3)
    assert seen["r"] == 2 and same_bits(seen["y0"], want_y0) and not np.array_equal(want_y0[1], want_y0[2])
    a, b = EM.curve_ab(0.1)
    assert np.array_equal(got, EM.layout_host(EM.fuzzy_graph_host(*lists), 2, 5, a=a, b=b, init=want_y0, seed=3).astype(np.float32))
    assert np.array_equal(EM.patch_embedding([{"patch": rows.reshape(5, 3, 1)}], k=2, epochs=5, seed=3, init="pca", lists=lists)["embedding"], got)
    # the default is the hashed start; too few rows for dim components fall back to it
    EM.embed(rows, k=2, dim=2, epochs=5, seed=3, lists=lists)
    assert same_bits(seen["y0"], EM.init_positions(5, 2, 3))
    EM.embed(rows[:3], k=2, dim=3, epochs=5, seed=3, init="pca", lists=NB.neighbors_host(rows[:3], None, 2))
    assert same_bits(seen["y0"], EM.init_positions(3, 3, 3))
    for bad in ("spectral", "", "PCA"):
        with pytest.raises(ValueError, match="init"):
            EM.embed(rows, k=2, init=bad, lists=lists)
        with pytest.raises(ValueError, match="init"):
            EM.patch_embedding([{"patch": rows.reshape(5, 3, 1)}], k=2, init=bad)


def test_cli_flags(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    base = ["--model_path", "m", "--csv_save_path", "o.csv"]
    patches = ["--patches", "8", "--patches_save_path", "p.npz"]
    args = segment.parse_args(base + patches)
    assert args.pca is None and args.embed_init is None
    args = segment.parse_args(base + patches + ["--pca", "64", "--embed", "2", "--embed_init", "pca"])
    assert (args.pca, args.embed_init) == (64, "pca")
    assert segment.parse_args(base + patches + ["--embed", "3", "--embed_init", "hash"]).embed_init == "hash"
    assert segment.parse_args(base + ["--patches", "1", "--patches_save_path", "p.npz", "--pca", "64"]).pca == 64        # 80 columns
    for extra, word in ((["--pca", "2"], "pca"), (patches + ["--pca", "0"], "pca"), (patches + ["--pca", "65"], "pca"), (patches + ["--pca", "-1"], "pca"),
                        (patches + ["--pca", "x"], "pca"), (patches + ["--embed_init", "pca"], "embed_init"), (patches + ["--embed_init", "hash"], "embed_init"),
                        (patches + ["--embed", "2", "--embed_init", "spectral"], "embed_init"), (["--embed_init", "pca"], "embed_init")):
        with pytest.raises(SystemExit) as e:
            segment.main(base + extra)                       # refused by argparse, before a model is looked for
        assert e.value.code == 2 and word in capsys.readouterr().err, extra


def test_plan_through_the_library():
    """wseg_pca_scratch_bytes is host arithmetic (no device) and monotone; the launch entry points validate on the host, before they
    touch a device, and name the argument."""
    from whisperseg_amd import _lib
    lib = _lib.load()
    sizes_n = (1, 2, 255, 256, 257, 1027, 4096, 10 ** 5, 10 ** 6, 2 ** 31 - 1)
    sizes_d = (1, 16, 64, 65, 80, 130, 2560, 2880, 5120, 8192)
    table = np.array([[PC.scratch_bytes(n, d) for d in sizes_d] for n in sizes_n])
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all() and (table % 256 == 0).all() and table.min() > 0
    assert all(table[i][j] == PCS.scratch_bytes_of(n, d) for i, n in enumerate(sizes_n) for j, d in enumerate(sizes_d))
    assert table.max() == 2048 * 64 * 65 * 8 and PC.scratch_bytes(2, 1) == (64 * 64 + 64) * 8
    for args, word in (((0, 5), "n must"), ((-1, 5), "n must"), ((2 ** 31, 5), "n must"), ((5, 0), "d must"), ((5, 8193), "d must")):
        assert lib.wseg_pca_scratch_bytes(*args) == 0 and word.encode() in lib.wseg_last_error(), args
        with pytest.raises(_lib.WsegError, match=word):
            PC.scratch_bytes(*args)
    big = 1 << 30

    def moments(rows=1 << 20, n=5, d=8, sum_=2 << 20, gram=3 << 20, scratch=4 << 20, nbytes=big):      # (pointers never dereferenced: every call is refused)
        return lib.wseg_pca_moments_f64(rows, n, d, sum_, gram, scratch, nbytes, None)

    def project(rows=1 << 20, n=5, d=8, mean=2 << 20, basis=3 << 20, r=2, out=4 << 20):
        return lib.wseg_pca_project_f64(rows, n, d, mean, basis, r, out, None)

    for kw, word in ((dict(n=0), b"n must"), (dict(n=2 ** 31), b"n must"), (dict(d=0), b"d must"), (dict(d=8193), b"d must"), (dict(rows=None), b"rows"),
                     (dict(rows=(1 << 20) + 2), b"rows"), (dict(sum_=None), b"sum"), (dict(sum_=(2 << 20) + 4), b"sum"), (dict(gram=None), b"gram"),
                     (dict(gram=(3 << 20) + 4), b"gram"), (dict(scratch=None), b"scratch"), (dict(scratch=(4 << 20) + 4), b"scratch"),
                     (dict(nbytes=PC.scratch_bytes(5, 8) - 1), b"scratch"), (dict(nbytes=0), b"scratch"), (dict(sum_=(1 << 20) + 8), b"overlap"),
                     (dict(gram=(2 << 20) + 8), b"overlap"), (dict(scratch=(3 << 20) + 8), b"overlap"), (dict(scratch=(1 << 20) - 8), b"overlap")):
        assert moments(**kw) == -1 and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())
    for kw, word in ((dict(n=0), b"n must"), (dict(d=0), b"d must"), (dict(d=8193), b"d must"), (dict(r=0), b"r must"), (dict(r=65), b"r must"),
                     (dict(rows=None), b"rows"), (dict(rows=(1 << 20) + 1), b"rows"), (dict(mean=None), b"mean"), (dict(mean=(2 << 20) + 4), b"mean"),
                     (dict(basis=None), b"basis"), (dict(basis=(3 << 20) + 4), b"basis"), (dict(out=None), b"out"), (dict(out=(4 << 20) + 4), b"out"),
                     (dict(out=(1 << 20) + 8), b"overlap"), (dict(out=2 << 20), b"overlap"), (dict(out=(3 << 20) + 64), b"overlap")):
        assert project(**kw) == -1 and word in lib.wseg_last_error(), (kw, lib.wseg_last_error())


def test_plan_check_program_under_the_sanitizer(tmp_path):
    """tools/pca_plan_check.cpp sweeps the plan over (n, d, cap); built with -fsanitize=undefined it must exit 0 and print ok."""
    exe = tmp_path / "pca_plan_check"
    subprocess.run(["c++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "pca_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
