"""A target rate in the file pipeline, without a GPU: FilePipeline / segment_files / the CLI with `sr=` on a host stand-in whose
`resample` is the oracle (oracle.resample.resample_poly_ref per row), the binding of wseg_resample_planar_f32, and the index
arithmetic of its launch plan (wseg_debug_resample_plan is host arithmetic) checked by brute force over every output."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle.resample import resample_poly_ref
from planar_cases import bits
from test_wav_planar_cpu import PlanarHostIngest, cli, digest, equal_items, folder, reader_threads, stub_segmenter  # noqa: F401
from whisperseg_amd import wavio
from whisperseg_amd.wavio import load_wav

# (sr_in, sr_out) of the planar resampler's tests, on the GPU too (tests/test_resample_planar_gpu.py)
RATIOS = [(48000, 16000), (44100, 16000), (16000, 44100), (32000, 48000), (300000, 250000), (300000, 16000), (250000, 44100),
          (8000, 16000)]
UNSTAGED = [(300000, 4000), (2500000, 44100)]                    # windows too long to stage: x is read from global memory


_ROWS = {}


def ref_row(row, sr_in, sr_out):
    """The oracle of one row, computed once per distinct row (the tests go over the same folder many times)."""
    key = (row.tobytes(), sr_in, sr_out)
    if key not in _ROWS:
        _ROWS[key] = resample_poly_ref(row, sr_in, sr_out)
        _ROWS[key].setflags(write=False)
    return _ROWS[key]


def ref(audio, sr_in, sr_out):
    """The oracle per row; a file of no frames or at its target is what it was."""
    if sr_in == sr_out or not audio.shape[-1]:
        return audio
    return ref_row(audio, sr_in, sr_out) if audio.ndim == 1 else np.stack([ref_row(r, sr_in, sr_out) for r in audio])


class ResamplingHostIngest(PlanarHostIngest):
    def resample(self, out, sr_in, sr_out):
        self.calls.append(("resample", out.shape, sr_in, sr_out))
        return ref(out, sr_in, sr_out)


def pick(audio, channel_id):
    if channel_id is None or channel_id == "all" or audio.ndim == 1:
        return audio
    return audio[channel_id]


def loaded(paths, channel_id):
    return [(pick(a, channel_id), sr) for a, sr in (load_wav(p, mono=channel_id is None) for p in paths)]


# ---- 1. the pipeline --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buffer_bytes", [1 << 20, 4096])
@pytest.mark.parametrize("channel_id", [None, "all", 1, -1])
def test_pipeline_resamples_each_file_once_behind_its_last_piece(tmp_path, channel_id, buffer_bytes):
    paths = folder(tmp_path)
    native = loaded(paths, channel_id)
    host = ResamplingHostIngest()
    got = list(wavio.FilePipeline(paths, host, sr=16000, channel_id=channel_id, buffer_bytes=buffer_bytes))
    equal_items(got, [(ref(a, sr, 16000), 16000) for a, sr in native])
    assert not reader_threads()
    # the call log, file by file: new_* opens a file, its submits follow, resample (if any) comes after the last of them
    per_file, cur = [], None
    for c in host.calls:
        if c[0].startswith("new_"):
            cur = []
            per_file.append(cur)
        cur.append(c)
    assert len(per_file) == len(paths)
    for calls, (a, sr) in zip(per_file, native):
        names = [c[0] for c in calls]
        if sr == 16000 or not a.shape[-1]:
            assert "resample" not in names
            continue
        assert names.count("resample") == 1 and names[-1] == "resample" and names[-2].startswith("submit")
        assert calls[-1] == ("resample", a.shape, sr, 16000)
        if isinstance(channel_id, int):
            assert len(calls[-1][1]) == 1                        # ONE plane, not all of them
    if buffer_bytes == 4096:
        assert sum(c[0].startswith("submit") for c in host.calls) > len(paths)


def test_pipeline_takes_a_rate_per_file_and_rejects_bad_ones(tmp_path):
    paths = folder(tmp_path)
    native = loaded(paths, None)
    rates = [None, 16000, None, 16000, 8000, 16000, None]
    host = ResamplingHostIngest()
    got = list(wavio.FilePipeline(paths, host, sr=rates))
    equal_items(got, [(ref(a, sr, sr if r is None else r), sr if r is None else r) for (a, sr), r in zip(native, rates)])
    assert [c[2:] for c in host.calls if c[0] == "resample"] == [(32000, 16000), (44100, 8000)]
    assert not reader_threads()
    for bad in (rates[:3], rates + [None], 0, -1, "16k", [16000] * 6 + [0], [16000] * 6 + ["16k"], 16000.0):
        with pytest.raises(ValueError):
            wavio.FilePipeline(paths, ResamplingHostIngest(), sr=bad)
        assert not reader_threads()
    with pytest.raises(ValueError):
        wavio.check_rate(True)
    # sr=None: the pipeline as it was, on a stand-in that cannot resample
    host = PlanarHostIngest()
    assert not hasattr(host, "resample")
    equal_items(list(wavio.FilePipeline(paths, host, sr=None)), native)
    equal_items(list(wavio.FilePipeline(paths, host, sr=[None] * len(paths), channel_id="all")), loaded(paths, "all"))
    assert not reader_threads()


# ---- 2. segment_files -------------------------------------------------------------------------------------------------------
def resampling_stub(buffer_bytes=1 << 20):
    seg = stub_segmenter(buffer_bytes)
    seg.host = ResamplingHostIngest()
    return seg


@pytest.mark.parametrize("buffer_bytes", [1 << 20, 4096])
def test_segment_files_hands_the_target_rate_to_the_front_end(tmp_path, buffer_bytes):
    paths = folder(tmp_path)
    seg = resampling_stub(buffer_bytes)
    planar = [(ref(a, sr, 16000), 16000) for a, sr in loaded(paths, "all")]
    got = seg.segment_files(paths, sr=16000, channel_id="all", eps=0.5)
    assert seg.batches == 1 and seg.kwargs == {"eps": 0.5}                          # ONE pooled segment_batch
    assert got == [[digest(row, 16000, 1) for row in (a if a.ndim == 2 else [a])] for a, _ in planar]
    # per-file lists, `sr` included, stay per FILE under "all"
    trials = [1, 2, 3, 4, 5, 6, 7]
    rates = [8000, None, 16000, None, 16000, None, 44100]
    want = [(ref(a, sr, sr if r is None else r), sr if r is None else r) for (a, sr), r in zip(loaded(paths, "all"), rates)]
    got = seg.segment_files(paths, sr=rates, channel_id="all", num_trials=trials)
    assert got == [[digest(row, sr, t) for row in (a if a.ndim == 2 else [a])] for (a, sr), t in zip(want, trials)]
    # an integer channel and the mono mix
    got = seg.segment_files(paths, sr=16000, channel_id=1, num_trials=trials)
    assert got == [digest(ref(a, sr, 16000), 16000, t) for (a, sr), t in zip(loaded(paths, 1), trials)]
    assert seg.segment_files(paths, sr=16000) == [digest(ref(a, sr, 16000), 16000, 1) for a, sr in loaded(paths, None)]
    with pytest.raises(ValueError):
        seg.segment_files(paths, sr=[16000], channel_id="all")
    with pytest.raises(ValueError):
        seg.segment_files(paths, sr=0)
    assert not reader_threads()


# ---- 3. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_sr_argument(cli):  # noqa: F811
    p = cli.build_parser()
    assert p.parse_args([]).sr is None
    assert p.parse_args(["--sr", "16000"]).sr == 16000
    args = p.parse_args(["--sr", "44100", "--channel_id", "all"])
    assert (args.sr, args.channel_id) == (44100, "all")
    for bad in ("0", "-5", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(["--sr", bad])


# ---- 4. the binding ---------------------------------------------------------------------------------------------------------
def test_resample_symbols_are_bound_with_the_declared_types():
    from whisperseg_amd import _lib, resample
    assert _lib.SYMBOLS["wseg_resample_planar_f32"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int32,
                                                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                                                  C.c_int64, C.c_void_p])
    assert _lib.SYMBOLS["wseg_debug_resample_plan"] == (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                                  C.c_int32] + [C.POINTER(C.c_int32)] * 4)
    with open(os.path.join(ROOT, "include", "wseg.h")) as f:
        header = " ".join(f.read().split())
    assert ("int wseg_resample_planar_f32(const float* x, int64_t n_in, int64_t x_plane_stride, int32_t n_planes, "
            "const float* taps, int32_t n_taps, int32_t up, int32_t down, int32_t pre_pad, int32_t pre_remove, "
            "float* y, int64_t n_out, int64_t y_plane_stride, void* stream);") in header
    assert ("int wseg_debug_resample_plan(int64_t n_in, int64_t n_out, int32_t n_taps, int32_t up, int32_t down, "
            "int32_t pre_pad, int32_t pre_remove, int32_t* tile, int32_t* window, int32_t* x_staged, int32_t* taps_staged);") in header
    assert "#define WSEG_ABI_VERSION 5" in header
    with open(os.path.join(ROOT, "whisperseg_amd", "csrc", "wseg_resample.hip")) as f:
        src = f.read()
    assert "constexpr int kResampleGridCap = %d;" % resample.PLANAR_GRID_CAP in src      # the exported constant is the kernel's


# ---- 5. the launch plan -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RATIOS + UNSTAGED)
def test_launch_plan_windows_cover_every_chain(sr_in, sr_out):
    from whisperseg_amd.resample import launch_plan, plan
    seen = set()
    for n_in in (1, 300, 3000, 20000):
        p = plan(n_in, sr_in, sr_out)
        lp = launch_plan(n_in, sr_in, sr_out)
        up, down, n_taps, n_out = p["up"], p["down"], len(p["taps"]), p["n_out"]
        tile = lp["tile"]
        assert tile > 0 and tile % 64 == 0 and lp["x_staged"] in (0, 1) and lp["taps_staged"] in (0, 1)
        seen.add((tile, lp["window"], lp["x_staged"], lp["taps_staged"]))
        assert lp["x_staged"] == ((sr_in, sr_out) not in UNSTAGED)
        if not lp["x_staged"]:
            continue
        assert 0 < lp["window"] <= math.ceil((tile - 1) * down / up) + math.ceil(n_taps / up) + 2
        m = np.arange(n_out, dtype=np.int64)
        c = (m + p["pre_remove"]) * down - p["pre_pad"]
        k_hi = np.minimum(c // up, n_in - 1)                                       # resample_kernel's, floor division included
        k_lo = np.maximum(0, -(-(c - n_taps + 1) // up))
        for m0 in range(0, n_out, tile):
            lo, hi = k_lo[m0:m0 + tile], k_hi[m0:m0 + tile]
            w0 = lo[0]                                                             # the window starts at k_lo of the tile's first output
            live = hi >= lo
            assert (lo[live] >= w0).all() and (hi[live] < w0 + lp["window"]).all(), (n_in, m0)
            assert hi[-1] == hi.max() and lo[0] == lo.min()                        # ... and ends at k_hi of its last
    assert len(seen) == 1                                                          # a function of the ratio alone


def test_launch_plan_of_the_named_ratios():
    from whisperseg_amd import _lib
    from whisperseg_amd.resample import launch_plan
    assert launch_plan(3000, 44100, 16000)["taps_staged"] == 1                     # 8 821 taps fit
    assert launch_plan(3000, 250000, 44100)["taps_staged"] == 0                    # 50 001 do not
    lib = _lib.load()
    out = [C.c_int32() for _ in range(4)]
    refs = [C.byref(v) for v in out]
    for bad in ((-1, 5, 61, 1, 3, 1, 1), (5, -1, 61, 1, 3, 1, 1), (5, 5, 0, 1, 3, 1, 1), (5, 5, 61, 0, 3, 1, 1), (5, 5, 61, 1, 0, 1, 1)):
        assert lib.wseg_debug_resample_plan(*bad, *refs) == -1 and b"wseg_debug_resample_plan" in lib.wseg_last_error()
    assert lib.wseg_debug_resample_plan(5, 2, 61, 1, 3, 1, 1, None, refs[1], refs[2], refs[3]) == -1
