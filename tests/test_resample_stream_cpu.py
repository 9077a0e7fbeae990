"""A file resampled piece by piece, without a GPU: resample.stream_plan / stream_capacity checked by brute force over every output
(index sets, and a numpy restatement of the chain run on the retained segments against the same restatement on the whole signal),
FilePipeline on a host ingest that offers open_resampled, and the binding of wseg_resample_planar_range_f32, whose range
validation answers before any launch."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from test_resample_pipeline_cpu import RATIOS, UNSTAGED, ResamplingHostIngest, loaded, ref
from test_wav_planar_cpu import equal_items, folder, reader_threads
from whisperseg_amd import wavio
from whisperseg_amd.resample import plan, stream_capacity, stream_plan


def chains(p, n_in):
    """resample_kernel's index arithmetic for every output -> (c, k_lo, k_c), int64 arrays."""
    m = np.arange(p["n_out"], dtype=np.int64)
    c = (m + p["pre_remove"]) * p["down"] - p["pre_pad"]
    return c, np.maximum(0, -(-(c - len(p["taps"]) + 1) // p["up"])), c // p["up"]


def chain_sum(h, up, c, k_lo, k_hi, x, x_first):
    """One output in float64: the taps and samples of k_lo .. k_hi, x[0] being sample x_first (oracle.resample's dot product)."""
    if k_hi < k_lo:
        return 0.0
    k = np.arange(k_lo, k_hi + 1)
    return float(np.dot(h[c - k * up], x[k - x_first]))


# ---- 1. the plan, by brute force --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RATIOS + UNSTAGED)
def test_stream_plan_by_brute_force(sr_in, sr_out):
    for n_in in (1, 17, 3000):
        p = plan(n_in, sr_in, sr_out)
        up, n_out = p["up"], p["n_out"]
        h = p["taps"].astype(np.float64)
        c, k_lo, k_c = chains(p, n_in)
        k_hi = np.minimum(k_c, n_in - 1)
        x = np.random.default_rng(n_in).standard_normal(n_in).astype(np.float32).astype(np.float64)
        whole = np.array([chain_sum(h, up, c[m], k_lo[m], k_hi[m], x, 0) for m in range(n_out)])
        row = -(-len(h) // up)
        for piece in sorted({16, 48, 4096, n_in}):
            cap = stream_capacity(sr_in, sr_out, piece)
            assert cap == row - 1 + piece                                        # the ratio and the piece size, nothing else
            seg = np.full(cap, np.nan)
            first = end = emitted = 0                                            # seg holds frames [first, end)
            got = np.full(n_out, np.nan)
            steps = list(stream_plan(n_in, sr_in, sr_out, piece))
            assert [(s["frame0"], s["n"]) for s in steps] == [(f, min(piece, n_in - f)) for f in range(0, n_in, piece)]
            for s in steps:
                frame0, n = s["frame0"], s["n"]
                assert s["x_first"] == (0 if frame0 == 0 else prev["keep_from"]) and first <= s["x_first"] <= end == frame0
                kept = end - s["x_first"]
                assert kept <= row - 1 and kept + n <= cap, (n_in, piece, s)
                seg[:kept] = seg[s["x_first"] - first:end - first].copy()       # the retained frames move to the front
                seg[kept:kept + n] = x[frame0:frame0 + n]
                seg[kept + n:] = np.nan
                first, end = s["x_first"], frame0 + n
                # exactly the outputs that have become computable, in order
                assert s["m_first"] == emitted and s["m_count"] >= 0
                m1 = emitted + s["m_count"]
                want_m1 = n_out if end == n_in else int(np.searchsorted(k_c, end - 1, side="right"))      # (k_c is non-decreasing)
                assert m1 == max(want_m1, emitted) == want_m1, (n_in, piece, s)
                for m in range(emitted, m1):
                    assert k_lo[m] >= first, (n_in, piece, s, m)                 # the range call's own condition, empty chains included
                    if k_hi[m] >= k_lo[m]:
                        assert first <= k_lo[m] and k_hi[m] < end, (n_in, piece, s, m)
                    got[m] = chain_sum(h, up, c[m], k_lo[m], k_hi[m], seg, first)
                emitted = m1
                assert s["keep_from"] == (min(k_lo[m1], end) if m1 < n_out else end)
                assert first <= s["keep_from"] <= end and end - s["keep_from"] <= row - 1
                prev = s
            assert emitted == n_out and first <= end == n_in
            assert np.array_equal(got, whole), (n_in, piece)                     # the same index sets, hence the same float64 sums


def test_stream_plan_of_the_named_corners():
    # 2 500 000 -> 44 100 in 16-frame pieces: a history of 1 133 frames behind every piece, and most pieces emit nothing
    steps = list(stream_plan(3000, 2500000, 44100, 16))
    assert stream_capacity(2500000, 44100, 16) == 1133 + 16 and sum(s["m_count"] == 0 for s in steps) > len(steps) // 2
    assert max(s["frame0"] + s["n"] - s["keep_from"] for s in steps) > 16
    assert sum(s["m_count"] for s in steps) == plan(3000, 2500000, 44100)["n_out"] == 53
    # one piece: one range, nothing kept; no frames: no piece
    assert list(stream_plan(300, 48000, 16000, 300)) == [dict(frame0=0, n=300, x_first=0, m_first=0, m_count=100, keep_from=300)]
    assert list(stream_plan(0, 48000, 16000, 16)) == []
    with pytest.raises(ValueError):
        list(stream_plan(10, 48000, 16000, 0))


# ---- 2. the pipeline on a host ingest that streams -------------------------------------------------------------------------------
class HostStream:
    """wavio.StreamResampler's interface in numpy: the output at the target rate, ONE segment of stream_capacity frames per plane,
    and per piece the move, the decode behind the retained frames and the outputs of stream_plan's range, each the oracle's dot
    product over the segment."""

    def __init__(self, host, info, sel, sr_out, piece_frames):
        self.host, self.info, self.sel = host, info, sel
        self.p = plan(info.n_frames, info.sr, sr_out)
        self.h = self.p["taps"].astype(np.float64)
        self.steps = stream_plan(info.n_frames, info.sr, sr_out, piece_frames)
        self.cap = stream_capacity(info.sr, sr_out, piece_frames)
        planes = 1 if sel is None else sel[1]
        self.out = host.new_output(self.p["n_out"]) if sel is None else host.new_planar_output(planes, self.p["n_out"])
        self.seg = np.full((planes, self.cap), np.nan, np.float32)
        self.first = self.end = 0
        self.chain = chains(self.p, info.n_frames)

    def submit(self, view, nbytes, frame0, n):
        s = next(self.steps)
        assert (s["frame0"], s["n"]) == (frame0, n) and frame0 == self.end
        kept = self.end - s["x_first"]
        assert kept + n <= self.cap
        self.seg[:, :kept] = self.seg[:, s["x_first"] - self.first:self.end - self.first].copy()
        self.seg[:, kept + n:] = np.nan
        if self.sel is None:
            event = self.host.submit(view, nbytes, self.info, self.seg[0, kept:], 0, n)
        else:
            event = self.host.submit_planar(view, nbytes, self.info, self.seg[:, kept:], 0, n, self.sel[0])
        self.host.calls.append(("range", frame0, n, s["m_first"], s["m_count"]))
        self.first, self.end = s["x_first"], frame0 + n
        c, k_lo, k_c = self.chain
        rows = self.out[None] if self.out.ndim == 1 else self.out
        for row, x in zip(rows, self.seg.astype(np.float64)):
            for m in range(s["m_first"], s["m_first"] + s["m_count"]):
                row[m] = chain_sum(self.h, self.p["up"], c[m], k_lo[m], min(k_c[m], self.info.n_frames - 1), x, self.first)
        return event

    def result(self):
        assert self.end == self.info.n_frames and next(self.steps, None) is None
        return self.out


class StreamingHostIngest(ResamplingHostIngest):
    def open_resampled(self, info, sel, sr_out, piece_frames):
        self.calls.append(("open_resampled", info.n_frames, sel, info.sr, sr_out, piece_frames))
        return HostStream(self, info, sel, sr_out, piece_frames)

    def resample(self, out, sr_in, sr_out):
        raise AssertionError("resample() behind an ingest that streams")


@pytest.mark.parametrize("buffer_bytes", [1 << 20, 4096])
@pytest.mark.parametrize("channel_id", [None, "all", 1, -1])
def test_pipeline_streams_on_an_ingest_that_offers_it(tmp_path, channel_id, buffer_bytes):
    paths = folder(tmp_path)
    native = loaded(paths, channel_id)
    want = list(wavio.FilePipeline(paths, ResamplingHostIngest(), sr=16000, channel_id=channel_id, buffer_bytes=buffer_bytes))
    equal_items(want, [(ref(a, sr, 16000), 16000) for a, sr in native])
    host = StreamingHostIngest()
    got = list(wavio.FilePipeline(paths, host, sr=16000, channel_id=channel_id, buffer_bytes=buffer_bytes))
    equal_items(got, want)                                                        # the items of the stand-in that cannot stream
    assert not reader_threads()
    names = [c[0] for c in host.calls]
    assert "resample" not in names
    resampled = [(a, sr) for a, sr in native if sr != 16000 and a.shape[-1]]
    opened = [c for c in host.calls if c[0] == "open_resampled"]
    assert len(resampled) == len(opened) == 4
    for (a, sr), c in zip(resampled, opened):
        assert c[1] == a.shape[-1] and c[3:5] == (sr, 16000) and 0 < c[5] <= a.shape[-1]
        if isinstance(channel_id, int) and c[2] is not None:
            assert c[2][1] == 1                                                  # ONE plane, not all of them
    # no tensor of a resampled file's native length: what new_* makes for it is its output at the target rate
    lengths = [c[-1] for c in host.calls if c[0].startswith("new_")]
    assert sorted(lengths) == sorted(a.shape[-1] for a, _ in want)
    assert not {a.shape[-1] for a, _ in resampled} & set(lengths)
    ranges = [c for c in host.calls if c[0] == "range"]
    assert sum(c[4] for c in ranges) == sum(a.shape[-1] for (a, _), (_, sr) in zip(want, native) if sr != 16000)
    if buffer_bytes == 4096:
        assert len(ranges) > 2 * len(resampled)                                  # every resampled file went through in pieces
    else:                                                                         # (the buffers hold the largest file less its last frames)
        one_piece = [c for c in opened if c[5] == c[1]]
        assert len(one_piece) == 3 and len(ranges) == len(resampled) + 1
        for c in one_piece:                                                       # a one-piece file is ONE range call for all its outputs
            assert [r[1:4] for r in ranges if r[2] == c[1]] == [(0, c[1], 0)]


def test_pipeline_takes_a_rate_per_file_on_a_streaming_ingest(tmp_path):
    paths = folder(tmp_path)
    rates = [None, 16000, None, 16000, 8000, 16000, None]
    want = list(wavio.FilePipeline(paths, ResamplingHostIngest(), sr=rates, buffer_bytes=4096))
    host = StreamingHostIngest()
    equal_items(list(wavio.FilePipeline(paths, host, sr=rates, buffer_bytes=4096)), want)
    assert [c[3:5] for c in host.calls if c[0] == "open_resampled"] == [(32000, 16000), (44100, 8000)]
    assert not reader_threads()


# ---- 3. the binding ---------------------------------------------------------------------------------------------------------
def test_range_symbol_is_bound_with_the_declared_types():
    from whisperseg_amd import _lib
    assert _lib.SYMBOLS["wseg_resample_planar_range_f32"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int64,
                                                                        C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                                        C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p])
    lib = _lib.load()
    assert lib.wseg_resample_planar_range_f32.restype is C.c_int
    assert list(lib.wseg_resample_planar_range_f32.argtypes) == _lib.SYMBOLS["wseg_resample_planar_range_f32"][1]
    with open(os.path.join(ROOT, "include", "wseg.h")) as f:
        header = " ".join(f.read().split())
    assert ("int wseg_resample_planar_range_f32(const float* x, int64_t x_first, int64_t x_frames, int64_t x_plane_stride, "
            "int32_t n_planes, int64_t n_in, const float* taps, int32_t n_taps, int32_t up, int32_t down, int32_t pre_pad, "
            "int32_t pre_remove, float* y, int64_t m_first, int64_t m_count, int64_t y_plane_stride, void* stream);") in header
    assert "#define WSEG_ABI_VERSION 5" in header                                 # an addition


def test_rejected_ranges_answer_before_any_launch():
    """Dummy non-null pointers: every one of these calls must return from the host validation."""
    from whisperseg_amd import _lib
    lib = _lib.load()
    n_in = 3000
    p = plan(n_in, 48000, 16000)                                                 # up 1, down 3, 61 taps: output m reads 3 m - 20 .. 3 m + 10
    c, k_lo, k_c = chains(p, n_in)
    X, H, Y = 4096, 8192, 12288

    def call(x_first, x_frames, m_first, m_count, planes=1, xs=0, ys=0, x=X, h=H, y=Y, n=n_in):
        return lib.wseg_resample_planar_range_f32(x, x_first, x_frames, xs, planes, n, h, len(p["taps"]), p["up"], p["down"], p["pre_pad"],
                                                  p["pre_remove"], y, m_first, m_count, ys, None)

    m0, m1 = 400, 500
    lo, hi = int(k_lo[m0]), int(k_c[m1 - 1])
    assert 0 < lo < hi < n_in - 1
    for args, word in (((lo + 1, hi - lo, m0, m1 - m0), "before the segment"),              # a chain starting before x_first
                       ((lo, hi - lo, m0, m1 - m0), "past the segment"),                   # a chain ending past the segment
                       ((0, n_in, -1, 10), "negative"), ((0, n_in, 0, -1), "negative"), ((-1, 10, 0, 0), "negative"),
                       ((0, -1, 0, 0), "negative"), ((1, n_in, 0, 0), "inside the recording"),
                       ((0, n_in, 1 << 62, 1), "index range")):
        assert call(*args) == -1, args
        assert word in lib.wseg_last_error().decode() and "wseg_resample_planar_range_f32" in lib.wseg_last_error().decode(), (args, lib.wseg_last_error())
    for planes in (0, 65):
        assert call(lo, hi - lo + 1, m0, m1 - m0, planes=planes, xs=n_in, ys=p["n_out"]) == -1 and b"n_planes" in lib.wseg_last_error()
    for xs, ys in ((hi - lo, p["n_out"]), (n_in, m1 - 1)):                       # a stride shorter than the segment / than the last output
        assert call(lo, hi - lo + 1, m0, m1 - m0, planes=2, xs=xs, ys=ys) == -1 and b"stride" in lib.wseg_last_error()
    for kw in (dict(x=None), dict(h=None), dict(y=None), dict(x=X + 2)):
        assert call(lo, hi - lo + 1, m0, m1 - m0, **kw) == -1 and b"pointer" in lib.wseg_last_error()
    assert call(0, n_in, 0, 10, n=-1) == -1 and b"negative" in lib.wseg_last_error()
    assert call(lo, hi - lo + 1, m0, 0) == 0 and call(0, 0, p["n_out"], 0, planes=2, xs=0, ys=p["n_out"]) == 0      # no output: nothing launched
