"""The channels of a multi-channel recording kept apart, without a GPU: wavio.load_wav(mono=False) against a restatement that
decodes the bytes of one channel at a time (planar_cases.planes), the file pipeline's `channel_id`, segment_files' pooling and
regrouping of channels on a stub segmenter, the CLI's --channel_id and the binding of wseg_pcm_to_planar_f32."""
import ctypes as C
import hashlib
import io
import os
import sys
import threading

import numpy as np
import pytest

import planar_cases as PC
import wav_cases as WC
from conftest import ROOT
from planar_cases import bits
from whisperseg_amd import wavio
from whisperseg_amd.wavio import load_wav, read_wav_raw


# ---- 1. load_wav(mono=False) -----------------------------------------------------------------------------------------------
def check_planar(blob, fmt, channels, n):
    raw = read_wav_raw(io.BytesIO(blob))
    assert (raw.channels, raw.n_frames) == (channels, n)
    got, sr = load_wav(io.BytesIO(blob), mono=False)
    want = PC.planes(raw.data, fmt, channels, n)
    assert sr == raw.sr and got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
    if channels == 1:
        assert got.shape == (n,)
        want = want[0]
    else:
        assert got.shape == (channels, n)
    assert np.array_equal(bits(got), bits(want)), (fmt, channels, n)
    # the mono mix is what it was: the restated mean of the interleaved bytes, and load_wav(blob) == load_wav(blob, mono=True)
    mono, _ = load_wav(io.BytesIO(blob))
    assert mono.shape == (n,) and np.array_equal(bits(mono), bits(WC.restate(raw.data, fmt, channels, n)))
    assert np.array_equal(bits(mono), bits(load_wav(io.BytesIO(blob), mono=True)[0]))
    if 1 < channels < 8:             # numpy sums fewer than 8 channels left to right
        s = got[0]
        with np.errstate(invalid="ignore", over="ignore"):
            for c in range(1, channels):
                s = s + got[c]
            mean = (np.float32(0) + s) / np.float32(channels)
        assert np.array_equal(bits(mono), bits(mean)), (fmt, channels, n)
    return got


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", WC.FORMATS)
def test_load_wav_keeps_the_channels_apart(fmt, channels):
    for n in (0, 1, 5, 64):
        check_planar(WC.make_wav(fmt, channels, n), fmt, channels, n)


@pytest.mark.parametrize("fmt", WC.FORMATS)
def test_load_wav_planar_of_extensible_and_ragged_files(fmt):
    data = PC.data_chunk(fmt, 3, 101, seed=5)
    got = check_planar(WC.wav_bytes(fmt, 3, 16000, data, extensible=True), fmt, 3, 101)
    width = WC.BYTES[WC.FORMATS.index(fmt)]
    cut = check_planar(WC.wav_bytes(fmt, 3, 16000, data[:len(data) - width]), fmt, 3, 100)      # ends inside a frame: whole frames only
    assert np.array_equal(bits(cut), bits(got[:, :100]))


# ---- 2. the file pipeline with a host stand-in for the device half --------------------------------------------------------
class PlanarHostIngest:
    """wavio.DeviceIngest's interface on the host, the planar half included; decodes with the numpy restatements.  An event
    completes at its second query."""

    def __init__(self):
        self.calls, self.views = [], []

    def acquire(self, count, nbytes):
        self.views = [np.zeros(nbytes, np.uint8) for _ in range(count)]
        return self.views

    def new_output(self, n_frames):
        self.calls.append(("new_output", n_frames))
        return np.full(n_frames, np.nan, np.float32)

    def new_planar_output(self, n_channels, n_frames):
        self.calls.append(("new_planar_output", n_channels, n_frames))
        return np.full((n_channels, n_frames), np.nan, np.float32)

    def submit(self, view, nbytes, info, out, frame0, n_frames):
        assert frame0 % 16 == 0 and nbytes == n_frames * info.frame_bytes <= len(view)
        self.calls.append(("submit", frame0, n_frames))
        out[frame0:frame0 + n_frames] = WC.restate(view[:nbytes], info.format, info.channels, n_frames)
        return {"queries": 0}

    def submit_planar(self, view, nbytes, info, out, frame0, n_frames, first_channel):
        assert frame0 % 16 == 0 and nbytes == n_frames * info.frame_bytes <= len(view) and out.ndim == 2
        self.calls.append(("submit_planar", frame0, n_frames, first_channel, out.shape[0]))
        out[:, frame0:frame0 + n_frames] = PC.planes(view[:nbytes], info.format, info.channels, n_frames, first_channel, out.shape[0])
        return {"queries": 0}

    def done(self, event, wait):
        event["queries"] += 1
        return wait or event["queries"] >= 2


def reader_threads():
    return [t for t in threading.enumerate() if t.name == "wseg-wav-reader"]


SPECS = [("s16", 2, 5000, 16000), ("s24", 1, 1021, 32000), ("f32", 3, 700, 48000), ("u8", 2, 0, 8000), ("s32", 5, 3333, 44100),
         ("f64", 2, 64, 16000), ("s24", 3, 1500, 22050)]


def folder(tmp_path, specs=SPECS):
    paths = []
    for i, (fmt, ch, n, sr) in enumerate(specs):
        p = tmp_path / f"{i}_{fmt}.wav"
        p.write_bytes(WC.make_wav(fmt, ch, n, seed=i, sr=sr))
        paths.append(str(p))
    return paths


def equal_items(got, want):
    assert len(got) == len(want)
    for (a, sr_a), (b, sr_b) in zip(got, want):
        assert sr_a == sr_b and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("buffer_bytes", [1 << 20, 4096])      # whole files; pieces of at most 4 KiB
def test_pipeline_yields_channels(tmp_path, buffer_bytes):
    paths = folder(tmp_path)
    planar = [load_wav(p, mono=False) for p in paths]
    host = PlanarHostIngest()
    equal_items(list(wavio.FilePipeline(paths, host, buffer_bytes=buffer_bytes, channel_id="all")), planar)
    assert not reader_threads()
    if buffer_bytes == 4096:
        assert sum(c[0] == "submit_planar" for c in host.calls) > len(paths)       # the larger files went through in pieces
    assert ("new_planar_output", 5, 3333) in host.calls and ("new_output", 1021) in host.calls
    for k in (1, -1, 0):
        host = PlanarHostIngest()
        want = [(a if a.ndim == 1 else a[k], sr) for a, sr in planar]            # the one-channel file gives its samples
        equal_items(list(wavio.FilePipeline(paths, host, buffer_bytes=buffer_bytes, channel_id=k)), want)
        planar_calls = [c for c in host.calls if c[0] == "submit_planar"]
        assert planar_calls and all(c[4] == 1 for c in planar_calls)              # one plane decoded, not all of them
        assert {c[3] for c in planar_calls} <= {0, 1, 2, 4}
        assert not reader_threads()
    # channel_id=None is the pipeline as it was: the mono mix through new_output / submit alone
    host = PlanarHostIngest()
    equal_items(list(wavio.FilePipeline(paths, host, buffer_bytes=buffer_bytes)), [load_wav(p) for p in paths])
    assert {c[0] for c in host.calls} == {"new_output", "submit"}


def test_pipeline_raises_index_error_with_the_files_name(tmp_path):
    paths = folder(tmp_path)
    for k in (2, -3):                # fine for the 3- and 5-channel files, out of range for the stereo ones
        it = iter(wavio.FilePipeline(paths[2:], PlanarHostIngest(), channel_id=k))
        a, _ = next(it)
        assert np.array_equal(bits(a), bits(load_wav(paths[2], mono=False)[0][k]))
        with pytest.raises(IndexError, match=r"3_u8\.wav.*channel_id"):
            next(it)
        assert not reader_threads()
    with pytest.raises(ValueError, match=r"0_s16\.wav.*channel_id"):
        list(wavio.FilePipeline(paths, PlanarHostIngest(), channel_id="left"))
    assert not reader_threads()


# ---- 3. segment_files / segment_channels on a stub segmenter -----------------------------------------------------------------
def digest(a, sr, trials=None):
    return dict(sr=sr, sha=hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest(), n=len(a), trials=trials)


def stub_segmenter(buffer_bytes=1 << 20):
    from whisperseg_amd.model import SegmenterBase, _per_item

    class Stub(SegmenterBase):
        def __init__(self):
            super().__init__()
            self.host, self.ingest_buffer_bytes, self.batches = PlanarHostIngest(), buffer_bytes, 0

        def ingest_backend(self):
            return self.host

        def segment_batch(self, audios, srs=None, num_trials=1, **kwargs):
            self.batches += 1
            self.kwargs = kwargs
            pairs = iter(audios) if srs is None else ((a, srs) for a in audios)
            return [digest(a, sr, nt) for (a, sr), nt in zip(pairs, _per_item(num_trials))]      # drawn as segment_batch draws them

    return Stub()


@pytest.mark.parametrize("buffer_bytes", [1 << 20, 4096])
def test_segment_files_pools_all_channels_and_regroups_them(tmp_path, buffer_bytes):
    paths = folder(tmp_path)
    planar = [load_wav(p, mono=False) for p in paths]
    seg = stub_segmenter(buffer_bytes)
    got = seg.segment_files(paths, channel_id="all", eps=0.5)
    assert seg.batches == 1 and seg.kwargs == {"eps": 0.5}                          # ONE pooled segment_batch
    assert got == [[digest(row, sr, 1) for row in (a if a.ndim == 2 else [a])] for a, sr in planar]
    assert [len(g) for g in got] == [2, 1, 3, 2, 5, 2, 3] and not reader_threads()
    # a per-recording list stays per FILE: a file's value applies to each of its channels
    trials = [1, 2, 3, 4, 5, 6, 7]
    got = seg.segment_files(paths, channel_id="all", num_trials=trials)
    assert [[r["trials"] for r in g] for g in got] == [[t] * len(g) for t, g in zip(trials, got)]
    with pytest.raises(ValueError, match="fewer entries"):
        seg.segment_files(paths, channel_id="all", num_trials=trials[:3])
    assert not reader_threads()
    # one channel of every file: a flat list, the one-channel file's samples among them
    got = seg.segment_files(paths, channel_id=1, num_trials=trials)
    assert got == [digest(a if a.ndim == 1 else a[1], sr, t) for (a, sr), t in zip(planar, trials)]
    # and without channel_id, what it gave before
    assert seg.segment_files(paths) == [digest(a, sr, 1) for a, sr in map(load_wav, paths)]
    with pytest.raises(IndexError, match=r"0_s16\.wav"):
        seg.segment_files(paths, channel_id=2)
    assert not reader_threads() and seg.segment_files([], channel_id="all") == []


def test_segment_channels_is_segment_batch_over_the_rows():
    seg = stub_segmenter()
    a, sr = load_wav(io.BytesIO(WC.make_wav("s16", 3, 300)), mono=False)
    assert seg.segment_channels(a, sr, num_trials=2) == [digest(row, sr, 2) for row in a]
    assert seg.segment_channels(a[0], sr) == [digest(a[0], sr, 1)] and seg.batches == 2
    with pytest.raises(ValueError):
        seg.segment_channels(a[None], sr)


# ---- 4. the CLI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    return segment


def test_cli_channel_id_argument(cli):
    p = cli.build_parser()
    assert p.parse_args([]).channel_id is None
    assert p.parse_args(["--channel_id", "2"]).channel_id == 2 and p.parse_args(["--channel_id", "-1"]).channel_id == -1
    assert p.parse_args(["--channel_id", "all"]).channel_id == "all"
    for bad in ("x", "1.5", "ALL", ""):
        with pytest.raises(SystemExit):
            p.parse_args(["--channel_id", bad])


def test_cli_columns_and_row_order(cli):
    r = lambda *rows: dict(onset=[x[0] for x in rows], offset=[x[1] for x in rows], cluster=[x[2] for x in rows])
    per_file = [[r((0.1, 0.2, "a"), (0.3, 0.4, "b")), r()], [r((1.0, 1.5, "c"))], [r(), r(), r((2.0, 2.25, "a"))]]
    names = ["x.wav", "y.wav", "z.WAV"]
    text = io.StringIO()
    cli.write_csv(*cli.table(per_file, names, all_channels=True), text)
    assert text.getvalue() == ("filename,channel,onset,offset,cluster\nx.wav,0,0.1,0.2,a\nx.wav,0,0.3,0.4,b\ny.wav,0,1.0,1.5,c\n"
                               "z.WAV,2,2.0,2.25,a\n")
    text = io.StringIO()
    cli.write_csv(*cli.table([per_file[0]], all_channels=True), text)               # one file (--audio_path)
    assert text.getvalue() == "channel,onset,offset,cluster\n0,0.1,0.2,a\n0,0.3,0.4,b\n"
    # an integer channel_id and no channel_id: the columns as they were
    flat = [per_file[0][0], per_file[1][0]]
    assert cli.table(flat, names[:2]) == (["filename", "onset", "offset", "cluster"],
                                          [("x.wav", 0.1, 0.2, "a"), ("x.wav", 0.3, 0.4, "b"), ("y.wav", 1.0, 1.5, "c")])
    assert cli.table(flat[:1]) == (["onset", "offset", "cluster"], [(0.1, 0.2, "a"), (0.3, 0.4, "b")])


# ---- 5. the binding ---------------------------------------------------------------------------------------------------------
def test_planar_symbol_is_bound_with_the_declared_types():
    from whisperseg_amd import _lib
    assert _lib.SYMBOLS["wseg_pcm_to_planar_f32"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                                C.c_void_p, C.c_int64, C.c_void_p])
    with open(os.path.join(ROOT, "include", "wseg.h")) as f:
        header = " ".join(f.read().split())
    assert ("int wseg_pcm_to_planar_f32(const void* raw, int64_t n_frames, int32_t channels, int32_t format, int32_t first_channel, "
            "int32_t n_out_channels, float* out, int64_t plane_stride, void* stream);") in header
    assert wavio.PLANAR_TILE_FRAMES % 16 == 0
    with open(os.path.join(ROOT, "whisperseg_amd", "csrc", "wseg_ingest.hip")) as f:
        src = f.read()
    assert "constexpr int kPlanarTile = %d;" % wavio.PLANAR_TILE_FRAMES in src      # the exported constants are the kernel's
    assert "constexpr int kPlanarGridCap = %d;" % wavio.PLANAR_GRID_CAP in src
