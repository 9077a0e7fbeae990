"""The signal-to-noise ratio on the GPU (wseg_frame_energy_f32, wseg_snr_rows_f64: whisperseg_amd/csrc/wseg_snr.hip) against the host
definition whisperseg_amd.snr, stage by stage and up to segment(snr=True) and the CLI's --snr.

The selection is exact: N must be np.sort(window)[r] bit for bit, M the host's maximum bit for bit, S within count 2^-53 S of the
host's float64 sum (any order of adding non-negative terms stays inside that).  The track's tolerance and the end-to-end intervals
are tests/snr_cases.py's, taken from the float32 run of the definition and not from the code under test."""
import ctypes as C
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

import golden_inputs as GI
import measure_cases as MC
import snr_cases as SC
import wav_cases as WC
from conftest import GOLDEN, ROOT
from tools import tiny_model as TM
from whisperseg_amd import measure as M
from whisperseg_amd import pitch as P
from whisperseg_amd import snr as S
from whisperseg_amd.audio_utils import get_n_fft_given_sr

pytestmark = pytest.mark.gpu
MODEL_DIR = os.path.join(GOLDEN, "tiny_model")
GUARD = 64
BYTE_GUARD = 0xa5
SENTINEL = np.float32(-12345.5)


def device_rows(track, table, windows):
    """The launch on a host float32 track, into rows held between sentinel rows, with guard bytes behind the scratch -> float64
    [n_seg, 3]; every guard must survive."""
    from whisperseg_amd import _lib
    lib = _lib.load(require_device=True)
    track = np.ascontiguousarray(track, dtype=np.float32)
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
    windows = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 3)
    dev = torch.from_numpy(np.array(track)).cuda()
    held = torch.full((len(table) + 2 * GUARD, 3), float(SENTINEL), dtype=torch.float64, device="cuda")
    nbytes = S.scratch_bytes(len(track), table, windows)
    scratch = torch.full((nbytes + 256,), BYTE_GUARD, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wseg_snr_rows_f64(dev.data_ptr(), len(track), table.ctypes.data_as(C.c_void_p), len(table), windows.ctypes.data_as(C.c_void_p),
                                     len(windows), scratch.data_ptr(), nbytes, held[GUARD:].data_ptr(), _lib.stream_ptr()))
    host = held.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + len(table):] == SENTINEL).all()
    assert (scratch[nbytes:].cpu().numpy() == BYTE_GUARD).all()
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), track.view(np.uint32))          # the track is read only
    return host[GUARD:GUARD + len(table)]


def assert_rows(got, track, table, windows, what=""):
    """N and M bit for bit, S inside its bound, for every row."""
    floors = {}
    for i, ((j0, j1, w), g) in enumerate(zip(table, got)):
        w0, w1, r = (int(v) for v in windows[w])
        where = (what, i, int(j0), int(j1), w0, w1, r, g.tolist())
        if j1 == j0:
            assert np.isnan(g).all(), where
            continue
        if (w0, w1, r) not in floors:
            floors[w0, w1, r] = np.sort(track[w0:w1])[r]
        e = track[j0:j1]
        mean = e.astype(np.float64).sum() / len(e)
        assert SC.same_value(g[2], floors[w0, w1, r]), where
        assert SC.same_value(g[1], e.max()), where
        if np.isfinite(mean):
            assert abs(g[0] - mean) <= len(e) * 2.0 ** -53 * mean, where
        else:
            assert np.isnan(g[0]) == np.isnan(mean) and (np.isnan(mean) or g[0] == mean), where


# ---- the selection ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def select_case():
    """Every value family at every window length, back to back in ONE track, a window per quantile over each piece and a row over
    the piece itself: 9 lengths x 8 families x 4 quantiles = 288 windows, short and split, in one call."""
    pieces, table, windows = [], [], []
    pos = 0
    for length in SC.SELECT_LENGTHS:
        for family in SC.VALUE_FAMILIES:
            pieces.append(SC.select_values(family, length))
            for q in SC.QUANTILES:
                table.append((pos, pos + length, len(windows)))
                windows.append((pos, pos + length, SC.rank(q, length)))
            pos += length
    track = np.concatenate(pieces)
    track.setflags(write=False)
    return track, np.asarray(table, np.int64), np.asarray(windows, np.int64)


def test_select_is_bit_equal_to_the_sort(gpu_lib):
    track, table, windows = select_case()
    assert np.isnan(track).any() and np.isinf(track).any() and (track == 0).any() and (track.view(np.uint32) >> 31).any()
    assert_rows(device_rows(track, table, windows), track, table, windows)


def overlapping_case(n_rows, seed):
    """Windows that overlap, nest and repeat over one random track with ties, zeros, inf and NaN: a few dozen distinct triples
    — short ones, split ones, the whole track — drawn again and again by `n_rows` rows."""
    rng = np.random.default_rng(SC.SEED + seed)
    J = 3 * SC.SPLIT + 77
    track = (rng.standard_normal(J) ** 2).astype(np.float32)
    track[rng.random(J) < 0.05] = 0.0
    track[rng.random(J) < 0.05] = np.float32(0.5)
    track[rng.random(J) < 0.01] = np.inf
    track[rng.random(J) < 0.01] = np.nan
    spans = [(0, J), (0, J), (5, J - 5), (100, 100 + SC.SPLIT), (100, 101 + SC.SPLIT), (100, 99 + SC.SPLIT), (2000, 2300), (2100, 2200),
             (2100, 2200), (2150, 2151), (J - 1, J), (0, 1), (SC.SPLIT - 3, 2 * SC.SPLIT + 9), (0, 2 * SC.SPLIT + 1)]
    triples = [(a, b, SC.rank(q, b - a)) for a, b in spans for q in (0.1, 0.5, 1.0)]
    picks = rng.integers(0, len(triples), n_rows)
    windows = np.asarray([triples[i] for i in picks], np.int64)                # one window per row: repeats are the plan's to find
    j0 = rng.integers(0, J - 1, n_rows)
    j1 = np.minimum(J, j0 + 1 + rng.integers(0, 300, n_rows))
    table = np.stack([j0, j1, np.arange(n_rows)], axis=1).astype(np.int64)
    if n_rows > 3:
        table[3, 1] = table[3, 0]                                               # a row without a frame
        table[2, :2] = 0, J                                                     # a row over everything
    return track, table, windows


@pytest.mark.parametrize("n_rows", (1, 1000))
def test_overlapping_nested_and_repeated_windows(gpu_lib, n_rows, monkeypatch):
    track, table, windows = overlapping_case(n_rows, n_rows)
    got = device_rows(track, table, windows)
    assert_rows(got, track, table, windows)
    # the same rows through shared windows in another order: the dedup changes nothing
    shuffled = np.random.default_rng(3).permutation(len(windows))
    inverse = np.argsort(shuffled)
    again = device_rows(track, np.stack([table[:, 0], table[:, 1], inverse[table[:, 2]]], axis=1), windows[shuffled])
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    for cap in ("1", "3"):                                                      # the same bits for every grid
        monkeypatch.setenv("WSEG_SNR_GRID", cap)
        assert np.array_equal(device_rows(track, table, windows).view(np.uint64), got.view(np.uint64)), cap


# ---- the track ----------------------------------------------------------------------------------------------------------------------
def device_track(x, sr, band):
    """frame_energy on a slice of a larger tensor whose other samples are NaN, into a track between sentinels -> float32 [J]."""
    n_fft = get_n_fft_given_sr(sr)
    whole = torch.full((len(x) + 2 * n_fft,), float("nan"), dtype=torch.float32, device="cuda")
    whole[n_fft:n_fft + len(x)] = torch.from_numpy(np.array(x)).cuda()
    J = S.frame_count(len(x), n_fft)
    held = torch.full((J + 2 * GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    out = S.frame_energy(whole[n_fft:n_fft + len(x)], sr, *SC.bands(sr)[band], out=held[GUARD:GUARD + J])
    assert J == 0 or out.data_ptr() == held[GUARD:].data_ptr()
    host = held.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + J:] == SENTINEL).all()
    return host[GUARD:GUARD + J]


@pytest.mark.parametrize("sr", SC.RATES)
def test_track_within_the_fp32_spread(gpu_lib, sr, monkeypatch):
    x = SC.recording(sr)
    for n in SC.track_lengths(sr):
        for band in range(3):
            got = device_track(x[:n], sr, band)
            want, tol = SC.energy64(sr, band, n), SC.delta(sr, band, n)
            assert got.shape == want.shape and len(got) == S.frame_count(n, get_n_fft_given_sr(sr))
            err = np.abs(got.astype(np.float64) - want)
            print(sr, n, band, len(got), float((err / tol).max()) if len(got) else None)
            assert np.isfinite(got).all() and (err <= tol).all(), (sr, n, band, int(np.argmax(err / tol)), float((err / tol).max()))
    n, band = SC.track_lengths(sr)[-1], 1
    first = device_track(x[:n], sr, band)
    for cap in ("1", "3"):                                                      # the same bits on every run and for every grid
        monkeypatch.setenv("WSEG_SNR_GRID", cap)
        assert np.array_equal(device_track(x[:n], sr, band).view(np.uint32), first.view(np.uint32)), cap


# ---- end to end: snr() against the definition's intervals ---------------------------------------------------------------------------
@pytest.mark.parametrize("sr", SC.RATES)
def test_snr_lies_in_the_definitions_intervals(gpu_lib, sr):
    x = SC.recording(sr)
    bounds = SC.segments(sr)
    pred = MC.prediction(bounds, sr, len(x))
    pcm = torch.from_numpy(np.array(x)).cuda()
    for band, quantile, context in ((0, 0.1, None), (1, 0.1, None), (1, 0.5, 0.05), (0, 0.0, 0.0), (2, 1.0, 0.01)):
        lo, hi = SC.column_intervals(sr, band, bounds, quantile, context)
        low, high = SC.bands(sr)[band]
        got = S.snr(pcm, sr, pred, min_frequency=low, max_frequency=high, quantile=quantile, context=context)
        assert list(got) == list(S.COLUMNS)
        for c in S.COLUMNS:
            g = got[c].astype(np.float64)
            assert got[c].dtype == np.float32 and g.shape == (len(bounds),)
            empty = bounds[:, 0] == bounds[:, 1]
            assert np.isnan(g[empty]).all() and not np.isnan(g[~empty]).any(), (sr, band, c)
            inside = (lo[c] <= g) & (g <= hi[c])
            assert inside[~empty].all(), (sr, band, quantile, context, c, np.flatnonzero(~inside & ~empty)[:5], g[~inside & ~empty][:5],
                                          lo[c][~inside & ~empty][:5], hi[c][~inside & ~empty][:5])


def test_public_calls_and_conventions(gpu_lib):
    sr, n = 16000, 16000
    x = np.zeros(n, np.float32)
    x[12000:14000] = MC.tone(sr, 40, 2000, 0.25)
    pred = MC.prediction([(12000, 14000), (2000, 4000), (5000, 5000)], sr, n)
    want = S.snr_host(x, sr, pred, track=True)
    for audio in (x, torch.from_numpy(x).cuda(), torch.from_numpy(x)):
        got = S.snr(audio, sr, pred, track=True)
        assert list(got) == list(S.COLUMNS) + list(S.TRACK_KEYS) and got["hop"] == 128 and got["n_fft"] == 512
        assert got["frame_energy"].dtype == np.float32 and got["frame_energy"].shape == want["frame_energy"].shape
        for c in ("noise_level_db", "snr_db", "peak_snr_db"):                   # a zero floor: -inf, +inf and NaN as numpy has them
            assert np.array_equal(got[c][1:], want[c][1:], equal_nan=True) and got[c][0] == want[c][0], c
        assert np.isneginf(got["signal_level_db"][1]) and abs(got["signal_level_db"][0] - want["signal_level_db"][0]) < 1e-3
    assert all(len(v) == 0 for v in S.snr(x, sr, {"onset": [], "offset": []}).values())
    short = S.snr(x[:300], sr, MC.prediction([(0, 300)], sr, 300), track=True)    # J == 0: nothing launches
    assert all(np.isnan(short[c][0]) for c in S.COLUMNS) and len(short["frame_energy"]) == 0
    # a float file may hold NaN: the frames over it are NaN, sort last and leave the floor a number
    bad = SC.recording(sr).copy()
    bad[100] = np.nan
    got, want = S.snr(bad, sr, MC.prediction([(8000, 9000), (0, 1000)], sr, n)), S.snr_host(bad, sr, MC.prediction([(8000, 9000), (0, 1000)], sr, n))
    assert np.isfinite(got["snr_db"][0]) and abs(got["snr_db"][0] - want["snr_db"][0]) < 1e-3 and np.isnan(got["snr_db"][1]) and np.isnan(want["snr_db"][1])
    # the launches themselves
    pcm = torch.from_numpy(np.array(SC.recording(sr))).cuda()
    track = S.frame_energy(pcm, sr, 500)
    assert track.is_cuda and track.dtype == torch.float32 and track.shape == (S.frame_count(n, 512),)
    rows = S.snr_rows(track, [(0, 3, 0)], [(0, 10, 4)])
    assert rows.is_cuda and rows.dtype == torch.float64 and rows.shape == (1, 3)
    assert S.snr_rows(track, np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)).shape == (0, 3)


def test_invalid_calls_are_refused_before_a_launch(gpu_lib):
    from whisperseg_amd import _lib
    sr = 16000
    pcm = torch.from_numpy(np.array(SC.recording(sr))).cuda()
    track = S.frame_energy(pcm, sr)
    J = int(track.numel())
    with pytest.raises(_lib.WsegError, match="device tensor"):
        S.snr_rows(track.cpu(), [(0, 3, 0)], [(0, 10, 4)])                       # a host tensor: no CPU path
    with pytest.raises(_lib.WsegError, match="contiguous"):
        S.snr_rows(track[::2], [(0, 3, 0)], [(0, 10, 4)])
    with pytest.raises(_lib.WsegError, match="device tensor"):
        S.frame_energy(pcm.cpu(), sr)
    with pytest.raises(_lib.WsegError, match="contiguous"):
        S.frame_energy(pcm[::2], sr)
    with pytest.raises(_lib.WsegError, match="out"):
        S.frame_energy(pcm, sr, out=torch.empty(J + 1, dtype=torch.float32, device="cuda"))
    with pytest.raises(_lib.WsegError, match="out"):
        S.snr_rows(track, [(0, 3, 0)], [(0, 10, 4)], out=torch.empty((1, 3), dtype=torch.float32, device="cuda"))
    for table, windows, word in (([(0, 3, 0)], [(0, 10, 10)], "rank"), ([(0, 3, 0)], [(0, 10, -1)], "rank"), ([(0, 3, 0)], [(4, 4, 0)], "rank"),
                                 ([(0, 3, 0)], [(0, J + 1, 0)], "windows"), ([(0, J + 1, 0)], [(0, 10, 0)], "bounds"), ([(3, 2, 0)], [(0, 10, 0)], "bounds"),
                                 ([(0, 3, 1)], [(0, 10, 0)], "window of row")):
        with pytest.raises(_lib.WsegError, match=word):
            S.snr_rows(track, table, windows)
    lib = _lib.load(require_device=True)
    table, windows = np.array([[0, 3, 0]], np.int64), np.array([[0, 10, 4]], np.int64)
    nbytes = S.scratch_bytes(J, table, windows)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 3), 7.0, dtype=torch.float64, device="cuda")
    args = (track.data_ptr(), J, table.ctypes.data_as(C.c_void_p), 1, windows.ctypes.data_as(C.c_void_p), 1)
    assert lib.wseg_snr_rows_f64(*args, scratch.data_ptr(), nbytes - 1, out.data_ptr(), _lib.stream_ptr()) != 0      # scratch too small
    assert b"scratch" in lib.wseg_last_error() and (out.cpu().numpy() == 7.0).all()
    assert lib.wseg_snr_rows_f64(*args, scratch.data_ptr(), nbytes, out.data_ptr(), _lib.stream_ptr()) == 0
    assert out.cpu().numpy()[0, 2] == np.sort(track[:10].cpu().numpy())[4]
    for kw in (dict(quantile=1.5), dict(context=-1.0), dict(min_frequency=9000)):
        with pytest.raises(ValueError):
            S.snr(pcm, sr, {"onset": [0.1], "offset": [0.2]}, **kw)


# ---- the interface ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seg():
    from whisperseg_amd.model import WhisperSegmenter
    return WhisperSegmenter(MODEL_DIR, device="cuda", device_ids=[0], dtype="f32")


ROW_KEYS = ("onset", "offset", "cluster")
KW = dict(spec_time_step=TM.STS)


def same_columns(a, b):
    return all(np.array_equal(np.float32(a[c]), np.float32(b[c]), equal_nan=True) for c in S.COLUMNS)


def test_segment_with_snr_on_the_meerkat_recording(gpu_lib, seg):
    from whisperseg_amd.wavio import load_wav
    x, sr = load_wav(os.path.join(GOLDEN, "meerkat_5s.wav"))
    plain = seg.segment(x, sr, **KW)
    assert set(plain) == set(ROW_KEYS)
    pred = seg.segment(x, sr, snr=True, **KW)
    assert list(pred) == list(ROW_KEYS) + list(S.COLUMNS) and {k: pred[k] for k in ROW_KEYS} == plain
    mf = seg.default_segmentation_config.get("min_frequency", 0)
    want = S.snr(x, sr, plain, min_frequency=mf)
    assert all(isinstance(pred[c], list) and len(pred[c]) == len(plain["onset"]) for c in S.COLUMNS) and same_columns(pred, want)
    opts = {"quantile": 0.25, "context": 1.0, "max_frequency": 6000.0, "track": True}
    full = seg.segment(x, sr, snr=opts, **KW)
    want = S.snr(x, sr, plain, min_frequency=mf, **opts)
    assert list(full) == list(ROW_KEYS) + list(S.COLUMNS) + list(S.TRACK_KEYS) and same_columns(full, want)
    assert np.array_equal(full["frame_energy"], want["frame_energy"]) and len(full["frame_energy"]) == S.frame_count(len(x), get_n_fft_given_sr(sr))
    for bad in ("yes", {"hop": 3}, {"quantile": 2}, {"context": -1}):
        with pytest.raises(ValueError):
            seg.segment(x, sr, snr=bad)
        with pytest.raises(ValueError):
            seg.segment_batch([(x, sr)], snr=bad)


def s16(v):
    return np.clip(np.round(np.asarray(v, np.float64) * 32768), -32768, 32767).astype(np.int64)


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    """A recording of the fixture model's own signal family (the model finds rows in it) as a mono file and, with another
    recording as its second channel, as a two-channel file."""
    d = tmp_path_factory.mktemp("snr")
    a, b = s16(GI.tiny_recording(3, 2)), s16(0.5 * GI.tiny_recording(5, 2))
    a, b = a[:min(len(a), len(b))], b[:min(len(a), len(b))]
    mono, stereo = d / "tiny.wav", d / "two.wav"
    mono.write_bytes(WC.wav_bytes("s16", 1, TM.SR, WC.sample_bytes("s16", a)))
    stereo.write_bytes(WC.wav_bytes("s16", 2, TM.SR, WC.sample_bytes("s16", np.stack([a, b], axis=1).reshape(-1))))
    return str(mono), str(stereo)


def test_every_entry_point_and_each_channels_plane(gpu_lib, seg, wavs):
    from whisperseg_amd.wavio import load_wav
    mono, stereo = wavs
    x, sr = load_wav(mono)
    plain = seg.segment(x, sr, **KW)
    assert len(plain["onset"]) >= 3
    pred = seg.segment(x, sr, snr=True, **KW)
    assert {k: pred[k] for k in ROW_KEYS} == plain and same_columns(pred, S.snr(x, sr, plain))
    assert np.isfinite(np.float32(pred["snr_db"])).all() and max(pred["snr_db"]) > 3
    every = seg.segment(x, sr, measure=True, patches=8, pitch=True, snr=True, **KW)
    assert list(every) == list(ROW_KEYS) + list(M.COLUMNS) + list(P.COLUMNS) + list(S.COLUMNS) + ["patch"] and same_columns(every, pred)
    batch = seg.segment_batch([(x, sr), (x[::-1].copy(), sr)], snr=True, **KW)
    files = seg.segment_files([mono], snr=True, **KW)
    for other in (batch[0], files[0]):
        assert {k: other[k] for k in ROW_KEYS} == plain and same_columns(other, pred)
    planes = np.stack([x, 0.5 * x[::-1]]).astype(np.float32)
    per_channel = seg.segment_channels(planes, sr, snr=True, **KW)
    assert same_columns(per_channel[0], pred)
    rows1 = {k: per_channel[1][k] for k in ROW_KEYS}
    assert same_columns(per_channel[1], S.snr(planes[1], sr, rows1))
    # a two-channel file: each channel rated on its own plane
    both = seg.segment_files([stereo], channel_id="all", snr={"track": True}, **KW)[0]
    assert len(both) == 2
    from whisperseg_amd.wavio import load_audio
    planes, sr2 = load_audio(stereo, mono=False)
    for channel, got in enumerate(both):
        rows = {k: got[k] for k in ROW_KEYS}
        want = S.snr(planes[channel], sr2, rows, track=True)
        assert same_columns(got, want) and np.array_equal(got["frame_energy"], want["frame_energy"]), channel
    assert not np.array_equal(both[0]["frame_energy"], both[1]["frame_energy"])


def test_cli_snr(gpu_lib, seg, wavs, tmp_path, monkeypatch):
    from whisperseg_amd.wavio import load_wav
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import segment
    finally:
        sys.path.pop(0)
    monkeypatch.setenv("WHISPERSEG_AMD_DTYPE", "f32")
    mono, _ = wavs
    x, sr = load_wav(mono)
    base = ["--model_path", MODEL_DIR, "--audio_path", mono, "--spec_time_step", str(TM.STS)]
    plain_csv, full_csv, both_csv, archive = tmp_path / "plain.csv", tmp_path / "full.csv", tmp_path / "both.csv", tmp_path / "snr.npz"
    segment.main(base + ["--csv_save_path", str(plain_csv)])
    segment.main(base + ["--csv_save_path", str(full_csv), "--snr", "--snr_save_path", str(archive)])
    segment.main(base + ["--csv_save_path", str(both_csv), "--pitch", "--snr", "--snr_quantile", "0.3", "--snr_context", "0.5"])
    plain = seg.segment(x, sr, **KW)
    text = io.StringIO()
    segment.write_csv(["onset", "offset", "cluster"], list(zip(plain["onset"], plain["offset"], plain["cluster"])), text)
    assert plain_csv.read_text() == text.getvalue() and plain["onset"]          # byte for byte what the existing path writes
    full = seg.segment(x, sr, snr=True, **KW)
    text = io.StringIO()
    segment.write_csv(*segment.table([full], snr=True), text)
    lines = full_csv.read_text().splitlines()
    assert full_csv.read_text() == text.getvalue()
    assert lines[0] == "onset,offset,cluster," + ",".join(S.COLUMNS) and len(lines) == 1 + len(plain["onset"])
    assert [ln.split(",")[:3] for ln in lines] == [ln.split(",") for ln in plain_csv.read_text().splitlines()]
    lines = both_csv.read_text().splitlines()
    assert lines[0] == "onset,offset,cluster," + ",".join(P.COLUMNS + S.COLUMNS)
    other = seg.segment(x, sr, snr={"quantile": 0.3, "context": 0.5}, **KW)
    assert [ln.split(",")[-4:] for ln in lines[1:]] == [[repr(float(other[c][i])) for c in S.COLUMNS] for i in range(len(plain["onset"]))]
    saved = np.load(str(archive))
    assert set(saved.files) == {"frame_energy", "frame_offsets", "hop", "n_fft"}
    want = S.snr(x, sr, plain, track=True)
    assert np.array_equal(saved["frame_energy"], want["frame_energy"]) and saved["frame_offsets"].tolist() == [0, len(want["frame_energy"])]
    assert saved["hop"].tolist() == [want["hop"]] and saved["n_fft"].tolist() == [want["n_fft"]]
