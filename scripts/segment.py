#!/usr/bin/env python3
"""Command-line segmentation — counterpart of reference scripts/segment.py (same flags, same CSV).

    python scripts/segment.py --model_path DIR --audio_path a.wav --csv_save_path out.csv
    python scripts/segment.py --model_path DIR --audio_folder wavs/ --csv_save_path out.csv
    cat a.wav | python scripts/segment.py --model_path DIR --audio_path - --csv_save_path buffer
    python scripts/segment.py --model_path DIR --audio_folder wavs/ --channel_id all --csv_save_path out.csv
    python scripts/segment.py --model_path DIR --audio_folder wavs/ --sr 16000 --csv_save_path out.csv
    python scripts/segment.py --model_path DIR --audio_folder mixed/ --audio_ext wav aiff aifc au --csv_save_path out.csv

Recordings may be RIFF/WAVE (RF64 / BW64 and IMA ADPCM included), AIFF / AIFF-C or AU files (whisperseg_amd/wavio.py), whatever their names.

--channel_id (the `channel_id` of the reference's interactive entry points: segment_service.py:73-80, scripts/backend.py:279-282,
demo.py:76-78) segments one channel of multi-channel recordings instead of their mono mix — an integer: the same columns, rows
of that channel (a one-channel file gives its samples) — or `all`: every channel, with a `channel` column behind `filename`.
--sr N (`librosa.load(..., sr=N)` of the same entry points) resamples every recording to N Hz on the GPU before it is segmented,
whatever --channel_id says; absent, recordings keep their native rate, as in the reference's CLI.
--measure appends eight acoustic measurements of every row behind the existing columns (whisperseg_amd.measure.COLUMNS: level,
zero-crossing rate, peak / centroid / 5 % / 95 % frequency, spectral entropy), taken on the GPU from the samples the rows were cut from.
--patches W --patches_save_path FILE.npz (each needs the other) saves one time-normalised log-mel picture of W columns per row
(whisperseg_amd.patches, computed on the GPU from the same samples): `patch` float32 [rows, 80, W] in the CSV's row order, with `onset`,
`offset`, `cluster` and, where the CSV has those columns, `filename` / `channel`.  The CSV is what it is without the flags.
--neighbors K (needs --patches and --patches_save_path) adds the K nearest neighbours of every row among all rows of the archive,
found on the GPU (whisperseg_amd.neighbors): `neighbor_index` int32 [rows, K] — rows of the archive, which is the CSV's row order;
-1 where fewer than K other rows exist — and `neighbor_distance` float32 [rows, K], the squared Euclidean distance of the pictures.
--neighbors_metric dtw [--neighbors_band R] (needs --neighbors or --embed; --patches W up to 64) compares two pictures by banded
dynamic time warping over their columns instead (whisperseg_amd.dtw, on the GPU): a warping path may leave the diagonal by up to R
columns (0 .. W - 1, default max(1, W // 8); 0 is the Euclidean distance again).  The lists of --neighbors are then DTW lists and the
archive also holds `neighbor_metric` ("dtw") and `neighbor_band`; --embed builds its graph from DTW lists of --embed_neighbors rows.
--clusters stays Euclidean: the spanning tree computes its own distances.
--clusters MIN_SIZE [--cluster_min_samples S] (needs --patches and --patches_save_path) groups the rows of the archive into call
types by HDBSCAN over the pictures (whisperseg_amd.linkage; the mutual-reachability minimum spanning tree is built on the GPU):
`patch_cluster` int32 [rows] — clusters of at least MIN_SIZE rows numbered by their first row, -1: noise (the archive's `cluster`
stays the model's label) — with the tree itself, `mst_edges` int32 [rows - 1, 2] and `mst_weight` float32 [rows - 1] (squared
distances), for a cut at another level (linkage.cut).  S (1 .. 64, default 5; lowered to rows - 1) counts OTHER rows.
--embed DIM [--embed_neighbors K] [--embed_min_dist X] [--embed_seed S] (needs --patches and --patches_save_path) adds the map of
the rows of the archive: `embedding` float32 [rows, DIM], DIM 2 or 3 — the UMAP layout (whisperseg_amd.embed; its epochs run on the
GPU) of the fuzzy graph of the K (1 .. 64, default 15) nearest neighbours of every picture, with min_dist X (0 <= X < 1, default
0.1) and the hash seed S (default 0): the same bits for the same rows on every run.  With --neighbors K of the same K the lists
are computed once.
--embed_init pca (needs --embed) starts the layout from the first DIM principal-component scores of the pictures instead of the
hashed cloud (whisperseg_amd.embed.pca_start): the global arrangement of the call types then comes from the data; absent or `hash`,
the archive is what it is without the flag.
--pca R (needs --patches and --patches_save_path) adds the first R (1 .. 64, at most 80 W and rows - 1) principal components of the
pictures (whisperseg_amd.pca; the second moments and the scores are computed on the GPU in float64): `pca_mean` float64 [80 W],
`pca_components` float64 [R, 80 W], `pca_variance` and `pca_variance_ratio` float64 [R], `pca_scores` float32 [rows, R] in the
archive's row order; with no row or a single one the arrays are empty ([0], [0, 80 W], [0], [0], [0, R]) and nothing runs.
--onto LIBRARY.npz [--embed_neighbors K] [--embed_min_dist X] [--embed_seed S] [--cluster_min_samples S] (needs --patches W and
--patches_save_path, W the library's; excludes --clusters, --embed and --pca) reads an archive an earlier run wrote as a LIBRARY
and expresses this run's rows in it (whisperseg_amd.library.patch_onto; nothing of the library moves, and a row's values do not
depend on the other rows of the run): `library_index` int32 [rows, K] and `library_distance` float32 [rows, K], the K (default 15)
nearest library rows of every row; `patch_cluster` int32 [rows], the library's call type or -1, if the library was made with
--clusters; `embedding` float32 [rows, DIM], the row on the library's map, if it was made with --embed; `pca_scores` float32
[rows, R] on the library's axes, if it was made with --pca.  X, the seed S and the min_samples S mean what they meant when the
library was made: give the values it was made with.
--pitch [--pitch_min_hz F] [--pitch_max_hz F] [--pitch_threshold X] appends seven pitch columns behind the measurement columns
(whisperseg_amd.pitch.COLUMNS: mean, lowest, highest, first and last fundamental frequency of the row's YIN contour in Hz, the voiced
fraction and the aperiodicity), tracked on the GPU in the samples the rows were cut from; F default to the widest range the
estimator takes at the recording's rate (2 sr / n_fft .. sr / 8), X (0 < X < 1, default 0.1) is YIN's threshold.
--pitch_save_path FILE.npz (needs --pitch) saves the contours themselves: `f0` (Hz, NaN where unvoiced), `aperiodicity` and
`frame_time` (seconds), all float [frames], the frames of row 0, then of row 1, ... in the CSV's row order, `frame_offsets` int64
[rows + 1] — row r owns the frames frame_offsets[r] .. frame_offsets[r + 1] — and `onset`, `offset`, `cluster`, `filename` / `channel`
as --patches_save_path has them.
--snr [--snr_quantile Q] [--snr_context SECONDS] appends four signal-to-noise columns behind the pitch columns
(whisperseg_amd.snr.COLUMNS: the row's level and the recording's noise floor in dB re a full-scale sine inside the band, their ratio
and the ratio of the row's loudest frame to the floor), rated on the GPU in the samples the rows were cut from: the floor is the
Q-quantile (0 <= Q <= 1, default 0.1) of the band energy of every frame of the recording or, with --snr_context, of the frames up
to SECONDS around the row.
--snr_save_path FILE.npz (needs --snr) saves the band-energy tracks themselves: `frame_energy` float32 [frames], the frames of
recording 0, then of recording 1, ... (a recording is a file, or with --channel_id all a channel of a file, in the CSV's order),
`frame_offsets` int64 [recordings + 1], `hop` and `n_fft` int64 [recordings] in samples of the rate the recording was segmented at.
--audio_ext EXT [EXT ...] names the extensions folder mode looks for: for each one in order `*.ext`, then `*.EXT`; absent, `*.wav`
then `*.WAV`, as in the reference's CLI.
"""
import argparse
import csv
import glob
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from model import WhisperSegmenter, WhisperSegmenterFast  # noqa: E402  (root-level shim, as upstream imports it)
from whisperseg_amd import dtw as DW, embed as EM, library as LB, linkage as LK, neighbors as NB, pca as PC, resident as RS  # noqa: E402
from whisperseg_amd.measure import COLUMNS as MEASURE_COLUMNS  # noqa: E402
from whisperseg_amd.pitch import COLUMNS as PITCH_COLUMNS  # noqa: E402
from whisperseg_amd.snr import COLUMNS as SNR_COLUMNS  # noqa: E402
from whisperseg_amd.wavio import load_audio, load_wav_device  # noqa: E402


def channel_id_arg(text):
    return "all" if text == "all" else int(text)


def sr_arg(text):
    value = int(text)
    if value <= 0:
        raise argparse.ArgumentTypeError("--sr must be a positive integer")
    return value


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--model_path")
    p.add_argument("--audio_path", default=None, help="one audio file, or '-' to read one from stdin")
    p.add_argument("--audio_folder", default=None, help="directory of .wav/.WAV files, or of --audio_ext's (when --audio_path is absent)")
    p.add_argument("--csv_save_path")
    p.add_argument("--device", default="cuda", help="'cuda' (an MI355X is required; 'cpu' raises)")
    p.add_argument("--device_ids", type=int, nargs="+", default=[0, ], help="GPU indices, one model replica each")
    p.add_argument("--batch_size", default=8, type=int)
    p.add_argument("--min_frequency", default=None, type=int)
    p.add_argument("--spec_time_step", default=None, type=float)
    p.add_argument("--num_trials", default=1, type=int)
    p.add_argument("--channel_id", default=None, type=channel_id_arg,
                   help="segment this channel of multi-channel recordings (an integer, negative from the end), or 'all' of them; "
                        "absent: the mono mix")
    p.add_argument("--sr", default=None, type=sr_arg,
                   help="resample every recording to this rate (Hz) on the GPU before segmenting; absent: the native rate")
    p.add_argument("--audio_ext", default=None, nargs="+", metavar="EXT",
                   help="folder mode: the file extensions to look for, each as *.ext then *.EXT, in this order; absent: wav")
    p.add_argument("--measure", action="store_true",
                   help="append the eight per-segment measurements (peak_amplitude .. spectral_entropy) to every row")
    p.add_argument("--patches", default=None, type=int, metavar="W",
                   help="save one log-mel picture of W columns (1 .. 256) per row to --patches_save_path")
    p.add_argument("--patches_save_path", default=None, metavar="FILE.npz", help="where --patches W saves the pictures (numpy .npz)")
    p.add_argument("--neighbors", default=None, type=int, metavar="K",
                   help="add the K (1 .. 64) nearest neighbours of every row among the saved pictures to --patches_save_path")
    p.add_argument("--neighbors_metric", default=None, choices=("euclidean", "dtw"),
                   help="--neighbors / --embed: the distance of two pictures — euclidean (default), or dtw: banded dynamic time warping over "
                        "their columns (--patches up to 64)")
    p.add_argument("--neighbors_band", default=None, type=int, metavar="R",
                   help="--neighbors_metric dtw: columns a warping path may leave the diagonal by (0 .. W - 1, default max(1, W // 8))")
    p.add_argument("--clusters", default=None, type=int, metavar="MIN_SIZE",
                   help="add HDBSCAN clusters of at least MIN_SIZE (>= 2) rows over the saved pictures, and their spanning tree, to --patches_save_path")
    p.add_argument("--cluster_min_samples", default=None, type=int, metavar="S",
                   help="--clusters: the core distance of a row is the distance to its S-th nearest other row (1 .. 64, default 5)")
    p.add_argument("--embed", default=None, type=int, metavar="DIM",
                   help="add the 2-D or 3-D UMAP layout of the saved pictures (`embedding` [rows, DIM]) to --patches_save_path")
    p.add_argument("--embed_neighbors", default=None, type=int, metavar="K", help="--embed: neighbours a row of the graph (1 .. 64, default 15)")
    p.add_argument("--embed_min_dist", default=None, type=float, metavar="X", help="--embed: UMAP's min_dist, 0 <= X < 1 (default 0.1)")
    p.add_argument("--embed_seed", default=None, type=int, metavar="S", help="--embed: the seed of the start and the negative samples (default 0)")
    p.add_argument("--embed_init", default=None, choices=("hash", "pca"),
                   help="--embed: the start of the layout — hash (default): the hashed cloud; pca: the first DIM principal-component scores")
    p.add_argument("--pca", default=None, type=int, metavar="R",
                   help="add the first R (1 .. 64) principal components of the saved pictures and their scores to --patches_save_path")
    p.add_argument("--onto", default=None, metavar="LIBRARY.npz",
                   help="express the saved pictures in an earlier archive's call types, map and principal axes (adds library_index, "
                        "library_distance and, for what the library holds, patch_cluster, embedding, pca_scores to --patches_save_path)")
    p.add_argument("--pitch", action="store_true",
                   help="append the seven per-segment pitch columns (f0_mean .. aperiodicity) to every row")
    p.add_argument("--pitch_min_hz", default=None, type=float, metavar="F", help="--pitch: the lowest fundamental looked for (default 2 sr / n_fft)")
    p.add_argument("--pitch_max_hz", default=None, type=float, metavar="F", help="--pitch: the highest fundamental looked for (default sr / 8)")
    p.add_argument("--pitch_threshold", default=None, type=float, metavar="X", help="--pitch: YIN's threshold, 0 < X < 1 (default 0.1)")
    p.add_argument("--pitch_save_path", default=None, metavar="FILE.npz", help="--pitch: where to save the pitch contours (numpy .npz)")
    p.add_argument("--snr", action="store_true",
                   help="append the four per-segment signal-to-noise columns (signal_level_db .. peak_snr_db) to every row")
    p.add_argument("--snr_quantile", default=None, type=float, metavar="Q", help="--snr: the noise floor is this quantile of the frame energies, 0 <= Q <= 1 (default 0.1)")
    p.add_argument("--snr_context", default=None, type=float, metavar="SECONDS",
                   help="--snr: take the floor from the frames up to SECONDS around a row (default: from the whole recording)")
    p.add_argument("--snr_save_path", default=None, metavar="FILE.npz", help="--snr: where to save the band-energy tracks (numpy .npz)")
    return p


def parse_args(argv=None):
    """The parsed arguments; --patches and --patches_save_path without each other, a width outside 1 .. 256, --neighbors or --clusters
    without them, a K outside 1 .. 64, --neighbors_metric without --neighbors or --embed, --neighbors_band without the metric dtw or
    outside 0 .. W - 1, the metric dtw with more than 64 columns, a MIN_SIZE below 2, an S outside 1 .. 64 or --cluster_min_samples without --clusters are argparse
    errors; so are --embed without the patches, a DIM other than 2 or 3, --embed_neighbors outside 1 .. 64, --embed_min_dist outside
    [0, 1), a negative --embed_seed and any of the three, or --embed_init, without --embed; --pca without the patches or with an R outside
    1 .. min(64, 80 W); and --pitch_min_hz, --pitch_max_hz, --pitch_threshold or
    --pitch_save_path without --pitch, a frequency that is not positive, a range that is none, a threshold outside (0, 1) and a
    --pitch_save_path that does not end with .npz.  --onto without the patches, with --clusters, --embed or --pca, or with a
    LIBRARY that does not end with .npz is one too; with --onto, --embed_neighbors, --embed_min_dist, --embed_seed and
    --cluster_min_samples need no --embed / --clusters.  --snr_quantile, --snr_context or --snr_save_path without --snr, a Q outside
    [0, 1], a negative or non-finite context and a --snr_save_path that does not end with .npz are errors as well."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.onto is not None:
        if args.patches is None:
            parser.error("--onto LIBRARY.npz needs --patches W and --patches_save_path FILE.npz")
        for name in ("clusters", "embed", "pca"):
            if getattr(args, name) is not None:
                parser.error(f"--onto LIBRARY.npz excludes --{name}: the library's own are used")
        if not args.onto.endswith(".npz"):
            parser.error("--onto must name a .npz archive")
    if (args.patches is None) != (args.patches_save_path is None):
        parser.error("--patches W and --patches_save_path FILE.npz need each other")
    if args.patches is not None and not 1 <= args.patches <= 256:
        parser.error("--patches must be 1 .. 256 columns")
    if args.patches_save_path is not None and not args.patches_save_path.endswith(".npz"):
        parser.error("--patches_save_path must end with .npz")
    if args.neighbors is not None and args.patches is None:
        parser.error("--neighbors K needs --patches W and --patches_save_path FILE.npz")
    if args.neighbors is not None and not 1 <= args.neighbors <= 64:
        parser.error("--neighbors must be 1 .. 64")
    if args.neighbors_metric is not None and args.neighbors is None and args.embed is None:
        parser.error("--neighbors_metric needs --neighbors K or --embed DIM")
    if args.neighbors_metric is None:
        args.neighbors_metric = "euclidean"
    if args.neighbors_band is not None and args.neighbors_metric != "dtw":
        parser.error("--neighbors_band R needs --neighbors_metric dtw")
    if args.neighbors_metric == "dtw" and args.patches is not None and args.patches > 64:
        parser.error("--neighbors_metric dtw takes --patches of up to 64 columns")
    if args.neighbors_band is not None and args.patches is not None and not 0 <= args.neighbors_band <= args.patches - 1:
        parser.error("--neighbors_band must be 0 .. W - 1 columns")
    if args.clusters is not None and args.patches is None:
        parser.error("--clusters MIN_SIZE needs --patches W and --patches_save_path FILE.npz")
    if args.clusters is not None and args.clusters < 2:
        parser.error("--clusters must be at least 2 rows")
    if args.cluster_min_samples is not None and args.clusters is None and args.onto is None:
        parser.error("--cluster_min_samples S needs --clusters MIN_SIZE")
    if args.cluster_min_samples is None:
        args.cluster_min_samples = 5
    elif not 1 <= args.cluster_min_samples <= 64:
        parser.error("--cluster_min_samples must be 1 .. 64")
    if args.embed is not None and args.patches is None:
        parser.error("--embed DIM needs --patches W and --patches_save_path FILE.npz")
    if args.embed is not None and args.embed not in (2, 3):
        parser.error("--embed must be 2 or 3 dimensions")
    for name in ("embed_neighbors", "embed_min_dist", "embed_seed", "embed_init"):
        if getattr(args, name) is not None and args.embed is None and (args.onto is None or name == "embed_init"):
            parser.error(f"--{name} needs --embed DIM")
    if args.embed_neighbors is None:
        args.embed_neighbors = 15
    elif not 1 <= args.embed_neighbors <= 64:
        parser.error("--embed_neighbors must be 1 .. 64")
    if args.embed_min_dist is None:
        args.embed_min_dist = 0.1
    elif not 0 <= args.embed_min_dist < 1:
        parser.error("--embed_min_dist must lie in [0, 1)")
    if args.embed_seed is None:
        args.embed_seed = 0
    elif not 0 <= args.embed_seed < 2 ** 64:
        parser.error("--embed_seed must be 0 .. 2^64 - 1")
    if args.pca is not None and args.patches is None:
        parser.error("--pca R needs --patches W and --patches_save_path FILE.npz")
    if args.pca is not None and not 1 <= args.pca <= min(64, 80 * args.patches):
        parser.error("--pca must be 1 .. 64 components, and at most the 80 W columns of a picture")
    for name in ("pitch_min_hz", "pitch_max_hz", "pitch_threshold", "pitch_save_path"):
        if getattr(args, name) is not None and not args.pitch:
            parser.error(f"--{name} needs --pitch")
    for name in ("pitch_min_hz", "pitch_max_hz"):
        if getattr(args, name) is not None and not 0 < getattr(args, name) < float("inf"):
            parser.error(f"--{name} must be a positive frequency in Hz")
    if args.pitch_min_hz is not None and args.pitch_max_hz is not None and args.pitch_min_hz > args.pitch_max_hz:
        parser.error("--pitch_min_hz must not lie above --pitch_max_hz")
    if args.pitch_threshold is not None and not 0 < args.pitch_threshold < 1:
        parser.error("--pitch_threshold must lie in (0, 1)")
    if args.pitch_save_path is not None and not args.pitch_save_path.endswith(".npz"):
        parser.error("--pitch_save_path must end with .npz")
    for name in ("snr_quantile", "snr_context", "snr_save_path"):
        if getattr(args, name) is not None and not args.snr:
            parser.error(f"--{name} needs --snr")
    if args.snr_quantile is not None and not 0 <= args.snr_quantile <= 1:
        parser.error("--snr_quantile must lie in [0, 1]")
    if args.snr_context is not None and not 0 <= args.snr_context < float("inf"):
        parser.error("--snr_context must be a non-negative number of seconds")
    if args.snr_save_path is not None and not args.snr_save_path.endswith(".npz"):
        parser.error("--snr_save_path must end with .npz")
    return args


def pitch_keyword(args):
    """The `pitch=` of the segmenter calls for the parsed flags (None without --pitch): True, or the dict of what was given."""
    if not args.pitch:
        return None
    given = {key: value for key, value in (("f_min", args.pitch_min_hz), ("f_max", args.pitch_max_hz), ("threshold", args.pitch_threshold))
             if value is not None}
    if args.pitch_save_path is not None:
        given["contour"] = True
    return given or True


def snr_keyword(args):
    """The `snr=` of the segmenter calls for the parsed flags (None without --snr): True, or the dict of what was given."""
    if not args.snr:
        return None
    given = {key: value for key, value in (("quantile", args.snr_quantile), ("context", args.snr_context)) if value is not None}
    if args.snr_save_path is not None:
        given["track"] = True
    return given or True


def folder_patterns(audio_ext=None):
    """The glob patterns of folder mode, in the order their files are segmented."""
    if audio_ext is None:
        return ["*.wav", "*.WAV"]
    return [pattern for ext in audio_ext for pattern in ("*." + ext.lstrip(".").lower(), "*." + ext.lstrip(".").upper())]


def write_csv(columns, rows, dest):
    """Same text pandas' DataFrame.to_csv(index=False) produces for these columns (repr-shortest floats)."""
    w = csv.writer(dest, lineterminator="\n")
    w.writerow(columns)
    for row in rows:
        w.writerow([repr(v) if isinstance(v, float) else v for v in row])


def table(results, names=None, all_channels=False, measure=False, pitch=False, snr=False):
    """-> (columns, rows) of the CSV.  `results`: one prediction dict per recording, or with all_channels one LIST of dicts (one
    per channel) per recording, which adds the `channel` column; `names`: the recordings' file names for the `filename` column
    (folder mode); `measure`: the dicts carry the eight measurement columns, appended behind `cluster`; `pitch`: the seven pitch
    columns, behind those; `snr`: the four signal-to-noise columns, behind those.  Rows run in file, channel, row order."""
    columns = (["filename"] if names is not None else []) + (["channel"] if all_channels else []) + ["onset", "offset", "cluster"]
    extra = (list(MEASURE_COLUMNS) if measure else []) + (list(PITCH_COLUMNS) if pitch else []) + (list(SNR_COLUMNS) if snr else [])
    columns += extra
    rows = []
    for i, res in enumerate(results):
        for channel, r in enumerate(res if all_channels else [res]):
            head = ((names[i],) if names is not None else ()) + ((channel,) if all_channels else ())
            rows += [head + row for row in zip(r["onset"], r["offset"], r["cluster"], *(r[name] for name in extra))]
    return columns, rows


def identifying_columns(results, names=None, all_channels=False):
    """-> {name: array} of the columns that say which row of the CSV a row of an archive is: `onset`, `offset`, `cluster` and, where
    the CSV has them, `filename` / `channel`, in table()'s row order."""
    flat = [(i, channel, r) for i, res in enumerate(results) for channel, r in enumerate(res if all_channels else [res])]
    out = {"onset": np.array([v for _, _, r in flat for v in r["onset"]], dtype=np.float64),
           "offset": np.array([v for _, _, r in flat for v in r["offset"]], dtype=np.float64),
           "cluster": np.array([str(v) for _, _, r in flat for v in r["cluster"]], dtype=str)}
    if names is not None:
        out["filename"] = np.array([names[i] for i, _, r in flat for _ in r["onset"]], dtype=str)
    if all_channels:
        out["channel"] = np.array([channel for _, channel, r in flat for _ in r["onset"]], dtype=np.int64)
    return out


def patch_archive(results, names=None, all_channels=False, width=0):
    """-> {name: array} of the .npz: `patch` [rows, 80, W] (neighbors.patch_pictures_of: the one statement of the row order) and the
    CSV's identifying columns, in table()'s row order."""
    return {"patch": NB.patch_pictures_of(results, none=(80, width)), **identifying_columns(results, names, all_channels)}


def pitch_archive(results, names=None, all_channels=False):
    """-> {name: array} of the pitch .npz: the contours of all rows back to back, their offsets and the CSV's identifying columns,
    in table()'s row order."""
    flat = [r for res in results for r in (res if all_channels else [res])]

    def joined(key, dtype):
        return np.concatenate([np.asarray(a, dtype=dtype) for r in flat for a in r[key]] or [np.zeros(0, dtype)])

    counts = [len(a) for r in flat for a in r["f0_contour"]]
    return {"f0": joined("f0_contour", np.float32), "aperiodicity": joined("aperiodicity_contour", np.float32),
            "frame_time": joined("frame_time", np.float64),
            "frame_offsets": np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64),
            **identifying_columns(results, names, all_channels)}


def snr_archive(results, all_channels=False):
    """-> {name: array} of the signal-to-noise .npz: the tracks of all recordings back to back, their offsets, hops and transform sizes,
    in table()'s recording order."""
    flat = [r for res in results for r in (res if all_channels else [res])]
    tracks = [np.asarray(r["frame_energy"], dtype=np.float32) for r in flat]
    return {"frame_energy": np.concatenate(tracks or [np.zeros(0, np.float32)]),
            "frame_offsets": np.concatenate([[0], np.cumsum([len(t) for t in tracks], dtype=np.int64)]).astype(np.int64),
            "hop": np.array([r["hop"] for r in flat], dtype=np.int64), "n_fft": np.array([r["n_fft"] for r in flat], dtype=np.int64)}


def analyses(patch, args, device="cuda"):
    """-> {name: array} of what --neighbors, --clusters, --embed and --pca add to the archive, in that order, for the archive's
    pictures `patch` [rows, 80, W].  The pictures go to the device once and every analysis that was asked for searches that one
    tensor where it lies; with --neighbors K of the map's K the lists are computed once."""
    out = {}
    if args.neighbors is None and args.clusters is None and args.embed is None and args.pca is None:
        return out
    pictures = RS.resident(patch, device)
    dtw = args.neighbors_metric == "dtw"

    def lists_of(k):
        return DW.patch_dtw_neighbors(pictures, k, args.neighbors_band) if dtw else NB.patch_neighbors(pictures, k)

    lists = None
    if args.neighbors is not None:
        lists = lists_of(args.neighbors)
        out.update(lists)
        if dtw:                                              # (absent: the archive as it was)
            out.update(neighbor_metric=np.array("dtw"), neighbor_band=np.array(DW.check_band(args.neighbors_band, args.patches), dtype=np.int64))
    if args.clusters is not None:
        found = LK.patch_clusters(pictures, args.clusters, args.cluster_min_samples)
        out.update(patch_cluster=found["cluster"], mst_edges=found["mst_edges"], mst_weight=found["mst_weight"])
    if args.embed is not None:
        if args.neighbors != args.embed_neighbors:           # (the same K: the lists are computed once)
            lists = lists_of(args.embed_neighbors) if dtw else None      # the graph of the map is the warping distance's; else embed's own
        out.update(EM.patch_embedding(pictures, args.embed_neighbors, args.embed, args.embed_min_dist, seed=args.embed_seed,
                                      lists=None if lists is None else (lists["neighbor_index"], lists["neighbor_distance"]),
                                      **({"init": "pca"} if args.embed_init == "pca" else {})))       # (absent or hash: the call as it was)
    if args.pca is not None:
        out.update(PC.patch_pca(pictures, args.pca))         # more components than rows - 1: pca's ValueError says so
    return out


def stdin_wav(sr=None, channel_id=None):
    """The audio file on stdin, decoded on the host -> (audio, rate): the mono mix, or with `channel_id` the channels kept apart and the
    reference's selection (`audio[channel_id]` of a 2-D array; "all" keeps them).  `sr`: resampled to it on the GPU, 1-D or planes."""
    audio, native = load_audio(io.BytesIO(sys.stdin.buffer.read()), mono=channel_id is None)
    if audio.ndim == 2 and channel_id != "all":
        audio = audio[channel_id]
    if sr is None or sr == native or not audio.shape[-1]:
        return audio, (native if sr is None else sr)
    from whisperseg_amd.resample import resample
    return resample(audio, native, sr), sr


def main(argv=None):
    args = parse_args(argv)
    assert args.csv_save_path.endswith(".csv") or args.csv_save_path == "buffer", \
        "csv_save_path must ends with .csv or be 'buffer'"
    library = None
    if args.onto is not None:                                # read before the model is: a wrong library costs nothing
        library = LB.patch_library(args.onto)
        if library["patch"].shape[2] != args.patches:
            build_parser().error(f"--patches must be the library's {library['patch'].shape[2]} columns (got {args.patches})")
    try:
        segmenter = WhisperSegmenterFast(args.model_path, device=args.device, device_ids=args.device_ids)
    except Exception:
        segmenter = WhisperSegmenter(args.model_path, device=args.device, device_ids=args.device_ids)
    kwargs = dict(min_frequency=args.min_frequency, spec_time_step=args.spec_time_step, num_trials=args.num_trials,
                  batch_size=args.batch_size, **({"measure": True} if args.measure else {}),      # (absent: the calls as they were)
                  **({} if args.patches is None else {"patches": args.patches}),
                  **({} if not args.pitch else {"pitch": pitch_keyword(args)}),
                  **({} if not args.snr else {"snr": snr_keyword(args)}))
    rate = {} if args.sr is None else {"sr": args.sr}        # (absent: the calls as they were)
    if args.audio_path is None:
        assert args.audio_folder is not None, "Either audio_path or audio_folder needs to be specified!"
        paths = [p for pattern in folder_patterns(args.audio_ext) for p in glob.glob(args.audio_folder + "/" + pattern)]
        # same rows as the reference's serial loop, but the windows of many files share the engine's decode slots; files
        # are read by a second thread while the GPU works and their samples are decoded on the device, group by group, so
        # a large folder needs no more memory than a small one
        results = segmenter.segment_files(paths, **({} if args.channel_id is None else {"channel_id": args.channel_id}), **rate, **kwargs)
        tabled = (results, [os.path.basename(p) for p in paths], args.channel_id == "all")
    elif args.channel_id is None:
        audio, sr = stdin_wav(args.sr) if args.audio_path == "-" else load_wav_device(args.audio_path, **rate)
        tabled = ([segmenter.segment(audio, sr, **kwargs)], None, False)
    else:
        if args.audio_path == "-":       # the channels kept apart on the host, and the reference's selection (`audio[channel_id]` of a 2-D array)
            audio, sr = stdin_wav(args.sr, args.channel_id)
        elif args.channel_id == "all":
            audio, sr = load_wav_device(args.audio_path, mono=False, **rate)
        else:
            audio, sr = load_wav_device(args.audio_path, channel_id=args.channel_id, **rate)
        if args.channel_id == "all":
            tabled = ([segmenter.segment_channels(audio, sr, **kwargs)], None, True)
        else:
            tabled = ([segmenter.segment(audio, sr, **kwargs)], None, False)
    columns, rows = table(*tabled, measure=args.measure, pitch=args.pitch, **({"snr": True} if args.snr else {}))
    if args.snr_save_path is not None:
        np.savez(args.snr_save_path, **snr_archive(tabled[0], tabled[2]))
    if args.pitch_save_path is not None:
        np.savez(args.pitch_save_path, **pitch_archive(*tabled))
    if args.patches is not None:
        archive = patch_archive(*tabled, width=args.patches)
        archive.update(analyses(archive["patch"], args))
        if library is not None:
            archive.update(LB.patch_onto(archive["patch"], library, args.embed_neighbors, args.embed_min_dist, args.embed_seed,
                                         args.cluster_min_samples))
        np.savez(args.patches_save_path, **archive)
    if args.csv_save_path == "buffer":
        buf = io.StringIO()
        write_csv(columns, rows, buf)
        print(buf.getvalue())
    else:
        with open(args.csv_save_path, "w", newline="") as f:
            write_csv(columns, rows, f)


if __name__ == "__main__":
    main()
