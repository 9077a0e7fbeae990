#!/usr/bin/env python3
"""A/B of the audio ingest on one MI355X: host decode (wavio.load_wav, numpy, one thread) against the device decode
(wseg_pcm_to_mono_f32 / wseg_samples_to_mono_f32) and the folder pipeline on top of it (SegmenterBase.segment_files).

    python tools/ingest_bench.py [--files 64] [--seconds 60] [--out profiles/ingest_ab.txt]
    python tools/ingest_bench.py --planar [--out profiles/ingest_planar_ab.txt]
    python tools/ingest_bench.py --resample [--out profiles/resample_planar_ab.txt]
    python tools/ingest_bench.py --stream [--out profiles/resample_stream_ab.txt]
    python tools/ingest_bench.py --encodings [--out profiles/ingest_encodings_ab.txt]
    python tools/ingest_bench.py --adpcm [--out profiles/ingest_adpcm_ab.txt]

For each of three recorder formats — s16 mono 16 kHz, s16 stereo 48 kHz, s24 stereo 96 kHz — it writes `--files` files of
`--seconds` seconds into a temporary directory and reports
  * load_wav: frames/s of the host decode (file read from the page cache included, as the folder mode pays it),
  * the kernel alone: GB/s (bytes read + bytes written) from HIP events, warm, median of 20, on one file's samples and on the
    samples of the whole folder in one launch,
  * wall time of the folder through segment_batch((load_wav(p) for p in paths)) and through segment_files(paths): the same
    engine, the same results (checked), one process.
The engine is bench.py's: whisperseg-large geometry with seeded random weights in the default mode, spec_time_step 0.01 (10 s
windows), decode length capped at --max-length (random weights emit no meaningful EOS, so every window runs that long).

--planar measures the two decode kernels alone, no engine: wseg_pcm_to_planar_f32 with all channels beside wseg_pcm_to_mono_f32 on
the same bytes (random, generated on the device), for PLANAR_CASES x 60 s and 600 s of audio.  GB/s = (input bytes + output
bytes) over HIP-event time — the planar kernel writes `channels` times the mono kernel's output, so rates compare, times do not.
A repetition is a train of back-to-back launches (as many as move about 2 GB, at least one) between two events; one warm-up
train, then three repetitions of each kernel, alternating; all three rates are printed, the median is the figure.

--encodings measures the decode kernels alone on the encodings of wseg_sample_encoding that RIFF/WAVE PCM does not carry, each
beside its sibling of the same width (ENCODING_PAIRS: s16be | s16, s24be | s24, f64be | f64, u-law | u8), through
wseg_samples_to_mono_f32 with one and two channels and wseg_samples_to_planar_f32 with two, on the same random bytes (600 s at
48 kHz).  A repetition is a train of back-to-back launches that moves about 400 GB (a tenth of a second or more) between two HIP
events; one warm-up train of each encoding, then five repetitions, the two encodings alternating; all five rates are printed, the
median is the figure.  Bytes in and out are equal within a pair, so
the rates compare directly; a line says whether the new encoding's median lies inside the spread of its sibling's own repetitions.

--adpcm measures the IMA ADPCM decode alone (wseg_ima_adpcm_to_mono_f32, and wseg_ima_adpcm_to_planar_f32 with all channels for a
multi-channel case) beside wseg_samples_to_mono_f32 / wseg_samples_to_planar_f32 on the same number of frames as s16 — the file the
recorder would otherwise have written — for ADPCM_CASES x 600 s, on random bytes generated on the device.  A repetition is a train
of back-to-back launches that moves about 20 GB between two HIP events; one warm-up train of each, then five repetitions, the two
alternating; the figure is the median time per launch in ms and with it GB/s = (bytes in + bytes out) / time and M frames/s (all
five times are printed).  The host line is load_audio on a 60 s file of the same geometry, read from the page cache.

--resample measures the two resamplers alone, no engine, by the same protocol: wseg_resample_planar_f32 (one launch for all planes)
beside the loop it replaces (one wseg_resample_f32 launch per plane, back to back) on the same planes (seeded normal samples,
generated on the device) and the same taps, for RESAMPLE_CASES x 1, 2 and 8 planes of 600 s.  The figure is time per call in ms
(all planes), and with it M output samples/s, G fmaf/s and the GB/s of the planes read and written once.

--stream measures the file path at a target rate, no engine, through the public entry points only (so the same file runs at any
commit that has `sr=`): load_wav_device(path, sr=) and a pass over FilePipeline([path], sr=) as segment_files makes it, on ONE
s16 file per case that goes through in pieces of --piece-mb MiB (chunk_frames / buffer_bytes), for STREAM_CASES x mono and 8
channels kept apart.  Per call: HIP-event time (first enqueue to last kernel), wall time (file read from the page cache included,
ends in a synchronise) and the rise of torch.cuda.max_memory_allocated over the call.  One warm-up of each entry point, then five
repetitions, the two entry points alternating; all five are printed, the median is the figure."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = (("s16", 1, 16000), ("s16", 2, 48000), ("s24", 2, 96000))
PLANAR_CASES = CASES + (("s16", 8, 48000), ("s24", 5, 96000))


def write_folder(d, fmt, channels, sr, files, seconds):
    import wav_cases as WC
    rng = np.random.default_rng(1)
    n = seconds * sr
    t = np.arange(n) / sr
    blobs = []
    for k in range(4):                       # four distinct signals, cycled
        x = 0.3 * np.sin(2 * np.pi * (700 + 300 * k) * t) + 0.05 * rng.standard_normal(n)
        full = 1 << (WC.TAG_BITS[fmt][1] - 1)
        q = np.clip(np.round(x * full), -full, full - 1).astype(np.int64)
        inter = np.stack([q] + [q // (c + 2) for c in range(channels - 1)], axis=1).reshape(-1)
        blobs.append(WC.wav_bytes(fmt, channels, sr, WC.sample_bytes(fmt, inter)))
    paths = []
    for i in range(files):
        paths.append(os.path.join(d, "rec%03d.wav" % i))
        with open(paths[-1], "wb") as f:
            f.write(blobs[i % 4])
    return paths


def kernel_gbps(lib, raw_bytes, n_frames, channels, fmt_code):
    import torch
    from whisperseg_amd import _lib
    raw = torch.zeros(-(-len(raw_bytes) // 16) * 16, dtype=torch.uint8, device="cuda")
    raw[:len(raw_bytes)] = torch.from_numpy(np.frombuffer(raw_bytes, np.uint8).copy()).cuda()
    out = torch.empty(n_frames, dtype=torch.float32, device="cuda")
    call = lambda: _lib.check(lib.wseg_pcm_to_mono_f32(raw.data_ptr(), n_frames, channels, fmt_code, out.data_ptr(), _lib.stream_ptr()))
    for _ in range(3):
        call()
    ms = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    return (len(raw_bytes) + 4 * n_frames) / (med * 1e-3) / 1e9, med


def planar_section(lib, emit):
    import torch
    import wav_cases as WC
    from whisperseg_amd import _lib
    stream = lambda: _lib.stream_ptr()
    ratios = {}
    for fmt, channels, sr in PLANAR_CASES:
        code = WC.FORMATS.index(fmt)
        for seconds in (60, 600):
            n = seconds * sr
            nbytes = n * channels * WC.BYTES[code]
            raw = torch.randint(0, 256, (-(-nbytes // 16) * 16,), dtype=torch.uint8, device="cuda")
            planes = torch.empty((channels, n), dtype=torch.float32, device="cuda")
            mono = torch.empty(n, dtype=torch.float32, device="cuda")
            kernels = {
                "planar": (nbytes + 4 * n * channels, lambda: _lib.check(lib.wseg_pcm_to_planar_f32(
                    raw.data_ptr(), n, channels, code, 0, channels, planes.data_ptr(), n, stream()))),
                "mono": (nbytes + 4 * n, lambda: _lib.check(lib.wseg_pcm_to_mono_f32(raw.data_ptr(), n, channels, code, mono.data_ptr(), stream()))),
            }

            launches = {k: max(1, int(2e9 // moved)) for k, (moved, _) in kernels.items()}

            def train(name):
                moved, call = kernels[name]
                iters = launches[name]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    call()
                b.record()
                b.synchronize()
                return moved * iters / (a.elapsed_time(b) * 1e-3) / 1e9

            rates = {"planar": [], "mono": []}
            for name in kernels:
                train(name)
            for _ in range(3):
                for name in kernels:
                    rates[name].append(train(name))
            med = {k: statistics.median(v) for k, v in rates.items()}
            ratios[(fmt, channels, seconds)] = med["planar"] / med["mono"]
            for name in ("planar", "mono"):
                emit("%-3s x%d %6d Hz %4d s  %-6s %8.1f GB/s  (%s; %d launches per repetition, %.1f MB in + %.1f MB out per launch)"
                     % (fmt, channels, sr, seconds, name, med[name], " ".join("%.1f" % r for r in rates[name]), launches[name],
                        nbytes / 1e6, (kernels[name][0] - nbytes) / 1e6))
            spread = max(max(v) - min(v) for v in rates.values())
            emit("%-3s x%d %6d Hz %4d s  planar / mono GB/s = %.2f  (largest spread of three repetitions: %.1f GB/s)"
                 % (fmt, channels, sr, seconds, ratios[(fmt, channels, seconds)], spread))
            del raw, planes, mono
    return ratios


ENCODING_PAIRS = (("s16be", 7, "s16", 1, 2), ("s24be", 8, "s24", 2, 3), ("f64be", 11, "f64", 5, 8), ("ulaw", 12, "u8", 0, 1))


def encodings_section(lib, emit, seconds=600, sr=48000, reps=5):
    import torch
    from whisperseg_amd import _lib
    stream = lambda: _lib.stream_ptr()
    n = seconds * sr
    for new, new_code, old, old_code, width in ENCODING_PAIRS:
        for kernel, channels in (("mono", 1), ("mono", 2), ("planar", 2)):
            nbytes = n * channels * width
            raw = torch.randint(0, 256, (-(-nbytes // 16) * 16,), dtype=torch.uint8, device="cuda")
            out = torch.empty((channels if kernel == "planar" else 1, n), dtype=torch.float32, device="cuda")
            moved = nbytes + 4 * out.numel()
            iters = max(1, int(4e11 // moved))

            def call(code):
                if kernel == "mono":
                    _lib.check(lib.wseg_samples_to_mono_f32(raw.data_ptr(), n, channels, code, out.data_ptr(), stream()))
                else:
                    _lib.check(lib.wseg_samples_to_planar_f32(raw.data_ptr(), n, channels, code, 0, channels, out.data_ptr(), n, stream()))

            def train(code):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    call(code)
                b.record()
                b.synchronize()
                return moved * iters / (a.elapsed_time(b) * 1e-3) / 1e9

            codes = {new: new_code, old: old_code}
            rates = {new: [], old: []}
            for name in codes:
                train(codes[name])
            for _ in range(reps):
                for name in codes:
                    rates[name].append(train(codes[name]))
            med = {k: statistics.median(v) for k, v in rates.items()}
            for name in (new, old):
                emit("%-6s x%d %-6s %-6s %8.1f GB/s  (%s; %d launches per repetition, %.1f MB in + %.1f MB out per launch)"
                     % (kernel, channels, "%d Hz" % sr, name, med[name], " ".join("%.1f" % r for r in rates[name]), iters, nbytes / 1e6,
                        (moved - nbytes) / 1e6))
            inside = min(rates[old]) <= med[new] <= max(rates[old])
            emit("%-6s x%d %s / %s GB/s = %.3f  (%s median %s the spread of %s's repetitions, %.1f .. %.1f GB/s)"
                 % (kernel, channels, new, old, med[new] / med[old], new, "inside" if inside else "OUTSIDE", old, min(rates[old]), max(rates[old])))
            del raw, out


ADPCM_CASES = ((1, 16000, 256), (2, 48000, 2048), (8, 48000, 8192))       # (channels, rate, block bytes)


def adpcm_section(lib, emit, seconds=600, reps=5):
    import torch
    import ima_adpcm_cases as IC
    from whisperseg_amd import _lib
    from whisperseg_amd.wavio import load_audio
    stream = lambda: _lib.stream_ptr()
    for channels, sr, block_bytes in ADPCM_CASES:
        spb = IC.block_frames(channels, block_bytes)
        n = seconds * sr
        n_blocks = -(-n // spb)
        name = "x%d %d Hz, blocks of %d bytes (%d frames)" % (channels, sr, block_bytes, spb)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "rec.wav")
            host_frames = 60 * sr
            with open(path, "wb") as f:
                f.write(IC.make_wav(channels, block_bytes, -(-host_frames // spb), sr=sr))
            load_audio(path)
            t0 = time.perf_counter()
            frames = len(load_audio(path)[0])
            host_s = time.perf_counter() - t0
        emit("%-48s load_audio (host, a 60 s file)  %8.2f M frames/s  (%.2f s)" % (name, frames / host_s / 1e6, host_s))
        adpcm_bytes, s16_bytes = n_blocks * block_bytes, 2 * n * channels
        raw = {"adpcm": torch.randint(0, 256, (-(-adpcm_bytes // 16) * 16,), dtype=torch.uint8, device="cuda"),
               "s16": torch.randint(0, 256, (-(-s16_bytes // 16) * 16,), dtype=torch.uint8, device="cuda")}
        for kernel in ("mono",) + (("planar",) if channels > 1 else ()):
            out = torch.empty((channels if kernel == "planar" else 1, n), dtype=torch.float32, device="cuda")
            moved = {"adpcm": adpcm_bytes + 4 * out.numel(), "s16": s16_bytes + 4 * out.numel()}
            iters = {k: max(1, int(2e10 // v)) for k, v in moved.items()}

            def call(which):
                if which == "adpcm" and kernel == "mono":
                    _lib.check(lib.wseg_ima_adpcm_to_mono_f32(raw["adpcm"].data_ptr(), n_blocks, block_bytes, channels, n, out.data_ptr(), stream()))
                elif which == "adpcm":
                    _lib.check(lib.wseg_ima_adpcm_to_planar_f32(raw["adpcm"].data_ptr(), n_blocks, block_bytes, channels, n, 0, channels,
                                                                out.data_ptr(), n, stream()))
                elif kernel == "mono":
                    _lib.check(lib.wseg_samples_to_mono_f32(raw["s16"].data_ptr(), n, channels, 1, out.data_ptr(), stream()))
                else:
                    _lib.check(lib.wseg_samples_to_planar_f32(raw["s16"].data_ptr(), n, channels, 1, 0, channels, out.data_ptr(), n, stream()))

            def train(which):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters[which]):
                    call(which)
                b.record()
                b.synchronize()
                return a.elapsed_time(b) / iters[which]

            ms = {"adpcm": [], "s16": []}
            for which in ms:
                train(which)
            for _ in range(reps):
                for which in ms:
                    ms[which].append(train(which))
            med = {k: statistics.median(v) for k, v in ms.items()}
            for which in ("adpcm", "s16"):
                emit("%-48s %-6s %-5s %9.4f ms  %8.1f GB/s  %9.1f M frames/s  (%s; %d launches per repetition, %.1f MB in + %.1f MB out per launch)"
                     % (name, kernel, which, med[which], moved[which] / med[which] / 1e6, n / med[which] / 1e3,
                        " ".join("%.4f" % v for v in ms[which]), iters[which], (moved[which] - 4 * out.numel()) / 1e6, 4 * out.numel() / 1e6))
            emit("%-48s %-6s adpcm / s16 time = %.2f" % (name, kernel, med["adpcm"] / med["s16"]))
            del out
        del raw


RESAMPLE_CASES = ((44100, 16000), (48000, 16000), (96000, 16000), (16000, 44100), (250000, 44100))


def resample_section(lib, emit, seconds=600, plane_counts=(1, 2, 8)):
    import torch
    from whisperseg_amd import _lib
    from whisperseg_amd.resample import launch_plan, plan
    stream = lambda: _lib.stream_ptr()
    verdicts = {}
    for sr_in, sr_out in RESAMPLE_CASES:
        n_in = seconds * sr_in
        p = plan(n_in, sr_in, sr_out)
        n_out, n_taps, up, down = p["n_out"], len(p["taps"]), p["up"], p["down"]
        h = torch.from_numpy(p["taps"]).cuda()
        emit("%d -> %d Hz: up / down %d / %d, %d taps, plan %s" % (sr_in, sr_out, up, down, n_taps, launch_plan(n_in, sr_in, sr_out)))
        for planes in plane_counts:
            g = torch.Generator(device="cuda").manual_seed(planes)
            x = torch.randn((planes, n_in), dtype=torch.float32, device="cuda", generator=g)
            y = {name: torch.empty((planes, n_out), dtype=torch.float32, device="cuda") for name in ("planar", "loop")}

            def planar():
                _lib.check(lib.wseg_resample_planar_f32(x.data_ptr(), n_in, n_in, planes, h.data_ptr(), n_taps, up, down, p["pre_pad"],
                                                        p["pre_remove"], y["planar"].data_ptr(), n_out, n_out, stream()))

            def loop():
                for c in range(planes):
                    _lib.check(lib.wseg_resample_f32(x[c].data_ptr(), n_in, h.data_ptr(), n_taps, up, down, p["pre_pad"], p["pre_remove"],
                                                     y["loop"][c].data_ptr(), n_out, stream()))

            calls = {"planar": planar, "loop": loop}
            moved = 4 * planes * (n_in + n_out)
            iters = max(1, int(2e9 // moved))

            def train(name):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    calls[name]()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) / iters

            ms = {"planar": [], "loop": []}
            for name in calls:
                train(name)
            equal = bool(torch.equal(y["planar"].view(torch.int32), y["loop"].view(torch.int32)))
            for _ in range(3):
                for name in calls:
                    ms[name].append(train(name))
            med = {k: statistics.median(v) for k, v in ms.items()}
            fma = planes * n_out * (n_taps / up)
            for name in ("planar", "loop"):
                emit("%6d -> %6d Hz x%d %4d s  %-6s %9.3f ms  (%s; %d calls per repetition)  %8.1f M out/s  %7.1f G fmaf/s  %7.1f GB/s"
                     % (sr_in, sr_out, planes, seconds, name, med[name], " ".join("%.3f" % v for v in ms[name]), iters,
                        planes * n_out / med[name] / 1e3, fma / med[name] / 1e6, moved / med[name] / 1e6))
            spread = max(max(v) - min(v) for v in ms.values())
            ok = med["planar"] <= med["loop"] + spread
            verdicts[(sr_in, sr_out, planes)] = ok and equal
            emit("%6d -> %6d Hz x%d %4d s  loop / planar time = %.2f  (largest spread of three repetitions: %.3f ms; not slower: %s; bits equal: %s)"
                 % (sr_in, sr_out, planes, seconds, med["loop"] / med["planar"], spread, ok, equal))
            del x, y
    return verdicts


STREAM_CASES = ((250000, 44100, 120), (48000, 16000, 480))       # (native rate, target rate, seconds of audio)


def stream_section(lib, emit, piece_mb=4, channel_counts=(1, 8), reps=5):
    import torch
    import wav_cases as WC
    from whisperseg_amd import wavio
    ingest = wavio.device_ingest("cuda")
    piece_bytes = piece_mb << 20
    for sr_in, sr_out, seconds in STREAM_CASES:
        for channels in channel_counts:
            n = seconds * sr_in
            rng = np.random.default_rng(channels)
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "rec.wav")
                with open(path, "wb") as f:
                    f.write(WC.wav_bytes("s16", channels, sr_in, rng.integers(-32768, 32768, n * channels, dtype=np.int16).tobytes()))
                chunk_frames = piece_bytes // (2 * channels) // 16 * 16
                kw = dict(mono=False) if channels > 1 else {}

                def load():
                    return wavio.load_wav_device(path, sr=sr_out, chunk_frames=chunk_frames, **kw)[0]

                def pipeline():
                    items = list(wavio.FilePipeline([path], ingest, buffer_bytes=piece_bytes, sr=sr_out, **({"channel_id": "all"} if channels > 1 else {})))
                    return items[0][0]

                calls = {"load_wav_device": load, "FilePipeline": pipeline}

                def timed(name):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    out = calls[name]()
                    b.record()
                    b.synchronize()
                    wall = time.perf_counter() - t0
                    peak = torch.cuda.max_memory_allocated() - base
                    shape = tuple(out.shape)
                    del out
                    return a.elapsed_time(b), wall * 1e3, peak, shape

                for name in calls:
                    timed(name)
                runs = {name: [] for name in calls}
                for _ in range(reps):
                    for name in calls:
                        runs[name].append(timed(name))
                pieces = -(-n // chunk_frames)
                for name, r in runs.items():
                    ev, wall = [v[0] for v in r], [v[1] for v in r]
                    emit("%6d -> %6d Hz x%d %4d s (%d pieces of %d MiB, %.0f MB native planes, output %s)  %-15s events %8.2f ms (%s)  wall %8.2f ms (%s)  "
                         "peak rise %7.1f MiB"
                         % (sr_in, sr_out, channels, seconds, pieces, piece_mb, 4e-6 * n * channels, "x".join(map(str, r[0][3])), name,
                            statistics.median(ev), " ".join("%.2f" % v for v in ev), statistics.median(wall), " ".join("%.2f" % v for v in wall),
                            max(v[2] for v in r) / 2 ** 20))


def _tool_section(args, title, section):
    """A kernels-only mode: print the section's lines and keep them in --out."""
    import torch
    from whisperseg_amd import _lib
    lib = _lib.load(require_device=True)
    lines = [title + ", " + torch.cuda.get_device_name(0)]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    section(lib, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--max-length", type=int, default=32)
    ap.add_argument("--model", default="large")
    ap.add_argument("--dtype", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--planar", action="store_true", help="only the kernels: wseg_pcm_to_planar_f32 beside wseg_pcm_to_mono_f32")
    ap.add_argument("--resample", action="store_true",
                    help="only the kernels: wseg_resample_planar_f32 beside one wseg_resample_f32 launch per plane")
    ap.add_argument("--stream", action="store_true",
                    help="only the file path at a target rate: load_wav_device(sr=) and FilePipeline(sr=) on a file that goes through in pieces")
    ap.add_argument("--encodings", action="store_true",
                    help="only the kernels: every new sample encoding beside its sibling of the same width")
    ap.add_argument("--adpcm", action="store_true",
                    help="only the kernels: the IMA ADPCM decode beside the s16 decode of the same frames, and the host decode")
    ap.add_argument("--piece-mb", type=int, default=4, help="--stream: MiB per piece of the file")
    args = ap.parse_args(argv)
    if args.stream:
        return _tool_section(args, "file path at a target rate: load_wav_device(sr=) and a pass over FilePipeline(sr=) on one multi-piece s16 file, "
                                   "HIP events and wall time per call in ms, median of five repetitions after one warm-up, the two entry "
                                   "points alternating (all five in brackets); peak rise of torch.cuda.max_memory_allocated over a call",
                             lambda lib, emit: stream_section(lib, emit, piece_mb=args.piece_mb))
    if args.encodings:
        return _tool_section(args, "sample encodings A/B: wseg_samples_to_mono_f32 / wseg_samples_to_planar_f32 on a new encoding beside its "
                                   "sibling of the same width on the same bytes, HIP events, GB/s = (bytes in + bytes out) / time, median of "
                                   "five repetitions after one warm-up, the two alternating (all five in brackets)", encodings_section)
    if args.adpcm:
        return _tool_section(args, "IMA ADPCM decode A/B: wseg_ima_adpcm_to_mono_f32 / _planar_f32 beside wseg_samples_to_mono_f32 / _planar_f32 on the "
                                   "same frames as s16, 600 s of audio, HIP events, ms per launch, GB/s = (bytes in + bytes out) / time, median of "
                                   "five repetitions after one warm-up, the two alternating (all five in brackets); host: load_audio", adpcm_section)
    if args.resample:
        return _tool_section(args, "resample A/B: wseg_resample_planar_f32 (one launch, all planes) beside a loop of wseg_resample_f32 launches "
                                   "over the same planes and taps, HIP events, ms per call of all planes, median of three repetitions after one "
                                   "warm-up (all three in brackets)", resample_section)
    import torch
    from whisperseg_amd import _lib
    if args.planar:
        return _tool_section(args, "planar decode A/B: wseg_pcm_to_planar_f32 (all channels) beside wseg_pcm_to_mono_f32 on the same bytes, "
                                   "HIP events, GB/s = (bytes in + bytes out) / time, median of three repetitions after one warm-up (all "
                                   "three in brackets)", planar_section)
    import bench
    from whisperseg_amd.engine import Engine
    from whisperseg_amd.model import DEFAULT_DTYPE
    from whisperseg_amd.wavio import load_wav, read_wav_raw
    lib = _lib.load(require_device=True)
    args.dtype = args.dtype or DEFAULT_DTYPE
    seg = bench.make_segmenter(args, Engine.random(bench.hf_config(args.model), "cuda:0", args.dtype, seed=0))
    kw = dict(spec_time_step=0.01, max_length=args.max_length)
    lines = ["ingest A/B: %d files x %d s per format, whisperseg-%s %s (seeded random weights), spec_time_step 0.01, max_length %d, %s"
             % (args.files, args.seconds, args.model, args.dtype, args.max_length, torch.cuda.get_device_name(0))]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for fmt, channels, sr in CASES:
        with tempfile.TemporaryDirectory() as d:
            paths = write_folder(d, fmt, channels, sr, args.files, args.seconds)
            name = "%s x%d %d Hz" % (fmt, channels, sr)
            t0 = time.perf_counter()
            frames = sum(len(load_wav(p)[0]) for p in paths)
            host_s = time.perf_counter() - t0
            emit("%-18s load_wav (host)      %8.1f M frames/s  (%.2f s for the folder)" % (name, frames / host_s / 1e6, host_s))
            raw = read_wav_raw(paths[0])
            one = bytes(raw.data)
            for label, data, n in (("one file", one, raw.n_frames), ("folder, one launch", one * min(args.files, 16), raw.n_frames * min(args.files, 16))):
                gbps, ms = kernel_gbps(lib, data, n, raw.channels, raw.format)
                emit("%-18s kernel, %-18s %8.1f GB/s  %8.1f M frames/s  (%.3f ms, median of 20)" % (name, label, gbps, n / ms / 1e3, ms))
            seg.segment_files(paths[:4], **kw)                         # warm: workspace, pinned buffers, filterbanks
            seg.segment_batch((load_wav(p) for p in paths[:4]), **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a = seg.segment_batch((load_wav(p) for p in paths), **kw)
            torch.cuda.synchronize()
            t_host = time.perf_counter() - t0
            t0 = time.perf_counter()
            b = seg.segment_files(paths, **kw)
            torch.cuda.synchronize()
            t_dev = time.perf_counter() - t0
            emit("%-18s folder wall time     segment_batch(load_wav) %.2f s | segment_files %.2f s  (x%.2f; results equal: %s; %.0f audio-s)"
                 % (name, t_host, t_dev, t_host / t_dev, a == b, args.files * args.seconds))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
