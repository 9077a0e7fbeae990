"""Signals, lag ranges and segment lists shared by tests/test_pitch_cpu.py and tests/test_pitch_gpu.py (whisperseg_amd/pitch.py).

Everything is made from fixed seeds.  A CASE is one call of the kernel: a recording, int64 sample ranges, the lags, the hop and
the threshold.  The device test compares every case bit for bit with the host definition; the host test holds the definition
against its plain restatement on the cases with tau_max <= 65 and checks that the cases contain what they claim to."""
import collections
import functools

import numpy as np

from whisperseg_amd import pitch as P

SEED = 20251020
Case = collections.namedtuple("Case", "name x bounds tau_min tau_max hop threshold")

# (tau_min, tau_max): one candidate | one prefix block exactly | one lag past the block edge | five blocks, tau_max % 4 == 1 | the
# largest range (two frames only: 4 10^6 terms a frame on the host too)
LAGS = ((2, 3), (2, 64), (8, 65), (8, 257), (8, 2048))
HOPS = {3: 2, 64: 24, 65: 17, 257: 100, 2048: 1024}
SIGNALS = ("silence", "dc", "int16_noise", "float_noise", "tone", "stack", "missing_fundamental", "chirp", "edge_dip", "descent")


def signal(name, tau_max, n, seed=SEED):
    """float32 [n] of one signal family, its periods scaled to the lag range."""
    rng = np.random.default_rng(seed + 131 * tau_max + SIGNALS.index(name))
    t = np.arange(n, dtype=np.float64)
    if name == "silence":
        x = np.zeros(n)
    elif name == "dc":
        x = np.full(n, 0.25)
    elif name == "int16_noise":
        return (rng.integers(-3000, 3001, n).astype(np.float32) / np.float32(32768)).astype(np.float32)
    elif name == "float_noise":
        x = 0.25 * rng.standard_normal(n)
    elif name == "tone":
        x = 0.5 * np.sin(2 * np.pi * t / max(2.5, 0.45 * tau_max + 0.37) + 0.2)
    elif name == "stack":                             # partials 1, 2, 3
        w = 2 * np.pi / max(7.0, 0.6 * tau_max + 0.21)
        x = 0.4 * np.sin(w * t) + 0.3 * np.sin(2 * w * t + 1.0) + 0.2 * np.sin(3 * w * t + 2.0)
    elif name == "missing_fundamental":               # partials 2, 3, 4
        w = 2 * np.pi / max(9.0, 0.7 * tau_max + 0.13)
        x = 0.35 * np.sin(2 * w * t) + 0.3 * np.sin(3 * w * t + 1.0) + 0.25 * np.sin(4 * w * t + 2.0)
    elif name == "chirp":                             # the period falls from 0.8 tau_max to 0.3 tau_max
        period = np.linspace(max(3.0, 0.8 * tau_max), max(2.5, 0.3 * tau_max), n)
        x = 0.5 * np.sin(2 * np.pi * np.cumsum(1.0 / period))
    elif name == "edge_dip":                          # a period of exactly tau_max - 1 samples: the dip lies at the last candidate
        x = 0.5 * np.sin(2 * np.pi * t / (tau_max - 1) + 0.3)
    elif name == "descent":                           # a long period on a little noise: d' passes the threshold lags before its minimum
        x = 0.5 * np.sin(2 * np.pi * t / max(2.5, 0.8 * tau_max + 0.5)) + 0.002 * rng.standard_normal(n)
    else:
        raise KeyError(name)
    return x.astype(np.float32)


def piece_length(tau_max, hop):
    return 2 * tau_max + 3 * hop + 11


@functools.lru_cache(maxsize=None)
def recording(tau_max):
    """All SIGNALS back to back, piece_length samples each."""
    n = piece_length(tau_max, HOPS[tau_max])
    x = np.concatenate([signal(name, tau_max, n) for name in SIGNALS])
    x.setflags(write=False)
    return x


def structural_lengths(tau_max, hop):
    """One sample short of a frame, a frame, one short of the second frame, two frames, nothing, four frames."""
    w = 2 * tau_max
    return [w - 1, w, w + hop - 1, w + hop, 0, w + 3 * hop]


def structural_case(tau_min, tau_max, threshold=0.1):
    """Every signal x every structural length at odd starts inside the signal's piece, then a segment from sample 0 and one up to
    sample n (both reach across a seam of two signals).  (8, 2048): one segment of two frames over tone + noise."""
    hop = HOPS[tau_max]
    name = f"lags {tau_min}..{tau_max}" + ("" if threshold == 0.1 else f" threshold {threshold}")
    if tau_max == 2048:
        n = 2 * tau_max + hop + 2
        x = (signal("descent", tau_max, n) + signal("float_noise", tau_max, n) * np.float32(0.01)).astype(np.float32)
        return Case(name, x, np.asarray([(1, 1 + 2 * tau_max + hop)], dtype=np.int64), tau_min, tau_max, hop, threshold)
    x = recording(tau_max)
    piece = piece_length(tau_max, hop)
    rows = []
    for s in range(len(SIGNALS)):
        for start, length in zip((1, 3, 2, 5, 7, 1), structural_lengths(tau_max, hop)):
            rows.append((s * piece + start, s * piece + start + length))
    rows += [(0, 2 * tau_max + hop), (len(x) - 2 * tau_max - hop, len(x))]
    return Case(name, x, np.asarray(rows, dtype=np.int64), tau_min, tau_max, hop, threshold)


def poison_case(tau_min, tau_max):
    """One segment per signal that its frames fill exactly (the last frame ends at s1), each with a sample of its own in front and
    behind: what the leak test poisons.  -> (case, the same case with NaN at every s0 - 1 and s1)."""
    hop = HOPS[tau_max]
    x = recording(tau_max)
    piece = piece_length(tau_max, hop)
    bounds = np.asarray([(s * piece + 1, s * piece + 1 + 2 * tau_max + hop) for s in range(len(SIGNALS))], dtype=np.int64)
    assert bounds[0, 0] >= 1 and bounds[-1, 1] < len(x) and (bounds[1:, 0] - 1 > bounds[:-1, 1]).all()
    y = x.copy()
    y[bounds[:, 0] - 1] = np.nan
    y[bounds[:, 1]] = np.nan
    clean = Case(f"exact fit {tau_min}..{tau_max}", x, bounds, tau_min, tau_max, hop, 0.1)
    return clean, clean._replace(name="poisoned " + clean.name, x=y)


def normalise_sequential(d):
    """d' with run as ONE sequential sum over all lags — not the definition (its blocks of 64): what a kernel that forgot the order computes."""
    run = np.cumsum(d[:, 1:], axis=1)
    out = np.ones_like(d)
    tau = np.arange(1, d.shape[1], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:, 1:] = np.where(run > 0, (d[:, 1:] * tau) / run, 1.0)
    return out


@functools.lru_cache(maxsize=None)
def threshold_cases():
    """Two single-frame cases on float noise at the lags (8, 257) whose THRESHOLD is one of the frame's own d' values:
      tie     the threshold equals d'(c) at the lowest candidate c so far: `<` passes it by (a `<=` would stop there);
      order   at a c behind the first block edge where the two-level prefix sum and a plain sequential one give different bits and
              c is the lowest candidate so far under both, the threshold is the larger of the two values: the definition and a
              sequentially summed d' part ways at c (one is under the threshold there, the other is not).
    Found by a seeded search; the assertions say what was found."""
    tau_min, tau_max = 8, 257
    rng = np.random.default_rng(SEED + 5)
    tie = order = None
    for _ in range(200):
        x = (0.25 * rng.standard_normal(2 * tau_max)).astype(np.float32)
        d = P.difference(x[None, :], tau_max)
        two, seq = P.normalise(d)[0], normalise_sequential(d)[0]
        low_two = np.minimum.accumulate(two[tau_min:tau_max])
        low_seq = np.minimum.accumulate(seq[tau_min:tau_max])
        for c in range(tau_min + 1, tau_max):
            k = c - tau_min
            record = two[c] < low_two[k - 1] and seq[c] < low_seq[k - 1]
            if not (record and 0 < two[c] < 1):
                continue
            bounds = np.asarray([(0, 2 * tau_max)], dtype=np.int64)
            if tie is None:
                tie = Case("threshold tie", x, bounds, tau_min, tau_max, HOPS[tau_max], float(two[c]))
            if order is None and c > P.BLOCK and two[c] != seq[c]:
                threshold = float(max(two[c], seq[c]))
                a, b = P.pick(two, tau_min, tau_max, threshold), P.pick(seq, tau_min, tau_max, threshold)
                if not np.array_equal(a, b):
                    order = Case("prefix order", x, bounds, tau_min, tau_max, HOPS[tau_max], threshold)
        if tie is not None and order is not None:
            return tie, order
    raise AssertionError("the seeded search found no tie / order case")


RANDOM_COUNT = 300


@functools.lru_cache(maxsize=None)
def random_case():
    """300 random segments (0 .. 600 samples, overlaps as they fall) in one recording of chirps, tones and noise; lags (8, 65)."""
    tau_min, tau_max = 8, 65
    rng = np.random.default_rng(SEED + 9)
    n = 20000
    x = np.concatenate([signal(name, tau_max, n // 5, seed=SEED + 1) for name in ("chirp", "stack", "float_noise", "descent", "missing_fundamental")])
    x = (x + 0.01 * rng.standard_normal(n)).astype(np.float32)
    length = rng.integers(0, 601, RANDOM_COUNT)
    s0 = (rng.uniform(0, 1, RANDOM_COUNT) * (n - length)).astype(np.int64)
    return Case("300 random segments", x, np.stack([s0, s0 + length], axis=1).astype(np.int64), tau_min, tau_max, HOPS[tau_max], 0.1)


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case of the bit-equality test, the poisoned ones included."""
    cases = [structural_case(*lags) for lags in LAGS]
    cases += [structural_case(2, 64, threshold=0.35), structural_case(8, 257, threshold=0.02)]
    for lags in LAGS[:-1]:
        cases += list(poison_case(*lags))
    cases += list(threshold_cases()) + [random_case()]
    return tuple(cases)


def index_of(name):
    """The place of the case called `name` in all_cases()."""
    return [c.name for c in all_cases()].index(name)


@functools.lru_cache(maxsize=None)
def expected(index):
    """frames_host of all_cases()[index]: computed once, shared, never modified."""
    c = all_cases()[index]
    frames, offsets = P.frames_host(c.x, c.bounds, c.tau_min, c.tau_max, c.hop, c.threshold)
    frames.setflags(write=False)
    offsets.setflags(write=False)
    return frames, offsets


def prediction(bounds, sr, n):
    """{"onset", "offset"} in seconds whose sample_bounds are exactly `bounds`."""
    from whisperseg_amd.measure import sample_bounds
    pred = {"onset": [int(s0) / sr for s0, _ in bounds], "offset": [int(s1) / sr for _, s1 in bounds]}
    for (s0, s1), on, off in zip(bounds, pred["onset"], pred["offset"]):
        assert sample_bounds(on, off, sr, n) == (s0, s1)
    return pred


# ---- accuracy against known signals (tests/test_pitch_cpu.py) ----------------------------------------------------------------------
def synthetic(kind, f, sr, n, rng, noisy):
    """A tone, a three-partial stack (1, 2, 3) or a missing-fundamental stack (2, 3, 4) of fundamental f Hz; `noisy`: 0.01 of white
    noise, then rounded to int16 steps."""
    t = np.arange(n) / sr
    partials = {"tone": ((1, 0.5),), "stack": ((1, 0.3), (2, 0.25), (3, 0.2)), "missing": ((2, 0.3), (3, 0.25), (4, 0.2))}[kind]
    x = sum(a * np.sin(2 * np.pi * k * f * t + rng.uniform(0, 2 * np.pi)) for k, a in partials)
    if noisy:
        x = np.round((x + 0.01 * rng.standard_normal(n)) * 32768) / 32768
    return x.astype(np.float32)
