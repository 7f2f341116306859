"""Independent twins of the sed_eval protocol's pieces, and the builders the CPU and the GPU test share.

* ``double_threshold_ref``: a scalar restatement of utils/sed_utils.py:170-197 ``_double_threshold(..., return_arr=False)``
  (runs of x > low, those with a frame x > high kept, THEN connect_), comparing in float32 as numpy compares a float32 row with
  a Python float.  Pinned by tests/golden/sed_double_threshold.npz, which the imported reference wrote.
* ``brute_force_tp``: the event-based true positives as the best of EVERY injective assignment, in integer milliseconds.
* ``naive_segment_counts``: the segment-based counts by walking every millisecond of every event.
  Both raise ``Tie`` where an integer-millisecond comparison is an equality whose floating-point twin may land on either
  side: such a case has no implementation-independent answer.
* ``sed_counts_ref``: the (B, NT, 5) tensor ops.sed_counts must return, from utils/sed_metrics.py (the yardstick).
"""
import math

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ double threshold

def double_threshold_ref(x, high: float, low: float, n_connect: int):
    """x: 1-D float32 -> list of (onset, offset) rows [onset, offset)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1
    hi, lo = np.float32(high), np.float32(low)
    above_low, above_high = (x > lo).tolist() + [False], (x > hi).tolist() + [False]       # float32 comparisons
    kept, start, has_high = [], None, False
    for i, above in enumerate(above_low):
        if above:
            if start is None:
                start, has_high = i, False
            has_high = has_high or above_high[i]
        elif start is not None:
            if has_high:
                kept.append([start, i])
            start = None
    merged = []
    for on, off in kept:
        if merged and on - merged[-1][1] <= n_connect:
            merged[-1][1] = off
        else:
            merged.append([on, off])
    return [(a, b) for a, b in merged]


def golden_cases(path):
    """tests/golden/sed_double_threshold.npz -> [(x row float32, high, low, n_connect, regions (K,2) int64), ...]."""
    z = np.load(path)
    cases = []
    for T in z["lengths"]:
        x, regions, offsets = z[f"x{T}"], z[f"regions{T}"], z[f"offsets{T}"]
        k = 0
        for r in range(x.shape[0]):
            for n in z["n_connect"]:
                for high, low in z["pairs"]:
                    cases.append((x[r], float(high), float(low), int(n), regions[offsets[k]:offsets[k + 1]]))
                    k += 1
        assert k == len(offsets) - 1
    return cases


def cpu_segments_double(scores: torch.Tensor, high, low, n_connect: int):
    """list over clips of list over operating points of (K,2) int64, from ``double_threshold_ref``."""
    return [[np.array(double_threshold_ref(row, h, l, n_connect), dtype=np.int64).reshape(-1, 2) for h, l in zip(high, low)]
            for row in scores.numpy()]


# ------------------------------------------------------------------------------------------------ naive twins

class Tie(Exception):
    pass


def _ms(t: float) -> int:
    return int(round(t * 1000))


def brute_force_tp(det, gt, t_collar: float, percentage_of_length: float) -> int:
    """The largest number of (reference, estimate) pairs inside the collars over every injective assignment; integer
    milliseconds (the offset collar in exact fifths of a microsecond would be overkill: percentage * length is compared as a
    rational, cross-multiplied by 1000)."""
    det = [(_ms(a), _ms(b)) for a, b in det]
    gt = [(_ms(a), _ms(b)) for a, b in gt]
    collar, pct = _ms(t_collar), _ms(percentage_of_length)          # pct in thousandths

    def within(diff, limit_x1000):
        if abs(diff) * 1000 == limit_x1000:
            raise Tie()
        return abs(diff) * 1000 < limit_x1000

    ok = [[within(g[0] - d[0], collar * 1000) and within(g[1] - d[1], max(collar * 1000, pct * (g[1] - g[0]))) for d in det]
          for g in gt]

    def best(g, used):
        if g == len(gt):
            return 0
        top = best(g + 1, used)                                      # leave this reference event unmatched
        for d in range(len(det)):
            if ok[g][d] and d not in used:
                top = max(top, 1 + best(g + 1, used | {d}))
        return top

    return best(0, frozenset())


def naive_segment_counts(det, gt, resolution: float):
    """(tp, fp, fn, n) with a segment active when one of its milliseconds lies inside an event.  Events need a duration.  A
    boundary exactly on a segment edge is a Tie unless the resolution is a power of two (then the division is exact)."""
    res = _ms(resolution)
    dyadic = math.frexp(resolution)[0] == 0.5
    det = [(_ms(a), _ms(b)) for a, b in det]
    gt = [(_ms(a), _ms(b)) for a, b in gt]
    for on, off in det + gt:
        assert off > on
        if not dyadic and (on % res == 0 or off % res == 0):
            raise Tie()
    end = max([off for _, off in det + gt], default=0)
    n = -(-end // res)
    sys_active, ref_active = [False] * n, [False] * n
    for events, active in ((det, sys_active), (gt, ref_active)):
        for on, off in events:
            for t in range(on, off):
                active[t // res] = True
    tp = sum(s and r for s, r in zip(sys_active, ref_active))
    return tp, sum(sys_active) - tp, sum(ref_active) - tp, n


def random_events(rng, k: int, span_ms: int, step_ms: int, shift_ms: int = 0, disjoint: bool = True):
    """k events [onset, offset) seconds on a grid of step_ms (+ shift_ms); ascending and disjoint, or free to overlap."""
    if disjoint:
        cuts = np.sort(rng.choice(np.arange(1, span_ms // step_ms), size=2 * k, replace=False)) * step_ms + shift_ms
        return np.array([[cuts[2 * i] / 1000.0, cuts[2 * i + 1] / 1000.0] for i in range(k)]).reshape(-1, 2)
    on = rng.integers(0, span_ms // step_ms - 1, size=k) * step_ms + shift_ms
    length = rng.integers(1, max(span_ms // step_ms // 2, 2), size=k) * step_ms
    return np.stack([on / 1000.0, (on + length) / 1000.0], axis=1).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------ the device's yardstick

def sed_counts_ref(regions, counts, gt, gt_count, time_resolution, t_collar=0.2, percentage_of_length=0.2,
                   segment_resolution=1.0) -> torch.Tensor:
    """The (B, NT, 5) int32 tensor ops.sed_counts must return, from host arrays shaped like its arguments."""
    from texttoaudiogrounding_amd.utils import sed_metrics as SM
    regions, counts = np.asarray(regions), np.asarray(counts)
    gt, gt_count = np.asarray(gt, dtype=np.float64), np.asarray(gt_count)
    B, NT = counts.shape
    out = torch.zeros(B, NT, 5, dtype=torch.int32)
    for b in range(B):
        rows = gt[b, :gt_count[b]]
        for t in range(NT):
            det = regions[b, t, :counts[b, t]].astype(np.float64) * time_resolution
            ev_tp, _, _ = SM.event_based_counts(det, rows, t_collar, percentage_of_length)
            out[b, t] = torch.tensor([ev_tp, *SM.segment_based_counts(det, rows, segment_resolution)], dtype=torch.int32)
    return out


GREEDY_BREAKER = (np.array([[0.88, 1.00], [1.08, 1.28]]), np.array([[1.0, 1.2], [0.8, 0.9]]))     # (det, gt): maximum 2


def near_ground_truth(regions, counts, G, gmax: int, res: float, seed: int = 1, pad: float = -1.0e30):
    """(gt (B,gmax,2) float64, gt_count (B,) int32): G rows per clip (an int or a list over clips), most of them a detection of
    the clip's first operating point moved by -6 .. 6 frames at either end (5 frames = the 0.2 s collar: ties all the time),
    every fourth anywhere on the grid, every seventh off the grid; free to overlap; garbage in the padding."""
    rng = np.random.default_rng(seed)
    regions, counts = np.asarray(regions), np.asarray(counts)
    B = counts.shape[0]
    gt_count = np.broadcast_to(np.asarray(G, dtype=np.int32), (B,)).copy()
    gt = np.full((B, gmax, 2), pad, dtype=np.float64)
    for b in range(B):
        D = int(counts[b, 0])
        span = int(regions[b, 0, D - 1, 1]) if D else 60
        for i in range(int(gt_count[b])):
            if D and i % 4 != 3:
                on, off = regions[b, 0, int(rng.integers(0, D))]
                on, off = max(int(on) + int(rng.integers(-6, 7)), 0), int(off) + int(rng.integers(-6, 7))
                off = max(off, on)                               # (a zero-duration row now and then)
            else:
                on = int(rng.integers(0, span + 1))
                off = on + int(rng.integers(1, 150))
            gt[b, i] = [on * res, off * res]
            if i % 7 == 6:
                gt[b, i] += rng.uniform(0.0, 0.04)
    return gt, gt_count
