"""Scalar twin of csrc/psds_scores.hip for ONE pair, in plain Python loops and independent of utils/psds_scores.py: sort the row and
squeeze out duplicates, walk the frames of every regime for its runs, count them with the scalar fp64 restatement of
tests/grounding_eval_ref.py (``pair_counts``: the order of every addition written out) -- and the builders of the inputs and of
the expected output tensors that the score-based PSDS tests share.

The yardstick is utils/psds_scores.py ``pair_regimes`` (numpy, through ``psds_operating_point``); the twin must agree with it, and
the kernel with both.
"""
import math

import numpy as np
import torch

from tests import grounding_eval_ref as G


def regimes_ref(row, gt_rows, res, dtc=0.5, gtc=0.5):
    """(values: ascending distinct non-NaN float32 scores as Python floats, counts: m + 1 (psds_tp, psds_fp) tuples)."""
    row = [float(np.float32(x)) for x in row]
    row = [0.0 if x == 0.0 else x for x in row]                 # -0.0 -> +0.0
    values = []
    for x in sorted(x for x in row if not math.isnan(x)):
        if not values or x != values[-1]:
            values.append(x)
    gt = [(float(a), float(b)) for a, b in gt_rows]
    counts = []
    for v in [-math.inf] + values:
        det, on = [], None
        for t, x in enumerate(row + [math.nan]):                # the NaN closes a run that reaches the end
            active = x > v
            if active and on is None:
                on = t
            if not active and on is not None:
                det.append((float(on) * res, float(t) * res))
                on = None
        counts.append(G.pair_counts(det, gt, dtc, gtc)[2:])
    return values, counts


def expected_outputs(scores, gt, gt_count, res, regimes, dtc=0.5, gtc=0.5):
    """The four tensors ops.psds_score_deltas must return, from host arrays shaped like its arguments; ``regimes`` is
    ``regimes_ref`` or utils.psds_scores.pair_regimes."""
    scores = np.asarray(scores, dtype=np.float32)
    B, T = scores.shape
    values = torch.full((B, T), float("inf"), dtype=torch.float32)
    deltas = torch.zeros(B, T, 2, dtype=torch.int32)
    base = torch.zeros(B, 2, dtype=torch.int32)
    n_values = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        v, c = regimes(scores[b], np.asarray(gt)[b, :int(gt_count[b])], res, dtc, gtc)
        c = np.asarray(c, dtype=np.int64).reshape(-1, 2)
        m = len(v)
        assert c.shape[0] == m + 1 and tuple(c[m]) == (0, 0)
        values[b, :m] = torch.as_tensor(np.asarray(v, dtype=np.float32))
        deltas[b, :m] = torch.as_tensor(np.diff(c, axis=0).astype(np.int32))
        base[b] = torch.as_tensor(c[0].astype(np.int32))
        n_values[b] = m
    return values, deltas, base, n_values


def same_outputs(got, want):
    """Equality of the four tensors, the values bit for bit (so that +0.0 is told from -0.0)."""
    gv, gd, gb, gn = [t.cpu() for t in got]
    wv, wd, wb, wn = want
    return (torch.equal(gv.view(torch.int32), wv.view(torch.int32)) and torch.equal(gd, wd) and torch.equal(gb, wb)
            and torch.equal(gn, wn))


def build_scores(B, T, kind, seed=0):
    """(B, T) float32 on the host.  "continuous": tests.grounding_eval_ref.build_scores; "eighths": the same quantised to 1 / 8,
    so that equal values occur inside a row and across rows; "equal": one value everywhere; a number: quantised to that step."""
    s = G.build_scores(B, T, seed=seed)
    if kind == "continuous":
        return s
    if kind == "equal":
        return torch.full((B, T), 0.375)
    step = 0.125 if kind == "eighths" else float(kind)
    return (torch.round(s / step) * step).to(torch.float32)


def grid_ground_truth(B, Gn, T, res, seed=9):
    """(gt (B, Gn, 2) float64, gt_count (B,) int32): Gn rows per pair ON the frame grid inside the clip (1 .. T frames long), so
    that the ratios land on dtc / gtc; pair b uses 1 + b % Gn of them when B > 1."""
    rng = np.random.default_rng(seed)
    gt = np.full((B, max(Gn, 1), 2), -1.0e30, dtype=np.float64)
    gt_count = np.array([Gn if B == 1 else (1 + b % Gn if Gn else 0) for b in range(B)], dtype=np.int32)
    for b in range(B):
        for i in range(int(gt_count[b])):
            k = int(rng.integers(0, T))
            n = int(rng.integers(1, max(T // 2, 2)))
            gt[b, i] = [k * res, (k + n) * res]
    return gt[:, :Gn] if Gn else gt[:, :0], gt_count


def tables(scores, gt, gt_count, res, prefix="pair"):
    """({key: (T,) float32}, {key: (G, 2)}, {key: seconds}) of a batch, for the host functions."""
    scores = np.asarray(scores, dtype=np.float32)
    keys = [f"{prefix}{b}" for b in range(scores.shape[0])]
    return ({k: scores[b] for b, k in enumerate(keys)},
            {k: np.asarray(gt)[b, :int(gt_count[b])].reshape(-1, 2) for b, k in enumerate(keys)},
            {k: scores.shape[1] * res for k in keys})
