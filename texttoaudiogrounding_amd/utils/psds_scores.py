"""Score-based PSDS: intersection-based PSDS over EVERY decision threshold the frame scores define -- the number the reference
reports (utils/eval_util.py:226-292 compute_psds_sed_scores -> sed_scores_eval.intersection_based.psd_roc on the raw frame
scores; run_strong.py:867-888, :938-949 and the weak / class-mapping runners print it, validation calls it every epoch).

Host code (numpy) and the definition of record: ``ops.psds_score_deltas`` (csrc/psds_scores.hip) and
``device_eval.ScorePsdsEvaluator`` must give these integers and floats exactly.  Nothing here is taken from sed_scores_eval,
which is not installed: the operating point is ``grounding_eval.psds_operating_point`` and the curve is
``grounding_eval.psds_intersection``; what is new is the SET of operating points, all of them.

Definition.  A pair is one (clip, phrase) row of scores, one file of the tables (``{key: (K, 2) [onset, offset] seconds}``, as in
grounding_eval.py).  Frame t spans [t res, (t + 1) res]; the detections of a pair at threshold theta are the maximal runs
[on, off) of frames with ``score > theta``, as seconds (on res, off res) -- no median filter, no connect step.  With
v_1 < ... < v_m the distinct non-NaN values of the row (-0.0 and +0.0 are one value; a NaN is never active and is no
threshold) and v_0 = -inf, regime k is every theta in [v_k, v_{k+1}): its active set is ``score > v_k`` and c_k = (psds_tp,
psds_fp) of that one file; c_m = (0, 0).  The operating points of an evaluation are theta = -inf and every distinct value over
all pairs; the counts at theta are the sums over the pairs of c_{k_p(theta)}.  (``>`` or ``>=``: {score > v_k} and
{score >= v_{k+1}} are the same family of sets, so the curve does not move.)

Delta form.  Pair p contributes base_p = c_0 and at value v_k the delta c_k - c_{k-1}; sort all entries by value, take the
inclusive prefix sum, add the sum of the bases, and keep the LAST entry of each run of equal values (a prefix sum inside a run
is no operating point) beside the base point.  The counts are integers, so the order inside a run does not matter.

Pinned: equality of the device path with these functions, and of the delta form with the brute force.  **Unpinned: parity with
sed_scores_eval itself** -- its ``time_decimals = 6`` rounding, its treatment of overlapping ground truths of one class and its
exact thresholds (midpoints between scores) cannot be run here.
"""
from __future__ import annotations

import csv
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .grounding_eval import EPS, Table, _rows, psd_roc, psds_intersection, psds_operating_point, staircase_auc

#: the max_efpr values the reference's drivers report (run_strong.py:867-888)
REFERENCE_MAX_EFPRS = (400, 600, 800, 1000, None)


def canonical_scores(row) -> np.ndarray:
    """(T,) float32 with -0.0 turned into +0.0 (NaNs stay)."""
    row = np.asarray(row, dtype=np.float32).reshape(-1)
    return row + np.float32(0.0)


def distinct_values(row) -> np.ndarray:
    """The ascending distinct non-NaN values of a row, float32."""
    row = canonical_scores(row)
    return np.unique(row[~np.isnan(row)])


def detections_above(row, threshold: float, time_resolution: float) -> np.ndarray:
    """(K, 2) float64 seconds: the maximal runs of frames with ``score > threshold`` (a NaN is not above anything)."""
    with np.errstate(invalid="ignore"):
        active = np.asarray(row, dtype=np.float32).reshape(-1) > threshold
    edges = np.diff(np.concatenate(([0], active.astype(np.int8), [0])))
    frames = np.stack([np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)], axis=1).astype(np.int64)
    return frames.astype(np.float64) * time_resolution


def file_counts(det: np.ndarray, gt: np.ndarray, dtc: float, gtc: float) -> Tuple[int, int]:
    """The integers (psds_tp, psds_fp) ``psds_operating_point`` counts for ONE file: it returns tp / n_gt and fp per hour, so it
    is asked with one hour of audio (fp / 1.0 is fp) and the TP ratio is turned back (tp <= n_gt <= a few hundred: exact)."""
    n_gt = int(np.asarray(gt).reshape(-1, 2).shape[0])
    ratio, per_hour = psds_operating_point({"f": det}, {"f": gt}, 3600.0, dtc, gtc)
    return int(round(ratio * n_gt)), int(round(per_hour))


def pair_regimes(scores_row, gt_rows, time_resolution: float, dtc: float = 0.5, gtc: float = 0.5):
    """(values (m,) float32 ascending, counts (m + 1, 2) int64): counts[k] = (psds_tp, psds_fp) of the pair in regime k, the
    active set ``score > v_k`` with v_0 = -inf, every regime evaluated through ``psds_operating_point``."""
    row = canonical_scores(scores_row)
    values = distinct_values(row)
    gt = np.asarray(gt_rows, dtype=np.float64).reshape(-1, 2)
    counts = np.zeros((values.size + 1, 2), dtype=np.int64)
    for k, v in enumerate(np.concatenate(([-np.inf], values))):
        counts[k] = file_counts(detections_above(row, v, time_resolution), gt, dtc, gtc)
    return values, counts


def points_from_deltas(values, deltas, base):
    """The merge of the delta form: values (N,) and deltas (N, 2) integer entries of all pairs in any order, base (2,) the sum
    of the pairs' c_0 -> (thresholds (P,), counts (P, 2) int64), P = 1 + the number of distinct values: row 0 is theta = -inf
    with ``base``, row i the i-th distinct value ascending with base + every delta at a value <= it.  Stable sort by value,
    inclusive prefix sum, the last entry of each run of equal values.  numpy arrays give numpy arrays; torch tensors are merged
    where they live and give tensors (the boolean selection is the one host synchronisation)."""
    as_numpy = not torch.is_tensor(values)
    v = torch.as_tensor(np.asarray(values) if as_numpy else values).reshape(-1)
    d = torch.as_tensor(np.asarray(deltas) if as_numpy else deltas).reshape(-1, 2).to(torch.int64)
    b = torch.as_tensor(np.asarray(base) if as_numpy else base).reshape(1, 2).to(torch.int64).to(v.device)
    if v.numel() != d.shape[0]:
        raise ValueError(f"points_from_deltas: {v.numel()} values but {d.shape[0]} deltas")
    v, order = torch.sort(v, stable=True)
    running = torch.cumsum(d[order], 0) + b
    last = torch.ones_like(v, dtype=torch.bool)
    last[:-1] = v[1:] != v[:-1]
    thresholds = torch.cat([torch.full((1,), -float("inf"), dtype=v.dtype, device=v.device), v[last]])
    counts = torch.cat([b, running[last]])
    return (thresholds.numpy(), counts.numpy()) if as_numpy else (thresholds, counts)


def psds_from_counts(counts, n_refs: int, total_duration_s: float, max_efpr=None):
    """Operating-point counts (P, 2) [psds_tp, psds_fp] -> (psds, efpr, etpr): the expressions of ``psds_operating_point`` and
    ``psds_intersection`` on integers.  max_efpr: None (the largest eFPR), a number, or a sequence of those -> {max_efpr: psds}."""
    pts = [(int(tp) / max(int(n_refs), EPS), int(fp) / (total_duration_s / 3600.0)) for tp, fp in np.asarray(counts).tolist()]
    x, y = psd_roc(pts)

    def score(limit):
        if limit is None:
            limit = float(x.max())
        return float(y.max()) if limit <= 0 else staircase_auc(x, y, limit) / limit

    if isinstance(max_efpr, (list, tuple, np.ndarray)):
        return {m: score(m) for m in max_efpr}, x, y
    return score(max_efpr), x, y


def all_thresholds(scores: Dict[str, np.ndarray]) -> np.ndarray:
    """-inf and every distinct non-NaN value over all rows, ascending (float32 values as float64)."""
    rows = [distinct_values(r) for r in scores.values()]
    values = np.unique(np.concatenate(rows)) if rows else np.zeros(0, dtype=np.float32)
    return np.concatenate(([-np.inf], values.astype(np.float64)))


def threshold_tables(scores: Dict[str, np.ndarray], time_resolution: float) -> Dict[float, Table]:
    """{theta: {key: detections}} for every threshold of ``all_thresholds``: the operating-point tables of the brute force."""
    return {float(th): {k: detections_above(canonical_scores(r), th, time_resolution) for k, r in scores.items()}
            for th in all_thresholds(scores)}


def psds_from_scores(scores: Dict[str, np.ndarray], ground_truth: Table, durations: Dict[str, float], time_resolution: float,
                     dtc_threshold: float = 0.5, gtc_threshold: float = 0.5, max_efpr: Optional[float] = None) -> float:
    """The brute force, slow on purpose: ``psds_intersection`` over the detection tables of every distinct threshold.
    scores: {key: (T,) float32}; ground_truth, durations as for ``psds_intersection``."""
    return psds_intersection(threshold_tables(scores, time_resolution), ground_truth, durations, dtc_threshold, gtc_threshold,
                             max_efpr)


def _durations(duration, ground_truth, fname_to_aid) -> Dict[str, float]:
    if not isinstance(duration, dict):                          # the reference's tab-separated audio_id / duration file
        with open(duration, newline="") as fh:
            duration = {r["audio_id"]: float(r["duration"]) for r in csv.DictReader(fh, delimiter="\t")}
    duration = {str(k): v for k, v in duration.items()}
    return {f: float(duration[str(fname_to_aid[f] if fname_to_aid is not None else f)]) for f in ground_truth}


def compute_psds_sed_scores(scores: Dict[str, np.ndarray], ground_truth: Table, duration, fname_to_aid: Optional[dict] = None,
                            dtc_threshold: float = 0.5, gtc_threshold: float = 0.5,
                            max_efpr: Union[None, float, Sequence] = None, time_resolution: float = None):
    """utils/eval_util.py:250-292 without pandas and without the plot.  scores: {fname: (T,) frame scores} (the reference passes
    data frames of onset / offset / score rows; ``time_resolution`` is the frame length those carry); ground_truth: {fname:
    [[onset, offset], ...]}; duration: {audio id: seconds}, or the path of the reference's tab-separated ``audio_id`` /
    ``duration`` file; fname_to_aid: {fname: audio id} (None: the durations are keyed by fname).  max_efpr: None, a number, or
    a sequence -> {max_efpr: psds}.  The delta form: ``pair_regimes`` per file, ``points_from_deltas``, ``psds_from_counts`` --
    equal to ``psds_from_scores`` as a float."""
    if time_resolution is None or not time_resolution > 0:
        raise ValueError("compute_psds_sed_scores: time_resolution (seconds per frame) must be given and positive")
    durations = _durations(duration, ground_truth, fname_to_aid)
    values, deltas, base = [], [], np.zeros(2, dtype=np.int64)
    for f in sorted(set(scores) | set(ground_truth)):
        v, c = pair_regimes(scores.get(f, np.zeros(0, dtype=np.float32)), _rows(ground_truth, f), time_resolution, dtc_threshold,
                            gtc_threshold)
        values.append(v)
        deltas.append(np.diff(c, axis=0))
        base += c[0]
    _, counts = points_from_deltas(np.concatenate(values) if values else np.zeros(0, dtype=np.float32),
                                   np.concatenate(deltas) if deltas else np.zeros((0, 2), dtype=np.int64), base)
    n_refs = int(sum(_rows(ground_truth, f).shape[0] for f in ground_truth))
    psds, _, _ = psds_from_counts(counts, n_refs, float(sum(durations.values())), max_efpr)
    return psds
