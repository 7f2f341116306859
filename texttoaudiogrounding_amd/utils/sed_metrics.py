"""The reference's second evaluation protocol on the host: event-based and segment-based F-score / error rate as
``sed_eval`` defines them, for tables in which every (clip, phrase) pair is one file with the single label ``fake_event``
(python_scripts/evaluation/evaluate_sed_eval.py -> utils/eval_util.py:354-425 ``compute_sed_eval``).

Plain numpy / Python, and the definition of record: ``ops.sed_counts`` (csrc/sed_eval.hip) must give these integers exactly,
and ``utils.device_eval.SedEvaluator`` turns its sums into scores with ``scores_from_counts`` below.

Pinning: ``sed_eval`` / ``dcase_util`` are third-party packages that are neither vendored in the reference nor installed here,
so **parity with those packages is unpinned**.  The functions restate the published definitions (Mesaros, Heittola, Virtanen,
"Metrics for polyphonic sound event detection", Applied Sciences 2016, and the sed_eval 0.2.x documentation):

* event-based, ``event_matching_type='optimal'``: a reference and an estimated event can be matched when their onsets are
  within ``t_collar`` and their offsets within ``max(t_collar, percentage_of_length * reference length)``; true positives =
  the maximum cardinality of a matching.  With one label there is no substitution: FP = Nsys - TP, FN = Nref - TP.
* segment-based: both event lists become 0/1 rolls over segments of ``resolution`` seconds, an event covering segments
  ``floor(onset / resolution) .. ceil(offset / resolution) - 1``, both padded to ``ceil(largest offset / resolution)``
  segments; per segment TP = both active, FP = estimate only, FN = reference only.
* precision = TP / (Nsys + eps), recall = TP / (Nref + eps), F = 2 P R / (P + R) (0 when both are 0), deletion rate =
  FN / (Nref + eps), insertion rate = FP / (Nref + eps), error rate = their sum (no substitutions), eps = numpy.spacing(1):
  an empty system output scores precision 0, an empty reference recall 0.

They are pinned by hand-derivable answers, a brute-force matching and a millisecond-walking roll (tests/sed_eval_ref.py,
tests/test_sed_metrics_cpu.py).  Times are seconds >= 0.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

from .grounding_eval import Table, _rows

EPS = float(np.spacing(1))


def _events(a) -> list:
    return [(float(on), float(off)) for on, off in np.asarray(a, dtype=np.float64).reshape(-1, 2)]


def can_match(det_event, gt_event, t_collar: float, percentage_of_length: float) -> bool:
    """The collar test of one (estimated, reference) pair: plain fp64 operations, which csrc/sed_eval.hip repeats."""
    (on_d, off_d), (on_g, off_g) = det_event, gt_event
    by_length = percentage_of_length * (off_g - on_g)
    offset_collar = by_length if by_length > t_collar else t_collar
    return math.fabs(on_g - on_d) <= t_collar and math.fabs(off_g - off_d) <= offset_collar


def event_based_counts(det, gt, t_collar: float = 0.2, percentage_of_length: float = 0.2) -> Tuple[int, int, int]:
    """det (D,2), gt (G,2) seconds of ONE file -> (tp, fp, fn): tp = the size of a maximum matching of the pairs that
    ``can_match`` (augmenting paths, one depth-first search per reference event), fp = D - tp, fn = G - tp."""
    det, gt = _events(det), _events(gt)
    edges = [[d for d, e in enumerate(det) if can_match(e, g, t_collar, percentage_of_length)] for g in gt]
    owner = [-1] * len(det)                                    # the reference event a detection is matched with

    def augment(g, seen):
        for d in edges[g]:
            if d not in seen:
                seen.add(d)
                if owner[d] < 0 or augment(owner[d], seen):
                    owner[d] = g
                    return True
        return False

    tp = sum(augment(g, set()) for g in range(len(gt)))
    return tp, len(det) - tp, len(gt) - tp


def _roll(events, resolution: float, n_segments: int) -> np.ndarray:
    roll = np.zeros(n_segments, dtype=bool)
    for on, off in events:
        roll[max(int(math.floor(on / resolution)), 0):max(int(math.ceil(off / resolution)), 0)] = True
    return roll


def segment_based_counts(det, gt, resolution: float = 1.0) -> Tuple[int, int, int, int]:
    """det (D,2), gt (G,2) seconds of ONE file -> (tp, fp, fn, n_segments) over the padded event rolls."""
    det, gt = _events(det), _events(gt)
    ends = [off for _, off in det + gt]
    n = max(int(math.ceil(max(ends) / resolution)), 0) if ends else 0
    sys_roll, ref_roll = _roll(det, resolution, n), _roll(gt, resolution, n)
    return (int((sys_roll & ref_roll).sum()), int((sys_roll & ~ref_roll).sum()), int((~sys_roll & ref_roll).sum()), n)


def _family(tp, n_sys, n_ref, fp, fn) -> Dict[str, np.ndarray]:
    tp, n_sys, n_ref, fp, fn = (np.asarray(v, dtype=np.float64) for v in (tp, n_sys, n_ref, fp, fn))
    precision, recall = tp / (n_sys + EPS), tp / (n_ref + EPS)
    both = precision + recall
    f = np.where(both > 0, 2.0 * precision * recall / np.where(both > 0, both, 1.0), 0.0)
    deletion, insertion = fn / (n_ref + EPS), fp / (n_ref + EPS)
    return {"precision": precision, "recall": recall, "f_measure": f, "error_rate": deletion + insertion,
            "deletion_rate": deletion, "insertion_rate": insertion}


def scores_from_counts(ev_tp, n_sys, n_ref, seg_tp, seg_fp, seg_fn, seg_n=None) -> Dict[str, Dict[str, np.ndarray]]:
    """Summed integers (scalars, or arrays with one entry per operating point) -> {"event": {...}, "segment": {...}}, each with
    precision, recall, f_measure, error_rate, deletion_rate, insertion_rate as float64 arrays of the inputs' shape.  ev_tp,
    n_sys, n_ref: matched, estimated and reference EVENTS; seg_tp, seg_fp, seg_fn: SEGMENTS; seg_n (optional): all segments, for
    the segment-based "accuracy" (TP + TN) / N (0 without a segment)."""
    seg_tp, seg_fp, seg_fn = (np.asarray(v, dtype=np.float64) for v in (seg_tp, seg_fp, seg_fn))
    ev_tp, n_sys, n_ref = (np.asarray(v, dtype=np.float64) for v in (ev_tp, n_sys, n_ref))
    out = {"event": _family(ev_tp, n_sys, n_ref, n_sys - ev_tp, n_ref - ev_tp),
           "segment": _family(seg_tp, seg_tp + seg_fp, seg_tp + seg_fn, seg_fp, seg_fn)}
    if seg_n is not None:
        seg_n = np.asarray(seg_n, dtype=np.float64)
        out["segment"]["accuracy"] = (seg_n - seg_fp - seg_fn) / (seg_n + EPS)
    return out


def count_tables(ground_truth_table: Table, prediction_table: Table, t_collar: float = 0.2, time_resolution: float = 1.0,
                 percentage_of_length: float = 0.2) -> np.ndarray:
    """The seven integers {ev_tp, seg_tp, seg_fp, seg_fn, seg_n, n_sys, n_ref} summed over the files of the GROUND-TRUTH table
    (eval_util.py:367 evaluates ``reference["filename"].unique()``: a file only the predictions name is not evaluated, one
    they do not name has no estimated event), as an int64 vector -- the row ``SedEvaluator`` accumulates per operating point."""
    total = np.zeros(7, dtype=np.int64)
    for f in ground_truth_table:
        gt, det = _rows(ground_truth_table, f), _rows(prediction_table, f)
        ev_tp, _, _ = event_based_counts(det, gt, t_collar, percentage_of_length)
        total += np.array([ev_tp, *segment_based_counts(det, gt, time_resolution), len(det), len(gt)], dtype=np.int64)
    return total


def compute_sed_eval(ground_truth_table: Table, prediction_table: Table, t_collar: float = 0.2, time_resolution: float = 1.0,
                     percentage_of_length: float = 0.2) -> Dict[str, Dict[str, np.ndarray]]:
    """eval_util.compute_sed_eval (:418-425) over ``{filename: (K, 2)}`` tables: ``scores_from_counts`` of the summed counts, plus
    "counts" (``count_tables``' vector).  ``time_resolution`` is the SEGMENT length, as in the reference's signature."""
    counts = count_tables(ground_truth_table, prediction_table, t_collar, time_resolution, percentage_of_length)
    ev_tp, seg_tp, seg_fp, seg_fn, seg_n, n_sys, n_ref = (int(v) for v in counts)
    out = scores_from_counts(ev_tp, n_sys, n_ref, seg_tp, seg_fp, seg_fn, seg_n)
    out["counts"] = counts
    return out
