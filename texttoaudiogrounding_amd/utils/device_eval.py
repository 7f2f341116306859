"""Grounding evaluation with the operating-point arithmetic on the device: the counterpart of Runner.eval_inference +
compute_th_auc / compute_psds of the reference (python_scripts/training/run_strong.py:171-276, utils/eval_util.py:136-330).

``eval_util.segments_for_thresholds`` -> ``grounding_eval.tables_from_segments`` -> ``compute_th_auc`` / ``psds_intersection``
is the host path: it copies every segment of every (clip, threshold) pair to the host and walks files x thresholds in Python.
Here ``ops.segments`` and ``ops.grounding_counts`` (csrc/grounding_eval.hip) leave four integers per pair on the device, a batch
adds them into ONE (NT, 6) int64 tensor, and ``compute`` reads that tensor once.  The host functions of grounding_eval.py stay
the yardstick: the counts are theirs exactly, so precision, recall, th-AUC and PSDS are equal as floats.

``SedEvaluator`` does the same for the reference's second protocol (python_scripts/evaluation/evaluate_sed_eval.py ->
utils/eval_util.py:354-425 compute_sed_eval): ``ops.segments`` or the double threshold ``ops.segments_double``, then
``ops.sed_counts`` (csrc/sed_eval.hip), whose yardstick is utils/sed_metrics.py.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .. import ops
from . import eval_util
from .grounding_eval import EPS, GroundingPrecisionRecall, psd_roc, staircase_auc

MAX_GROUND_TRUTHS = 128          # rows per (clip, phrase) pair tag_grounding_counts takes


def ground_truth_arrays(items: Sequence[Sequence[Sequence[float]]]):
    """A batch's ground truths, a list over the pairs of ``[[onset, offset], ...]`` seconds -> (gt (B, Gmax, 2) float64 padded
    with zeros, gt_count (B,) int32), on the host.  ``(0, 0)`` rows are dropped as run_strong.py:186-187 drops them; more than
    128 rows for one pair raise."""
    rows = [[(float(on), float(off)) for on, off in item if not (on == 0 and off == 0)] for item in items]
    gmax = max((len(r) for r in rows), default=0)
    if gmax > MAX_GROUND_TRUTHS:
        raise ValueError(f"ground_truth_arrays: a pair has {gmax} ground-truth rows; the device evaluation takes at most "
                         f"{MAX_GROUND_TRUTHS}")
    gt = np.zeros((len(rows), gmax, 2), dtype=np.float64)
    for b, r in enumerate(rows):
        if r:
            gt[b, :len(r)] = r
    return gt, np.array([len(r) for r in rows], dtype=np.int32)


class GroundingEvaluator:
    """Accumulates the operating points of ``thresholds`` over batches on the device and turns them into th-AUC and PSDS.

    ``counts`` is an (NT, 6) int64 device tensor: tp_preds, tp_refs, psds_tp, psds_fp, n_preds, n_refs per threshold, summed
    over every pair passed to ``update`` (a data-parallel caller all-reduces it before ``compute``).  A pair is one file of the
    host tables, so the sums are what ``evaluate_detections`` and ``psds_operating_point`` count over a table that holds every
    pair once and whose ground-truth table holds exactly those pairs.

    Thresholds must be strictly ascending.  The reference's ``add_operating_point`` (restated in
    ``GroundingPrecisionRecall.add_operating_point``) does not evaluate a detection table equal to ANY earlier one: it appends a
    copy of the LAST row.  With ascending thresholds that cannot change a value: binarize (score > threshold), the median
    filter of a 0/1 sequence and connect_clusters are monotone, so the active frames at a higher threshold are a subset of
    those at a lower one; the sets between two equal tables are squeezed between equal sets, so a table equal to an earlier one
    equals the one immediately before it, whose row is the last row -- the copy is the value the evaluation would give.  Plain
    per-threshold evaluation, which is what the counts are, therefore gives the reference's th-AUC.
    """

    def __init__(self, thresholds, window_size: int, time_resolution: float, dtc: float = 0.5, gtc: float = 0.5, device="cuda"):
        th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        if th.size == 0 or not np.all(np.diff(th) > 0):
            raise ValueError("GroundingEvaluator: thresholds must be strictly ascending (and not empty)")
        if not 0.0 <= dtc <= 1.0 or not 0.0 <= gtc <= 1.0:
            raise ValueError("GroundingEvaluator: dtc and gtc must be between 0 and 1")
        if not time_resolution > 0:
            raise ValueError("GroundingEvaluator: time_resolution must be positive")
        self.thresholds = th
        self.window_size, self.time_resolution = int(window_size), float(time_resolution)
        self.n_connect = eval_util.n_connect_for(self.time_resolution)
        self.dtc, self.gtc = float(dtc), float(gtc)
        self.device = torch.device(device)
        self._th = torch.as_tensor(th).to(self.device)
        self.counts = torch.zeros(th.size, 6, device=self.device, dtype=torch.int64)

    def reset(self):
        self.counts.zero_()

    def update(self, frame_sim: torch.Tensor, gt, gt_count):
        """frame_sim (B, T) float32 on the device; gt, gt_count as ``ground_truth_arrays`` returns them (host arrays are
        checked here and copied over; device tensors are taken as they are).  No host read."""
        gt, gt_count = torch.as_tensor(gt), torch.as_tensor(gt_count)
        if not gt_count.is_cuda and gt_count.numel() and (int(gt_count.min()) < 0 or int(gt_count.max()) > gt.shape[1]):
            raise ValueError(f"gt_count must lie in [0, {gt.shape[1]}]")
        gt_count = gt_count.to(self.device)
        regions, counts = ops.segments(frame_sim, self._th, self.window_size, self.n_connect)
        out = ops.grounding_counts(regions, counts, gt, gt_count, self.time_resolution, self.dtc, self.gtc, check=False)
        self.counts[:, :4] += out.sum(0)
        self.counts[:, 4] += counts.sum(0)
        self.counts[:, 5] += gt_count.sum()

    def compute(self, total_duration_s: float, max_efpr: Optional[float] = None, beta: float = 1.0, min_threshold: float = 0.0,
                max_threshold: float = 1.0) -> dict:
        """ONE host read of ``counts`` -> {"th_auc", "psds", "precision" (NT), "recall" (NT), "thresholds"}: the expressions of
        ``evaluate_detections``, ``GroundingPrecisionRecall.th_auc``, ``psds_operating_point`` and ``psds_intersection`` on the
        summed integers.  total_duration_s: seconds of audio of the evaluated files (the PSDS metadata)."""
        rows = self.counts.cpu().tolist()
        ev = GroundingPrecisionRecall(self.dtc, self.gtc, {})
        points = []
        for th, (tp_preds, tp_refs, psds_tp, psds_fp, n_preds, n_refs) in zip(self.thresholds, rows):
            ev.operating_points.append({"precision": tp_preds / max(n_preds, EPS), "recall": tp_refs / max(n_refs, EPS),
                                        "threshold": float(th)})
            points.append((psds_tp / max(n_refs, EPS), psds_fp / (total_duration_s / 3600.0)))
        x, y = psd_roc(points)
        if max_efpr is None:
            max_efpr = float(x.max())
        psds = float(y.max()) if max_efpr <= 0 else staircase_auc(x, y, max_efpr) / max_efpr
        return {"th_auc": ev.th_auc(beta=beta, low_th=min_threshold, high_th=max_threshold), "psds": psds,
                "precision": np.array([r["precision"] for r in ev.operating_points]),
                "recall": np.array([r["recall"] for r in ev.operating_points]), "thresholds": self.thresholds.copy()}


def best_tp_per_fp(counts: torch.Tensor) -> torch.Tensor:
    """Operating-point counts (P, 2) int64 [psds_tp, psds_fp] on the device -> (U, 2) [the largest psds_tp, psds_fp] per
    distinct psds_fp, ascending.  ``psd_roc`` keeps the best TP ratio at equal eFPR anyway, so its staircase is the same."""
    fp, inverse = torch.unique(counts[:, 1], return_inverse=True)
    best_tp = torch.full_like(fp, -1).scatter_reduce_(0, inverse, counts[:, 0], "amax")
    return torch.stack([best_tp, fp], 1)


class ScorePsdsEvaluator:
    """Score-based PSDS (the reference's ``compute_psds_sed_scores``; utils/psds_scores.py is the definition and the yardstick)
    over batches on the device: every distinct frame score of the evaluation is a decision threshold, no median filter and no
    connect step.

    ``update`` runs ``ops.psds_score_deltas`` (csrc/psds_scores.hip), which leaves per pair the sorted distinct scores and the
    change of (psds_tp, psds_fp) at each of them, and keeps the batch's tensors on the device: 12 bytes per evaluated frame
    (4 for the value, 8 for the two int32 deltas) plus 4 per pair, until ``reset``.  ``compute`` merges them there --
    ``psds_scores.points_from_deltas``: sort by value, prefix sum, the last entry of each run of equal values -- and keeps the
    best TP count per distinct FP count, which is all ``psd_roc`` looks at.  The host functions stay the yardstick: the score
    equals ``psds_scores.psds_from_scores`` over a table that holds every pair once, as a float.

    A data-parallel caller gathers ``state()`` of every rank before ``compute`` (not done here).
    """

    def __init__(self, time_resolution: float, dtc: float = 0.5, gtc: float = 0.5, device="cuda"):
        if not 0.0 <= dtc <= 1.0 or not 0.0 <= gtc <= 1.0:
            raise ValueError("ScorePsdsEvaluator: dtc and gtc must be between 0 and 1")
        if time_resolution is None or not time_resolution > 0:
            raise ValueError("ScorePsdsEvaluator: time_resolution must be positive")
        self.time_resolution, self.dtc, self.gtc = float(time_resolution), float(dtc), float(gtc)
        self.device = torch.device(device)
        self.reset()

    def reset(self):
        self._values, self._deltas, self._n_values = [], [], []
        self.base = torch.zeros(2, device=self.device, dtype=torch.int64)       # sum of the pairs' c_0
        self.n_refs = torch.zeros((), device=self.device, dtype=torch.int64)
        self.bytes_read = 0                                                      # size of the tensor the last compute read

    def update(self, frame_sim: torch.Tensor, gt, gt_count):
        """frame_sim (B, T) float32 on the device (B and T may differ between batches); gt, gt_count as
        ``ground_truth_arrays`` returns them (host arrays are checked here and copied over; device tensors are taken as they
        are).  One kernel launch, no host read."""
        gt, gt_count = torch.as_tensor(gt), torch.as_tensor(gt_count)
        if not gt_count.is_cuda and gt_count.numel() and (int(gt_count.min()) < 0 or int(gt_count.max()) > gt.shape[1]):
            raise ValueError(f"gt_count must lie in [0, {gt.shape[1]}]")
        gt_count = gt_count.to(self.device)
        values, deltas, base, n_values = ops.psds_score_deltas(frame_sim, gt, gt_count, self.time_resolution, self.dtc, self.gtc,
                                                               check=False)
        self._values.append(values)
        self._deltas.append(deltas)
        self._n_values.append(n_values)
        self.base += base.sum(0)
        self.n_refs += gt_count.sum()

    def state(self) -> dict:
        """The held tensors: per batch ``values`` (B,T) fp32, ``deltas`` (B,T,2) int32 and ``n_values`` (B,) int32 (the entries
        j < n_values[b] of a row count), and the running sums ``base`` (2,) and ``n_refs`` () int64."""
        return {"values": list(self._values), "deltas": list(self._deltas), "n_values": list(self._n_values),
                "base": self.base, "n_refs": self.n_refs}

    def compute(self, total_duration_s: float, max_efpr=None) -> dict:
        """{"psds": float, or {max_efpr: float} for a sequence, "efpr", "etpr" (the PSD-ROC staircase), "n_refs",
        "n_operating_points" (1 + the distinct scores)}.  max_efpr per hour; None: the largest eFPR; <= 0: the largest eTPR.
        total_duration_s: seconds of audio of the evaluated files (the PSDS metadata).

        The merge runs on the device.  Host reads: the sizes of three data-dependent selections (the entries in use, the
        operating points, the distinct FP counts) and ONE (U + 1, 2) int64 tensor, U = the distinct FP counts among the
        operating points -- 16 (U + 1) bytes; nothing proportional to the number of frames."""
        from . import psds_scores
        if self._values:
            used = torch.cat([(torch.arange(v.shape[1], device=v.device) < n[:, None]).reshape(-1)
                              for v, n in zip(self._values, self._n_values)])
            values = torch.cat([v.reshape(-1) for v in self._values])[used]
            deltas = torch.cat([d.reshape(-1, 2) for d in self._deltas])[used]
        else:
            values = torch.zeros(0, device=self.device, dtype=torch.float32)
            deltas = torch.zeros(0, 2, device=self.device, dtype=torch.int32)
        thresholds, counts = psds_scores.points_from_deltas(values, deltas, self.base)
        head = torch.stack([self.n_refs, torch.full_like(self.n_refs, thresholds.numel())])
        table = torch.cat([head[None, :], best_tp_per_fp(counts)]).cpu().numpy()
        self.bytes_read = int(table.nbytes)
        n_refs, n_points = int(table[0, 0]), int(table[0, 1])
        psds, efpr, etpr = psds_scores.psds_from_counts(table[1:], n_refs, float(total_duration_s), max_efpr)
        return {"psds": psds, "efpr": efpr, "etpr": etpr, "n_refs": n_refs, "n_operating_points": n_points}


class SedEvaluator:
    """Accumulates the sed_eval protocol (event-based and segment-based F-score / error rate, utils/sed_metrics.py) over
    batches on the device, for a row of operating points.

    Exactly one of ``thresholds`` (strictly ascending; binarize -> median filter of ``window_size`` -> connect, ``ops.segments``)
    and ``double_thresholds`` (a sequence of ``(high, low)`` pairs, high >= low; ``ops.segments_double``, which takes no median
    filter: ``window_size`` is not used) says how frame scores become detections.  ``n_connect`` defaults to
    ``eval_util.n_connect_for(time_resolution)``.

    ``counts`` is an (NT, 7) int64 device tensor: ev_tp, seg_tp, seg_fp, seg_fn, seg_n, n_sys, n_ref per operating point,
    summed over every pair passed to ``update`` (a data-parallel caller all-reduces it, and ``overflow``, before ``compute``).
    A pair is one file of the host tables, so the sums are ``sed_metrics.count_tables`` of a table that holds every pair once.
    """

    def __init__(self, thresholds=None, double_thresholds=None, window_size: int = 1, time_resolution: float = None,
                 t_collar: float = 0.2, percentage_of_length: float = 0.2, segment_resolution: float = 1.0, n_connect=None,
                 device="cuda"):
        if (thresholds is None) == (double_thresholds is None):
            raise ValueError("SedEvaluator: give exactly one of thresholds and double_thresholds")
        if time_resolution is None or not time_resolution > 0:
            raise ValueError("SedEvaluator: time_resolution (seconds per frame) must be given and positive")
        if not segment_resolution > 0 or not t_collar >= 0 or not percentage_of_length >= 0:
            raise ValueError("SedEvaluator: segment_resolution must be positive, t_collar and percentage_of_length not negative")
        self.device = torch.device(device)
        if thresholds is not None:
            th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
            if th.size == 0 or not np.all(np.diff(th) > 0):
                raise ValueError("SedEvaluator: thresholds must be strictly ascending (and not empty)")
            self.thresholds, self.double_thresholds = th, None
            self._th = torch.as_tensor(th).to(self.device)
        else:
            pairs = np.asarray(double_thresholds, dtype=np.float64)
            if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] == 0 or not np.all(pairs[:, 0] >= pairs[:, 1]):
                raise ValueError("SedEvaluator: double_thresholds must be (high, low) pairs with high >= low (and not empty)")
            self.thresholds, self.double_thresholds = None, pairs
            self._high = torch.as_tensor(np.ascontiguousarray(pairs[:, 0])).to(self.device)
            self._low = torch.as_tensor(np.ascontiguousarray(pairs[:, 1])).to(self.device)
        self.window_size, self.time_resolution = int(window_size), float(time_resolution)
        self.n_connect = eval_util.n_connect_for(self.time_resolution) if n_connect is None else int(n_connect)
        self.t_collar, self.percentage_of_length = float(t_collar), float(percentage_of_length)
        self.segment_resolution = float(segment_resolution)
        n_points = len(self.thresholds if self.thresholds is not None else self.double_thresholds)
        self.counts = torch.zeros(n_points, 7, device=self.device, dtype=torch.int64)
        self.overflow = torch.zeros((), device=self.device, dtype=torch.int64)     # pairs above ops.SED_MAX_SEGMENTS segments

    def reset(self):
        self.counts.zero_()
        self.overflow.zero_()

    def update(self, frame_sim: torch.Tensor, gt, gt_count):
        """frame_sim (B, T) float32 on the device; gt, gt_count as ``ground_truth_arrays`` returns them (host arrays are
        checked here and copied over; device tensors are taken as they are).  No host read."""
        gt, gt_count = torch.as_tensor(gt), torch.as_tensor(gt_count)
        if not gt_count.is_cuda and gt_count.numel() and (int(gt_count.min()) < 0 or int(gt_count.max()) > gt.shape[1]):
            raise ValueError(f"gt_count must lie in [0, {gt.shape[1]}]")
        gt_count = gt_count.to(self.device)
        if self.thresholds is not None:
            regions, counts = ops.segments(frame_sim, self._th, self.window_size, self.n_connect)
        else:
            regions, counts = ops.segments_double(frame_sim, self._high, self._low, self.n_connect)
        out = ops.sed_counts(regions, counts, gt, gt_count, self.time_resolution, self.t_collar, self.percentage_of_length,
                             self.segment_resolution, check=False)
        self.overflow += (out[..., 4] < 0).sum()
        self.counts[:, :5] += out.sum(0)
        self.counts[:, 5] += counts.sum(0)
        self.counts[:, 6] += gt_count.sum()

    def compute(self) -> dict:
        """ONE host read of ``counts`` (and ``overflow``) -> ``sed_metrics.scores_from_counts`` with one entry per operating
        point: {"event": {...}, "segment": {...}, "counts" (NT, 7) int64, "thresholds" or "double_thresholds"}."""
        from . import sed_metrics
        flat = torch.cat([self.counts.reshape(-1), self.overflow.reshape(1)]).cpu().numpy()
        if flat[-1] != 0:
            raise RuntimeError(f"SedEvaluator: segment_resolution = {self.segment_resolution} cut {int(flat[-1])} (pair, operating "
                               f"point) entries into more than {ops.SED_MAX_SEGMENTS} segments; their counts were not taken")
        counts = flat[:-1].reshape(-1, 7)
        ev_tp, seg_tp, seg_fp, seg_fn, seg_n, n_sys, n_ref = counts.T
        out = sed_metrics.scores_from_counts(ev_tp, n_sys, n_ref, seg_tp, seg_fp, seg_fn, seg_n)
        out["counts"] = counts
        if self.thresholds is not None:
            out["thresholds"] = self.thresholds.copy()
        else:
            out["double_thresholds"] = self.double_thresholds.copy()
        return out
