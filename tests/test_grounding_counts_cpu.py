"""CPU: the scalar restatement of the operating-point counts (tests/grounding_eval_ref.py, the reference of the device kernel)
against the host functions of utils/grounding_eval.py, which stay the yardstick; and the host layer of utils/device_eval.py."""
import numpy as np
import pytest

from tests import grounding_eval_ref as R
from texttoaudiogrounding_amd.utils import eval_util as EU
from texttoaudiogrounding_amd.utils import grounding_eval as GE

RES = 0.04
TH = EU.eval_thresholds(50)
SETS = [(3, 63), (9, 250), (12, 250), (17, 63), (17, 250)]          # (Gmax, T): Gmax 3, 9, 12, 17 and T 63, 250
_cache = {}


def built_set(gmax, T):
    """(names, ground-truth table, durations, per-clip ground truths, segments) of one seeded set, built once."""
    key = (gmax, T)
    if key not in _cache:
        B = 10
        scores = R.build_scores(B, T, seed=17 + gmax)
        items = R.build_ground_truth(B, gmax, T, RES, seed=5 + T + gmax)
        names = [f"clip{i}_0" for i in range(B)]
        gt = {n: np.array(rows, dtype=np.float64).reshape(-1, 2) for n, rows in zip(names, items)}
        segments = R.cpu_segments(scores, TH, 1, EU.n_connect_for(RES))
        _cache[key] = (names, gt, {n: T * RES for n in names}, items, segments)
    return _cache[key]


def summed_counts(items, segments, dtc=0.5, gtc=0.5):
    """(NT, 6) integers: the four counts of the restatement summed over the clips, n_preds, n_refs."""
    out = np.zeros((len(TH), 6), dtype=np.int64)
    for rows, per_th in zip(items, segments):
        for t, seg in enumerate(per_th):
            out[t, :4] += R.pair_counts(np.asarray(seg, dtype=np.float64) * RES, rows, dtc, gtc)
            out[t, 4] += len(seg)
            out[t, 5] += len(rows)
    return out


@pytest.mark.parametrize("gmax,T", SETS)
def test_restatement_equals_host_functions_on_every_operating_point(gmax, T):
    names, gt, dur, items, segments = built_set(gmax, T)
    assert min(len(r) for r in items) == 0 and max(len(r) for r in items) == gmax
    assert any(on == off for rows in items for on, off in rows) or gmax < 9          # a zero-duration row in the larger sets
    tables = GE.tables_from_segments(segments, names, TH, RES)
    total = float(sum(dur.values()))
    counts = summed_counts(items, segments)
    assert counts[:, 4].max() > 0 and counts[:, :4].max() > 0
    for t, th in enumerate(TH):
        tp_preds, tp_refs, psds_tp, psds_fp, n_preds, n_refs = (int(v) for v in counts[t])
        precision, recall = GE.evaluate_detections(tables[float(th)], gt, 0.5, 0.5)
        tpr, fph = GE.psds_operating_point(tables[float(th)], gt, total, 0.5, 0.5)
        assert tp_preds / max(n_preds, GE.EPS) == precision and tp_refs / max(n_refs, GE.EPS) == recall, (th, counts[t])
        assert psds_tp / max(n_refs, GE.EPS) == tpr and psds_fp / (total / 3600.0) == fph, (th, counts[t])


@pytest.mark.parametrize("dtc,gtc", [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.5, 1.0)])
def test_restatement_at_the_ends_of_the_criteria(dtc, gtc):
    names, gt, dur, items, segments = built_set(9, 250)
    tables = GE.tables_from_segments(segments, names, TH, RES)
    counts = summed_counts(items, segments, dtc, gtc)
    for t, th in enumerate(TH):
        tp_preds, tp_refs, psds_tp, psds_fp, n_preds, n_refs = (int(v) for v in counts[t])
        assert (tp_preds / max(n_preds, GE.EPS), tp_refs / max(n_refs, GE.EPS)) == GE.evaluate_detections(tables[float(th)], gt, dtc, gtc)
        assert (psds_tp / max(n_refs, GE.EPS), psds_fp / 0.5) == GE.psds_operating_point(tables[float(th)], gt, 1800.0, dtc, gtc)


@pytest.mark.parametrize("D,G", [(1, 1), (9, 1), (65, 1), (125, 1), (300, 1), (125, 2), (65, 7), (65, 8), (40, 9), (20, 17),
                                 (12, 64), (9, 65), (7, 128)])
def test_restatement_on_hand_built_regions(D, G):
    """More detections than a wave has lanes, both of numpy's orders for either axis (a single ground truth makes the sum over
    the detections a contiguous one: pairwise, and recursive above 128 terms), ground truths up to the kernel's limit."""
    regions, counts = R.hand_regions(2, 3, D, D + 3, seed=D + G)
    gt, gt_count = R.grid_ground_truth(2, G, G + 2, int(regions[0, 0, D - 1, 1]), RES, seed=D * 7 + G)
    for b in range(2):
        table_gt = {"f": gt[b, :G]}
        for t in range(3):
            det = regions[b, t, :D].astype(np.float64) * RES
            tp_preds, tp_refs, psds_tp, psds_fp = R.pair_counts(det, gt[b, :G])
            assert (tp_preds / D, tp_refs / G) == GE.evaluate_detections({"f": det}, table_gt, 0.5, 0.5)
            assert (psds_tp / G, psds_fp / 1.0) == GE.psds_operating_point({"f": det}, table_gt, 3600.0, 0.5, 0.5)


def test_tie_prone_cases_and_that_the_order_of_the_sums_decides_them():
    """Pieces that fill exactly half of a span: the ratio sum is 1/2 up to rounding.  The restatement equals the host functions on
    every case, and each of its three orders is needed: with another order some case comes out differently."""
    cases = R.tie_cases()
    other = {"col1": dict(col_sum=R._seq_sum), "col2": dict(col_sum=R.np_sum), "row": dict(row_sum=R._seq_sum)}
    differ = dict.fromkeys(other, 0)
    for det, gt in cases:
        kind = "row" if len(det) == 1 else "col1" if len(gt) == 1 else "col2"
        seconds = det.astype(np.float64) * RES
        tp_preds, tp_refs, psds_tp, psds_fp = got = R.pair_counts(seconds, gt)
        assert (tp_preds / len(det), tp_refs / len(gt)) == GE.evaluate_detections({"f": seconds}, {"f": gt}, 0.5, 0.5)
        assert (psds_tp / len(gt), psds_fp / 1.0) == GE.psds_operating_point({"f": seconds}, {"f": gt}, 3600.0, 0.5, 0.5)
        differ[kind] += R.pair_counts(seconds, gt, **other[kind]) != got
    assert all(n > 0 for n in differ.values()), differ


def test_single_ground_truth_column_sum_is_not_left_to_right():
    """Why the rule has its G == 1 clause: numpy sums a (D, 1) array pairwise, and that differs from the running sum."""
    rng = np.random.default_rng(0)
    a = rng.random((125, 1))
    running = 0.0
    for v in a[:, 0]:
        running = running + float(v)
    assert float(a.sum(0)[0]) == R.np_sum([float(v) for v in a[:, 0]]) != running
    b = rng.random((125, 2))
    running = 0.0
    for v in b[:, 1]:
        running = running + float(v)
    assert float(b.sum(0)[1]) == running


def test_no_detections_and_no_ground_truths():
    assert R.pair_counts(np.zeros((0, 2)), [[1.0, 2.0]]) == (0, 0, 0, 0)
    assert R.pair_counts([[0.04, 0.4], [1.0, 1.2]], []) == (0, 0, 0, 2)
    assert R.pair_counts([[0.0, 1.0]], [[0.5, 0.5]]) == (0, 0, 0, 1)                   # zero-duration row: NaN compares false


def test_plain_per_threshold_evaluation_equals_compute_th_auc():
    """The quirk of add_operating_point (a copy of the LAST row for a table seen before) is value-neutral for ascending
    thresholds: th-AUC from one evaluation per threshold equals compute_th_auc, on a set with fewer distinct tables than
    thresholds."""
    fewer = False
    for gmax, T in SETS:
        names, gt, dur, items, segments = built_set(gmax, T)
        tables = GE.tables_from_segments(segments, names, TH, RES)
        distinct = len({GE._table_key(t) for t in tables.values()})
        fewer |= distinct < len(TH)
        ev = GE.GroundingPrecisionRecall(0.5, 0.5, gt)
        for th, det in tables.items():
            p, r = GE.evaluate_detections(det, gt, 0.5, 0.5)
            ev.operating_points.append({"precision": p, "recall": r, "threshold": th})
        assert ev.th_auc() == GE.compute_th_auc(tables, gt)
    assert fewer


def test_ground_truth_arrays():
    from texttoaudiogrounding_amd.utils.device_eval import ground_truth_arrays
    gt, n = ground_truth_arrays([[[0, 0], [1.5, 2.0], [0.0, 0.0], [3, 4]], [], [[0.5, 0.5]], [[0, 0]]])
    assert gt.dtype == np.float64 and gt.shape == (4, 2, 2) and n.dtype == np.int32 and n.tolist() == [2, 0, 1, 0]
    assert gt[0].tolist() == [[1.5, 2.0], [3.0, 4.0]] and gt[2].tolist() == [[0.5, 0.5], [0.0, 0.0]] and not gt[1].any()
    gt, n = ground_truth_arrays([[], []])
    assert gt.shape == (2, 0, 2) and n.tolist() == [0, 0]
    rows = [[0.1 * i, 0.1 * i + 0.05] for i in range(1, 130)]
    assert ground_truth_arrays([rows[:128]])[1].tolist() == [128]
    with pytest.raises(ValueError, match="at most 128"):
        ground_truth_arrays([rows])


def test_evaluator_refuses_unsorted_thresholds():
    from texttoaudiogrounding_amd.utils.device_eval import GroundingEvaluator
    for th in ([0.5, 0.3], [0.1, 0.1, 0.2], []):
        with pytest.raises(ValueError, match="strictly ascending"):
            GroundingEvaluator(th, 1, RES, device="cpu")
