"""CPU: the host yardstick of the sed_eval protocol (utils/sed_metrics.py) on hand-derived answers and against the naive twins
of tests/sed_eval_ref.py; the scalar double threshold against the fixture the imported reference wrote
(tests/golden/sed_double_threshold.npz), so that the GPU test's twin is itself checked; the new entry points in the header, the
signature table and the Makefile.  sed_eval / dcase_util are absent: parity with those packages is unpinned."""
import math
import os
import re

import numpy as np
import pytest

from tests import sed_eval_ref as R
from texttoaudiogrounding_amd.utils import sed_metrics as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sed_double_threshold.npz")


def math_is_inexact(res):
    """x / res is exact for a power of two; for any other resolution a boundary on a segment edge is a floating-point tie."""
    return math.frexp(res)[0] != 0.5


def ev(det, gt, t_collar=0.2, pct=0.2):
    return SM.event_based_counts(np.array(det).reshape(-1, 2), np.array(gt).reshape(-1, 2), t_collar, pct)


def seg(det, gt, res=1.0):
    return SM.segment_based_counts(np.array(det).reshape(-1, 2), np.array(gt).reshape(-1, 2), res)


def test_double_threshold_twin_equals_the_reference_fixture():
    cases = R.golden_cases(GOLDEN)
    assert len(cases) == 120 * 3 + 132 * 2 and sum(len(c[4]) for c in cases) > 500
    for x, high, low, n, want in cases:
        got = np.array(R.double_threshold_ref(x, high, low, n), dtype=np.int64).reshape(-1, 2)
        assert np.array_equal(got, want), (len(x), high, low, n, got.tolist(), want.tolist())
    # the rows the fixture was built for are in it: a frame equal to float32(0.3) is not above 0.3, and the low-only run
    # neither survives nor bridges
    x64 = [c for c in cases if len(c[0]) == 64]
    exact = next(c for c in x64 if (c[0] == np.float32(0.3)).sum() > 10 and (c[1], c[2], c[3]) == (0.3, 0.3, 0))
    assert exact[4].tolist() == [[32, 33]]
    hand = [c for c in x64 if c[0][41] == np.float32(0.4) and c[0][36] == np.float32(0.95)]
    by_key = {(c[1], c[2], c[3]): c[4].tolist() for c in hand}
    assert by_key[(0.75, 0.25, 1)] == [[5, 12], [22, 30], [36, 40], [45, 49]] and by_key[(0.75, 0.25, 13)] == [[5, 49]]
    assert by_key[(0.9, 0.1, 0)] == [[5, 12], [22, 30], [36, 40], [45, 49]] and by_key[(0.5, 0.5, 1)] == [[5, 12], [22, 33], [36, 40], [45, 49]]


def test_event_based_hand_derived():
    # the collar tie |0.4 - 0.2| <= 0.2 on the onset (0.4 - 0.2 == 0.2 in fp64), offsets equal
    assert ev([[0.4, 1.0]], [[0.2, 1.0]]) == (1, 0, 0)
    assert 0.9 - 0.7 > 0.2 and ev([[0.9, 2.0]], [[0.7, 2.0]]) == (0, 1, 1)         # ... and a "tie" that fp64 puts outside
    # a 5 s reference: the offset collar is 0.2 * 5 = 1 s, not 0.2 s
    assert ev([[1.0, 6.9]], [[1.0, 6.0]]) == (1, 0, 0) and ev([[1.0, 7.1]], [[1.0, 6.0]]) == (0, 1, 1)
    assert ev([[1.0, 6.9]], [[1.0, 6.0]], pct=0.0) == (0, 1, 1)
    # a zero-duration ground truth: the offset collar is t_collar
    assert ev([[2.0, 2.12]], [[2.04, 2.04]]) == (1, 0, 0) and ev([[2.0, 2.4]], [[2.04, 2.04]]) == (0, 1, 1)
    assert ev([], [[1.0, 2.0], [3.0, 4.0]]) == (0, 0, 2) and ev([[1.0, 2.0]], []) == (0, 1, 0) and ev([], []) == (0, 0, 0)
    # one detection cannot serve two overlapping ground truths; t_collar 0 asks for equal onsets
    assert ev([[1.0, 2.0]], [[1.0, 2.0], [1.1, 2.1]]) == (1, 0, 1)
    assert ev([[1.0, 2.0]], [[1.0, 2.0]], t_collar=0.0, pct=0.0) == (1, 0, 0)
    assert ev([[1.0, 2.04]], [[1.0, 2.0]], t_collar=0.0, pct=0.0) == (0, 1, 1)


def test_the_matching_is_maximum_not_first_fit():
    det, gt = R.GREEDY_BREAKER
    assert ev(det, gt) == (2, 0, 0)
    first_fit, used = 0, set()
    for g in gt:
        for d, e in enumerate(det):
            if d not in used and SM.can_match(e, g, 0.2, 0.2):
                used.add(d)
                first_fit += 1
                break
    assert first_fit == 1


def test_segment_based_hand_derived():
    # reference 0.5 .. 2.5 covers segments 0, 1, 2; detection 1.2 .. 1.8 covers segment 1
    assert seg([[1.2, 1.8]], [[0.5, 2.5]]) == (1, 0, 2, 3)
    # a detection running past the last reference offset pads the reference roll, and the converse
    assert seg([[0.2, 4.5]], [[0.5, 1.5]]) == (2, 3, 0, 5) and seg([[0.5, 1.5]], [[0.2, 4.5]]) == (2, 0, 3, 5)
    # offsets exactly on a segment boundary: floor for the onset, ceil for the offset, nothing of the next segment
    assert seg([[1.0, 2.0]], [[2.0, 3.0]]) == (0, 1, 1, 3) and seg([[1.0, 2.0]], [[1.0, 2.0]]) == (1, 0, 0, 2)
    assert seg([[0.5, 1.0]], [[0.5, 1.0]], res=0.5) == (1, 0, 0, 2)
    # a boundary that fp64 division moves: 0.6 / 0.2 = 2.9999999999999996, so an event from 0.6 starts in segment 2
    assert 0.6 / 0.2 < 3 and seg([[0.6, 0.8]], [], res=0.2) == (0, 2, 0, 4)
    assert seg([], [[1.0, 2.0]]) == (0, 0, 1, 2) and seg([[1.0, 2.0]], []) == (0, 1, 0, 2) and seg([], []) == (0, 0, 0, 0)
    # zero duration: inside a segment it marks it, on a boundary it marks nothing
    assert seg([], [[1.5, 1.5]]) == (0, 0, 1, 2) and seg([], [[2.0, 2.0]]) == (0, 0, 0, 2)


def test_scores_and_tables():
    s = SM.scores_from_counts(ev_tp=3, n_sys=4, n_ref=6, seg_tp=5, seg_fp=1, seg_fn=3, seg_n=12)
    e, g = s["event"], s["segment"]
    assert abs(e["precision"] - 0.75) < 1e-12 and abs(e["recall"] - 0.5) < 1e-12 and abs(e["f_measure"] - 0.6) < 1e-12
    assert abs(e["deletion_rate"] - 0.5) < 1e-12 and abs(e["insertion_rate"] - 1 / 6) < 1e-12
    assert abs(e["error_rate"] - (0.5 + 1 / 6)) < 1e-12
    assert abs(g["precision"] - 5 / 6) < 1e-12 and abs(g["recall"] - 5 / 8) < 1e-12 and abs(g["error_rate"] - 0.5) < 1e-12
    assert abs(g["accuracy"] - 8 / 12) < 1e-12
    # an empty system output scores precision 0 and F 0, an empty reference recall 0; per-operating-point arrays keep their shape
    z = SM.scores_from_counts(np.array([0, 0, 2]), np.array([0, 3, 2]), np.array([4, 0, 2]), np.zeros(3), np.zeros(3), np.zeros(3))
    assert z["event"]["precision"].tolist() == [0.0, 0.0, 1.0] and z["event"]["recall"].tolist() == [0.0, 0.0, 1.0]
    assert z["event"]["f_measure"].tolist() == [0.0, 0.0, 1.0] and z["segment"]["f_measure"].tolist() == [0.0, 0.0, 0.0]
    assert z["event"]["error_rate"][0] == 1.0 and z["event"]["insertion_rate"][1] > 1e15
    # tables: the files of the ground-truth table are evaluated; a file only the predictions name is not
    gt = {"a_0": np.array([[1.0, 2.0]]), "b_0": np.array([[0.5, 2.5], [3.0, 4.0]]), "c_0": np.array([[1.0, 1.5]])}
    pred = {"a_0": np.array([[1.1, 2.1]]), "b_0": np.array([[0.6, 2.6]]), "zzz_0": np.array([[0.0, 9.0]])}
    out = SM.compute_sed_eval(gt, pred, t_collar=0.2, time_resolution=1.0)
    # a_0: segments {1,2} vs {1}: tp 1, fp 1, n 3;  b_0: {0,1,2} vs {0,1,2,3}: tp 3, fn 1, n 4;  c_0: fn 1, n 2
    assert out["counts"].tolist() == [2, 4, 1, 2, 9, 2, 4]
    assert abs(out["event"]["f_measure"] - 2 / 3) < 1e-12 and abs(out["segment"]["f_measure"] - 8 / 11) < 1e-12


@pytest.mark.parametrize("seed", range(8))
def test_event_based_counts_equal_brute_force(seed):
    """Up to 6 x 6 events, ground truths free to overlap.  Most cases shift the ground truths by 3 ms against the detections'
    10 ms grid, so that no difference can equal a collar; one case in forty shares the grid and may tie.  The naive twin skips a
    tie; the seeds are chosen so that at most 2 % of a seed's cases are skipped (asserted)."""
    rng = np.random.default_rng(720 + seed)
    checked = skipped = 0
    for _ in range(150):
        shift = 0 if rng.integers(0, 40) == 0 else 3
        det = R.random_events(rng, int(rng.integers(0, 7)), 3000, 10)
        gt = R.random_events(rng, int(rng.integers(0, 7)), 3000, 10, shift_ms=shift, disjoint=False)
        if len(det) and rng.integers(0, 2):                         # ground truths near the detections, so that edges exist
            pick = det[rng.integers(0, len(det), size=len(gt))]
            gt = pick + (rng.integers(-30, 31, size=pick.shape) * 10 + shift) / 1000.0
            gt[:, 1] = np.maximum(gt[:, 1], gt[:, 0] + 0.01)
            gt = np.maximum(gt, 0.0)
        t_collar, pct = [(0.2, 0.2), (0.2, 0.5), (0.1, 0.0), (0.05, 1.0)][int(rng.integers(0, 4))]
        try:
            want = R.brute_force_tp(det, gt, t_collar, pct)
        except R.Tie:
            skipped += 1
            continue
        assert SM.event_based_counts(det, gt, t_collar, pct) == (want, len(det) - want, len(gt) - want), (seed, det, gt)
        checked += 1
    print(f"seed {seed}: {checked} checked, {skipped} skipped on a tie")
    assert skipped <= 0.02 * (checked + skipped)


def test_event_fuzz_is_not_degenerate():
    rng = np.random.default_rng(700)
    sizes = []
    for _ in range(150):
        det = R.random_events(rng, int(rng.integers(1, 7)), 3000, 10)
        pick = det[rng.integers(0, len(det), size=int(rng.integers(1, 7)))]
        gt = np.maximum(pick + (rng.integers(-30, 31, size=pick.shape) * 10 + 3) / 1000.0, 0.0)
        gt[:, 1] = np.maximum(gt[:, 1], gt[:, 0] + 0.01)
        sizes.append(SM.event_based_counts(det, gt, 0.2, 0.5)[0])
    assert max(sizes) >= 3 and len(set(sizes)) >= 4, sorted(set(sizes))


@pytest.mark.parametrize("seed", range(6))
def test_segment_based_counts_equal_the_millisecond_walk(seed):
    rng = np.random.default_rng(900 + seed)
    checked = skipped = 0
    for _ in range(120):
        res = [1.0, 0.5, 0.25, 0.3, 0.04][int(rng.integers(0, 5))]
        det = R.random_events(rng, int(rng.integers(0, 6)), 4000, 1)
        gt = R.random_events(rng, int(rng.integers(0, 5)), 4000, 1, disjoint=False)
        if math_is_inexact(res):                                    # move most boundaries off the segment edges
            for a in (det, gt):
                for idx in np.ndindex(a.shape):
                    if round(a[idx] * 1000) % round(res * 1000) == 0 and rng.random() > 0.02:
                        a[idx] += 0.001
            det, gt = (a[a[:, 1] - a[:, 0] > 0.0005] for a in (det, gt))
        try:
            want = R.naive_segment_counts(det, gt, res)
        except R.Tie:
            skipped += 1
            continue
        assert SM.segment_based_counts(det, gt, res) == want, (seed, res, det, gt)
        checked += 1
    print(f"seed {seed}: {checked} checked, {skipped} skipped on a tie")
    assert skipped <= 0.02 * (checked + skipped)


def test_new_entry_points_are_declared_and_the_abi_version_stays():
    from texttoaudiogrounding_amd import dispatch, lib
    header = open(os.path.join(ROOT, "include", "tag_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\btag_segments_double\s*\(", code) and re.search(r"\btag_sed_counts\s*\(", code)
    assert {"tag_segments_double", "tag_sed_counts"} <= set(lib.declared_symbols())
    assert int(re.search(r"#define TAG_ABI_VERSION (\d+)", header).group(1)) == lib.ABI_VERSION == 3
    assert int(re.search(r"#define TAG_SED_MAX_SEGMENTS (\d+)", header).group(1)) == dispatch.SED_MAX_SEGMENTS
    make = open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "Makefile")).read()
    assert "sed_eval.hip" in re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    heads = open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "heads.hip")).read()
    assert "segments_double" not in heads
    note = next(c for c in re.findall(r"/\*.*?\*/", header, flags=re.S) if "P1 with a double threshold" in c)
    assert "fp32" in note and "fp64" in note and header.index("* P1: post-processing") < header.index(note) < header.index("* O1:")


def test_wrappers_refuse_before_any_launch():
    """No GPU is touched: the library names the bad size, the wrapper the bad thresholds and a host tensor."""
    import ctypes
    import torch
    from texttoaudiogrounding_amd import lib, ops
    h = lib.load()
    a = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)
    assert h.tag_sed_counts(a, a, 4, a, a, 129, 2, 2, 0.04, 0.2, 0.2, 1.0, a, None) != 0 and b"max_gt = 129" in h.tag_last_error()
    assert h.tag_sed_counts(a, a, 4, a, a, 3, 2, 2, 0.04, 0.2, 0.2, 0.0, a, None) != 0 and b"segment_resolution" in h.tag_last_error()
    assert h.tag_sed_counts(a, a, 40000, a, a, 3, 2, 2, 0.04, 0.2, 0.2, 1.0, a, None) != 0 and b"max_regions" in h.tag_last_error()
    assert h.tag_segments_double(a, 8, 2, 9, a, a, 2, 1, a, a, 5, None) != 0 and b"ld 8" in h.tag_last_error()
    assert h.tag_segments_double(a, 9, 2, 9, a, a, 2, 1, a, a, 4, None) != 0 and b"max_regions = 4" in h.tag_last_error()
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X"):
        ops.segments_double(torch.zeros(2, 8), [0.75], [0.25])
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X"):
        ops.sed_counts(torch.zeros(1, 1, 2, 2, dtype=torch.int64), torch.zeros(1, 1, dtype=torch.int32), np.zeros((1, 1, 2)),
                       np.zeros(1, dtype=np.int32), 0.04)


def test_evaluate_sed_eval_tool_writes_both_reports(tmp_path):
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("evaluate_sed_eval_tool", os.path.join(ROOT, "tools", "evaluate_sed_eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    gt = [{"audiocap_id": "a", "phrases": [{"start_index": 0, "segments": [[1.0, 2.0], [0, 0]]},
                                            {"start_index": 3, "segments": [[0, 0]]}]},
          {"audiocap_id": "b", "phrases": [{"start_index": 0, "segments": [[0.5, 2.5], [3.0, 4.0]]}]},
          {"audiocap_id": "c", "phrases": [{"start_index": 0, "segments": [[1.0, 1.5]]}]}]
    (tmp_path / "gt.json").write_text(json.dumps(gt))
    (tmp_path / "pred.tsv").write_text("filename\tonset\toffset\tevent_label\na_0\t1.1\t2.1\tfake_event\nb_0\t0.6\t2.6\tfake_event\n"
                                       "zzz_0\t0.0\t9.0\tfake_event\na_3\t0.0\t1.0\tfake_event\n")
    tool.main([str(tmp_path / "gt.json"), str(tmp_path / "pred.tsv"), str(tmp_path / "out" / "event.txt"),
               str(tmp_path / "out" / "segment.txt"), "--t_collar", "0.2", "--time_resolution", "1.0"])
    event = dict(line.split(": ") for line in (tmp_path / "out" / "event.txt").read_text().splitlines()[1:])
    segment = dict(line.split(": ") for line in (tmp_path / "out" / "segment.txt").read_text().splitlines()[1:])
    assert (event["files"], event["n_ref"], event["n_sys"], event["tp"], event["fp"], event["fn"]) == ("3", "4", "2", "2", "0", "2")
    assert abs(float(event["f_measure"]) - 2 / 3) < 1e-6 and abs(float(event["error_rate"]) - 0.5) < 1e-6
    assert (segment["segments"], segment["tp"], segment["fp"], segment["fn"]) == ("9", "4", "1", "2")
    assert abs(float(segment["f_measure"]) - 8 / 11) < 1e-6
