"""GPU: ops.grounding_counts (csrc/grounding_eval.hip) against the scalar restatement of tests/grounding_eval_ref.py, entry by
entry; GroundingEvaluator and StrongRunner.evaluate against the host path (segments_for_thresholds -> tables_from_segments ->
compute_th_auc / psds_intersection) over the same scores, as floats."""
import numpy as np
import pytest
import torch

from tests import grounding_eval_ref as R
from texttoaudiogrounding_amd.utils import eval_util as EU
from texttoaudiogrounding_amd.utils import grounding_eval as GE

pytestmark = pytest.mark.gpu
RES = 0.04


def device_counts(dev, regions, counts, gt, gt_count, res=RES, dtc=0.5, gtc=0.5, **kw):
    from texttoaudiogrounding_amd import ops
    return ops.grounding_counts(torch.as_tensor(regions).to(dev), torch.as_tensor(counts).to(dev), torch.as_tensor(gt).to(dev),
                                torch.as_tensor(gt_count).to(dev), res, dtc, gtc, **kw).cpu()


def check(dev, regions, counts, gt, gt_count, dtc=0.5, gtc=0.5, what=""):
    got = device_counts(dev, regions, counts, gt, gt_count, RES, dtc, gtc)
    want = R.counts_ref(regions, counts, gt, gt_count, RES, dtc, gtc)
    assert got.dtype == torch.int32 and torch.equal(got, want), (what, (got != want).nonzero()[:8].tolist())
    return got


@pytest.mark.parametrize("D,max_regions", [(0, 4), (1, 1), (1, 9), (65, 125), (125, 125), (300, 301)])
def test_hand_built_regions(dev, D, max_regions):
    """No detection, one, more detections than lanes, max_regions larger than needed with garbage beyond the counts, and more
    than 128 detections (beside a single ground truth the sum over them is numpy's recursive pairwise one)."""
    regions, counts = R.hand_regions(3, 2, D, max_regions, seed=D)
    span = int(regions[0, 0, D - 1, 1]) if D else 40
    gt, gt_count = R.grid_ground_truth(3, [1, 2, 5], 7, span, RES, seed=D + 1)
    got = check(dev, regions, counts, gt, gt_count)
    assert D == 0 or got.sum() > 0


@pytest.mark.parametrize("G", [0, 1, 7, 8, 9, 16, 17, 64, 65, 128])
def test_ground_truth_counts(dev, G):
    """Both of numpy's orders, the remainder, more ground truths than lanes; max_gt above every gt_count (up to the limit of
    128, where only the second clip's 127 rows leave padding), garbage in the padding."""
    mixed = np.array([[3, 40, 9], [12, 1, 0]], dtype=np.int32)
    regions, counts = R.hand_regions(2, 3, mixed, 40, seed=G)
    gt, gt_count = R.grid_ground_truth(2, [G, max(G - 1, 0)], min(G + 3, 128), 150, RES, seed=G + 11)
    got = check(dev, regions, counts, gt, gt_count)
    assert got[1, 2].tolist() == [0, 0, 0, 0] and (G > 0 or got[0, :, 3].tolist() == [3, 40, 9])


@pytest.mark.parametrize("B,NT", [(1, 1), (3, 2), (5, 7), (64, 50)])
def test_batch_and_threshold_counts_from_scores(dev, B, NT):
    """Scores -> ops.segments -> ops.grounding_counts, ground truths of the three kinds (on the grid, off it, zero duration)."""
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils.device_eval import ground_truth_arrays
    T = 250
    th = EU.eval_thresholds(NT)
    regions, counts = ops.segments(R.build_scores(B, T, seed=B).to(dev), th, 1, EU.n_connect_for(RES))
    gt, gt_count = ground_truth_arrays(R.build_ground_truth(B, 5, T, RES, seed=NT))
    got = ops.grounding_counts(regions, counts, gt, gt_count, RES).cpu()
    assert torch.equal(got, R.counts_ref(regions.cpu().numpy(), counts.cpu().numpy(), gt, gt_count, RES))


@pytest.mark.parametrize("T", [1, 2])
def test_shortest_clips(dev, T):
    from texttoaudiogrounding_amd import ops
    scores = torch.tensor([[0.9, 0.2][:T], [0.1, 0.8][:T], [0.6, 0.7][:T]])
    regions, counts = ops.segments(scores.to(dev), [0.05, 0.5, 0.95], 1, EU.n_connect_for(RES))
    assert regions.shape[2] == 1
    gt = np.array([[[0.0, 0.04]], [[0.04, 0.08]], [[0.0, 0.02]]])
    gt_count = np.array([1, 1, 1], dtype=np.int32)
    got = ops.grounding_counts(regions, counts, gt, gt_count, RES).cpu()
    assert torch.equal(got, R.counts_ref(regions.cpu().numpy(), counts.cpu().numpy(), gt, gt_count, RES)) and got.sum() > 0


@pytest.mark.parametrize("dtc,gtc", [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (0.5, 0.5), (0.5, 1.0)])
def test_tie_prone_cases_and_criteria(dev, dtc, gtc):
    """Pieces filling exactly half of a span (the order of the additions decides the comparison, test_grounding_counts_cpu shows
    it) and the grid sets with a zero-duration row, at the ends and the middle of both criteria."""
    check(dev, *R.pack_cases(R.tie_cases()), dtc=dtc, gtc=gtc, what="ties")
    T = 250
    items = R.build_ground_truth(6, 9, T, RES, seed=3)
    assert any(on == off for rows in items for on, off in rows)
    regions, counts = R.pack_segments(R.cpu_segments(R.build_scores(6, T, seed=2), EU.eval_thresholds(10), 1, 13), 125)
    gt = np.full((6, 10, 2), 7.0e9)
    for b, rows in enumerate(items):
        gt[b, :len(rows)] = np.array(rows).reshape(-1, 2)
    check(dev, regions, counts, gt, np.array([len(r) for r in items], dtype=np.int32), dtc=dtc, gtc=gtc, what="grid")


def test_every_entry_is_written(dev):
    mixed = np.array([[0, 5], [7, 0], [2, 3]], dtype=np.int32)
    regions, counts = R.hand_regions(3, 2, mixed, 8)
    gt, gt_count = R.grid_ground_truth(3, [2, 0, 3], 4, 30, RES)
    out = torch.full((3, 2, 4), -12345, device=dev, dtype=torch.int32)
    got = device_counts(dev, regions, counts, gt, gt_count, out=out)
    assert (out.cpu() >= 0).all() and torch.equal(got, out.cpu()) and torch.equal(got, R.counts_ref(regions, counts, gt, gt_count, RES))


def test_argument_checks(dev):
    regions, counts = R.hand_regions(2, 2, 3, 4)
    gt, gt_count = R.grid_ground_truth(2, 2, 3, 30, RES)
    with pytest.raises(RuntimeError, match="max_gt"):
        device_counts(dev, regions, counts, np.zeros((2, 129, 2)), gt_count)
    with pytest.raises(RuntimeError, match="gt_count"):
        device_counts(dev, regions, counts, gt, np.array([2, 4], dtype=np.int32))
    with pytest.raises(RuntimeError, match="gt_count"):                                  # (a host gt_count as well)
        from texttoaudiogrounding_amd import ops
        ops.grounding_counts(torch.as_tensor(regions).to(dev), torch.as_tensor(counts).to(dev), gt, np.array([-1, 1], dtype=np.int32), RES)
    with pytest.raises(RuntimeError, match="counts"):
        device_counts(dev, regions, np.array([[3, 5], [0, 1]], dtype=np.int32), gt, gt_count)
    with pytest.raises(RuntimeError, match="time_resolution"):
        device_counts(dev, regions, counts, gt, gt_count, res=-0.04)
    with pytest.raises(RuntimeError, match="dtc"):
        device_counts(dev, regions, counts, gt, gt_count, dtc=1.5)
    # what the wrapper refuses the kernel clamps: nothing is read out of bounds, and the run is that of the clamped counts
    got = device_counts(dev, regions, np.array([[3, 9], [3, 3]], dtype=np.int32), gt, np.array([2, 7], dtype=np.int32), check=False)
    clamped = np.array([[3, 4], [3, 3]], dtype=np.int32)
    assert torch.equal(got, R.counts_ref(regions, clamped, gt, np.array([2, 3], dtype=np.int32), RES))


def host_metrics(scores_dev, names, gt_table, durations, thresholds, window, max_efpr):
    segments = EU.segments_for_thresholds(scores_dev, thresholds, window, EU.n_connect_for(RES))
    tables = GE.tables_from_segments(segments, names, thresholds, RES)
    ev = GE.GroundingPrecisionRecall(0.5, 0.5, gt_table)
    for th, det in tables.items():
        ev.add_operating_point(det, th)
    return (GE.compute_th_auc(tables, gt_table), GE.psds_intersection(tables, gt_table, durations, max_efpr=max_efpr),
            np.array([r["precision"] for r in ev.operating_points]), np.array([r["recall"] for r in ev.operating_points]))


@pytest.mark.parametrize("max_efpr", [None, 800.0])
def test_evaluator_over_unequal_batches_equals_the_host_path(dev, max_efpr):
    from texttoaudiogrounding_amd.utils.device_eval import GroundingEvaluator, ground_truth_arrays
    T, th = 250, EU.eval_thresholds(50)
    sizes = [7, 12, 3]
    scores = R.build_scores(sum(sizes), T, seed=23)
    items = [rows or [[1.0, 2.5]] for rows in R.build_ground_truth(sum(sizes), 6, T, RES, seed=29)]
    names = [f"clip{i}_0" for i in range(sum(sizes))]
    gt_table = {n: np.array(rows).reshape(-1, 2) for n, rows in zip(names, items)}
    durations = {n: T * RES for n in names}
    ev = GroundingEvaluator(th, 1, RES, device=dev)
    at = 0
    for n in sizes:
        ev.update(scores[at:at + n].to(dev), *ground_truth_arrays(items[at:at + n]))
        at += n
    assert ev.counts.shape == (50, 6) and ev.counts.dtype == torch.int64 and ev.counts.is_cuda
    got = ev.compute(float(sum(durations.values())), max_efpr=max_efpr)
    auc, psds, precision, recall = host_metrics(scores.to(dev), names, gt_table, durations, th, 1, max_efpr)
    print(f"th_auc {got['th_auc']:.6f} (host {auc:.6f}); psds {got['psds']:.6f} (host {psds:.6f})")
    assert got["th_auc"] == auc and got["psds"] == psds and 0.0 < auc < 1.0 and 0.0 < psds <= 1.0
    assert np.array_equal(got["precision"], precision) and np.array_equal(got["recall"], recall)
    assert np.array_equal(got["thresholds"], th)


def test_runner_evaluate_equals_the_host_path(dev):
    """StrongRunner.evaluate on a small BiEncoder, two batches, one pair without ground truth: th-AUC and PSDS equal to the host
    path over the same frame_sim with that pair left out."""
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import StrongRunner
    torch.manual_seed(5)
    model = audio_text_model.BiEncoder(audio_encoder.CrnnEncoder(32000, 256), text_encoder.EmbeddingAgg(5221, 256),
                                       match.DotProduct(), 256)
    with torch.no_grad():                                   # freshly initialised, the scores stay within 0.01 of 0.5: widen the logits
        for p in model.text_encoder.parameters():
            p.mul_(60.0)
    runner = StrongRunner(model, device=str(dev))
    g = torch.Generator().manual_seed(6)

    def batch(n, first):
        return {"waveform": 0.1 * torch.randn(n, 64000, generator=g), "waveform_len": np.full(n, 64000),
                "text": torch.randint(2, 5221, (n, 3), generator=g), "text_len": np.full(n, 3),
                "audiocap_id": [100 + first + i for i in range(n)], "start_index": [i % 2 for i in range(n)]}

    batches = [batch(3, 0), batch(2, 3)]
    keys = [f"{a}_{s}" for b in batches for a, s in zip(b["audiocap_id"], b["start_index"])]
    ground_truth = {k: [[0.2 * i, 0.2 * i + 0.6], [0.0, 0.0], [1.0, 1.4]] for i, k in enumerate(keys)}
    ground_truth[keys[1]] = [[0.0, 0.0]]                                     # no row left: the pair is left out
    durations = {k: 2.0 for k in keys}
    res = runner.model.audio_encoder.time_resolution
    cfg = {"n_thresholds": 50, "window_size": 1, "time_resolution": res, "max_efpr": 800.0}
    got = runner.evaluate([dict(b) for b in batches], ground_truth, durations, cfg)

    th = EU.eval_thresholds(50)
    with torch.no_grad():
        sims = torch.cat([runner.forward(dict(b), training=False)["frame_sim"] for b in batches])
    kept = [i for i, k in enumerate(keys) if k != keys[1]]
    segments = EU.segments_for_thresholds(sims[kept].contiguous(), th, 1, EU.n_connect_for(res))
    tables = GE.tables_from_segments(segments, [keys[i] for i in kept], th, res)
    gt_table = {k: np.array([r for r in v if r != [0.0, 0.0]]).reshape(-1, 2) for k, v in ground_truth.items()}
    auc = GE.compute_th_auc(tables, gt_table)
    psds = GE.psds_intersection(tables, gt_table, durations, max_efpr=800.0)
    print(f"evaluate: th_auc {got['th_auc']:.6f} (host {auc:.6f}); psds {got['psds']:.6f} (host {psds:.6f}); "
          f"score range {float(sims.min()):.3f} .. {float(sims.max()):.3f}")
    assert got["th_auc"] == auc and got["psds"] == psds
    assert not runner.model.training and got["precision"].shape == (50,) and got["precision"].max() > 0
