"""GPU: ops.psds_score_deltas (csrc/psds_scores.hip) against the host yardstick utils/psds_scores.py pair_regimes, every output
compared for equality; ScorePsdsEvaluator and StrongRunner.evaluate_psds_scores against the brute force psds_from_scores over
the same scores, as floats."""
import functools

import numpy as np
import pytest
import torch

from tests import psds_scores_ref as R
from texttoaudiogrounding_amd.utils import psds_scores as PS

pytestmark = pytest.mark.gpu
RES = 0.04


def run(dev, scores, gt, gt_count, **kw):
    from texttoaudiogrounding_amd import ops
    return ops.psds_score_deltas(torch.as_tensor(scores).to(dev), gt, gt_count, RES, **kw)


@functools.lru_cache(maxsize=None)
def case(B, Gn, T, kind):
    """One seeded input and what pair_regimes says about it, computed once."""
    scores = R.build_scores(B, T, kind, seed=B + T)
    gt, gt_count = R.grid_ground_truth(B, Gn, T, RES, seed=Gn + T)
    return scores, gt, gt_count, R.expected_outputs(scores.numpy(), gt, gt_count, RES, PS.pair_regimes)


@pytest.mark.parametrize("kind", ["continuous", "eighths", "equal"])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 250])
@pytest.mark.parametrize("B,Gn", [(1, 1), (3, 2), (64, 4)])
def test_outputs_equal_pair_regimes(dev, B, Gn, T, kind):
    """Ground truths on the frame grid, so the ratio sums land on dtc / gtc; more than one workgroup at B = 64; T below, at
    and above a wave's chunk of 64 frames."""
    scores, gt, gt_count, want = case(B, Gn, T, kind)
    got = run(dev, scores, gt, gt_count)
    assert got[0].shape == (B, T) and got[1].shape == (B, T, 2) and got[2].shape == (B, 2) and got[3].shape == (B,)
    assert got[0].dtype == torch.float32 and all(t.dtype == torch.int32 and t.is_cuda for t in got[1:])
    assert R.same_outputs(got, want)
    m = want[3]
    assert int(m.max()) == 1 if kind == "equal" else (int(m.max()) > 1 or T < 63)
    assert kind != "eighths" or T < 63 or int(m.max()) < T // 2        # equal values inside the rows
    # the deltas of a pair add up to minus its base: the last regime counts nothing
    assert torch.equal(got[1].sum(1).cpu(), -want[2])


def test_one_ground_truth_and_more_than_eight_detections(dev):
    """Alternating rows of T = 40: up to 20 one-frame detections against ONE ground truth, whose coverage sum numpy forms
    pairwise, not left to right; the spans are chosen so that the sum sits at gtc."""
    T, B = 40, 6
    scores = np.tile(np.array([0.9, 0.1], dtype=np.float32), (B, T // 2))
    scores[:, ::2] -= np.arange(T // 2, dtype=np.float32)[None, :] * np.float32(0.01)
    scores[1::2] = scores[1::2, ::-1].copy()
    gt = np.array([[[0.0, 40 * RES]], [[0.0, 40 * RES]], [[0.0, 38 * RES]], [[RES, 37 * RES]], [[2 * RES, 34 * RES]],
                   [[0.0, 26 * RES]]])
    gt_count = np.ones(B, dtype=np.int32)
    want = R.expected_outputs(scores, gt, gt_count, RES, PS.pair_regimes)
    assert int(want[3].min()) == 21
    assert R.same_outputs(run(dev, scores, gt, gt_count), want)
    assert R.same_outputs(want, R.expected_outputs(scores, gt, gt_count, RES, R.regimes_ref))


@pytest.mark.parametrize("Gn", [0, 8, 128])
def test_ground_truth_counts(dev, Gn):
    """No ground truth (every detection a false positive), 8 (numpy's unrolled sum begins) and the maximum of 128, with one
    zero-duration row."""
    B, T = 3, 64
    scores = R.build_scores(B, T, "eighths", seed=Gn)
    one, _ = R.grid_ground_truth(1, Gn, T, RES, seed=Gn)                  # (a single pair gets all Gn rows)
    gt, gt_count = np.repeat(one, B, axis=0), np.full(B, Gn, dtype=np.int32)
    if Gn:
        gt[:, 1] = [17 * RES, 17 * RES]
    want = R.expected_outputs(scores.numpy(), gt, gt_count, RES, PS.pair_regimes)
    got = run(dev, scores, gt, gt_count)
    assert R.same_outputs(got, want)
    if Gn == 0:
        assert int(want[2][:, 0].abs().sum()) == 0 and int(want[1][..., 0].abs().sum()) == 0 and int(want[2][:, 1].min()) == 1
    # gt_count outside [0, Gmax] is refused by the check and clamped by the kernel
    with pytest.raises(RuntimeError, match="gt_count must lie in"):
        run(dev, scores, gt, np.array([Gn + 1, 0, 0], dtype=np.int32))
    clamped = run(dev, scores, gt, np.array([Gn + 5, -3, Gn], dtype=np.int32), check=False)
    want_clamped = R.expected_outputs(scores.numpy(), gt, np.array([Gn, 0, Gn]), RES, PS.pair_regimes)
    assert R.same_outputs(clamped, want_clamped)


def test_special_values(dev):
    nan, inf = np.nan, np.inf
    rows = [[-0.0, 0.0, 0.5, nan, -0.0, nan, 0.5, inf, -inf, 0.25],
            [nan] * 10,
            [inf, inf, -inf, -inf, inf, 0.0, -0.0, 0.0, nan, -1.0],
            [-0.0] * 10,
            [0.1, nan, 0.1, nan, 0.2, 0.2, nan, nan, 0.3, 0.1],
            [-inf] * 10]
    scores = np.array(rows, dtype=np.float32)
    gt, gt_count = R.grid_ground_truth(len(rows), 2, 10, RES, seed=1)
    want = R.expected_outputs(scores, gt, gt_count, RES, PS.pair_regimes)
    got = run(dev, scores, gt, gt_count)
    assert R.same_outputs(got, want)
    assert want[3].tolist() == [5, 0, 4, 1, 3, 1]
    values = got[0].cpu()
    assert values[0, :5].tolist() == [-inf, 0.0, 0.25, 0.5, inf] and not np.signbit(values[0, 1].item())
    assert not np.signbit(values[3, 0].item()) and bool(torch.isinf(values[1]).all())
    assert got[2].cpu()[1].tolist() == [0, 0] and int(got[1].cpu()[1].abs().sum()) == 0


def test_strided_input(dev):
    """A column of a (B, T, N) tensor (copied by the wrapper) and a (B, T) view of wider rows (ld > T, taken as it is)."""
    from texttoaudiogrounding_amd import ops
    B, T, N = 5, 65, 3
    scores, gt, gt_count, want = case(B, 2, T, "eighths")
    cube = torch.full((B, T, N), 7.0)
    cube[:, :, 1] = scores
    assert R.same_outputs(ops.psds_score_deltas(cube.to(dev)[:, :, 1], gt, gt_count, RES), want)
    wide = torch.full((B, T + 11), 9.0)
    wide[:, :T] = scores
    view = wide.to(dev)[:, :T]
    assert view.stride() == (T + 11, 1) and not view.is_contiguous()
    assert R.same_outputs(ops.psds_score_deltas(view, gt, gt_count, RES), want)


def test_every_entry_is_written(dev):
    """The entry point on poisoned buffers: the padding of values and deltas included."""
    from texttoaudiogrounding_amd import ops
    B, T = 3, 65
    scores, gt, gt_count, want = case(B, 2, T, "eighths")
    x = scores.to(dev)
    values = torch.full((B, T), float("nan"), device=dev)
    deltas = torch.full((B, T, 2), -77, device=dev, dtype=torch.int32)
    base = torch.full((B, 2), -77, device=dev, dtype=torch.int32)
    n_values = torch.full((B,), -77, device=dev, dtype=torch.int32)
    gt_dev, count_dev = torch.as_tensor(gt).to(dev), torch.as_tensor(gt_count).to(dev)       # (held: the call takes addresses)
    ops.call("tag_psds_score_deltas", ops.ptr(x), T, B, T, ops.ptr(gt_dev), ops.ptr(count_dev), gt.shape[1], RES, 0.5, 0.5,
             ops.ptr(values), ops.ptr(deltas), ops.ptr(base), ops.ptr(n_values))
    assert int(want[3].max()) < T and R.same_outputs((values, deltas, base, n_values), want)


def test_limits(dev):
    from texttoaudiogrounding_amd import ops
    T = ops.PSDS_SCORES_MAX_T
    assert T >= 1024
    scores = R.build_scores(2, T, "continuous", seed=2)
    scores[1] = torch.round(scores[1] * 64) / 64
    gt, gt_count = R.grid_ground_truth(2, 2, T, RES, seed=4)
    want = R.expected_outputs(scores.numpy(), gt, gt_count, RES, PS.pair_regimes)
    assert int(want[3][0]) > T // 2
    assert R.same_outputs(run(dev, scores, gt, gt_count), want)
    with pytest.raises(RuntimeError, match=f"T = {T + 1}"):
        run(dev, torch.zeros(2, T + 1), gt, gt_count)
    with pytest.raises(RuntimeError, match="max_gt = 129"):
        run(dev, torch.zeros(2, 8), np.zeros((2, 129, 2)), gt_count)
    x = torch.zeros(2, 8, device=dev)
    out = [torch.zeros(2, 8, 2, device=dev, dtype=torch.int32) for _ in range(4)]
    with pytest.raises(RuntimeError, match="ld = 7"):
        ops.call("tag_psds_score_deltas", ops.ptr(x), 7, 2, 8, None, ops.ptr(out[0]), 0, RES, 0.5, 0.5, ops.ptr(out[1]),
                 ops.ptr(out[2]), ops.ptr(out[3]), ops.ptr(out[0]))


# ------------------------------------------------------------------------------------------------ evaluator and runner

def test_evaluator_over_unequal_batches_equals_the_brute_force(dev):
    from texttoaudiogrounding_amd.utils.device_eval import ScorePsdsEvaluator
    ev = ScorePsdsEvaluator(RES, device=dev)
    scores, ground_truth, durations = {}, {}, {}
    for i, (B, T) in enumerate([(5, 12), (1, 7), (3, 12)]):
        s = R.build_scores(B, T, "eighths", seed=40 + i)
        gt, gt_count = R.grid_ground_truth(B, 3, T, RES, seed=50 + i)
        ev.update(s.to(dev), gt, gt_count)
        for d, part in zip((scores, ground_truth, durations), R.tables(s.numpy(), gt, gt_count, RES, prefix=f"b{i}_")):
            d.update(part)
    state = ev.state()
    assert sorted(state) == ["base", "deltas", "n_refs", "n_values", "values"] and len(state["values"]) == 3
    assert all(t.is_cuda for t in state["values"] + state["deltas"] + state["n_values"]) and state["base"].is_cuda
    total = sum(durations.values())
    got = ev.compute(total)
    want = PS.psds_from_scores(scores, ground_truth, durations, RES)
    print(f"score-based PSDS {got['psds']!r} over {got['n_operating_points']} operating points")
    assert got["psds"] == want and 0.0 < want < 1.0
    assert got["n_operating_points"] == len(PS.all_thresholds(scores)) and got["n_refs"] == sum(len(g) for g in ground_truth.values())
    assert len(got["efpr"]) == len(got["etpr"]) > 2
    many = ev.compute(total, max_efpr=list(PS.REFERENCE_MAX_EFPRS))["psds"]
    assert many == {m: PS.psds_from_scores(scores, ground_truth, durations, RES, max_efpr=m) for m in PS.REFERENCE_MAX_EFPRS}
    assert many[None] == want and ev.compute(total, max_efpr=0)["psds"] == float(got["etpr"].max())
    ev.reset()
    assert ev.compute(total)["n_operating_points"] == 1 and ev.state()["values"] == []


def test_runner_evaluate_psds_scores(dev):
    """StrongRunner.evaluate_psds_scores on the small BiEncoder of test_gpu_sed_eval's runner test (two batches, one pair
    without ground truth, which is left out) equals the brute force over the same frame_sim."""
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import StrongRunner
    torch.manual_seed(5)
    model = audio_text_model.BiEncoder(audio_encoder.CrnnEncoder(32000, 256), text_encoder.EmbeddingAgg(5221, 256),
                                       match.DotProduct(), 256)
    with torch.no_grad():
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
    ground_truth[keys[1]] = [[0.0, 0.0]]
    durations = {k: 2.0 for k in keys}
    res = runner.model.audio_encoder.time_resolution
    got = runner.evaluate_psds_scores([dict(b) for b in batches], ground_truth, durations,
                                      {"time_resolution": res, "max_efprs": list(PS.REFERENCE_MAX_EFPRS)})
    one = runner.evaluate_psds_scores([dict(b) for b in batches], ground_truth, durations, {"time_resolution": res, "max_efpr": 800.0})
    with torch.no_grad():
        sims = torch.cat([runner.forward(dict(b), training=False)["frame_sim"] for b in batches]).cpu().numpy()
    scores = {k: sims[i] for i, k in enumerate(keys) if k != keys[1]}
    full_gt = {k: np.array([r for r in v if r != [0.0, 0.0]]).reshape(-1, 2) for k, v in ground_truth.items()}
    want = {m: PS.psds_from_scores(scores, full_gt, durations, res, max_efpr=m) for m in PS.REFERENCE_MAX_EFPRS}
    print(f"runner: score-based PSDS {got['psds']}")
    assert got["psds"] == want and one["psds"] == want[800] and got["n_refs"] == 8
    assert got["n_operating_points"] == len(PS.all_thresholds(scores)) > 8 and not runner.model.training
    assert max(want.values()) > 0.0
