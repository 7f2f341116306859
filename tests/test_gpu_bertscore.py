"""The BERTScore phrase-to-label map on the MI355X (csrc/bertscore.hip through ops.bertscore_map, utils.bertscore_map.BertScoreMap
and tools/prepare_phrase_bertscore.py) against the fp64 restatement of tests/bertscore_ref.py.

Inputs (bertscore_ref.make_case): every token is scale * unit(g + common), each phrase's tokens noisy copies of one planted label's
tokens, so every cosine is positive; what stands past a length would score high if it were let in.  On the host in fp64 the cases
below give P, R >= 0.29 and a gap of at least 4.9e-2 between the two largest F of every row; the tests assert a gap > 1e-3 for
EVERY row (a condition on the inputs), so every row takes part in the index comparison.

Bounds: the error of P, R and F is taken relative to the tensor's largest entry.  The project's rule (tests/test_gpu_text_rnn.py):
5e-6 where the deviation of the same restatement run in fp32 on the host, measured in the test, is below 1.25e-6 (it was at
most 3.9e-7 for these cases where measured), otherwise 4 x that deviation.  Every measured error is printed.

Shapes (N, C, La, Lb, D), the smallest that reach each hazard: (3, 1, 1, 1, 1) smallest everything; (17, 5, 4, 2, 20) the D tail
and 4-byte reads; (17, 33, 8, 8, 100) 136 token rows cross a row tile, 264 label rows make three column tiles, D % 32 != 0;
(130, 33, 32, 32, 36) full-size slots, many row blocks, several slices; (40, 527, 16, 8, 768) the workload's C and D on the
FAST path.  Lengths are random in 1 .. L with one item at full length and one at length 1."""
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

from tests import bertscore_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND, DEV_LIMIT = 5e-6, 1.25e-6
MIN_GAP = 1e-3
SHAPES = [(3, 1, 1, 1, 1), (17, 5, 4, 2, 20), (17, 33, 8, 8, 100), (130, 33, 32, 32, 36), (40, 527, 16, 8, 768)]
KEYS = ("a", "a_len", "a_w", "b", "b_len", "b_w")


def bound_for(dev32):
    return BOUND if dev32 < DEV_LIMIT else 4.0 * dev32


def on(case, dev, **change):
    args = {k: case[k] for k in KEYS}
    args.update(change)
    return [None if args[k] is None else args[k].to(dev) for k in KEYS]


def reference(case, **change):
    """(fp64 scores, the fp32 deviation of the restatement per quantity)"""
    args = {k: case[k] for k in KEYS}
    args.update(change)
    r64 = R.scores(args["a"].double(), args["a_len"], args["a_w"], args["b"].double(), args["b_len"], args["b_w"])
    r32 = R.scores(args["a"], args["a_len"], args["a_w"], args["b"], args["b_len"], args["b_w"])
    return r64, [R.rel_err(r32[q], r64[q]) for q in range(3)]


@pytest.fixture(scope="module")
def runs(dev):
    """Per shape: the case, its fp64 scores with the fp32 deviation, and ONE run on the device with the scores."""
    from texttoaudiogrounding_amd import ops
    out = {}
    for k, shape in enumerate(SHAPES):
        case = R.make_case(100 + k, *shape)
        r64, dev32 = reference(case)
        res = ops.bertscore_map(*on(case, dev), want_scores=True)
        torch.cuda.synchronize()
        out[shape] = (case, r64, dev32, res)
    return out


def check_against(name, res, r64, dev32):
    """P, R, F of the full scores and of the best values (against the fp64 scores at ``best``) within the rule's bound"""
    got = res.scores.cpu()
    best = res.best.cpu().long()
    rows = torch.arange(got.shape[1])
    assert tuple(got.shape) == tuple(r64.shape) and torch.isfinite(got).all()
    for q, (label, vec) in enumerate(zip("PRF", (res.best_p, res.best_r, res.best_f))):
        e_all = R.rel_err(got[q], r64[q])
        e_best = ((vec.cpu().double() - r64[q][rows, best]).abs().max() / r64[q].abs().max()).item()
        bound = bound_for(dev32[q])
        print(f"bertscore {name} {label}: scores {e_all:.2e}, best {e_best:.2e}, fp32 restatement {dev32[q]:.2e}, bound {bound:.1e}")
        assert e_all < bound and e_best < bound, (name, label, e_all, e_best, bound)
        assert torch.equal(vec.cpu(), got[q][rows, best])              # the best values ARE the scores at best


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scores_and_best_against_fp64(runs, shape):
    case, r64, dev32, res = runs[shape]
    gap = R.top_two_gap(r64)
    assert (gap > MIN_GAP).all(), gap.min()                           # a condition on the inputs: no row is left out below
    check_against(str(shape), res, r64, dev32)
    want = R.select(r64)[0]
    assert res.best.dtype == torch.int32 and res.best.cpu().tolist() == want.tolist()
    if shape[1] > 1:
        assert want.tolist() == case["plant"].tolist()                # (the planted label is the answer)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_runs_are_bit_equal_and_scores_are_optional(runs, dev, shape):
    from texttoaudiogrounding_amd import ops
    case, _, _, res = runs[shape]
    again = ops.bertscore_map(*on(case, dev), want_scores=True)
    plain = ops.bertscore_map(*on(case, dev))
    assert plain.scores is None
    for name in ("best", "best_f", "best_p", "best_r"):
        assert torch.equal(getattr(again, name), getattr(res, name)) and torch.equal(getattr(plain, name), getattr(res, name)), name
    assert torch.equal(again.scores, res.scores)


@pytest.mark.parametrize("shape", [(17, 5, 8, 8, 20), (8, 32, 16, 8, 64)], ids=lambda s: "x".join(map(str, s)))
def test_a_base_pointer_offset_by_one_float_gives_the_same_bits(dev, shape):
    """Slot-sized unit rows with normalize=False reach the kernel as they are: at a 16-byte aligned base (float4 reads; the second
    shape is whole tiles and whole chunks, the FAST form) and at that base + 4 bytes (4-byte reads)."""
    from texttoaudiogrounding_amd import ops
    case = R.make_case(31, *shape)
    a, b = R.unit(case["a"].double()).float().to(dev), R.unit(case["b"].double()).float().to(dev)

    def shifted(x, off):
        buf = torch.zeros(x.numel() + 4, device=dev)
        view = buf[off: off + x.numel()].view(x.shape)
        view.copy_(x)
        assert view.data_ptr() % 16 == 4 * off
        return view
    rest = on(case, dev)
    res = [ops.bertscore_map(shifted(a, oa), rest[1], rest[2], shifted(b, ob), rest[4], rest[5], want_scores=True, normalize=False)
           for oa, ob in ((0, 0), (1, 1), (1, 0), (0, 1))]
    for other in res[1:]:
        assert all(torch.equal(x, y) for x, y in zip(other, res[0]))
    r64 = R.scores(a.cpu().double(), case["a_len"], case["a_w"], b.cpu().double(), case["b_len"], case["b_w"], normalize=False)
    r32 = R.scores(a.cpu(), case["a_len"], case["a_w"], b.cpu(), case["b_len"], case["b_w"], normalize=False)
    check_against(f"offset {shape}", res[1], r64, [R.rel_err(r32[q], r64[q]) for q in range(3)])


def test_padded_positions_enter_no_maximum(dev):
    """Phrases near +common, labels near -common: every valid cosine is negative, the slots (8) are larger than the lengths (at
    most 5 and 3), and a padded position scores 0 (the zero fill) or high (what the case leaves past a length)."""
    from texttoaudiogrounding_amd import ops
    case = R.make_case(7, 9, 6, 5, 3, 40, sign=-1.0)
    r64, dev32 = reference(case)
    assert r64[0].max() < -0.1 and r64[1].max() < -0.1
    res = ops.bertscore_map(*on(case, dev), want_scores=True)
    got = res.scores.cpu()
    assert (got[0] < 0).all() and (got[1] < 0).all()
    check_against("all-negative", res, r64, dev32)


def test_a_duplicated_label_ties_bit_for_bit_and_the_lower_index_wins(dev):
    """Label 0 copied to index 40 (slot 8: token rows 320 .., the third column tile, another slice) and planted for every phrase."""
    from texttoaudiogrounding_amd import ops
    N, C = 20, 48
    case = R.make_case(11, N, C, 8, 8, 72)
    plant0 = R.make_case(11, N, 1, 8, 8, 72)                        # (same seed: phrases that copy the tokens of one label)
    case.update(a=plant0["a"], a_len=plant0["a_len"], a_w=plant0["a_w"])
    for k in ("b", "b_len", "b_w"):
        case[k][0] = plant0[k][0]
        case[k][40] = plant0[k][0]
    res = ops.bertscore_map(*on(case, dev), want_scores=True)
    got = res.scores.cpu()
    assert torch.equal(got[:, :, 0], got[:, :, 40])
    r64, dev32 = reference(case)
    check_against("tie", res, r64, dev32)
    others = torch.ones(C, dtype=torch.bool)
    others[[0, 40]] = False
    assert (r64[2][:, 0] - r64[2][:, others].max(dim=1).values > MIN_GAP).all()       # labels 0 and 40 lead every row
    assert res.best.cpu().tolist() == [0] * N and torch.equal(res.best_f.cpu(), got[2, :, 40])


def test_default_weights(runs, dev):
    from texttoaudiogrounding_amd import ops
    shape = (17, 33, 8, 8, 100)
    case = dict(runs[shape][0])
    case["a_len"], case["b_len"] = case["a_len"].clone(), case["b_len"].clone()
    case["a_len"][3], case["b_len"][5] = 2, 2                          # items of two tokens: [CLS] [SEP] and nothing between
    a_w, b_w = R.default_weights(case["a_len"], shape[2]), R.default_weights(case["b_len"], shape[3])
    implied = ops.bertscore_map(*on(case, dev, a_w=None, b_w=None), want_scores=True)
    given = ops.bertscore_map(*on(case, dev, a_w=a_w, b_w=b_w), want_scores=True)
    assert all(torch.equal(x, y) for x, y in zip(implied, given))
    got = implied.scores.cpu()
    short_a, short_b = case["a_len"] <= 2, case["b_len"] <= 2
    assert short_a[3] and short_a[-1] and short_b[5] and short_b[-1]
    assert (got[0][short_a] == 0).all() and (got[1][:, short_b] == 0).all()
    assert (got[2][short_a] == 0).all() and (got[2][:, short_b] == 0).all()
    assert (got[0][~short_a] > 0).all() and (got[1][:, ~short_b] > 0).all()
    r64, dev32 = reference(case, a_w=a_w, b_w=b_w)
    check_against("default weights", implied, r64, dev32)
    assert implied.best.cpu()[short_a].tolist() == [0] * int(short_a.sum())      # every F of such a row is 0: the lowest index


def _ragged(case, key):
    return [case[key][k, : int(n)].numpy() for k, n in enumerate(case[key + "_len"])]


def test_bertscoremap_in_chunks_equals_one_call(runs):
    from texttoaudiogrounding_amd.utils.bertscore_map import BertScoreMap
    case, r64, _, _ = runs[(130, 33, 32, 32, 36)]
    phrases, labels = _ragged(case, "a"), _ragged(case, "b")
    whole = BertScoreMap(labels, special_tokens=False).map(phrases, want_scores=True)
    parts = BertScoreMap(labels, special_tokens=False, chunk_rows=47).map(phrases, want_scores=True)
    assert all(np.array_equal(x, y) for x, y in zip(parts, whole))
    ones_a, ones_b = R.default_weights(case["a_len"], 32, False), R.default_weights(case["b_len"], 32, False)
    want, dev32 = reference(case, a_w=ones_a, b_w=ones_b)
    assert (R.top_two_gap(want) > MIN_GAP).all()
    for q in range(3):
        assert R.rel_err(whole.scores[q], want[q]) < bound_for(dev32[q])
    assert whole.best.dtype == np.int64 and whole.best.tolist() == R.select(want)[0].tolist()


def test_tool_round_trip(runs, tmp_path):
    case, _, _, _ = runs[(17, 5, 4, 2, 20)]
    phrases = {f"phrase {k}": v for k, v in enumerate(_ragged(case, "a"))}
    labels = {f"label {k}": v for k, v in enumerate(_ragged(case, "b"))}
    paths = {k: str(tmp_path / k) for k in ("p.pkl", "l.pkl", "o.tsv")}
    for name, table in (("p.pkl", phrases), ("l.pkl", labels)):
        with open(paths[name], "wb") as f:
            pickle.dump(table, f)
    spec = importlib.util.spec_from_file_location("prepare_phrase_bertscore_tool", os.path.join(ROOT, "tools", "prepare_phrase_bertscore.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(tool.build_parser().parse_args(["--phrase_emb", paths["p.pkl"], "--label_emb", paths["l.pkl"], "--output", paths["o.tsv"],
                                              "--no_special_tokens"]))
    ones_a, ones_b = R.default_weights(case["a_len"], 4, False), R.default_weights(case["b_len"], 2, False)
    want, dev32 = reference(case, a_w=ones_a, b_w=ones_b)
    assert (R.top_two_gap(want) > MIN_GAP).all()
    best, f, _, _ = R.select(want)
    lines = open(paths["o.tsv"]).read().split("\n")
    assert lines[0] == "phrase\tindex\tsim" and lines[-1] == "" and len(lines) == 17 + 2
    for line, phrase, index, value in zip(lines[1:], phrases, best, f):
        name, idx, sim = line.split("\t")
        assert name == phrase and int(idx) == index and str(np.float32(sim)) == sim
        assert abs(float(sim) - value) < bound_for(dev32[2]) * np.abs(f).max()
