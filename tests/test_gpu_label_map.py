"""csrc/label_map.hip (ops.label_map, tag_label_map / tag_label_map_topk), utils/label_map.py, the ASMapping datasets and
tools/map_phrase_to_event.py against the fp64 oracle of tests/label_map_ref.py and the recorded items of the reference's datasets
(tests/golden/make_golden_asmapping.py).

Shapes (N, C, D): the smallest that reach every path of the marching kernel (128 rows per workgroup, 128-label tiles, 32-wide K
chunks; the plain float4 loaders need whole tiles, whole chunks and 16-byte aligned rows per operand):
(300, 527, 384) four whole label tiles + a 15-column tail, three row blocks;  (1, 1, 1);  (127, 128, 32) whole label tiles
(the plain loader for e) under a partial row block;  (129, 129, 33) one row / one label / one k past a tile;  (257, 15, 386)
row strides above D and bases off 16-byte alignment (scalar loads);  (128, 128, 31) whole tiles with a K tail.

Two kinds of checks.  EXACT: with ``sim`` requested, every other output equals the oracle's selection rules applied to the op's
OWN sim; without it the other outputs have the same bits; two runs have the same bits; nothing outside the outputs is written.
AGAINST fp64: |sim - oracle| <= (D + 8) 2^-24 (label_map_ref.bound), and a selection is compared wherever the oracle decides it by
more than twice that bound; the undecided share is asserted to stay below 0.5 % of the elements and 2 % of the rows.  One
element is 0.5 % of a shape only from 200 elements on, one row 2 % from 50 rows on: (1, 1, 1), whose quantile thresholds EQUAL its
one similarity, takes the exact checks and the similarity bound, and its shares are printed, not asserted."""
import functools
import importlib.util
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import label_map_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 527, 384), (1, 1, 1), (127, 128, 32), (129, 129, 33), (257, 15, 386), (128, 128, 31)]
STRIDED = (257, 15, 386)
IDS = lambda s: "x".join(map(str, s))       # noqa: E731
GUARD = 64


@functools.lru_cache(maxsize=None)
def inputs(N, C, D):
    g = np.random.RandomState(N + 7 * C + 31 * D)
    x, e = g.randn(N, D).astype(np.float32), g.randn(C, D).astype(np.float32)
    s64 = R.cosine64(x, e)
    th0, th1 = (float(t) for t in np.quantile(s64, [0.6, 0.999]).astype(np.float32))
    for a in (x, e, s64):
        a.setflags(write=False)
    return x, e, s64, th0, th1


def to_dev(a, dev, shape=None):
    """The array on the device; for the STRIDED shape as a view with row stride D + 3 whose base is 4 bytes past an aligned one."""
    t = torch.from_numpy(np.array(a)).to(dev)
    if shape != STRIDED:
        return t
    rows, D = t.shape
    view = torch.full((rows * (D + 3) + 1,), float("nan"), device=dev)[1:].view(rows, D + 3)[:, :D]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.stride(0) == D + 3
    return view


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_rules(res, sim, th0, th1, tag):
    """Every output of ``res`` equals the selection rules on ``sim`` (numpy float32), bit for bit."""
    sel = R.select(sim, th0, th1)
    got = {k: getattr(res, k).cpu().numpy() for k in ("best", "best_sim", "min_sim", "win_best", "win_count", "win_bits")}
    for k in ("best", "win_best", "win_count"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], sel[k]), (tag, k)
    for k in ("best_sim", "min_sim"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.int32), sel[k].view(np.int32)), (tag, k)
    assert np.array_equal(got["win_bits"].view(np.uint32), sel["win_bits"]), (tag, "win_bits")
    C = sim.shape[1]
    if C % 32:
        assert (got["win_bits"].view(np.uint32)[:, -1] >> np.uint32(C % 32) == 0).all(), (tag, "bits past C")
    return sel


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_outputs_equal_the_rules_on_the_ops_own_sim(dev, shape):
    from texttoaudiogrounding_amd import ops
    N, C, D = shape
    x, e, _, th0, th1 = inputs(*shape)
    tx, te = to_dev(x, dev, shape), to_dev(e, dev, shape)
    assert ops.query("tag_label_map_ws_bytes", N, C, D) == 4 * (N + C)
    with_sim = ops.label_map(tx, te, th0, th1, topk=3, want_sim=True)
    again = ops.label_map(tx, te, th0, th1, topk=3, want_sim=True)
    without = ops.label_map(tx, te, th0, th1)
    assert without.sim is None and without.idx is None and with_sim.sim.shape == (N, C) and with_sim.sim.dtype == torch.float32
    for k in ("best", "best_sim", "min_sim", "win_best", "win_count", "win_bits"):
        assert same_bits(getattr(with_sim, k), getattr(without, k)), (k, "with and without sim")
        assert same_bits(getattr(with_sim, k), getattr(again, k)), (k, "two runs")
    assert same_bits(with_sim.sim, again.sim) and (C < 2 or same_bits(with_sim.idx, again.idx))
    sim = with_sim.sim.cpu().numpy()
    sel = check_rules(with_sim, sim, th0, th1, shape)
    print(f"{shape}: th0 {th0:.6f} th1 {th1:.6f}, window sizes {sel['win_count'].min()} .. {sel['win_count'].max()}, "
          f"empty windows {int((sel['win_best'] < 0).sum())}")
    for k in (3, 32):
        kk = min(k, C)
        idx = ops.label_map(tx, te, th0, th1, topk=k).idx
        if kk < 2:
            assert idx is None
            continue
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), R.topk(sim, th0, th1, kk)), (shape, k)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_raw_call_writes_nothing_outside_its_outputs(dev, shape):
    """The C entry points on caller-owned buffers inside NaN guard bands (sim with a row stride of C + 5: the gap columns are a
    guard too), top-k for k = 1, 3, 32 on that strided sim; the results equal ops.label_map's bit for bit."""
    from texttoaudiogrounding_amd import lib, ops
    N, C, D = shape
    x, e, _, th0, th1 = inputs(*shape)
    tx, te = to_dev(x, dev, shape), to_dev(e, dev, shape)
    W, lds = (C + 31) // 32, C + 5
    nan_bits = int(np.float32("nan").view(np.int32))

    def guarded(n, dtype):
        buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev).view(torch.int32)
        assert int(buf[0]) == nan_bits
        return buf, buf[GUARD: GUARD + n].view(dtype)

    bufs = {k: guarded(N, torch.int32) for k in ("best", "win_best", "win_count")}
    bufs.update({k: guarded(N, torch.float32) for k in ("best_sim", "min_sim")})
    bufs["win_bits"] = guarded(N * W, torch.int32)
    bufs["sim"] = guarded(N * lds, torch.float32)
    ws = torch.empty(ops.query("tag_label_map_ws_bytes", N, C, D) // 4 + 4, device=dev)
    p = lib.ptr
    lib.call("tag_label_map", p(tx), tx.stride(0), p(te), te.stride(0), th0, th1, *(p(bufs[k][1]) for k in
             ("best", "best_sim", "min_sim", "win_best", "win_count", "win_bits")), p(bufs["sim"][1]), lds, N, C, D, p(ws))
    idx_bufs = {}
    for k in (1, 3, 32):
        idx_bufs[k] = guarded(N * k, torch.int32)
        lib.call("tag_label_map_topk", p(bufs["sim"][1]), lds, th0, th1, p(idx_bufs[k][1]), N, C, k)
    torch.cuda.synchronize()
    for name, (buf, view) in list(bufs.items()) + [(f"idx{k}", b) for k, b in idx_bufs.items()]:
        assert (buf[:GUARD] == nan_bits).all() and (buf[GUARD + view.numel():] == nan_bits).all(), (shape, name, "guard band")
    sim_rows = bufs["sim"][1].view(N, lds)
    assert torch.isnan(sim_rows[:, C:]).all(), (shape, "the columns between sim's rows")
    want = ops.label_map(tx, te, th0, th1, want_sim=True)
    for k in ("best", "best_sim", "min_sim", "win_best", "win_count"):
        assert same_bits(bufs[k][1], getattr(want, k)), (shape, k)
    assert same_bits(bufs["win_bits"][1].view(N, W), want.win_bits) and same_bits(sim_rows[:, :C].contiguous(), want.sim)
    sim = want.sim.cpu().numpy()
    for k in (1, 3, 32):
        got = idx_bufs[k][1].view(N, k).cpu().numpy()
        assert np.array_equal(got, R.topk(sim, th0, th1, k)), (shape, k)
    assert np.array_equal(idx_bufs[1][1].cpu().numpy(), want.win_best.cpu().numpy())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_the_fp64_oracle(dev, shape):
    from texttoaudiogrounding_amd import ops
    N, C, D = shape
    x, e, s64, th0, th1 = inputs(*shape)
    res = ops.label_map(to_dev(x, dev, shape), to_dev(e, dev, shape), th0, th1, want_sim=True)
    sim = res.sim.cpu().numpy().astype(np.float64)
    err = np.abs(sim - s64).max()
    bit_ok, best_ok, win_ok = R.decided(s64, th0, th1, D)
    row_ok = best_ok & win_ok
    print(f"{shape}: sim err {err:.3g} (bound {R.bound(D):.3g}); undecided at 2 x bound: {(~bit_ok).mean():.3%} of the elements, "
          f"{(~row_ok).mean():.3%} of the rows")
    assert err <= R.bound(D)
    if N * C >= 200:
        assert (~bit_ok).mean() <= 0.005
    if N >= 50:
        assert (~row_ok).mean() <= 0.02
    want = R.select(s64, th0, th1)
    from texttoaudiogrounding_amd.utils.label_map import window_members
    bits = window_members(res.win_bits.cpu().numpy(), C)
    assert np.array_equal(bits[bit_ok], want["mask"][bit_ok])
    assert np.array_equal(res.best.cpu().numpy()[best_ok], want["best"][best_ok])
    assert np.array_equal(res.win_best.cpu().numpy()[win_ok], want["win_best"][win_ok])
    rows = np.arange(N)
    assert (np.abs(res.best_sim.cpu().numpy() - s64.max(1)) <= R.bound(D)).all()
    assert (np.abs(res.min_sim.cpu().numpy() - s64.min(1)) <= R.bound(D)).all()
    assert np.array_equal(res.best_sim.cpu().numpy(), res.sim.cpu().numpy()[rows, res.best.cpu().numpy()])


def test_special_rows(dev):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils.label_map import window_members
    N, C, D = 70, 40, 24
    g = np.random.RandomState(77)
    x, e = g.randn(N, D).astype(np.float32), g.randn(C, D).astype(np.float32)
    x[3] = 0                                        # a zero phrase
    e[5] = 0                                        # a zero label
    e[17] = e[9]
    e[30] = e[9]                                    # one label three times
    x[11] = e[9] + 0.05 * g.randn(D).astype(np.float32)
    x[10] = 2.5 * e[20]                             # a phrase equal to a label up to its length
    tx, te = to_dev(x, dev), to_dev(e, dev)
    r = ops.label_map(tx, te, -2.0, 1.5, topk=3, want_sim=True)
    sim, bits = r.sim.cpu().numpy(), window_members(r.win_bits.cpu().numpy(), C)
    check_rules(r, sim, -2.0, 1.5, "special")
    assert (sim[3] == 0).all() and (sim[:, 5] == 0).all()                                         # exactly 0
    assert not bits[3].any() and not bits[:, 5].any()
    assert int(r.win_count[3]) == 0 and int(r.win_best[3]) == -1 and r.idx[3].tolist() == [-1, -1, -1] and int(r.best[3]) == 0
    others = np.delete(np.arange(N), 3)
    assert (r.win_count.cpu().numpy()[others] == C - 1).all()                                     # everything but the zero label
    assert np.array_equal(sim[:, 17].view(np.int32), sim[:, 9].view(np.int32))
    assert np.array_equal(sim[:, 30].view(np.int32), sim[:, 9].view(np.int32))
    assert int(r.best[11]) == 9 and int(r.win_best[11]) == 9 and r.idx[11].tolist() == [9, 17, 30]
    assert int(r.best[10]) == 20 and abs(float(r.best_sim[10]) - 1.0) <= R.bound(D) and bits[10, 20]
    for th0, th1 in ((2.0, 3.0), (0.9, 0.1)):                                                     # an empty window; th0 > th1
        r = ops.label_map(tx, te, th0, th1, topk=32)
        assert (r.win_best == -1).all() and (r.win_count == 0).all() and (r.win_bits == 0).all() and (r.idx == -1).all()
        assert r.idx.shape == (N, 32) and int(r.best[11]) == 9
    with pytest.raises(ValueError, match="exceeds 32"):
        ops.label_map(tx, te, 0.0, 1.0, topk=33)
    with pytest.raises(RuntimeError, match="expected x's device"):
        ops.label_map(tx, te[:, :8], 0.0, 1.0)
    with pytest.raises(RuntimeError, match="expected a float32 matrix"):
        ops.label_map(tx.double(), te, 0.0, 1.0)


def test_label_map_class_chunks_and_lists(dev):
    from texttoaudiogrounding_amd.utils.label_map import LabelMap
    x, e, s64, th0, th1 = inputs(129, 129, 33)
    whole = LabelMap(e, device=dev).map(x, (th0, th1), topk=0, want_sim=True)
    chunked = LabelMap(e, device=dev, chunk_rows=50).map(x, (th0, th1), topk=0, want_sim=True)
    assert np.array_equal(whole.best, chunked.best) and np.array_equal(whole.sim, chunked.sim) and whole.best.dtype == np.int64
    mask = R.window(whole.sim, th0, th1)
    for lists in (whole.labels, chunked.labels):
        assert len(lists) == 129 and all(np.array_equal(l, np.flatnonzero(m)) for l, m in zip(lists, mask))
    top1 = LabelMap(e, device=dev).map(x, (th0, th1), topk=1)
    top4 = LabelMap(e, device=dev, chunk_rows=50).map(x, (th0, th1), topk=4)
    want = R.topk(whole.sim, th0, th1, 4)
    assert top1.sim is None and [l.tolist() for l in top1.labels] == [[w] if w >= 0 else [] for w in want[:, 0]]
    assert [l.tolist() for l in top4.labels] == [row[row >= 0].tolist() for row in want]
    everything = LabelMap(e, device=dev).map(x)                      # no thresholds: the best label of every phrase
    assert [l.tolist() for l in everything.labels] == [[b] for b in whole.best.tolist()]


def test_asmapping_datasets_equal_the_reference(dev, golden_dir, tmp_path):
    assert R.check_datasets_against_golden(golden_dir, tmp_path, device=dev, sim_tol=R.bound(8)) >= 4 * 8 + 32


def test_map_phrase_to_event_tool(dev, golden_dir, tmp_path):
    spec = importlib.util.spec_from_file_location("map_phrase_to_event_tool", os.path.join(ROOT, "tools", "map_phrase_to_event.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    phrase_pkl = os.path.join(golden_dir, "multi_phrase", "phrase_emb.pkl")
    label_pkl = os.path.join(golden_dir, "asmapping", "as_label_emb.pkl")
    out = str(tmp_path / "phrase_to_event.tsv")
    tool.main(tool.build_parser().parse_args(["--phrase_emb", phrase_pkl, "--label_emb", label_pkl, "--output", out, "--device", str(dev)]))
    with open(phrase_pkl, "rb") as f:
        emb = pickle.load(f)
    with open(label_pkl, "rb") as f:
        labels = pickle.load(f)
    s64 = R.cosine64(np.stack(list(emb.values())), np.stack(list(labels.values())))
    top = np.sort(s64, axis=1)
    assert (top[:, -1] - top[:, -2] > 2 * R.bound(8)).all()
    lines = open(out).read().splitlines()
    assert lines[0] == "phrase\tindex\tsim" and len(lines) == 1 + len(emb)
    for line, phrase, s in zip(lines[1:], emb, s64):
        got_phrase, index, sim = line.split("\t")
        assert got_phrase == phrase and int(index) == s.argmax() and abs(float(sim) - s.max()) <= R.bound(8)
        assert str(np.float32(sim)) == sim


def test_strong_dataset_batch_takes_a_training_step(dev, golden_dir, tmp_path):
    """ASMappingStrongDataset -> VarLenPadCollate -> ClassMappingRunner + ClipMaskedFrameBceLoss: strong_label_mask has a producer."""
    from texttoaudiogrounding_amd.datasets import ASMappingStrongDataset, VarLenPadCollate, write_waveform_pack
    from texttoaudiogrounding_amd.losses import ClipMaskedFrameBceLoss
    from texttoaudiogrounding_amd.models import audio_encoder
    from texttoaudiogrounding_amd.models.audio_text_model import AudioTagging
    from texttoaudiogrounding_amd.runner import ClassMappingRunner
    fix = os.path.join(golden_dir, "asmapping")
    with open(os.path.join(fix, "config.json")) as f:
        cfg = json.load(f)
    g = np.random.RandomState(3)
    waves = [("S0.wav", (0.1 * g.randn(20480)).astype(np.float16)), ("S1.wav", (0.1 * g.randn(16000)).astype(np.float16))]
    tsv = write_waveform_pack(str(tmp_path / "pack.npz"), waves)
    phrases = cfg["phrases"]
    clips = [{"audio_id": aid, "audiocap_id": i, "tokens": "t",
              "phrases": [{"phrase": phrases[2 * i + j], "start_index": j, "end_index": j + 1, "segments": [[0.04 * j, 0.04 * j + 0.2]]}
                          for j in range(2)]} for i, (aid, _) in enumerate(waves)]
    label, as_tsv = str(tmp_path / "label.json"), str(tmp_path / "as.tsv")
    with open(label, "w") as f:
        json.dump(clips, f)
    with open(as_tsv, "w") as f:
        f.write("audio_id\tevent_labels\nS0.wav\tBird;Speech\nS1.wav\tRain\n")
    ds = ASMappingStrongDataset(waveform=tsv, label=label, audioset_label=as_tsv,
                                phrase_embed=os.path.join(golden_dir, "multi_phrase", "phrase_emb.pkl"),
                                as_label_embed=os.path.join(fix, "as_label_emb.pkl"), label_encoder=os.path.join(fix, "classes.json"),
                                time_resolution=0.04, thresholds=cfg["thresholds"]["low"], topk=2, device=dev)
    items = [ds[0], ds[1]]
    assert items[0]["strong_label"].shape == (17, 9) and items[1]["strong_label"].shape == (13, 9)
    assert all(it["strong_label_mask"].sum() >= 2 and (it["weak_label"] >= it["strong_label_mask"]).all() for it in items)
    assert all(((it["strong_label"].max(0) > 0) <= (it["strong_label_mask"] > 0)).all() for it in items)
    batch = VarLenPadCollate(pad_keys=["waveform", "strong_label"])(items)
    torch.manual_seed(0)
    model = AudioTagging(audio_encoder.Cnn8Rnn(32000), ds.classes_num).to(dev)
    runner = ClassMappingRunner(model, loss_fn=ClipMaskedFrameBceLoss(0.5), device=dev)
    before = model.fc_output.weight.detach().clone()
    loss = runner.loss_value(runner.train_step(batch))
    assert np.isfinite(loss) and loss > 0
    after = runner.model.fc_output.weight
    assert not torch.equal(after, before) and torch.isfinite(after).all()
