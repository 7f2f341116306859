"""ops.phrase_sim_count (phrase_sim.hip) against the fp64 reference of tests/phrase_sim_ref.py.  The inputs keep every cosine at
least 1e-4 from every threshold under test (the builder asserts it), which is more than an fp32 dot product of unit rows can
err by, so every comparison here is exact integer equality."""
import functools
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import phrase_sim_ref as R

pytestmark = pytest.mark.gpu

# Column slices of phrase_sim.hip: a launch wants FILL_WGS = 512 workgroups of T = 128 query rows, so ONE query block against
# more than 512 column tiles is the smallest shape with several slices that march over more than one tile each: N = 512 * 128
# + 129 columns are 514 tiles = 257 slices of 2 tiles (the last column tile holds one bank row).
T, FILL_WGS = 128, 512
SLICED = (3, FILL_WGS * T + T + 1, 40)

SHAPES = [(1, 1, 1), (1, 300, 512), (33, 65, 5), (64, 64, 32), (65, 129, 33), (130, 257, 48), (257, 300, 512), (257, 300, 768),
          (128, 256, 64),       # whole tiles, whole chunks, aligned rows: the loader without tail tests
          (1152, 256, 32),      # the same with 9 query blocks: a full group of 8 and a short one
          SLICED]


@functools.lru_cache(maxsize=None)
def inputs(M, N, D, same=False, raw=False, thresholds=R.THRESHOLDS):
    q, bank, rounds = R.build_inputs(M, N, D, thresholds, seed=0, same=same, raw=raw)
    w = np.random.RandomState(1).randint(0, 1001, size=bank.shape[0]).astype(np.int64)
    return q, bank, w, rounds


def run(q, bank, w, thr, dev, **kw):
    from texttoaudiogrounding_amd import ops
    out = ops.phrase_sim_count(q, bank, w, threshold=thr, **kw)
    assert out.dtype == torch.int64 and out.shape == (q.shape[0],) and out.device.type == "cuda"
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_equal_fp64_reference(dev, shape):
    from texttoaudiogrounding_amd import ops
    M, N, D = shape
    q, bank, w, rounds = inputs(M, N, D)
    if shape == SLICED:
        assert ops.query("tag_phrase_sim_count_ws_bytes", M, N, D) == 257 * M * 8
    tq, tb, tw = torch.from_numpy(q).to(dev), torch.from_numpy(bank).to(dev), torch.from_numpy(w).to(dev)
    for thr in R.THRESHOLDS:
        for weight, tweight in ((None, None), (w, tw)):
            want = R.count_ref(q, bank, weight, thr)
            got = run(tq, tb, tweight, thr, dev, normalize=False)
            print(f"{shape} thr {thr} weight {'int64' if weight is not None else 'None'}: re-draw rounds {rounds}, "
                  f"sum {int(want.sum())}, mismatches {int((got != want).sum())}")
            assert np.array_equal(got, want)
    if N >= 64:
        assert R.count_ref(q, bank, None, 0.9).sum() > 0        # the planted near-duplicates are counted


@pytest.mark.parametrize("D,pad", [(48, 4), (33, 3), (512, 8)])
def test_row_strides_larger_than_D(dev, D, pad):
    """Views of wider buffers whose padding holds NaN: a read past D turns a score into NaN and the count changes."""
    M, N = 65, 129
    q, bank, w, _ = inputs(M, N, D)
    wq = torch.full((M, D + pad), float("nan"), device=dev)
    wb = torch.full((N, D + 2 * pad), float("nan"), device=dev)
    wq[:, :D] = torch.from_numpy(q).to(dev)
    wb[:, :D] = torch.from_numpy(bank).to(dev)
    vq, vb = wq[:, :D], wb[:, :D]
    assert vq.stride(0) == D + pad and vb.stride(0) == D + 2 * pad
    for thr in R.THRESHOLDS:
        assert np.array_equal(run(vq, vb, None, thr, dev, normalize=False), R.count_ref(q, bank, None, thr))


def test_q_is_bank_counts_the_diagonal(dev):
    q, bank, w, _ = inputs(257, 257, 64, same=True)
    assert q is bank
    t, tw = torch.from_numpy(q).to(dev), torch.from_numpy(w).to(dev)
    for thr in R.THRESHOLDS:
        want = R.count_ref(q, q, w, thr)
        assert np.array_equal(run(t, t, tw, thr, dev, normalize=False), want)
        assert np.all(want >= w)                                  # every row counts itself (cosine 1)
        assert np.array_equal(run(t, t, tw, thr, dev, normalize=True), want)      # unit rows stay unit rows


def test_exact_arithmetic_tells_ge_from_gt(dev):
    """Rows +-e_k at D = 4: every dot is exactly -1, 0 or 1.  With >=, threshold 1 counts the row itself and threshold 0 counts
    everything but the opposite row; with > they would count nothing / the row itself only."""
    rows = np.concatenate([np.eye(4), -np.eye(4)]).astype(np.float32)           # row i and row (i + 4) % 8 are opposite
    w = np.arange(1, 9, dtype=np.int64)
    t, tw = torch.from_numpy(rows).to(dev), torch.from_numpy(w).to(dev)
    assert np.array_equal(run(t, t, tw, 1.0, dev, normalize=False), w)
    assert np.array_equal(run(t, t, tw, 0.0, dev, normalize=False), w.sum() - np.roll(w, 4))
    assert np.array_equal(run(t, t, None, 0.0, dev, normalize=False), np.full(8, 7))
    assert np.array_equal(run(t, t, None, 1.0, dev, normalize=True), np.ones(8, dtype=np.int64))


def test_normalize_unnormalised_rows_with_zero_rows(dev):
    thresholds = (0.5, 0.9)
    M, N, D = 70, 131, 48
    q, bank, w, _ = inputs(M, N, D, raw=True, thresholds=thresholds)
    assert not q[0].any() and not bank[0].any() and abs(np.linalg.norm(q[1]) - 1) > 1e-3
    uq, ub = R.unit_rows64(q), R.unit_rows64(bank)
    R.assert_gap(uq, ub, thresholds)
    tq, tb, tw = torch.from_numpy(q).to(dev), torch.from_numpy(bank).to(dev), torch.from_numpy(w).to(dev)
    for thr in thresholds:
        want = R.count_ref(uq, ub, w, thr)
        assert want[0] == 0                                        # the all-zero query row stays zero: cosine 0 with everything
        assert np.array_equal(run(tq, tb, tw, thr, dev, normalize=True), want)


def test_two_calls_agree_and_side_stream(dev):
    M, N, D = 257, 300, 512
    q, bank, w, _ = inputs(M, N, D)
    tq, tb, tw = torch.from_numpy(q).to(dev), torch.from_numpy(bank).to(dev), torch.from_numpy(w).to(dev)
    want = R.count_ref(q, bank, w, 0.5)
    a = run(tq, tb, tw, 0.5, dev, normalize=False)
    b = run(tq, tb, tw, 0.5, dev, normalize=False)
    assert np.array_equal(a, b) and np.array_equal(a, want)
    torch.cuda.synchronize()
    busy = torch.randn(2048, 2048, device=dev)
    side = torch.cuda.Stream()
    for _ in range(8):
        busy = busy @ busy * 1e-3                                  # keeps the default stream busy while the side stream runs
    with torch.cuda.stream(side):
        c = run(tq, tb, tw, 0.5, dev, normalize=False)
    torch.cuda.synchronize()
    assert np.array_equal(c, want)


def test_errors_are_reported_before_any_launch(dev):
    from texttoaudiogrounding_amd import lib, ops
    q = torch.zeros(4, 8, device=dev)
    out, ws = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(64, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="row strides"):
        lib.call("tag_phrase_sim_count", lib.ptr(q), 4, lib.ptr(q), 8, None, 0.5, lib.ptr(out), 4, 4, 8, lib.ptr(ws))
    with pytest.raises(RuntimeError, match="must be >= 1"):
        lib.call("tag_phrase_sim_count", lib.ptr(q), 8, lib.ptr(q), 8, None, 0.5, lib.ptr(out), 4, 0, 8, lib.ptr(ws))
    with pytest.raises(RuntimeError, match=r"N = 2147483647 exceeds 2147483519"):          # each limit has its own message
        lib.call("tag_phrase_sim_count", lib.ptr(q), 8, lib.ptr(q), 8, None, 0.5, lib.ptr(out), 4, 2**31 - 1, 8, lib.ptr(ws))
    with pytest.raises(RuntimeError, match=r"M = 2147483647 exceeds 2147483519"):
        lib.call("tag_phrase_sim_count", lib.ptr(q), 8, lib.ptr(q), 8, None, 0.5, lib.ptr(out), 2**31 - 1, 4, 8, lib.ptr(ws))
    assert ops.query("tag_phrase_sim_count_ws_bytes", 0, 4, 8) == 0
    with pytest.raises(RuntimeError, match="expected q's device"):
        ops.phrase_sim_count(q, torch.zeros(4, 9, device=dev))
    with pytest.raises(RuntimeError, match="weight: expected int64"):
        ops.phrase_sim_count(q, q, torch.zeros(4, device=dev, dtype=torch.int32))


def test_phrase_stats_equals_the_reference_script(dev, golden_dir):
    """utils.phrase_stats.phrase_sim_count over the 40-phrase pickle = the recorded output of the reference's
    calc_phrase_sim_count.main on the same files (tests/golden/make_golden_multi_phrase.py); the gap holds on the fixture."""
    from texttoaudiogrounding_amd.utils import phrase_stats
    d = os.path.join(golden_dir, "multi_phrase")
    with open(os.path.join(d, "sim40_emb.pkl"), "rb") as f:
        emb = pickle.load(f)
    with open(os.path.join(d, "sim40_count.json")) as f:
        counts = json.load(f)
    with open(os.path.join(d, "sim40_sim_count.json")) as f:
        want = json.load(f)
    rows = R.unit_rows64(np.stack(list(emb.values())))
    R.assert_gap(rows, rows, (0.5,))
    got = phrase_stats.phrase_sim_count(emb, counts, threshold=0.5, device=dev)
    assert list(got) == list(want) == list(emb) and all(type(v) is int for v in got.values())
    assert got == want
    assert any(got[p] > counts[p] for p in got)                  # some phrase has a neighbour above the threshold


def test_end_to_end_counts_dataset_collate_train_step(dev, golden_dir, tmp_path):
    """The loader feeds the weak-phrase classes: counts made on the device by phrase_stats.phrase_sim_count -> the phrase_count
    file of SamplePhrasesCountDataset (similarity, phrase_num = 3, two 1-second clips) -> TextCollate(DictTokenizer) -> two
    WeakPhraseRunner.train_step calls with MultiTextBiEncoder(Cnn8Rnn, EmbeddingAgg, DotProduct) and ClipBceLossFreqWeight."""
    from texttoaudiogrounding_amd import losses
    from texttoaudiogrounding_amd.datasets import DictTokenizer, SamplePhrasesCountDataset, TextCollate, write_waveform_pack
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import WeakPhraseRunner
    from texttoaudiogrounding_amd.utils import phrase_stats
    d = os.path.join(golden_dir, "multi_phrase")
    with open(os.path.join(d, "phrase_emb.pkl"), "rb") as f:
        emb = pickle.load(f)
    with open(os.path.join(d, "phrase_count.json")) as f:
        occurrences = json.load(f)
    with open(os.path.join(d, "label.json")) as f:
        clips = json.load(f)[:2]                                   # one and two positives
    sim_counts = phrase_stats.phrase_sim_count(emb, occurrences, threshold=0.5, device=dev)
    assert all(sim_counts[p] >= occurrences[p] for p in emb)       # every phrase counts itself
    with open(tmp_path / "phrase_sim_count.json", "w") as f:
        json.dump(sim_counts, f)
    with open(tmp_path / "label.json", "w") as f:
        json.dump(clips, f)
    g = np.random.RandomState(5)
    tsv = write_waveform_pack(str(tmp_path / "pack.npz"), [(c["audio_id"], 0.1 * g.randn(32000)) for c in clips])
    ds = SamplePhrasesCountDataset(tsv, str(tmp_path / "label.json"), 3, False, "similarity", phrase_embed=os.path.join(d, "phrase_emb.pkl"),
                                   sim_threshold=0.5, negative_pool=os.path.join(d, "negative_pool.txt"),
                                   phrase_count=str(tmp_path / "phrase_sim_count.json"))
    collate = TextCollate(DictTokenizer(os.path.join(golden_dir, "formats", "vocab.pkl")), text_key="phrases", pad_keys=["waveform"])
    torch.manual_seed(0)
    model = audio_text_model.MultiTextBiEncoder(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512),
                                                match.DotProduct(), 512, ["text"])
    runner = WeakPhraseRunner(model, loss_fn=losses.ClipBceLossFreqWeight(100, 0.5), device=dev)
    np.random.seed(2)
    before = runner.flat.flat.detach().clone()
    for step in range(2):
        batch = collate([ds[0], ds[1]])
        assert tuple(batch["waveform"].shape) == (2, 32000) and tuple(batch["text"].shape[:2]) == (2, 3)
        counts = np.asarray(batch["counts"])
        assert counts.shape == (2, 3) and [[sim_counts[p] for p in ps] for ps in batch["phrases"]] == counts.tolist()
        assert batch["label"].tolist() == [[1, 0, 0], [1, 1, 0]]
        if step == 0:
            with torch.no_grad():
                out = runner.forward({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, training=True)
            assert tuple(out["clip_sim"].shape) == np.asarray(out["counts"]).shape == (2, 3)
        loss = runner.train_step(batch)
        value = runner.loss_value(loss)
        print(f"end to end, step {step}: loss {value:.6f}")
        assert np.isfinite(value)
    assert not torch.equal(before, runner.flat.flat)
    assert torch.isfinite(runner.flat.flat).all()
