"""CPU: the plain-torch twins of tests/align_ref.py reproduce tests/golden/with_align.npz (the imported reference's ExpNegL2 and
MultiTextBiEncoderWithAlign), and the host-side interface of the new classes: constructor signatures, state-dict keys, YAML-style
construction, the empty-positive check and WeakPhraseRunner's evaluation-time phrase axis."""
import inspect
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import align_ref as R
from tests.golden import ref_import


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(f"{golden_dir}/with_align.npz")


def _t(gold, k, dt):
    return torch.from_numpy(gold[k]).to(dt)


def test_expnegl2_twin_reproduces_the_fixture(gold):
    for dt, sfx, tol in ((torch.float64, "f64", 1e-12), (torch.float32, "ref32", 1e-6)):
        a = _t(gold, "a_audio", dt).requires_grad_(True)
        t = _t(gold, "a_text", dt).requires_grad_(True)
        out = R.exp_neg_l2(a, t)
        (out * _t(gold, "a_dout", dt)).sum().backward()
        assert out.dtype == dt and out.shape == (3, 3, 5, 4)
        for got, key in ((out.detach(), "a_out_"), (a.grad, "a_daudio_"), (t.grad, "a_dtext_")):
            assert (got.double() - _t(gold, key + sfx, torch.float64)).abs().max().item() <= tol, (key, sfx)
    # the copied frame and the doubled frame score exactly 1.0 in the reference
    assert gold["a_out_ref32"][0, 1, 3, 2] == 1.0 and gold["a_out_ref32"][1, 2, 1, 0] == 1.0
    assert np.isfinite(gold["a_daudio_ref32"]).all() and np.isfinite(gold["a_dtext_ref32"]).all()


def test_with_align_twin_reproduces_the_fixture(gold):
    label = _t(gold, "b_label", torch.float64)
    ids = torch.from_numpy(gold["b_text"]).reshape(-1)
    for dt, sfx, tol in ((torch.float64, "f64", 1e-12), (torch.float32, "ref32", 1e-6)):
        e = _t(gold, "b_emb", dt).requires_grad_(True)
        tb = _t(gold, "b_table", dt).requires_grad_(True)
        tw = R.with_align_tail(e, tb[ids], torch.from_numpy(gold["b_length"]), label.to(dt), 4)
        loss = R.clip_plus_sentence_loss(tw, label.to(dt), 0.1)
        loss.backward()
        assert tw["sim_matrix"].shape == gold["b_sim_matrix_" + sfx].shape == (3, 3, 7, 3)
        for k in ("frame_sim", "clip_sim", "sentence_sim", "sim_matrix"):
            assert (tw[k].detach().double() - _t(gold, f"b_{k}_{sfx}", torch.float64)).abs().max().item() <= tol, (k, sfx)
        assert abs(loss.item() - float(gold["b_loss_" + sfx])) <= tol
        assert (e.grad.double() - _t(gold, "b_demb_" + sfx, torch.float64)).abs().max().item() <= tol
        assert (tb.grad.double() - _t(gold, "b_dtable_" + sfx, torch.float64)).abs().max().item() <= tol


def test_full_width_with_text_len_pools_like_the_padded_matrix(gold):
    """The model hands align_fn all N phrases and lets the pooling mask by text_len = label.sum(1); the reference gathers and
    pads.  Every reducer of the twin gives the same (B,B) either way."""
    from oracle import tag_oracle as O
    e = _t(gold, "b_emb", torch.float64)
    seq = _t(gold, "b_table", torch.float64)[torch.from_numpy(gold["b_text"]).reshape(-1)].reshape(3, 4, -1)
    num = torch.from_numpy(gold["b_label"]).sum(1).long().tolist()
    length = torch.from_numpy(gold["b_length"])
    padded = torch.nn.utils.rnn.pad_sequence([seq[i, :num[i]] for i in range(3)], batch_first=True)
    for am in ("mean", "max", "linear_softmax", "exp_softmax"):
        for tm in ("mean", "sum", "max", "mean_sum"):
            full = O.sim_pooling(R.exp_neg_l2(e, seq), length, num, am, tm)
            pad = O.sim_pooling(R.exp_neg_l2(e, padded), length, num, am, tm)
            assert (full - pad).abs().max().item() < 1e-14, (am, tm)


@pytest.mark.skipif(not ref_import.available(), reason="the reference is not on this machine")
def test_constructor_signatures_match_the_reference():
    from texttoaudiogrounding_amd.models import align, audio_text_model
    mods = ref_import.install()
    try:
        ref_model = mods["models.audio_text_model"].MultiTextBiEncoderWithAlign
        ref_align = mods["models.align"].ExpNegL2
        ours, theirs = (inspect.signature(c.__init__) for c in (audio_text_model.MultiTextBiEncoderWithAlign, ref_model))
        assert list(ours.parameters) == list(theirs.parameters)
        assert {k: p.default for k, p in ours.parameters.items()} == {k: p.default for k, p in theirs.parameters.items()}
        assert list(inspect.signature(align.ExpNegL2.__init__).parameters) == list(inspect.signature(ref_align.__init__).parameters)
        assert list(inspect.signature(align.ExpNegL2.forward).parameters) == list(inspect.signature(ref_align.forward).parameters)
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "losses", "utils")]:
            del sys.modules[k]


def _models():
    from texttoaudiogrounding_amd.models import align, audio_encoder, audio_text_model, match, sim_pooling, text_encoder
    plain = audio_text_model.MultiTextBiEncoder(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512),
                                                match.DotProduct(), 512, ["text"])
    both = audio_text_model.MultiTextBiEncoderWithAlign(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512),
                                                        match.DotProduct(), align.ExpNegL2(), sim_pooling.AudioMeanTextMean(),
                                                        512, ["text"])
    return plain, both


def test_state_dict_keys_are_those_of_multitext_biencoder():
    plain, both = _models()
    assert list(both.state_dict()) == list(plain.state_dict())
    assert both.text_forward_keys == ["text", "text_len"] and both.pooling == "linear_softmax"
    assert isinstance(both, type(plain))


def test_build_model_resolves_the_new_type_names():
    import texttoaudiogrounding_amd as pkg
    from texttoaudiogrounding_amd.runner import build_model
    pkg.install_aliases(force=True)
    try:
        cfg = {"audio_encoder": {"type": "models.audio_encoder.Cnn8Rnn", "args": {"sample_rate": 32000}},
               "text_encoder": {"type": "models.text_encoder.EmbeddingAgg", "args": {"embed_dim": 512, "vocab_size": 5221}},
               "match_fn": {"type": "models.match.DotProduct", "args": {"text_level": "seq"}},
               "align_fn": {"type": "models.align.ExpNegL2"},
               "sentence_pooling": {"type": "models.sim_pooling.AudioMeanTextMean"},
               "type": "models.audio_text_model.MultiTextBiEncoderWithAlign",
               "args": {"shared_dim": 512, "text_forward_keys": ["text"], "phrase_pooling": "max"}}
        model = build_model(cfg)
        assert type(model).__name__ == "MultiTextBiEncoderWithAlign" and type(model).__module__.startswith("texttoaudiogrounding_amd")
        assert type(model.align_fn).__name__ == "ExpNegL2" and type(model.align_fn).__module__.startswith("texttoaudiogrounding_amd")
        assert type(model.sentence_pooling).__name__ == "AudioMeanTextMean" and model.pooling == "max"
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "losses", "utils")]:
            del sys.modules[k]


def test_host_label_with_an_empty_row_raises_before_any_launch():
    _, both = _models()
    both.train()
    batch = {"waveform": torch.zeros(2, 32000), "waveform_len": [32000, 32000], "text": torch.ones(2, 3, 2, dtype=torch.long),
             "text_len": torch.ones(2, 3, dtype=torch.long), "label": torch.tensor([[1.0, 0, 0], [0, 0, 0]]), "specaug": False}
    with pytest.raises(ValueError, match="at least one positive phrase"):
        both(batch)


def test_expnegl2_asserts_like_the_reference_and_has_no_cpu_fallback():
    from texttoaudiogrounding_amd.models import align
    with pytest.raises(AssertionError):
        align.ExpNegL2()(torch.zeros(2, 3, 8), torch.zeros(2, 4, 6))
    with pytest.raises(AssertionError):
        align.ExpNegL2()(torch.zeros(2, 3, 8), torch.zeros(3, 4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align.ExpNegL2()(torch.zeros(2, 3, 8), torch.zeros(2, 4, 8))


def test_weak_phrase_runner_forward_adds_the_phrase_axis_at_evaluation():
    from texttoaudiogrounding_amd.runner import WeakPhraseRunner

    class Stub(nn.Module):
        text_forward_keys = ["text", "text_len"]

        def __init__(self):
            super().__init__()
            self.w = nn.Parameter(torch.zeros(1))
            self.seen = None

        def forward(self, d):
            self.seen = dict(d)
            return {"clip_sim": torch.full((d["text"].shape[0], d["text"].shape[1]), 0.5)}

    runner = WeakPhraseRunner(Stub(), device="cpu")
    assert type(runner.loss_fn).__name__ == "ClipBceLoss"
    batch = {"text": torch.ones(2, 5, dtype=torch.int32), "text_len": torch.tensor([5, 3]), "waveform": torch.zeros(2, 8, dtype=torch.float64)}
    out = runner.forward(batch, training=False)
    seen = runner.model.seen
    assert seen["text"].shape == (2, 1, 5) and seen["text"].dtype == torch.int64
    assert seen["text_len"].shape == (2, 1) and seen["text_len"].dtype == torch.float32      # run_weak_phrase.py:41-46 stages floats
    assert seen["waveform"].dtype == torch.float32 and seen["specaug"] is False
    assert "text" not in out                                                                  # no output.update(batch) at evaluation
    batch = {"text": torch.ones(2, 3, 5, dtype=torch.long), "text_len": torch.ones(2, 3), "label": torch.ones(2, 3)}
    out = runner.forward(batch, training=True)
    assert runner.model.seen["text"].shape == (2, 3, 5) and out["label"] is batch["label"] and "clip_sim" in out


def test_shape_beyond_the_index_limits_is_refused_before_any_launch():
    """B*T beyond 2^31 - 1 (and a non-positive size): TAG_EINVAL with the limit named, decided on the host before a launch."""
    from texttoaudiogrounding_amd import lib
    h = lib.load()
    fake = 4096                                            # never dereferenced: the shape check returns first
    assert h.tag_align_expnegl2_forward(fake, fake, fake, 70000, 70000, 2, 8, None) != 0
    msg = h.tag_last_error().decode()
    assert "B*T" in msg and "2147483647" in msg, msg
    assert h.tag_align_expnegl2_backward(fake, fake, fake, fake, fake, 2, 0, 2, 8, fake, None) != 0
    assert ">= 1" in h.tag_last_error().decode()
    assert h.tag_align_expnegl2_ws_bytes(2, 3, 4, 8) >= 2 * 3 * 2 * 4 * 4
