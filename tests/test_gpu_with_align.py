"""MultiTextBiEncoderWithAlign, WeakPhraseRunner and WeakPhraseSelfSupervisionRunner on the HIP path: the imported reference's
model on stub encoders (tests/golden/with_align.npz (b)), and the whole model against the fp64 composition of the oracle pieces
and the twin tests/align_ref.with_align_tail."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import tag_oracle as O
from tests import align_ref as R

pytestmark = pytest.mark.gpu


def rel(got, want):
    want = torch.as_tensor(want).double()
    return (got.detach().cpu().double() - want).abs().max().item() / (want.abs().max().item() + 1e-30)


class AudioStub(nn.Module):
    downsample_ratio = 1

    def __init__(self, emb, length):
        super().__init__()
        self.e = nn.Parameter(emb.clone())
        self.length, self.embed_dim = length, emb.shape[-1]

    def forward(self, d):
        return {"embedding": self.e, "length": self.length}


class TextStub(nn.Module):
    def __init__(self, table):
        super().__init__()
        self.table = nn.Parameter(table.clone())
        self.embed_dim = table.shape[-1]

    def forward(self, d):
        return {"seq_emb": self.table[d["text"][:, 0].to(self.table.device)]}


def _loss_fn(margin=0.1):
    from texttoaudiogrounding_amd.losses import ClipBceLoss, MaxMarginRankingLoss, MultipleLossSum
    return MultipleLossSum(["clip", "sentence"], [1, 1], clip=ClipBceLoss(),
                           sentence=MaxMarginRankingLoss(margin=margin, sim_key="sentence_sim"))


def _stub_model(gold, dev):
    from texttoaudiogrounding_amd.models import align, audio_text_model, match, sim_pooling
    model = audio_text_model.MultiTextBiEncoderWithAlign(
        AudioStub(torch.from_numpy(gold["b_emb"]), torch.from_numpy(gold["b_length"])), TextStub(torch.from_numpy(gold["b_table"])),
        match.DotProduct(), align.ExpNegL2(), sim_pooling.AudioMeanTextMean(), 32, ["text"])
    return model.to(dev)


def test_fixture_with_stub_encoders(dev, golden_dir):
    gold = np.load(f"{golden_dir}/with_align.npz")
    model = _stub_model(gold, dev).train()
    label = torch.from_numpy(gold["b_label"]).to(dev)
    out = model({"text": torch.from_numpy(gold["b_text"]), "text_len": torch.from_numpy(gold["b_text_len"]), "label": label,
                 "output_matrix": True})
    out["label"] = label
    loss = _loss_fn()(out)
    loss.backward()
    assert out["sim_matrix"].shape == (3, 3, 7, 3) and out["sentence_sim"].shape == (3, 3)
    errs = {k: rel(out[k], gold[f"b_{k}_f64"]) for k in ("frame_sim", "clip_sim", "sentence_sim", "sim_matrix")}
    errs.update(demb=rel(model.audio_encoder.e.grad, gold["b_demb_f64"]), dtable=rel(model.text_encoder.table.grad, gold["b_dtable_f64"]))
    e_loss = abs(loss.item() - float(gold["b_loss_f64"]))
    print("with_align fixture (b):", {k: f"{v:.1e}" for k, v in errs.items()}, f"loss {e_loss:.1e}")
    assert all(v < 5e-6 for v in errs.values()), errs
    assert e_loss < 2e-6


def test_eval_without_label_skips_the_sentence_level(dev, golden_dir):
    gold = np.load(f"{golden_dir}/with_align.npz")
    model = _stub_model(gold, dev).eval()
    inp = {"text": torch.from_numpy(gold["b_text"]), "text_len": torch.from_numpy(gold["b_text_len"])}
    with torch.no_grad():
        out = model(dict(inp))
        assert "sentence_sim" not in out and "sim_matrix" not in out and set(out) == {"frame_sim", "clip_sim", "length"}
        out = model(dict(inp, label=torch.from_numpy(gold["b_label"]).to(dev)))
    assert "sim_matrix" not in out
    assert rel(out["sentence_sim"], gold["b_sentence_sim_f64"]) < 5e-6
    with pytest.raises(ValueError, match="at least one positive phrase"):
        model(dict(inp, label=torch.tensor([[1.0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0]])))


def _batch(seed=5, text_seed=1):
    batch = O.synthetic_batch(2, 48000, seed=seed, ragged=True)
    N, L = 3, 4
    g = torch.Generator().manual_seed(text_seed)
    text = torch.randint(2, 5221, (2, N, L), generator=g)
    text_len = torch.randint(1, L + 1, (2, N), generator=g)
    for b in range(2):
        for n in range(N):
            text[b, n, text_len[b, n]:] = 0
    label = torch.tensor([[1.0, 1, 0], [1, 0, 0]])
    return {"waveform": batch["waveform"], "waveform_len": batch["waveform_len"], "text": text, "text_len": text_len, "label": label}


def _model(st, dev, align_fn, **kw):
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, sim_pooling, text_encoder
    kw.setdefault("match_fn", match.DotProduct())
    model = audio_text_model.MultiTextBiEncoderWithAlign(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512),
                                                        kw.pop("match_fn"), align_fn, sim_pooling.AudioMeanTextMean(), 512, ["text"],
                                                        **kw)
    missing = model.load_state_dict(st, strict=False)
    assert not missing.unexpected_keys and all("melspec" in k for k in missing.missing_keys)
    return model.to(dev)


@pytest.mark.parametrize("kind", ["expnegl2", "dot_scaled"])
def test_whole_model_through_the_runner(dev, kind):
    """Cnn8Rnn + EmbeddingAgg(512), N = 3, eval-mode BN, ClipBceLoss + MaxMarginRankingLoss(sentence_sim) through
    WeakPhraseRunner.forward_backward (direct gradients): the audio embedding feeds the phrase head AND the sentence head, and the
    encoder's parameters must receive the gradient of their sum, once."""
    from texttoaudiogrounding_amd.models import align
    from texttoaudiogrounding_amd.runner import WeakPhraseRunner
    st = O.init_state(seed=19, logit_gain=60.0)
    b = _batch()
    model = _model(st, dev, align.ExpNegL2() if kind == "expnegl2" else align.DotProduct(scaled=True)).eval()
    runner = WeakPhraseRunner(model, loss_fn=_loss_fn(), device=dev)
    runner.flat.zero_grad()
    loss = runner.forward_backward({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()})
    with torch.no_grad():
        out = runner.forward({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}, training=True)
    s64 = O.state_to(st, torch.float64, requires_grad=True)
    ao = O.cnn8rnn_forward(s64, b["waveform"].double(), b["waveform_len"], training=False)
    seq = O.embedding_agg_mean(s64, b["text"].reshape(6, 4), b["text_len"].reshape(-1))["seq_emb"]
    tw = R.with_align_tail(ao["embedding"], seq, ao["length"], b["label"].double(), 3,
                           align="expnegl2" if kind == "expnegl2" else {"scaled": True})
    lo = R.clip_plus_sentence_loss(tw, b["label"].double(), 0.1)
    lo.backward()
    errs = {k: (out[k].cpu().double() - tw[k].detach()).abs().max().item() for k in ("frame_sim", "clip_sim", "sentence_sim")}
    print(f"WithAlign {kind}:", {k: f"{v:.1e}" for k, v in errs.items()}, f"loss {loss.item():.6f} vs {lo.item():.6f}")
    assert out["frame_sim"].shape == tw["frame_sim"].shape == (2, 37, 3)
    assert all(v < 1e-4 for v in errs.values()), errs
    assert abs(loss.item() - lo.item()) < 2e-5
    for name in ("text_encoder.embedding.core.weight", "audio_encoder.fc1.weight", "audio_encoder.rnn.weight_ih_l0"):
        p = dict(model.named_parameters())[name]
        r = rel(p.grad, s64[name].grad)
        print(f"  grad {name}: {r:.1e}")
        assert r < 1e-4, name


def test_sentence_level_does_not_see_the_cross_encoder(dev):
    from texttoaudiogrounding_amd.models import align, match
    from texttoaudiogrounding_amd.models.cross_encoder import CrossAttentionGating
    st = O.init_state(seed=23, logit_gain=30.0)
    st.update(O.init_cross_state(7, 512))
    b = _batch(seed=6, text_seed=2)
    inp = {"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"], "text": b["text"], "text_len": b["text_len"],
           "label": b["label"].to(dev), "specaug": False, "output_matrix": True}
    plain_st = {k: v for k, v in st.items() if not k.startswith("cross_encoder.")}
    with torch.no_grad():
        crossed = _model(st, dev, align.ExpNegL2(), match_fn=match.DotProduct(text_level="token"),
                         cross_encoder=CrossAttentionGating(512), phrase_pooling="max").eval()(dict(inp))
        plain = _model(plain_st, dev, align.ExpNegL2()).eval()(dict(inp))
    assert crossed["clip_sim"].shape == (2, 3) and torch.isfinite(crossed["clip_sim"]).all()
    assert crossed["sim_matrix"].shape == plain["sim_matrix"].shape == (2, 2, 37, 2)
    assert torch.equal(crossed["sentence_sim"], plain["sentence_sim"])
    assert not torch.equal(crossed["clip_sim"], plain["clip_sim"])


def test_train_step_twice(dev):
    from texttoaudiogrounding_amd.models import align
    from texttoaudiogrounding_amd.runner import WeakPhraseRunner
    model = _model(O.init_state(seed=19, logit_gain=60.0), dev, align.ExpNegL2())
    runner = WeakPhraseRunner(model, loss_fn=_loss_fn(), device=dev)
    before = runner.flat.flat.clone()
    losses = [runner.loss_value(runner.train_step(_batch())) for _ in range(2)]
    print("WeakPhraseRunner.train_step x2:", losses)
    assert all(np.isfinite(v) for v in losses) and model.training
    assert (runner.flat.flat - before).abs().max().item() > 0
    assert runner.step_count == 2


def test_self_supervision_runner(dev):
    from texttoaudiogrounding_amd.models import align, audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import WeakPhraseSelfSupervisionRunner
    model = _model(O.init_state(seed=19, logit_gain=60.0), dev, align.ExpNegL2())
    teacher = audio_text_model.MultiTextBiEncoder(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512),
                                                  match.DotProduct(), 512, ["text"])
    teacher.load_state_dict(O.init_state(seed=29, logit_gain=60.0), strict=False)
    runner = WeakPhraseSelfSupervisionRunner(model, teacher, loss_fn=_loss_fn(), device=dev)
    assert not runner.teacher.training and not any(p.requires_grad for p in runner.teacher.parameters())
    assert runner.flat.numel == sum(p.numel() for p in model.parameters())
    state = {k: v.clone() for k, v in runner.teacher.state_dict().items()}
    b = _batch()
    with torch.no_grad():
        t_out = runner.teacher({"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"], "text": b["text"].to(dev),
                                "text_len": b["text_len"].float().to(dev), "label": b["label"].to(dev), "specaug": False})
    runner.model.train()
    out = runner.forward(_batch(), training=True)
    assert torch.equal(out["label"], torch.maximum(b["label"].to(dev), t_out["clip_sim"]))
    assert (out["label"] >= b["label"].to(dev)).all() and out["label"].shape == (2, 3)
    assert torch.equal(out["frame_label"], t_out["frame_sim"]) and not out["label"].requires_grad
    loss = runner.loss_value(runner.train_step(_batch()))
    assert np.isfinite(loss)
    after = runner.teacher.state_dict()
    assert set(after) == set(state) and all(torch.equal(after[k], state[k]) for k in state)      # parameters and BatchNorm buffers
    assert all(p.grad is None for p in runner.teacher.parameters())
