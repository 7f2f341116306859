"""CPU: AudioTextCrossAlignByPhrase without a GPU -- the twin tests/cross_align_ref.py against the imported reference
(tests/golden/cross_align.npz), the identity fc_s(attn @ tok) = attn @ (tok Ws^T) + b_s the fused kernel rests on, the
reference-shaped interface, the workspace cap of csrc/cross_pairs.hip and its refusals."""
import inspect
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import tag_oracle as O
from tests import cross_align_ref as R


def _gold(golden_dir):
    g = np.load(f"{golden_dir}/cross_align.npz")
    t = {k: torch.from_numpy(np.asarray(g[k])) for k in g.files}
    prm = [t["p_" + k.replace(".", "_")] for k in R.PARAMS]
    names = ["emb", "tok"] + [k.replace(".", "_") for k in R.PARAMS]
    return t, prm, names


def _tail(t, prm, dtype, project_first):
    lv = R.leaves([t["emb"], t["tok"], *prm], dtype)
    m = R.sim_matrix(lv[0], lv[1], t["length"], t["tok_len"], t["pnum"].tolist(), lv[2:], project_first=project_first)
    sim = O.audio_mean_text_mean(m, t["length"], t["pnum"])
    loss = O.max_margin_ranking_loss(sim, float(t["margin"]), 1.0)
    return m.detach(), sim.detach(), loss.detach(), torch.autograd.grad(loss, lv)


@pytest.mark.parametrize("project_first", [False, True])
def test_twin_fp32_reproduces_the_reference(golden_dir, project_first):
    t, prm, names = _gold(golden_dir)
    assert t["length"].tolist() == [6, 4, 6] and t["pnum"].tolist() == [2, 1, 3] and t["tok"].shape == (6, 4, 32)
    assert 1 <= int(t["tok_len"].min()) and int(t["tok_len"].max()) == 4
    m, sim, loss, grads = _tail(t, prm, torch.float32, project_first)
    errs = {"sim_matrix": (m - t["sim_matrix_ref32"]).abs().max().item(), "sim": (sim - t["sim_ref32"]).abs().max().item(),
            "loss": abs(loss.item() - t["loss_ref32"].item())}
    for k, g in zip(names, grads):
        errs["d_" + k] = (g - t[f"d_{k}_ref32"]).abs().max().item()
    print({k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-6, errs
    # the padded columns of the reference's zero matrix
    assert (m[:, 1, :, 1:] == 0).all() and (m[:, 0, :, 2:] == 0).all()


def _assoc_case(a, w, alen, wlen, pnum, prm, seed):
    dout = torch.randn(len(pnum), len(pnum), a.shape[1], max(pnum), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    o0, g0 = R.grads(a, w, alen, wlen, pnum, prm, dout, project_first=False)
    o1, g1 = R.grads(a, w, alen, wlen, pnum, prm, dout, project_first=True)
    rel = [(o0 - o1).abs().max().item() / o0.abs().max().item()]
    rel += [(x - y).abs().max().item() / (x.abs().max().item() + 1e-300) for x, y in zip(g0, g1)]
    return max(rel)


def test_the_two_associations_of_z_agree_in_fp64(golden_dir):
    t, prm, _ = _gold(golden_dir)
    # the fixture has two fully masked frames (clip 1, frames 4 and 5)
    r = _assoc_case(t["emb"], t["tok"], t["length"], t["tok_len"], t["pnum"].tolist(), prm, 1)
    # a phrase without a token (uniform weights over the padding) and a clip without a phrase
    g = torch.Generator().manual_seed(3)
    D, L = 16, 3
    a, w = torch.randn(3, 5, D, generator=g), torch.randn(4, L, D, generator=g)
    st = O.init_cross_state(5, D)
    prm2 = [st["cross_encoder." + k] for k in R.PARAMS]
    r2 = _assoc_case(a, w, [5, 3, 5], [2, 0, 3, 1], [3, 0, 1], prm2, 2)
    print(f"fc_s(attn @ tok) vs attn @ (tok Ws^T) + b_s in fp64: {r:.1e}, {r2:.1e}")
    assert r < 1e-12 and r2 < 1e-12


class _Enc(nn.Module):
    embed_dim, downsample_ratio = 32, 1

    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(2, 2)


def test_constructor_and_state_dict_follow_the_reference():
    from texttoaudiogrounding_amd.models import audio_text_model, match, sim_pooling
    from texttoaudiogrounding_amd.models.cross_encoder import CrossAttentionGating
    cls = audio_text_model.AudioTextCrossAlignByPhrase
    sig = inspect.signature(cls.__init__)
    assert list(sig.parameters) == ["self", "audio_encoder", "text_encoder", "match_fn", "sim_pooling", "shared_dim", "add_proj",
                                    "cross_encoder", "freeze_audio_encoder", "freeze_text_encoder"]
    assert sig.parameters["add_proj"].default is inspect.Parameter.empty
    assert [sig.parameters[k].default for k in ("cross_encoder", "freeze_audio_encoder", "freeze_text_encoder")] == [None, False, False]
    m = cls(_Enc(), _Enc(), match.DotProduct(text_level="token"), sim_pooling.AudioMeanTextMean(), 32, True,
            cross_encoder=CrossAttentionGating(32), freeze_text_encoder=True)
    assert not hasattr(m, "audio_proj") and not hasattr(m, "text_proj") and m.fused is None
    assert set(m.state_dict()) == {"audio_encoder.lin.weight", "audio_encoder.lin.bias", "text_encoder.lin.weight",
                                   "text_encoder.lin.bias", "cross_encoder.attn.h2attn.weight", "cross_encoder.attn.h2attn.bias",
                                   "cross_encoder.attn.v", "cross_encoder.gating.fc_u.weight", "cross_encoder.gating.fc_u.bias",
                                   "cross_encoder.gating.fc_s.weight", "cross_encoder.gating.fc_s.bias"}
    assert m.audio_encoder.lin.weight.requires_grad and not m.text_encoder.lin.weight.requires_grad


def test_yaml_style_construction_with_aliases():
    import texttoaudiogrounding_amd as pkg
    from texttoaudiogrounding_amd.runner import build_model
    pkg.install_aliases(force=True)
    try:
        cfg = {"audio_encoder": {"type": "models.audio_encoder.Cnn8Rnn", "args": {"sample_rate": 32000}},
               "text_encoder": {"type": "models.text_encoder.EmbeddingAgg",
                                "args": {"embed_dim": 512, "vocab_size": 5221, "aggregation": "mean"}},
               "match_fn": {"type": "models.match.DotProduct", "args": {"text_level": "token"}},
               "cross_encoder": {"type": "models.cross_encoder.CrossAttentionGating", "args": {"embed_dim": 512}},
               "type": "models.audio_text_model.AudioTextCrossAlignByPhrase",
               "sim_pooling": {"type": "models.sim_pooling.AudioMeanTextMean", "args": {}},
               "args": {"shared_dim": 512, "add_proj": False}}
        model = build_model(cfg)
        assert type(model).__name__ == "AudioTextCrossAlignByPhrase"
        assert type(model).__module__.startswith("texttoaudiogrounding_amd")
        assert type(model.cross_encoder).__module__.startswith("texttoaudiogrounding_amd") and model._fusable(8, 512)
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "losses", "utils")]:
            del sys.modules[k]


def test_workspace_cap_and_refusals():
    from texttoaudiogrounding_amd import lib, ops
    B, T, P, L, D = 32, 250, 128, 8, 512
    total = ops.query("tag_crosspairs_ws_bytes", B, T, P, L, D)
    bwd = ops.query("tag_crosspairs_backward_ws_bytes", B, T, P, L, D)
    print(f"cross_pairs at (32,250,128,8,512): {total / 1e6:.1f} MB kept + scratch, of which backward workspace {bwd / 1e6:.1f} MB; "
          f"one (B,P,T,D) fp32 tensor is {B * P * T * D * 4 / 1e6:.0f} MB")
    assert 0 < bwd < total < B * P * T * D * 4 / 8
    # at least alpha (B,P,T,L) and a dscore of its size
    assert total >= 2 * B * P * T * L * 4
    h = lib.load()
    for D_ok in range(32, 1025, 32):
        assert ops.query("tag_crosspairs_ws_bytes", 2, 3, 4, 32, D_ok) > 0 and ops.cross_pairs_served(32, D_ok)
    assert ops.query("tag_crosspairs_ws_bytes", 2, 3, 4, 33, 64) == 0 and b"L = 33" in h.tag_last_error()
    assert not ops.cross_pairs_served(33, 64)
    for bad in (48, 1056, 16):
        assert ops.query("tag_crosspairs_ws_bytes", 2, 3, 4, 8, bad) == 0
        assert f"D = {bad} is not served".encode() in h.tag_last_error()
        assert ops.query("tag_crosspairs_backward_ws_bytes", 2, 3, 4, 8, bad) == 0 and not ops.cross_pairs_served(8, bad)


def test_cpu_tensors_raise():
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.models import audio_text_model, match, sim_pooling
    from texttoaudiogrounding_amd.models.cross_encoder import CrossAttentionGating
    D = 64
    st = O.init_cross_state(3, D)
    prm = [st["cross_encoder." + k] for k in R.PARAMS]
    a, w = torch.randn(2, 3, D), torch.randn(3, 2, D)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.CrossPairsFunction.apply(a, [3, 2], w, [2, 1, 2], [2, 1], *prm, True)

    class Audio(nn.Module):
        def forward(self, d):
            return {"embedding": a, "length": torch.tensor([3, 2])}

    class Text(nn.Module):
        def forward(self, d):
            return {"token_emb": w}

    for fused in (None, False):
        model = audio_text_model.AudioTextCrossAlignByPhrase(Audio(), Text(), match.DotProduct(text_level="token"),
                                                             sim_pooling.AudioMeanTextMean(), D, False, CrossAttentionGating(D))
        model.fused = fused
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model({"text_key": "phrases", "phrases": torch.zeros(3, 2, dtype=torch.long), "phrases_len": torch.tensor([2, 1, 2]),
                   "phrases_num": [2, 1]})
