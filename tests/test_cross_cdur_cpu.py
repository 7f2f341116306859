"""CPU: the early-fusion CrossCDur (models/audio_text_model.py:461-568 in the reference) behind the reference interface --
constructor, YAML construction, state-dict keys, shapes and parameter count against the fixture made from the reference, the
seeded state dict, the refusals before any launch, the operator's fake kernel and the new C entry points."""
import os
import re

import numpy as np
import pytest
import torch

from tests import cross_cdur_state as CS


def _model(**kw):
    from texttoaudiogrounding_amd.models import audio_text_model as M, text_encoder as TE
    torch.manual_seed(0)
    return M.CrossCDur(32000, TE.EmbeddingAgg(CS.VOCAB, CS.D_TEXT), **kw)


FRONTEND_BUFFERS = ["melspec_extractor.spectrogram.window", "melspec_extractor.mel_scale.fb"]


def test_constructor_signature_and_attributes():
    import inspect
    from texttoaudiogrounding_amd.models import audio_text_model as M
    assert list(inspect.signature(M.CrossCDur.__init__).parameters) == ["self", "sample_rate", "text_encoder", "upsample"]
    assert inspect.signature(M.CrossCDur.__init__).parameters["upsample"].default is False
    assert list(inspect.signature(M.CDurTextBlock.__init__).parameters) == ["self", "cin", "cout", "text_emb_dim", "kernel_size",
                                                                            "padding"]
    m = _model(upsample=True)
    assert (m.hop_length, m.text_emb_dim, m.interpolate_ratio, m.upsample) == (640, 256, 4, True)
    assert _model().upsample is False
    assert m.get_rnn_input_dim() == 128 and m.gru.input_size == 128 and m.gru.hidden_size == 128 and m.gru.bidirectional
    for name in ("block1", "block2", "block3", "block4", "block5", "pool1", "pool2", "pool3", "dropout", "gru", "fc_text",
                 "fc_output", "text_encoder"):
        assert hasattr(m, name), name
    assert (m.pool1.kernel_size, m.pool3.kernel_size, m.dropout.p) == ((2, 4), (1, 4), 0.3)


def test_state_dict_matches_the_reference_fixture(golden_dir):
    gold = np.load(f"{golden_dir}/cross_cdur.npz")
    ref = [(str(k), tuple(int(v) for v in str(s).split(",") if v)) for k, s in zip(gold["keys"], gold["shapes"])]
    assert len(ref) == 53 and ref == CS.reference_keys()
    m = _model()
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert sorted(mine) == sorted([k for k, _ in ref] + FRONTEND_BUFFERS)
    for k, s in ref:
        assert mine[k] == s, k
    assert sum(p.numel() for n, p in m.named_parameters() if not n.startswith("text_encoder")) == 884_355
    assert sum(p.numel() for p in m.parameters()) == 884_355 + CS.VOCAB * CS.D_TEXT


def test_seeded_state_loads_and_matches_the_fixture_checksum(golden_dir):
    gold = np.load(f"{golden_dir}/cross_cdur.npz")
    st = CS.draw_state(gold["block1_bn_running"])
    assert np.allclose(CS.state_checksum(st), gold["state_checksum"], rtol=1e-9), "seeded weights drifted from the fixture"
    m = _model()
    res = m.load_state_dict(st, strict=False)
    assert sorted(res.missing_keys) == sorted(FRONTEND_BUFFERS) and res.unexpected_keys == []
    assert torch.equal(m.block3.fc_text.bias, st["block3.fc_text.bias"]) and int(m.block2.bn.num_batches_tracked) == 3
    b = CS.eval_batch()
    assert np.allclose(CS.checksum(b["waveform"]) + CS.checksum(b["text"].float()), gold["input_checksum"], rtol=1e-9)


def test_cdur_text_block_keys():
    from texttoaudiogrounding_amd.models.audio_text_model import CDurTextBlock
    blk = CDurTextBlock(32, 128, 256)
    assert list(blk.state_dict()) == ["bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked",
                                      "conv.weight", "fc_text.weight", "fc_text.bias"]
    assert blk.conv.bias is None and blk.conv.weight.shape == (128, 32, 3, 3) and blk.fc_text.weight.shape == (128, 256)
    assert isinstance(blk.activation, torch.nn.LeakyReLU) and blk.activation.negative_slope == 0.1


def test_constructor_reinitialises_the_embedding():
    """The reference quirk: ``self.apply(init_weights)`` runs over the text encoder too."""
    from texttoaudiogrounding_amd.models import audio_text_model as M, text_encoder as TE
    te = TE.EmbeddingAgg(300, 64)
    with torch.no_grad():
        te.embedding.core.weight.fill_(7.0)
    m = M.CrossCDur(32000, te)
    w = m.text_encoder.embedding.core.weight.detach()
    assert float(w.abs().max()) <= (6.0 / 64) ** 0.5 + 1e-6 and float(w.std()) > 0.05
    # zero biases, BatchNorm weight 1 / bias 0 (models/utils.py:5-20)
    assert all(float(t.detach().abs().max()) == 0 for t in (m.fc_text.bias, m.fc_output.bias, m.block2.fc_text.bias, m.block4.bn.bias))
    assert float((m.block5.bn.weight.detach() - 1).abs().max()) == 0


def test_yaml_construction_through_aliases():
    import texttoaudiogrounding_amd as P
    from texttoaudiogrounding_amd.runner import build_model
    P.install_aliases()
    cfg = {"type": "models.audio_text_model.CrossCDur", "args": {"sample_rate": 32000, "upsample": True},
           "text_encoder": {"type": "models.text_encoder.EmbeddingAgg", "args": {"vocab_size": 300, "embed_dim": 64}}}
    m = build_model(cfg)
    assert type(m).__name__ == "CrossCDur" and m.text_emb_dim == 64 and m.upsample is True
    assert m.block1.fc_text.weight.shape == (32, 64) and m.fc_text.weight.shape == (256, 64)


def _cpu_batch():
    # no "specaug" / "mixup_lambda" keys: the reference's forward reads neither
    return {"waveform": torch.zeros(2, 32000), "waveform_len": [32000, 30000], "text": torch.ones(2, 3, dtype=torch.long),
            "text_len": torch.tensor([3, 2])}


def test_cpu_tensor_refused_without_fallback():
    m = _model().train()
    with pytest.raises(RuntimeError, match="cuda|no CPU fallback"):
        m(_cpu_batch())


@pytest.mark.parametrize("setting", [("CONV_MATH", "x3"), ("ACT_DTYPE", "bf16"), ("GEMM_MATH", "bf16")])
def test_non_fp32_mode_refused_before_any_launch(setting):
    from texttoaudiogrounding_amd import ops
    m = _model().train()
    name, value = setting
    old = getattr(ops, name)
    try:
        setattr(ops, name, value)
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            m(_cpu_batch())
    finally:
        setattr(ops, name, old)


def test_operator_registered_with_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import texttoaudiogrounding_amd.torch_ops as T
    assert "cross_cdur" in T.OP_NAMES
    assert str(torch.ops.tag.cross_cdur.default._schema).startswith("tag::cross_cdur(")
    m = _model()
    tok = T.encoder_token(m)
    params = list(m._flat_params())
    assert len(params) == 25
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        wave = mode.from_tensor(torch.zeros(3, 64000))
        texts = [mode.from_tensor(torch.zeros(3, c)) for c in (32, 128, 128, 128, 128, 256)]
        out = torch.ops.tag.cross_cdur(wave, texts, [mode.from_tensor(p.detach()) for p in params], tok, False)
    assert tuple(out.shape) == (3, (64000 // 640 + 1) // 4)


def test_new_entry_points_declared_and_abi_version_unchanged():
    from texttoaudiogrounding_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "tag_hip.h")).read()
    for name in ("tag_conv3x3_forward_bias", "tag_conv3x3_c1_forward_bias", "tag_lppool_leaky_backward_clip",
                 "tag_bn_act_backward_clip", "tag_leaky_forward", "tag_leaky_backward"):
        assert name in lib.declared_symbols(), name
        assert re.search(rf"\b{name}\s*\(", header), name
    assert re.search(r"#define\s+TAG_ABI_VERSION\s+3\b", header) and lib.ABI_VERSION == 3
