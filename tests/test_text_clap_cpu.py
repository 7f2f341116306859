"""LaionClapEncoder (the trainable LAION-CLAP text tower) without a GPU: the fp64 restatement against the fixture made from the real
transformers modules, the reference-shaped interface (constructor, state-dict keys and shapes, embed_dim, YAML aliases,
build_model), the argument errors raised before any launch, operator registration with fake kernels, the registered autograd
formula and the direct-gradient node against plain autograd with the launches replaced by their restatement, TAG_EINVAL from
the new entry points, the no-CPU-fallback rule, the staging of the tokenizer's keys and HuggingFaceTokenizer itself."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import text_clap_ref as R
from tests import text_selfattn_ref as SA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_clap.npz")
CFG, FX = R.TINY, R.FIXTURE
NAMES = R.param_names(CFG["num_hidden_layers"])


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


def _fixture_inputs(fx):
    return torch.from_numpy(fx["input_ids"].astype(np.int64)), torch.from_numpy(fx["attention_mask"].astype(np.int64))


def test_restatement_reproduces_the_fixture_fp64(fx):
    ids, mask = _fixture_inputs(fx)
    ids2, mask2 = R.draw_inputs(FX["R"], FX["L"], FX["input_seed"], CFG["vocab_size"], CFG["pad_token_id"])
    assert torch.equal(ids, ids2) and torch.equal(mask, mask2)
    lens = mask.sum(-1)
    assert int(lens.min()) == 2 and int(lens.max()) == FX["L"] and int((ids == CFG["pad_token_id"]).sum()) > 0
    st = R.draw_state(CFG, FX["state_seed"])
    got = R.results(st, ids, mask, CFG["num_attention_heads"], torch.float64, CFG["layer_norm_eps"], CFG["pad_token_id"],
                    FX["objective_seed"])
    quantities = fx["quantities"].tolist()
    assert sorted(got) == quantities == sorted(["token_emb", "seq_emb"] + ["d" + k for k in NAMES])
    ref = {k: torch.from_numpy(fx["f64_" + k]) for k in quantities}
    for k in quantities:
        e = R.quantity_err(got, ref, k)
        assert e < 1e-12, (k, e)
    pad = CFG["pad_token_id"]
    for k in ("dmodel.embeddings.word_embeddings.weight", "dmodel.embeddings.position_embeddings.weight"):
        assert float(ref[k][pad].abs().max()) == 0.0 and float(got[k][pad].abs().max()) == 0.0 and float(ref[k].abs().max()) > 0
    # the recorded fp32 deviation of the real modules is of fp32 rounding size (what the GPU bounds are derived from)
    assert fx["f32_dev"].max() < 5e-6


def test_row_kernel_restatements_equal_autograd_fp64():
    g = torch.Generator().manual_seed(2)
    x, res, dy = (torch.randn(7, 48, generator=g, dtype=torch.float64) for _ in range(3))
    gamma, beta = 1 + 0.1 * torch.randn(48, generator=g, dtype=torch.float64), torch.randn(48, generator=g, dtype=torch.float64)
    xs, rs, gs, bs = (t.clone().requires_grad_(True) for t in (x, res, gamma, beta))
    y = torch.nn.functional.layer_norm(xs + rs, (48,), gs, bs, 1e-12)
    (y * dy).sum().backward()
    y2, xhat, rstd = R.ln_forward(x, res, gamma, beta, 1e-12)
    ds, dg, db = R.ln_backward(dy, xhat, rstd, gamma)
    assert R.rel_err(y2, y) < 1e-14 and R.rel_err(ds, xs.grad) < 1e-13 and torch.equal(xs.grad, rs.grad)
    assert R.rel_err(dg, gs.grad) < 1e-13 and R.rel_err(db, bs.grad) < 1e-13
    u = torch.linspace(-8, 8, 4099, dtype=torch.float64).requires_grad_(True)
    f = torch.nn.functional.gelu(u)
    df = torch.randn(4099, generator=g, dtype=torch.float64)
    (f * df).sum().backward()
    assert R.rel_err(R.gelu(u.detach()), f) < 1e-15 and R.rel_err(R.gelu_backward(u.detach(), df), u.grad) < 1e-14
    t = torch.tanh(u.detach()).requires_grad_(False)
    u2 = u.detach().clone().requires_grad_(True)
    (torch.tanh(u2) * df).sum().backward()
    assert R.rel_err(R.tanh_backward(t, df), u2.grad) < 1e-13


def test_constructor_surface_and_state_dict(fx):
    from texttoaudiogrounding_amd.models import hf_modeling_grounding as H
    from texttoaudiogrounding_amd.models.text_encoder import LaionClapEncoder
    sig = inspect.signature(LaionClapEncoder.__init__)
    assert list(sig.parameters) == ["self", "model_type", "config"] and sig.parameters["config"].default is None
    enc = LaionClapEncoder("laion/clap-htsat-fused", CFG)          # does not resolve locally: built from the configuration
    assert enc.embed_dim == CFG["projection_dim"] == 32 and enc.model_type == "laion/clap-htsat-fused"
    own = {k: ",".join(map(str, v.shape)) for k, v in enc.state_dict().items()}
    ref = dict(zip(fx["keys"].tolist(), fx["shapes"].tolist()))
    assert own == ref                                              # names and shapes of the real modules (registration order aside)
    assert sorted(k for k, _ in enc.named_parameters()) == sorted(NAMES) and enc._names == NAMES
    assert all(k.startswith(("model.", "projection.linear1.", "projection.linear2.")) for k in own)
    # the same tree as the inference class, so one checkpoint serves both
    assert list(enc.state_dict()) == list(H.LaionClapEncoder(None, CFG).state_dict())
    st = R.draw_state(CFG, FX["state_seed"])
    missing = enc.load_state_dict(st, strict=True)                 # the two index buffers are optional
    assert not missing.missing_keys and not missing.unexpected_keys
    assert all(torch.equal(enc.state_dict()[k], v) for k, v in st.items())
    enc2 = LaionClapEncoder(None, CFG)
    assert not enc2.load_state_dict(enc.state_dict(), strict=True).missing_keys
    assert all(torch.equal(a, b) for a, b in zip(enc.state_dict().values(), enc2.state_dict().values()))
    # defaults: RoBERTa-base shape, both dropouts 0.1 (ClapTextConfig)
    d = dict(H.CLAP_TEXT_DEFAULTS)
    assert d["hidden_size"] == 768 and d["num_hidden_layers"] == 12
    no_dropout_keys = {k: v for k, v in CFG.items() if not k.endswith("dropout_prob")}
    small = LaionClapEncoder(None, no_dropout_keys)
    assert small.config["hidden_dropout_prob"] == 0.1 and small.config["attention_probs_dropout_prob"] == 0.1
    for word in ("prefix", "position 0", "NOT read back", "counter-based", "local_files_only"):
        assert word in LaionClapEncoder.__doc__, word
    with pytest.raises(NotImplementedError, match="head_dim"):
        LaionClapEncoder(None, dict(CFG, hidden_size=48, num_attention_heads=1))
    with pytest.raises(ValueError, match="num_hidden_layers"):
        LaionClapEncoder(None, dict(CFG, num_hidden_layers=0))


def test_weights_are_copied_from_a_local_clap_model(tmp_path):
    """A ``ClapModel`` saved to a local directory (tiny text AND audio configuration): its text tower's configuration and weights
    are taken over; ``config`` is then not consulted.  Nothing is downloaded."""
    pytest.importorskip("transformers")
    from transformers import ClapConfig, ClapModel
    from texttoaudiogrounding_amd.models.text_encoder import LaionClapEncoder
    audio = dict(spec_size=64, num_mel_bins=16, patch_size=4, patch_stride=[4, 4], patch_embeds_hidden_size=8, depths=[1, 1],
                 num_attention_heads=[1, 2], hidden_size=16, window_size=4, enable_fusion=False, num_classes=3, projection_dim=32)
    text = dict(CFG, hidden_dropout_prob=0.05, attention_probs_dropout_prob=0.15)
    torch.manual_seed(0)
    clap = ClapModel(ClapConfig(text_config=text, audio_config=audio, projection_dim=32))
    clap.save_pretrained(str(tmp_path / "clap"))
    enc = LaionClapEncoder(str(tmp_path / "clap"), {"hidden_size": 128})
    assert enc.embed_dim == 32 and enc.config["hidden_size"] == 64 and enc.config["num_hidden_layers"] == 2
    assert enc.config["hidden_dropout_prob"] == 0.05 and enc.config["attention_probs_dropout_prob"] == 0.15
    own = enc.state_dict()
    for k, v in clap.text_model.state_dict().items():
        assert torch.equal(own["model." + k], v), k
    for k, v in clap.text_projection.state_dict().items():
        assert torch.equal(own["projection." + k], v), k
    assert all(p.requires_grad for p in enc.parameters())


def test_install_aliases_and_build_model():
    import importlib
    import texttoaudiogrounding_amd as pkg
    from texttoaudiogrounding_amd.runner import build_model
    pkg.install_aliases(force=True)
    assert importlib.import_module("models.text_encoder").LaionClapEncoder is pkg.models.text_encoder.LaionClapEncoder
    from texttoaudiogrounding_amd.datasets import text_tokenizer
    assert importlib.import_module("datasets.text_tokenizer").HuggingFaceTokenizer is text_tokenizer.HuggingFaceTokenizer
    model = build_model({"type": "models.audio_text_model.BiEncoder",
                         "audio_encoder": {"type": "models.audio_encoder.CrnnEncoder", "args": {"sample_rate": 32000, "embed_dim": 256}},
                         "text_encoder": {"type": "models.text_encoder.LaionClapEncoder",
                                          "args": {"model_type": "laion/clap-htsat-fused", "config": dict(CFG)}},
                         "match_fn": {"type": "models.match.DotProduct"},
                         "args": {"shared_dim": 64, "add_proj": True, "freeze_text_encoder": True}})
    assert type(model.text_encoder).__name__ == "LaionClapEncoder" and model.text_encoder.embed_dim == 32
    assert not any(p.requires_grad for p in model.text_encoder.parameters()) and model.text_proj.weight.requires_grad
    multi = build_model({"type": "models.audio_text_model.MultiTextBiEncoder",
                         "audio_encoder": {"type": "models.audio_encoder.CrnnEncoder", "args": {"sample_rate": 32000, "embed_dim": 256}},
                         "text_encoder": {"type": "models.text_encoder.LaionClapEncoder", "args": {"model_type": None, "config": dict(CFG)}},
                         "match_fn": {"type": "models.match.DotProduct"},
                         "args": {"shared_dim": 64, "add_proj": True, "text_forward_keys": ["input_ids", "attention_mask"]}})
    assert multi.text_forward_keys == ["input_ids", "attention_mask", "text_len"]


def test_argument_errors_before_any_launch():
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.models.text_encoder import LaionClapEncoder
    enc = LaionClapEncoder(None, CFG)                              # CPU parameters: nothing below may reach a launch
    for L in (1, 65):
        with pytest.raises(ValueError, match="2 ... 64 tokens"):
            enc({"input_ids": torch.zeros(2, L, dtype=torch.long), "attention_mask": torch.ones(2, L, dtype=torch.long)})
    with pytest.raises(ValueError, match="right-padded prefix"):
        enc({"input_ids": torch.zeros(2, 4, dtype=torch.long), "attention_mask": torch.tensor([[1, 1, 1, 0], [1, 0, 1, 0]])})
    with pytest.raises(ValueError, match="right-padded prefix"):
        enc({"input_ids": torch.zeros(1, 2, 3, dtype=torch.long), "attention_mask": torch.tensor([[[1, 1, 0], [0, 1, 1]]])})
    with pytest.raises(ValueError, match="differ in shape"):
        enc({"input_ids": torch.zeros(2, 4, dtype=torch.long), "attention_mask": torch.ones(2, 5, dtype=torch.long)})
    with pytest.raises(IndexError, match="out of range"):
        enc({"input_ids": torch.full((2, 4), 120), "attention_mask": torch.ones(2, 4, dtype=torch.long)})
    with pytest.raises(ValueError, match="2 ... 64 tokens"):
        ops.text_clap_check(64, 4, 65)
    with pytest.raises(ValueError, match="5 \\+ 16 per layer"):
        ops.text_clap_layers(12)
    s0, per = ops.text_clap_dropout_seeds(2 ** 62 - 1, 3)
    flat = [s0] + [s for t in per for s in t]
    assert len(set(flat)) == 10 and all(0 <= s < 2 ** 62 for s in flat)
    assert ops.text_clap_param_names(2) == NAMES


def test_cpu_tensors_raise():
    import texttoaudiogrounding_amd.torch_ops  # noqa: F401
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.models.text_encoder import LaionClapEncoder
    enc = LaionClapEncoder(None, CFG)
    ids, mask = R.draw_inputs(3, 5, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc({"input_ids": ids, "attention_mask": mask})
    ps = [p.detach() for p in enc._params()]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.tag.text_clap(ids, mask, ps, 4, 1e-12, 1, 0.0, 0.0, 0, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.TextClapFunction.apply(ids, mask, 4, 1e-12, 1, 0.0, 0.0, 0, *ps)
    x = torch.zeros(3, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.text_clap_resln_forward(x, None, x[0], x[0], 1e-12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.text_clap_resln_backward(x, x, x[:, 0], x[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.text_clap_embed_forward(ids, ps[0], ps[1], ps[2], ps[3], ps[4], 1e-12, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.text_clap_gelu_forward(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.text_clap_gelu_backward(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.text_clap_tanh_backward(x, x)


# ---------------------------------------------------------------------------------------------- the formula on the CPU
def _keep_mask(seed, shape, p):
    g = torch.Generator().manual_seed(int(seed) % (2 ** 31))
    return torch.rand(*shape, generator=g) >= p


def _strided(t, rows, cols, ld):
    return torch.as_strided(t, (rows, cols), (ld, 1), t.storage_offset())


def _cpu_patches(monkeypatch):
    """Replace the launches of dispatch.py by their restatement (any dtype, CPU); returns the list of launches made."""
    from texttoaudiogrounding_amd import dispatch, functions
    log = []

    def gemm(A, B, M, N, K, transA=False, transB=False, lda=None, ldb=None, out=None, ldc=None, bias=None, act=0,
             accumulate=False):
        log.append("gemm")
        a = _strided(A, K, M, lda or M).t() if transA else _strided(A, M, K, lda or K)
        b = _strided(B, N, K, ldb or K).t() if transB else _strided(B, K, N, ldb or N)
        c = a @ b
        if bias is not None:
            c = c + bias
        c = {0: lambda v: v, 1: torch.relu, 4: torch.tanh}[act](c)
        if out is None:
            assert not accumulate and ldc in (None, N)
            return c.contiguous()
        dst = _strided(out, M, N, ldc or N)
        dst.copy_(dst + c if accumulate else c)
        return out

    def colsum(x, M, N, ld=None, out=None):
        log.append("colsum")
        c = _strided(x, M, N, ld or N).sum(0)
        if out is not None:
            out.view(-1).copy_(c)
            return out
        return c

    def relu_backward(y, dy):
        dy.mul_((y > 0).to(dy.dtype))
        return dy

    def core(qkv, klen, heads, need_attn=True, drop_p=0.0, seed=0):
        log.append("core")
        R_, S = qkv.shape[:2]
        m = _keep_mask(seed, (R_, heads, S, S), drop_p) if drop_p > 0.0 else None
        ctx, attn = SA.core(qkv, klen.clamp(1, S), heads, m, drop_p)
        return ctx, (attn if need_attn else None)

    def core_backward(qkv, attn, dctx, klen, heads, drop_p=0.0, seed=0):
        log.append("core_backward")
        R_, S = qkv.shape[:2]
        m = _keep_mask(seed, (R_, heads, S, S), drop_p) if drop_p > 0.0 else None
        return SA.core_backward(qkv, attn, dctx, klen, heads, m, drop_p)

    def dropout(x2d, p, seed, backward):
        return x2d * _keep_mask(seed, x2d.shape, p).to(x2d.dtype) / (1.0 - p)

    def resln_forward(x, res, gamma, beta, eps, need_state=True, out=None):
        y, xhat, rstd = R.ln_forward(x, res, gamma, beta, eps)
        if out is not None:
            out.copy_(y)
            y = out
        return (y, xhat, rstd) if need_state else (y, None, None)

    def resln_backward(dy, xhat, rstd, gamma, need_dgamma=True, need_dbeta=True, dgamma_out=None, dbeta_out=None):
        log.append("resln_backward")
        ds, dg, db = R.ln_backward(dy, xhat, rstd, gamma)
        if dgamma_out is not None and need_dgamma:
            dg = dgamma_out.copy_(dg)
        if dbeta_out is not None and need_dbeta:
            db = dbeta_out.copy_(db)
        return ds, (dg if need_dgamma else None), (db if need_dbeta else None)

    def embed_forward(ids, word, type0, pos, gamma, beta, eps, pad_id, need_state=True):
        h, p, xhat, rstd = R.embed_forward(ids, word, type0, pos, gamma, beta, eps, pad_id)
        return (h, p, xhat, rstd) if need_state else (h, None, None, None)

    def embed_backward(dh, xhat, rstd, gamma, ids, pos_ids, V, P, pad_id, need=None, outs=None):
        log.append("embed_backward")
        g = list(R.embed_backward(dh, xhat, rstd, gamma, ids, pos_ids, V, P, pad_id))
        for i in range(5):
            if not need[i]:
                g[i] = None
            elif outs is not None and outs[i] is not None:
                g[i] = outs[i].add_(g[i].view_as(outs[i])) if i in (0, 2) else outs[i].copy_(g[i].view_as(outs[i]))
        return g

    def l2norm_backward(x, du):
        n = x.norm(dim=-1, keepdim=True)
        y = x / n
        return (du - y * (y * du).sum(-1, keepdim=True)) / n

    def ids_chk(ids, what):
        if ids.dtype != torch.long:
            raise RuntimeError(what)
        return ids.contiguous()

    monkeypatch.setattr(dispatch, "_chk", lambda t, name: t.contiguous())
    monkeypatch.setattr(dispatch, "_clap_ids_chk", ids_chk)
    for name, fn in dict(gemm=gemm, colsum=colsum, relu_backward=relu_backward, text_selfattn_core=core,
                         text_selfattn_core_backward=core_backward, text_gru_dropout=dropout, text_clap_resln_forward=resln_forward,
                         text_clap_resln_backward=resln_backward, text_clap_embed_forward=embed_forward,
                         text_clap_embed_backward=embed_backward, text_clap_gelu_forward=R.gelu,
                         text_clap_gelu_backward=R.gelu_backward, text_clap_tanh_backward=R.tanh_backward,
                         text_clap_l2norm_backward=l2norm_backward,
                         _l2norm_rows=lambda x, rows, D: torch.nn.functional.normalize(x, dim=-1)).items():
        monkeypatch.setattr(dispatch, name, fn)
    monkeypatch.setattr(functions, "_chk", lambda t, name: t.contiguous(), raising=False)
    return log


def _masks(R_, L, seed, p_h, p_a):
    from texttoaudiogrounding_amd import dispatch
    s_emb, per = dispatch.text_clap_dropout_seeds(seed, CFG["num_hidden_layers"])
    D, H = CFG["hidden_size"], CFG["num_attention_heads"]
    m = {}
    if p_h > 0.0:
        m["emb"] = _keep_mask(s_emb, (R_ * L, D), p_h)
    for l, (s_attn, s_ao, s_out) in enumerate(per):
        if p_a > 0.0:
            m[("attn", l)] = _keep_mask(s_attn, (R_, H, L, L), p_a)
        if p_h > 0.0:
            m[("ao", l)], m[("out", l)] = _keep_mask(s_ao, (R_ * L, D), p_h), _keep_mask(s_out, (R_ * L, D), p_h)
    return m


def _run(direct, s, ids, mask, p_h, p_a, seed, grad=True):
    from texttoaudiogrounding_amd import ops
    ps = [s[k] for k in NAMES]
    H, eps, pad = CFG["num_attention_heads"], CFG["layer_norm_eps"], CFG["pad_token_id"]
    if direct:
        return ops.TextClapFunction.apply(ids, mask, H, eps, pad, p_h, p_a, seed, *ps)
    need = grad and any(p.requires_grad for p in ps)
    return torch.ops.tag.text_clap(ids, mask, ps, H, eps, pad, p_h, p_a, seed, need)[:2]


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("p_h,p_a", [(0.0, 0.0), (0.2, 0.3), (0.0, 0.25)])
def test_registered_autograd_formula_equals_plain_autograd_fp64(fx, monkeypatch, p_h, p_a, direct):
    import texttoaudiogrounding_amd.torch_ops  # noqa: F401
    _cpu_patches(monkeypatch)
    ids, mask = _fixture_inputs(fx)
    st = R.draw_state(CFG, FX["state_seed"])
    seed = 777
    s = {k: v.double().clone().requires_grad_(True) for k, v in st.items()}
    tok, seq = _run(direct, s, ids, mask, p_h, p_a, seed)
    wt, ws = R.objective_weights(*tok.shape, FX["objective_seed"])
    R.objective(tok, seq, wt, ws).backward()
    ref = R.results(st, ids, mask, CFG["num_attention_heads"], torch.float64, CFG["layer_norm_eps"], CFG["pad_token_id"],
                    FX["objective_seed"], _masks(*ids.shape, seed, p_h, p_a), p_h, p_a)
    got = {"token_emb": tok.detach(), "seq_emb": seq.detach(), **{"d" + k: s[k].grad for k in NAMES}}
    for k in ref:
        assert got[k].shape == ref[k].shape, k
        e = R.quantity_err(got, ref, k)
        assert e < (1e-12 if k in ("token_emb", "seq_emb") else 1e-11), (k, e)
    if p_h == 0.0 and p_a == 0.0:
        assert R.rel_err(tok.detach(), fx["f64_token_emb"]) < 1e-12 and R.rel_err(seq.detach(), fx["f64_seq_emb"]) < 1e-12
    pad = CFG["pad_token_id"]
    assert float(got["dmodel.embeddings.word_embeddings.weight"][pad].abs().max()) == 0.0
    assert float(got["dmodel.embeddings.position_embeddings.weight"][pad].abs().max()) == 0.0


@pytest.mark.parametrize("direct", [False, True])
def test_one_frozen_parameter_and_one_output_fp64(fx, monkeypatch, direct):
    import texttoaudiogrounding_amd.torch_ops  # noqa: F401
    log = _cpu_patches(monkeypatch)
    ids, mask = _fixture_inputs(fx)
    st = R.draw_state(CFG, FX["state_seed"])
    frozen = "model.encoder.layer.1.intermediate.dense.weight"
    s = {k: v.double().clone().requires_grad_(k != frozen) for k, v in st.items()}
    tok, seq = _run(direct, s, ids, mask, 0.0, 0.0, 0)
    wt, ws = R.objective_weights(*tok.shape, FX["objective_seed"])
    (3.0 * (seq * ws).sum()).backward()                            # token_emb takes no part: its gradient arrives as None
    ref = R.results(st, ids, mask, CFG["num_attention_heads"], torch.float64, CFG["layer_norm_eps"], CFG["pad_token_id"],
                    wt=torch.zeros_like(wt), ws=ws)
    assert s[frozen].grad is None
    for k in NAMES:
        if k != frozen:
            got = {"d" + n: s[n].grad for n in NAMES if n != frozen}
            assert R.quantity_err(got, ref, "d" + k) < 1e-11, k
    # only the projection trains: the walk stops above the pooler, no layer's backward runs
    del log[:]
    s2 = {k: v.double().clone().requires_grad_(k.startswith("projection.")) for k, v in st.items()}
    tok2, seq2 = _run(direct, s2, ids, mask, 0.0, 0.0, 0)
    R.objective(tok2, seq2, wt, ws).backward()
    full = R.results(st, ids, mask, CFG["num_attention_heads"], torch.float64, CFG["layer_norm_eps"], CFG["pad_token_id"],
                     FX["objective_seed"])
    assert all(R.rel_err(s2[k].grad, full["d" + k]) < 1e-11 for k in NAMES if k.startswith("projection."))
    assert all(s2[k].grad is None for k in NAMES if not k.startswith("projection."))
    assert not {"resln_backward", "core_backward", "embed_backward"} & set(log)


@pytest.mark.parametrize("direct", [False, True])
def test_fully_frozen_encoder_saves_nothing(fx, monkeypatch, direct):
    import texttoaudiogrounding_amd.torch_ops  # noqa: F401
    from texttoaudiogrounding_amd import dispatch
    log = _cpu_patches(monkeypatch)
    seen = []
    forward = dispatch.text_clap_forward

    def spy(*a, **k):
        out = forward(*a, **k)
        seen.append((a[6], out[2]))
        return out
    monkeypatch.setattr("texttoaudiogrounding_amd.functions.text_clap_forward", spy)   # the node's; the operator returns its state
    ids, mask = _fixture_inputs(fx)
    st = R.draw_state(CFG, FX["state_seed"])
    s = {k: v.double().clone() for k, v in st.items()}              # nothing requires grad
    tok, seq = _run(direct, s, ids, mask, 0.0, 0.0, 0)
    assert not tok.requires_grad and not seq.requires_grad
    assert R.rel_err(tok, fx["f64_token_emb"]) < 1e-12 and R.rel_err(seq, fx["f64_seq_emb"]) < 1e-12
    if direct:
        assert seen and seen[-1] == (False, None)                   # need_grad False: no state was kept
    else:
        out = torch.ops.tag.text_clap(ids, mask, [s[k] for k in NAMES], 4, 1e-12, 1, 0.0, 0.0, 0, False)
        assert out[2] == []
    # under no_grad with trainable parameters: the same
    s3 = {k: v.double().clone().requires_grad_(True) for k, v in st.items()}
    with torch.no_grad():
        tok3, _ = _run(direct, s3, ids, mask, 0.0, 0.0, 0, grad=False)
    assert not tok3.requires_grad
    if direct:
        assert seen[-1] == (False, None)
    assert not {"resln_backward", "core_backward", "embed_backward"} & set(log)


def test_operator_fake_kernels():
    import texttoaudiogrounding_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("text_clap", "text_clap_backward"):
        assert name in T.OP_NAMES
        assert str(getattr(torch.ops.tag, name).default._schema).startswith(f"tag::{name}(")
    R_, L, D, I, P, H = 6, 5, CFG["hidden_size"], CFG["intermediate_size"], CFG["projection_dim"], CFG["num_attention_heads"]
    M = R_ * L
    with FakeTensorMode():
        ps = [torch.empty(*s, requires_grad=True) for s in R.param_shapes(CFG)]
        ids, mask = torch.empty(R_, L, dtype=torch.long), torch.empty(R_, L, dtype=torch.long)
        tok, seq, saved = torch.ops.tag.text_clap(ids, mask, ps, H, 1e-12, 1, 0.1, 0.1, 3, True)
        assert tok.shape == (R_, L, P) and seq.shape == (R_, P) and tok.dtype == torch.float32
        assert len(saved) == 7 + 11 * 2
        assert [tuple(t.shape) for t in saved[:7]] == [(M,), (R_,), (M, D), (M,), (M + R_, D), (M + R_, P), (R_, P)]
        assert [tuple(t.shape) for t in saved[7:18]] == [(M, D), (M, 3 * D), (R_, H, L, L), (M, D), (M, D), (M,), (M, D), (M, I),
                                                         (M, I), (M, D), (M,)]
        assert saved[0].dtype == torch.long and saved[1].dtype == torch.long
        (tok.sum() + seq.sum()).backward()                         # the formula runs through the backward operator's fake kernel
        assert all(p.grad.shape == p.shape for p in ps)
        need = [i % 2 == 0 for i in range(len(ps))]
        g = torch.ops.tag.text_clap_backward(tok.detach(), None, ids, [t.detach() for t in saved], [p.detach() for p in ps], H, 1, 0.1,
                                             0.1, 3, need)
        assert len(g) == len(ps) and all((t.shape == p.shape) if n else t.numel() == 0 for t, p, n in zip(g, ps, need))
        out = torch.ops.tag.text_clap(ids, mask, [p.detach() for p in ps], H, 1e-12, 1, 0.0, 0.0, 0, False)
        assert out[2] == [] and out[0].shape == (R_, L, P)


def test_symbols_declared_exported_and_einval():
    from texttoaudiogrounding_amd import lib, ops
    names = ("tag_text_clap_resln_forward", "tag_text_clap_resln_backward", "tag_text_clap_resln_backward_ws_bytes",
             "tag_text_clap_embed_forward", "tag_text_clap_embed_backward", "tag_text_clap_embed_backward_ws_bytes",
             "tag_text_clap_gelu_forward", "tag_text_clap_gelu_backward", "tag_text_clap_tanh_backward")
    for name in names:
        assert name in lib.declared_symbols(), name
    for name in ("TextClapFunction", "text_clap_forward", "text_clap_backward", "text_clap_resln_forward", "text_clap_resln_backward",
                 "text_clap_embed_forward", "text_clap_embed_backward", "text_clap_gelu_forward", "text_clap_gelu_backward",
                 "text_clap_tanh_backward", "text_clap_dropout_seeds", "text_clap_param_names"):
        assert hasattr(ops, name), name
    h = lib.load()
    assert h.tag_abi_version() == 3
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "tag_hip.h")).read()
    assert "models/text_encoder.py:311-327" in header and all(n in header for n in names)
    source = open(os.path.join(root, "texttoaudiogrounding_amd", "csrc", "text_clap.hip")).read()
    assert "atomic" not in source.replace("no atomics", "")
    one = 16                                                      # any non-null pointer value: the checks come before any use
    err = lambda: b"argument check failed" in h.tag_last_error()  # noqa: E731
    # residual + LayerNorm
    ok = dict(x=one, res=None, g=one, b=one, y=one, xhat=one, rstd=one, rows=3, D=64)
    for bad in (dict(x=None), dict(g=None), dict(b=None), dict(y=None), dict(xhat=None), dict(rstd=None), dict(rows=0), dict(D=0),
                dict(D=1025)):
        a = dict(ok, **bad)
        assert h.tag_text_clap_resln_forward(a["x"], a["res"], a["g"], a["b"], 1e-12, a["y"], a["xhat"], a["rstd"], a["rows"], a["D"],
                                             None) == -1 and err(), bad
    ok = dict(dy=one, xhat=one, rstd=one, g=one, ds=one, dg=one, db=one, rows=3, D=64, ws=one)
    for bad in (dict(dy=None), dict(xhat=None), dict(rstd=None), dict(g=None), dict(ds=None), dict(ws=None), dict(rows=0), dict(D=0),
                dict(D=1025)):
        a = dict(ok, **bad)
        assert h.tag_text_clap_resln_backward(a["dy"], a["xhat"], a["rstd"], a["g"], a["ds"], a["dg"], a["db"], a["rows"], a["D"],
                                              a["ws"], None) == -1 and err(), bad
    assert h.tag_text_clap_resln_backward_ws_bytes(0, 64) == 0 and h.tag_text_clap_resln_backward_ws_bytes(3, 1025) == 0
    assert h.tag_text_clap_resln_backward_ws_bytes(4100, 64) > 0
    # embedding block
    ok = dict(ids=one, word=one, type0=one, pos=one, g=one, b=one, h=one, pid=one, xhat=one, rstd=one, B=2, L=5, D=64, V=120, P=72,
              pad=1)

    def emb_fwd(**kw):
        a = dict(ok, **kw)
        return h.tag_text_clap_embed_forward(a["ids"], a["word"], a["type0"], a["pos"], a["g"], a["b"], 1e-12, a["h"], a["pid"],
                                             a["xhat"], a["rstd"], a["B"], a["L"], a["D"], a["V"], a["P"], a["pad"], None)
    for bad in (dict(ids=None), dict(word=None), dict(type0=None), dict(pos=None), dict(g=None), dict(b=None), dict(h=None),
                dict(xhat=None), dict(B=0), dict(L=0), dict(D=0), dict(D=2048), dict(V=0), dict(P=6), dict(pad=-1)):
        assert emb_fwd(**bad) == -1 and err(), bad
    okb = dict(dh=one, xhat=one, rstd=one, g=one, ids=one, pid=one, dword=one, dpos=one, dtype0=one, dg=one, db=one, B=2, L=5, D=64,
               V=120, P=72, pad=1, ws=one)

    def emb_bwd(**kw):
        a = dict(okb, **kw)
        return h.tag_text_clap_embed_backward(a["dh"], a["xhat"], a["rstd"], a["g"], a["ids"], a["pid"], a["dword"], a["dpos"],
                                              a["dtype0"], a["dg"], a["db"], a["B"], a["L"], a["D"], a["V"], a["P"], a["pad"], a["ws"],
                                              None)
    for bad in (dict(dh=None), dict(xhat=None), dict(rstd=None), dict(g=None), dict(ids=None), dict(pid=None), dict(ws=None),
                dict(dword=None, dpos=None, dtype0=None, dg=None, db=None), dict(B=0), dict(L=0), dict(D=0), dict(D=1025), dict(V=0),
                dict(P=6), dict(pad=-1)):
        assert emb_bwd(**bad) == -1 and err(), bad
    assert h.tag_text_clap_embed_backward_ws_bytes(0, 5, 64) == 0 and h.tag_text_clap_embed_backward_ws_bytes(2, 5, 64) > 0
    # element-wise
    for bad in ((None, one, 4), (one, None, 4), (one, one, 0)):
        assert h.tag_text_clap_gelu_forward(bad[0], bad[1], bad[2], None) == -1 and err(), bad
    for fn in (h.tag_text_clap_gelu_backward, h.tag_text_clap_tanh_backward):
        for bad in ((None, one, one, 4), (one, None, one, 4), (one, one, None, 4), (one, one, one, 0)):
            assert fn(*bad, None) == -1 and err(), bad


def test_stage_keeps_the_tokenizer_keys_int64():
    from texttoaudiogrounding_amd.runner import StrongRunner, WeakPhraseRunner
    for cls in (StrongRunner, WeakPhraseRunner):
        runner = cls.__new__(cls)
        runner.device = torch.device("cpu")
        batch = {"input_ids": torch.tensor([[0, 5, 2]], dtype=torch.int32), "attention_mask": torch.tensor([[1, 1, 1]], dtype=torch.int32),
                 "text": torch.tensor([[3, 4]], dtype=torch.int32), "label": torch.tensor([[1, 0]], dtype=torch.int64),
                 "waveform": torch.zeros(1, 8, dtype=torch.float64), "text_len": torch.tensor([3])}
        runner._stage(batch)
        assert batch["input_ids"].dtype == torch.int64 and batch["attention_mask"].dtype == torch.int64
        assert batch["text"].dtype == torch.int64
        assert batch["label"].dtype == torch.float32 and batch["waveform"].dtype == torch.float32
        assert torch.equal(batch["input_ids"], torch.tensor([[0, 5, 2]]))


def _save_tiny_tokenizer(path):
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    words = ["<s>", "<pad>", "</s>", "<unk>", "a", "dog", "barks", "loudly", "rain", "falls", "on", "roof"]
    tok = Tokenizer(models.WordLevel({w: i for i, w in enumerate(words)}, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, pad_token="<pad>", unk_token="<unk>", bos_token="<s>", eos_token="</s>")
    fast.save_pretrained(str(path))


def test_huggingface_tokenizer_on_a_local_directory(tmp_path):
    pytest.importorskip("transformers")
    from texttoaudiogrounding_amd.datasets.text_tokenizer import HuggingFaceTokenizer
    _save_tiny_tokenizer(tmp_path / "tok")
    t = HuggingFaceTokenizer(str(tmp_path / "tok"))
    out = t(["a dog barks", "rain"])
    assert set(out) >= {"input_ids", "attention_mask", "text_len"}
    assert out["input_ids"].dtype == torch.int64 and out["input_ids"].shape == (2, 3)
    assert out["input_ids"].tolist() == [[4, 5, 6], [8, 1, 1]] and out["attention_mask"].tolist() == [[1, 1, 1], [1, 0, 0]]
    assert out["text_len"].tolist() == [3, 1]
    nested = t([["a dog", "rain falls on roof"], ["barks loudly", "a"]])
    assert nested["input_ids"].shape == (2, 2, 4) and nested["attention_mask"].shape == (2, 2, 4)
    assert nested["text_len"].tolist() == [[2, 4], [2, 1]]
    with pytest.raises(AssertionError, match="same"):
        t([["a"], ["a", "dog"]])
    with pytest.raises(AssertionError, match="List"):
        t("a dog")
    assert inspect.signature(HuggingFaceTokenizer.__init__).parameters["model_name"].default == "laion/clap-htsat-fused"


def test_huggingface_tokenizer_missing_name_raises(tmp_path):
    from texttoaudiogrounding_amd.datasets.text_tokenizer import HuggingFaceTokenizer
    with pytest.raises(RuntimeError, match="not available locally"):
        HuggingFaceTokenizer(str(tmp_path / "no-such-tokenizer"))
