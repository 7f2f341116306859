"""RnnEncoder without a GPU: the reference-shaped interface (constructor, state-dict keys, embed_dim, YAML alias), the fp64
restatement against the fixture made from the imported reference, operator registration with fake kernels, the registered
autograd formula (layer loop, parameter-gradient GEMMs, dropout replay) against plain autograd with the launches replaced
by their restatement, TAG_EINVAL from the new entry points, and the no-CPU-fallback rule."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import text_rnn_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_rnn.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


def _fixture_case(fx, name):
    cfg = R.CONFIGS[name]
    st = {k: torch.from_numpy(fx[f"{name}_param_{k}"]) for k in R.param_names(cfg["layers"], cfg["dirs"])}
    return cfg, st, torch.from_numpy(fx[f"{name}_text"].astype(np.int64)), torch.from_numpy(fx[f"{name}_text_len"].astype(np.int64))


def test_constructor_surface():
    from texttoaudiogrounding_amd.models.text_encoder import EmbeddingLayer, RnnEncoder
    sig = inspect.signature(RnnEncoder.__init__)
    assert list(sig.parameters) == ["self", "vocab_size", "embed_dim", "hidden_dim", "num_layers", "dropout", "bidirectional",
                                    "rnn_type", "pooling"]
    assert sig.parameters["pooling"].default == "mean"
    enc = RnnEncoder(30, 12, 7, 2, 0.25, True, "GRU")
    assert isinstance(enc.embedding, EmbeddingLayer) and isinstance(enc.rnn, torch.nn.GRU)
    assert enc.rnn.batch_first and enc.rnn.bidirectional and enc.rnn.num_layers == 2 and enc.rnn.dropout == 0.25
    assert enc.rnn.input_size == 12 and enc.rnn.hidden_size == 7
    assert enc.embed_dim == 14 and RnnEncoder(30, 12, 7, 1, 0.0, False, "GRU").embed_dim == 7
    assert len(enc.state_dict()) == 17 and len(RnnEncoder(30, 12, 7, 1, 0.0, True, "GRU").state_dict()) == 9
    for kind in ("RNN", "LSTM"):
        with pytest.raises(NotImplementedError, match="no HIP kernel"):
            RnnEncoder(30, 12, 7, 1, 0.0, True, kind)
    with pytest.raises(AssertionError):
        RnnEncoder(30, 12, 7, 1, 0.0, True, "Transformer")
    assert "padded" in RnnEncoder.__doc__ and "row 0" in RnnEncoder.__doc__


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_state_dict_keys_and_shapes_match_the_reference(fx, name):
    from texttoaudiogrounding_amd.models.text_encoder import RnnEncoder
    cfg, st, _, _ = _fixture_case(fx, name)
    enc = RnnEncoder(cfg["V"], cfg["E"], cfg["H"], cfg["layers"], 0.0, cfg["dirs"] == 2, "GRU")
    own = {k: ",".join(map(str, v.shape)) for k, v in enc.state_dict().items()}
    assert list(own) == fx[f"{name}_keys"].tolist() == R.param_names(cfg["layers"], cfg["dirs"])
    assert list(own.values()) == fx[f"{name}_shapes"].tolist()
    assert enc.embed_dim == cfg["H"] * cfg["dirs"]
    missing = enc.load_state_dict(st, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    # the fixture's parameters and inputs are the seeded ones
    drawn = R.draw_params(cfg["V"], cfg["E"], cfg["H"], cfg["layers"], cfg["dirs"], cfg["seed"])
    assert all(torch.equal(drawn[k], st[k]) for k in st)


def test_install_aliases_exposes_the_class():
    import importlib
    import texttoaudiogrounding_amd as pkg
    pkg.install_aliases(force=True)
    mod = importlib.import_module("models.text_encoder")
    assert mod.RnnEncoder is pkg.models.text_encoder.RnnEncoder
    from texttoaudiogrounding_amd.utils import train_util
    if hasattr(train_util, "init_obj_from_str"):
        enc = train_util.init_obj_from_str({"type": "models.text_encoder.RnnEncoder",
                                            "args": dict(vocab_size=20, embed_dim=8, hidden_dim=4, num_layers=1, dropout=0.0,
                                                         bidirectional=True, rnn_type="GRU")})
        assert type(enc).__name__ == "RnnEncoder" and enc.embed_dim == 8


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_restatement_reproduces_the_fixture_fp64(fx, name):
    cfg, st, text, text_len = _fixture_case(fx, name)
    text2, len2 = R.draw_inputs(cfg)
    assert torch.equal(text, text2) and torch.equal(text_len, len2)
    assert int(text_len.min()) == 1 and int(text_len.max()) == cfg["L"]
    got = R.config_results(cfg, st, text, text_len, torch.float64)
    quantities = fx[f"{name}_quantities"].tolist()
    assert sorted(got) == quantities
    for k in quantities:
        e = R.rel_err(got[k], fx[f"{name}_f64_{k}"])
        assert e < 1e-12, (k, e)
    # the recorded fp32 deviation of the reference is of fp32 rounding size (what the GPU bounds are derived from)
    assert fx[f"{name}_f32_dev"].max() < 1.25e-6


def _cpu_patches(monkeypatch):
    """Replace the launches of dispatch.py by their restatement (any dtype, CPU)."""
    from texttoaudiogrounding_amd import dispatch

    def gemm(A, B, M, N, K, transA=False, transB=False, lda=None, ldb=None, out=None, ldc=None, bias=None, act=0,
             accumulate=False):
        # a 2-D operand may be a column window of a wider matrix (its leading dimension is the row stride of the view)
        a = (A[:, :M] if transA else A[:, :K]) if A.dim() == 2 else (A.reshape(K, M) if transA else A.reshape(M, K))
        b = (B[:, :K] if transB else B[:, :N]) if B.dim() == 2 else (B.reshape(N, K) if transB else B.reshape(K, N))
        c = (a.t() if transA else a) @ (b.t() if transB else b)
        if bias is not None:
            c = c + bias
        assert act == 0 and not accumulate
        if out is not None:
            out.copy_(c.view_as(out))
            return out
        return c

    def colsum(x, M, N, ld=None, out=None):
        c = x.reshape(M, N).sum(0)
        if out is not None:
            out.copy_(c)
            return out
        return c

    def recurrence(gi, w_hh, b_hh, text_len, need_grad):
        y, gates, seq, _, _ = R.recurrence(gi, w_hh, b_hh, text_len)
        return y, (gates if need_grad else None), seq

    def dropout(x2d, p, seed, backward):
        return x2d * _keep_mask(seed, x2d.shape, p).to(x2d.dtype) / (1.0 - p)

    monkeypatch.setattr(dispatch, "_chk", lambda t, name: t.contiguous())
    monkeypatch.setattr(dispatch, "gemm", gemm)
    monkeypatch.setattr(dispatch, "colsum", colsum)
    monkeypatch.setattr(dispatch, "text_gru_recurrence", recurrence)
    monkeypatch.setattr(dispatch, "text_gru_recurrence_backward", R.recurrence_backward)
    monkeypatch.setattr(dispatch, "text_gru_dropout", dropout)


def _keep_mask(seed, shape, p):
    g = torch.Generator().manual_seed(int(seed) % (2 ** 31))
    return (torch.rand(*shape, generator=g) >= p)


@pytest.mark.parametrize("name,p", [("l2_bi", 0.0), ("l1_bi", 0.0), ("l2_uni", 0.0), ("l2_bi", 0.3), ("l2_uni", 0.3)])
def test_registered_autograd_formula_equals_plain_autograd_fp64(fx, monkeypatch, name, p):
    import texttoaudiogrounding_amd.torch_ops  # noqa: F401
    from texttoaudiogrounding_amd import dispatch
    _cpu_patches(monkeypatch)
    cfg, st, text, text_len = _fixture_case(fx, name)
    layers, dirs, seed = cfg["layers"], cfg["dirs"], 4242
    s = {k: v.double().clone().requires_grad_(True) for k, v in st.items()}
    names = R.param_names(layers, dirs)[1:]
    x = s["embedding.core.weight"][text]
    tok, seq, saved = torch.ops.tag.text_gru(x, text_len, [s[k] for k in names], dirs, layers, p, seed)
    assert len(saved) == 2 * layers - 1
    wt, ws = R.objective_weights(cfg)
    R.objective(tok, seq, wt, ws).backward()
    masks = None
    if p > 0.0:
        D = cfg["H"] * dirs
        masks = [_keep_mask(dispatch.text_gru_dropout_seed(seed, l), (cfg["R"] * cfg["L"], D), p).view(cfg["R"], cfg["L"], D)
                 for l in range(layers - 1)]
    ref = R.config_results(cfg, st, text, text_len, torch.float64, masks, p)
    assert R.rel_err(tok, ref["token_emb"]) < 1e-12 and R.rel_err(seq, ref["seq_emb"]) < 1e-12
    if p == 0.0:
        assert R.rel_err(tok, fx[f"{name}_f64_token_emb"]) < 1e-12
    for k in ["embedding.core.weight"] + names:
        e = R.rel_err(s[k].grad, ref["d" + k])
        assert e < 1e-11, (k, e)
    # only one of the two outputs used, a frozen parameter and a frozen input: the formula returns None where nothing is needed
    s2 = {k: v.double().clone().requires_grad_(k != names[1]) for k, v in st.items()}
    x2 = s2["embedding.core.weight"][text].detach()
    tok2, seq2, _ = torch.ops.tag.text_gru(x2, text_len, [s2[k] for k in names], dirs, layers, p, seed)
    (seq2 * ws).sum().backward()
    assert s2[names[1]].grad is None and s2["embedding.core.weight"].grad is None
    s3 = {k: v.double().clone().requires_grad_(True) for k, v in st.items()}
    tok3, seq3 = R.encoder_forward(s3, text, text_len, layers, dirs, masks, p)
    (seq3 * ws).sum().backward()
    for k in names:
        if k != names[1]:
            assert R.rel_err(s2[k].grad, s3[k].grad) < 1e-11, k


@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("layers", [1, 2])
def test_operator_fake_kernels(dirs, layers):
    import texttoaudiogrounding_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "text_gru" in T.OP_NAMES and "text_gru_backward" in T.OP_NAMES
    for name in ("text_gru", "text_gru_backward"):
        assert str(getattr(torch.ops.tag, name).default._schema).startswith(f"tag::{name}(")
    E, H, R_, L = 12, 5, 6, 4
    with FakeTensorMode():
        ps = []
        for l in range(layers):
            I = E if l == 0 else dirs * H
            for _ in range(dirs):
                ps += [torch.empty(3 * H, I, requires_grad=True), torch.empty(3 * H, H, requires_grad=True),
                       torch.empty(3 * H, requires_grad=True), torch.empty(3 * H, requires_grad=True)]
        x = torch.empty(R_, L, E, requires_grad=True)
        tok, seq, saved = torch.ops.tag.text_gru(x, torch.empty(R_, dtype=torch.long), ps, dirs, layers, 0.5, 3)
        assert tok.shape == (R_, L, dirs * H) and seq.shape == (R_, dirs * H) and tok.dtype == seq.dtype == torch.float32
        assert [tuple(t.shape) for t in saved] == [(R_, L, dirs, 4 * H)] * layers + [(R_, L, dirs * H)] * (layers - 1)
        (tok.sum() + seq.sum()).backward()                       # the formula runs through the backward operator's fake kernel
        assert x.grad.shape == x.shape and all(p.grad.shape == p.shape for p in ps)
        g = torch.ops.tag.text_gru_backward(None, seq.detach(), x.detach(), torch.empty(R_, dtype=torch.long), tok.detach(),
                                            [t.detach() for t in saved], [p.detach() for p in ps], dirs, layers, 0.5, 3,
                                            [i % 2 == 0 for i in range(len(ps))], False)
        assert len(g) == 1 + len(ps) and g[0].numel() == 0 and g[1].shape == ps[0].shape and g[2].numel() == 0


def test_symbols_declared_exported_and_einval():
    from texttoaudiogrounding_amd import lib, ops
    for name in ("tag_text_gru_forward", "tag_text_gru_backward"):
        assert name in lib.declared_symbols(), name
    for name in ("TextGruFunction", "text_gru_forward", "text_gru_backward", "text_gru_recurrence",
                 "text_gru_recurrence_backward"):
        assert hasattr(ops, name), name
    h = lib.load()
    assert h.tag_abi_version() == 3
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tag_hip.h")).read()
    assert "models/text_encoder.py:117-125" in header
    # bad arguments are refused with TAG_EINVAL and a message; nothing is launched (no GPU is touched)
    one = 16                                                      # any non-null pointer value: the checks come before any use
    ok_fwd = dict(gi=one, w=one, b=one, lens=one, y=one, gates=None, seq=None, R=4, L=3, H=8, dirs=2)

    def fwd(**kw):
        a = dict(ok_fwd, **kw)
        return h.tag_text_gru_forward(a["gi"], a["w"], a["b"], a["lens"], a["y"], a["gates"], a["seq"], a["R"], a["L"], a["H"],
                                      a["dirs"], None)
    for bad in (dict(gi=None), dict(w=None), dict(b=None), dict(y=None), dict(R=0), dict(L=0), dict(H=0), dict(H=513),
                dict(dirs=0), dict(dirs=3), dict(seq=one, lens=None)):
        assert fwd(**bad) == -1, bad
        assert b"argument check failed" in h.tag_last_error()
    ok_bwd = dict(dy=one, dseq=None, lens=one, y=one, gates=one, w=one, dgi=one, dgh=one, hprev=one, R=4, L=3, H=8, dirs=1)

    def bwd(**kw):
        a = dict(ok_bwd, **kw)
        return h.tag_text_gru_backward(a["dy"], a["dseq"], a["lens"], a["y"], a["gates"], a["w"], a["dgi"], a["dgh"], a["hprev"],
                                       a["R"], a["L"], a["H"], a["dirs"], None)
    for bad in (dict(dy=None), dict(y=None), dict(gates=None), dict(w=None), dict(dgi=None), dict(dgh=None), dict(hprev=None),
                dict(dseq=one, lens=None), dict(R=-1), dict(L=0), dict(H=600), dict(dirs=4)):
        assert bwd(**bad) == -1, bad
        assert b"argument check failed" in h.tag_last_error()


def test_cpu_tensors_raise():
    import texttoaudiogrounding_amd.torch_ops  # noqa: F401
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.models.text_encoder import RnnEncoder
    H, E = 4, 6
    ps = [torch.zeros(3 * H, E), torch.zeros(3 * H, H), torch.zeros(3 * H), torch.zeros(3 * H)]
    x, lens = torch.zeros(2, 3, E), torch.tensor([3, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.tag.text_gru(x, lens, ps, 1, 1, 0.0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.TextGruFunction.apply(x, lens, 1, 1, 0.0, 0, *ps)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.text_gru_recurrence(torch.zeros(2, 3, 1, 3 * H), ps[1].view(1, 3 * H, H), ps[3].view(1, 3 * H), None, False)
    enc = RnnEncoder(10, E, H, 1, 0.0, False, "GRU")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc({"text": torch.tensor([[1, 2, 0], [3, 0, 0]]), "text_len": [2, 1]})
