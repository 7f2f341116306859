"""IntraAttention without a GPU: the fp64 restatement against the fixture made from the imported reference, the restatement on
what the reference cannot run (leading dimensions) and on text_len = 0, the reference-shaped interface (constructor, attributes,
state-dict keys and shapes, ConvGRUCell's init, YAML alias, build_model with a nested embedding), the argument errors raised at
construction or before any launch, operator registration with fake kernels, the explicit backward formulas, the registered
autograd formula and the direct-gradient node against plain autograd with the launches replaced by their restatement (gradients
shared over 3 layers, both dropout replays, frozen table / gates, no dseq, no dtok), TAG_EINVAL from the new entry points, and the
no-CPU-fallback rule."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import text_intra_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_intra.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


def _fixture_case(fx, name):
    cfg = R.CONFIGS[name]
    st = {k: torch.from_numpy(fx[f"{name}_param_{k}"]) for k in R.param_names(cfg["agg"])}
    st["pe.pe"] = R.position_table(cfg["E"])
    return cfg, st, torch.from_numpy(fx[f"{name}_text"].astype(np.int64)), torch.from_numpy(fx[f"{name}_text_len"].astype(np.int64))


def _inner(cfg):
    from texttoaudiogrounding_amd.models.text_encoder import EmbeddingAgg, EmbeddingLayer
    return (EmbeddingAgg if cfg["agg"] else EmbeddingLayer)(cfg["V"], cfg["E"])


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_restatement_reproduces_the_fixture_fp64(fx, name):
    cfg, st, text, text_len = _fixture_case(fx, name)
    text2, len2 = R.draw_inputs(cfg)
    assert torch.equal(text, text2) and torch.equal(text_len, len2)
    assert int(text_len.min()) == 1 and int(text_len.max()) == (cfg["L"] - 1 if cfg["short"] else cfg["L"])
    drawn = R.draw_params(cfg["V"], cfg["E"], cfg["seed"], cfg["scale"], cfg["agg"])
    assert all(torch.equal(drawn[k], st[k]) for k in st)
    assert all(float(st[k].abs().min()) > 0 for k in R.GATE_NAMES if k.endswith("bias")), "biases must be drawn non-zero"
    got = R.config_results(cfg, st, text, text_len, torch.float64)
    quantities = fx[f"{name}_quantities"].tolist()
    assert sorted(got) == quantities == sorted(["token_emb", "seq_emb"] + ["d" + k for k in R.param_names(cfg["agg"])])
    for k in quantities:
        e = R.rel_err(got[k], fx[f"{name}_f64_{k}"])
        assert e < 1e-12, (k, e)
    assert fx[f"{name}_keys"].tolist() == R.state_names(cfg["agg"])
    # the recorded fp32 deviation of the reference is of fp32 rounding size (what the GPU bounds are derived from)
    assert fx[f"{name}_f32_dev"].max() < 2.5e-6
    assert float(torch.from_numpy(fx[f"{name}_f64_token_emb"])[0, -1].abs().max()) > 0, "token_emb is non-zero at padded positions"


def test_restatement_leading_dimensions_and_empty_phrases(fx):
    """What the reference cannot run (a 3-D text) equals the flattened batch; text_len = 0 gives a finite token_emb in which the
    empty row is what a uniform attention over all L positions produces, and a 0/0 seq_emb."""
    cfg, st, text, text_len = _fixture_case(fx, "e64_n2")
    s = {k: v.double() for k, v in st.items()}
    tok, seq = R.encoder_forward(s, text, text_len, cfg["layers"])
    tok3, seq3 = R.encoder_forward(s, text.view(4, 12, -1), text_len.view(4, 12), cfg["layers"])
    assert tok3.shape == (4, 12, cfg["L"], cfg["E"]) and seq3.shape == (4, 12, cfg["E"])
    assert torch.equal(tok3.reshape(tok.shape), tok) and torch.equal(seq3.reshape(seq.shape), seq)
    ztext, zlen = R.draw_inputs(cfg, zero=True)
    assert int(zlen[0]) == 0
    ztok, zseq = R.encoder_forward(s, ztext, zlen, cfg["layers"])
    assert torch.isfinite(ztok).all() and torch.isnan(zseq[0]).all() and torch.isfinite(zseq[1:]).all()
    x = s["embedding.core.weight"][ztext[:1]]
    msg, attn = R.core(x, s["pe.pe"][0], zlen[:1])
    assert torch.equal(attn, torch.full_like(attn, 1.0 / cfg["L"])) and R.rel_err(msg, x.mean(1, keepdim=True).expand_as(x)) < 1e-14
    assert R.rel_err(ztok[1:], tok[1:]) < 1e-14, "rows never interact"


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_explicit_backward_formulas_equal_autograd_fp64(p):
    g = torch.Generator().manual_seed(5)
    R_, L, E = 6, 7, 16
    x = 0.4 * torch.randn(R_, L, E, generator=g, dtype=torch.float64)
    dmsg = torch.randn(R_, L, E, generator=g, dtype=torch.float64)
    pe = R.position_table(E)[0].double()
    lens = torch.tensor([1, L, 3, 0, 6, 2])
    ma, mb = (_keep_mask(9, (R_, L, E), p), _keep_mask(10, (R_, L, E), p)) if p > 0.0 else (None, None)
    ref = R.core_results(x, pe, lens, dmsg, torch.float64, ma, mb, p)
    assert R.rel_err(ref["attn"].sum(-1), torch.ones(R_, L)) < 1e-14
    assert torch.equal(ref["attn"][3], torch.full((L, L), 1.0 / L, dtype=torch.float64)) and float(ref["attn"][0, 0, 1:].min()) > 0
    assert R.rel_err(R.core_backward(dmsg, x, pe, ref["attn"], lens, ma, mb, p), ref["dx"]) < 1e-13
    # the cell's element-wise steps
    lens = lens.clamp(min=1)
    t = [torch.randn(R_, L, E, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(4)]
    u_pre, r_pre, o_raw, xx = t
    u, r, xr = R.cell_elementwise(u_pre, r_pre, xx)
    o, new = R.cell_update(o_raw + xr, u, xx)
    dnew, dseq = torch.randn(R_, L, E, generator=g, dtype=torch.float64), torch.randn(R_, E, generator=g, dtype=torch.float64)
    ((new * dnew).sum() + (R.masked_mean(new, lens) * dseq).sum()).backward()
    do_pre, du_pre, dx = R.cell_update_backward(dnew, dseq, lens, xx.detach(), u.detach(), o.detach())
    dr_pre, dx = R.cell_gates_backward(do_pre, xx.detach(), r.detach(), dx)
    assert R.rel_err(do_pre, o_raw.grad) < 1e-13 and R.rel_err(du_pre * 1.0, u_pre.grad) < 1e-13
    assert R.rel_err(dr_pre, r_pre.grad) < 1e-13 and R.rel_err(dx, xx.grad) < 1e-13


def test_constructor_surface():
    from texttoaudiogrounding_amd.models.text_encoder import ConvGRUCell, EmbeddingAgg, EmbeddingLayer, IntraAttention, PositionalEncoding
    sig = inspect.signature(IntraAttention.__init__)
    assert list(sig.parameters) == ["self", "embedding", "num_layers", "pooling"] and sig.parameters["pooling"].default == "mean"
    assert list(inspect.signature(ConvGRUCell.__init__).parameters) == ["self", "input_size", "hidden_size", "kernel_size"]
    inner = EmbeddingLayer(30, 32)
    enc = IntraAttention(inner, 3)
    assert enc.embedding is inner and enc.embed_dim == 32 and enc.num_layers == 3 and enc.pooling == "mean"
    assert isinstance(enc.pe, PositionalEncoding) and enc.pe.p == 0.2 and isinstance(enc.conv_gru, ConvGRUCell)
    assert enc.conv_gru.input_size == 32 and enc.conv_gru.hidden_size == 32
    for gate in (enc.conv_gru.reset_gate, enc.conv_gru.update_gate, enc.conv_gru.out_gate):
        w = gate.weight.detach().double()
        assert w.shape == (32, 64) and float(gate.bias.detach().abs().max()) == 0.0
        assert R.rel_err(w @ w.t(), torch.eye(32)) < 1e-5, "orthogonal rows"
    assert IntraAttention(EmbeddingAgg(30, 16), 1).embed_dim == 16
    for word in ("1e-10", "uniformly", "independent dropout masks", "x, not x + pe", "padded positions", "row 0", "counter-based",
                 "leading dimensions", "0/0", "num_layers", "accumulate"):
        assert word in IntraAttention.__doc__, word


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_state_dict_keys_and_shapes_match_the_reference(fx, name):
    from texttoaudiogrounding_amd.models.text_encoder import IntraAttention
    cfg, st, _, _ = _fixture_case(fx, name)
    enc = IntraAttention(_inner(cfg), cfg["layers"])
    own = {k: ",".join(map(str, v.shape)) for k, v in enc.state_dict().items()}
    assert list(own) == fx[f"{name}_keys"].tolist()
    assert list(own.values()) == fx[f"{name}_shapes"].tolist()
    assert [k for k, _ in enc.named_parameters()] == R.param_names(cfg["agg"])
    assert torch.equal(enc.pe.pe, st["pe.pe"]) and enc.pe.pe.shape == (1, 100, cfg["E"])
    missing = enc.load_state_dict(st, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys


def test_install_aliases_and_build_model():
    import importlib
    import texttoaudiogrounding_amd as pkg
    from texttoaudiogrounding_amd.runner import build_model
    pkg.install_aliases(force=True)
    mod = importlib.import_module("models.text_encoder")
    assert mod.IntraAttention is pkg.models.text_encoder.IntraAttention and mod.ConvGRUCell is pkg.models.text_encoder.ConvGRUCell
    model = build_model({"type": "models.audio_text_model.BiEncoder",
                         "audio_encoder": {"type": "models.audio_encoder.CrnnEncoder", "args": {"sample_rate": 32000, "embed_dim": 256}},
                         "text_encoder": {"type": "models.text_encoder.IntraAttention",
                                          "embedding": {"type": "models.text_encoder.EmbeddingLayer",
                                                        "args": {"vocab_size": 200, "embed_dim": 256}},
                                          "args": {"num_layers": 2}},
                         "match_fn": {"type": "models.match.DotProduct"}, "args": {"shared_dim": 256}})
    enc = model.text_encoder
    assert type(enc).__name__ == "IntraAttention" and enc.embed_dim == 256 and enc.num_layers == 2
    assert type(enc.embedding).__name__ == "EmbeddingLayer"
    own = [k for k in model.state_dict() if k.startswith("text_encoder.")]
    assert own == ["text_encoder." + k for k in R.state_names()]
    enc.load_state_dict(R.model_text_state(), strict=True)
    assert all(torch.equal(model.state_dict()["text_encoder." + k], v) for k, v in R.model_text_state().items())


def test_argument_errors_name_the_limit():
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.models.text_encoder import EmbeddingLayer, IntraAttention

    class Inner(torch.nn.Module):
        def __init__(self, E):
            super().__init__()
            self.embed_dim = E

    with pytest.raises(ValueError, match="odd"):
        IntraAttention(Inner(33), 1)
    with pytest.raises(ValueError, match="embed_dim <= 1024"):
        IntraAttention(Inner(1026), 1)
    with pytest.raises(ValueError, match="no embed_dim"):
        IntraAttention(torch.nn.Embedding(10, 8), 1)
    for E in (2, 6, 64, 130, 512, 1024):
        ops.text_intra_check(E, 1)
        ops.text_intra_check(E, 64)
    with pytest.raises(ValueError, match="1 ... 64 tokens"):
        ops.text_intra_check(32, 65)
    with pytest.raises(ValueError, match="1 ... 64 tokens"):
        ops.text_intra_check(32, 0)
    # more than 64 tokens: refused before the embedding lookup (CPU ids and CPU parameters never reach a launch)
    enc = IntraAttention(EmbeddingLayer(20, 32), 2)
    with pytest.raises(ValueError, match="at most 64"):
        enc({"text": torch.zeros(2, 65, dtype=torch.long), "text_len": [3, 65]})
    seeds = ops.text_intra_dropout_seeds(2 ** 62 - 2, 3)
    flat = [s for pair in seeds for s in pair]
    assert len(seeds) == 3 and len(set(flat)) == 6 and all(0 <= s < 2 ** 62 for s in flat)


def _keep_mask(seed, shape, p):
    g = torch.Generator().manual_seed(int(seed) % (2 ** 31))
    return (torch.rand(*shape, generator=g) >= p)


def _cpu_patches(monkeypatch):
    """Replace the launches of dispatch.py by their restatement (any dtype, CPU)."""
    from texttoaudiogrounding_amd import dispatch, functions

    def gemm(A, B, M, N, K, transA=False, transB=False, lda=None, ldb=None, out=None, ldc=None, bias=None, act=0,
             accumulate=False):
        a = A.reshape(K, M).t() if transA else A.reshape(M, K)
        b = B[:N, :K].t() if transB else B[:K, :N]
        assert (ldb or b.shape[1]) == B.stride(0) and act == 0
        c = a @ b
        if bias is not None:
            c = c + bias
        if out is None:
            assert not accumulate
            return c
        assert out.stride(0) == (ldc or N)
        dst = out[:, :N]
        dst.copy_(dst + c if accumulate else c)
        return out

    def colsum(x, M, N, ld=None, out=None):
        c = x.reshape(M, N).sum(0)
        if out is not None:
            out.copy_(c)
            return out
        return c

    def masks(seeds, shape, p):
        return (_keep_mask(seeds[0], shape, p), _keep_mask(seeds[1], shape, p)) if p > 0.0 else (None, None)

    def core(x, pe, text_len, need_attn=True, drop_p=0.0, seeds=(0, 0)):
        msg, attn = R.core(x, pe.to(x.dtype), text_len, *masks(seeds, x.shape, drop_p), drop_p)
        return msg, (attn if need_attn else None)

    def core_backward(dmsg, x, pe, attn, text_len, drop_p=0.0, seeds=(0, 0), out=None):
        dx = R.core_backward(dmsg, x, pe.to(x.dtype), attn, text_len, *masks(seeds, x.shape, drop_p), drop_p)
        if out is not None:
            out.add_(dx)
            return out
        return dx

    def gates_forward(u, r, x):
        u.copy_(torch.sigmoid(u))
        r.copy_(torch.sigmoid(r))
        return x * r

    def update_forward(o, u, x, R_, L, text_len=None):
        o.copy_(torch.tanh(o))
        new = x * (1 - u) + o * u
        return new, (R.masked_mean(new.view(R_, L, -1), text_len) if text_len is not None else None)

    def update_backward(dnew, dseq, text_len, x, u, o, R_, L):
        v = lambda t: t.reshape(R_, L, -1)                                             # noqa: E731
        outs = R.cell_update_backward(v(dnew) if dnew is not None else None, dseq, text_len, v(x), v(u), v(o))
        return tuple(t.reshape(R_ * L, -1).contiguous() for t in outs)

    def gates_backward(dxr, x, r, dx):
        dr_pre, new = R.cell_gates_backward(dxr, x, r, dx)
        dx.copy_(new)
        return dr_pre

    def empty(*shape, like, dtype=None):
        return torch.empty(shape, device=like.device, dtype=like.dtype)

    monkeypatch.setattr(dispatch, "_chk", lambda t, name: t.contiguous())
    monkeypatch.setattr(dispatch, "_empty", empty)
    monkeypatch.setattr(dispatch, "gemm", gemm)
    monkeypatch.setattr(dispatch, "colsum", colsum)
    monkeypatch.setattr(dispatch, "text_intra_core", core)
    monkeypatch.setattr(dispatch, "text_intra_core_backward", core_backward)
    monkeypatch.setattr(dispatch, "convgru_gates_forward", gates_forward)
    monkeypatch.setattr(dispatch, "convgru_update_forward", update_forward)
    monkeypatch.setattr(dispatch, "convgru_update_backward", update_backward)
    monkeypatch.setattr(dispatch, "convgru_gates_backward", gates_backward)
    monkeypatch.setattr(functions, "_chk", lambda t, name: t.contiguous(), raising=False)


def _masks(cfg, seed, p, layers):
    from texttoaudiogrounding_amd import dispatch
    if p == 0.0:
        return None
    shape = (cfg["R"], cfg["L"], cfg["E"])
    return [(_keep_mask(a, shape, p), _keep_mask(b, shape, p)) for a, b in dispatch.text_intra_dropout_seeds(seed, layers)]


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("name,p,zero", [("e64_n2", 0.0, False), ("e32_n1", 0.0, False), ("e64_n3", 0.0, False), ("e64_n3", 0.2, False),
                                         ("e32_n1", 0.2, True), ("e16_agg", 0.0, False)])
def test_registered_autograd_formula_equals_plain_autograd_fp64(fx, monkeypatch, name, p, zero, direct):
    import texttoaudiogrounding_amd.torch_ops  # noqa: F401
    from texttoaudiogrounding_amd import ops
    _cpu_patches(monkeypatch)
    cfg, st, text, text_len = _fixture_case(fx, name)
    if zero:
        text, text_len = R.draw_inputs(cfg, zero=True)
    seed, layers, tab = 4242, cfg["layers"], R.table_name(cfg["agg"])
    pnames = R.param_names(cfg["agg"])

    def fresh(frozen=()):
        return {k: v.double().clone().requires_grad_(k in pnames and k not in frozen) for k, v in st.items()}

    def run(s_, x_in):
        if direct:
            return ops.TextIntraFunction.apply(x_in, text_len, s_["pe.pe"][0], layers, p, seed, *[s_[k] for k in R.GATE_NAMES])
        return torch.ops.tag.text_intra(x_in, text_len, s_["pe.pe"][0], [s_[k] for k in R.GATE_NAMES], layers, p, seed)[:2]

    wt, ws = R.objective_weights(cfg)
    if zero:                                               # the empty row's seq_emb is 0/0: keep it out of the objective
        ws[0] = 0.0

    def loss(tok, seq, use_tok=True, use_seq=True):
        seq = seq if not zero else torch.cat([torch.zeros_like(seq[:1]), seq[1:]])
        return (tok * wt).sum() * float(use_tok) + (seq * ws).sum() * float(use_seq)

    def plain(use_tok=True, use_seq=True):
        s_ = fresh()
        tok, seq = R.encoder_forward(s_, text, text_len, layers, _masks(cfg, seed, p, layers), p, cfg["agg"])
        if zero:                                           # plain autograd sends 0/0 back through the empty row's division
            seq = R.masked_mean(tok, text_len.clamp(min=1))
        loss(tok, seq, use_tok, use_seq).backward()
        return tok.detach(), seq.detach(), {k: s_[k].grad for k in pnames}

    rtok, rseq, rg = plain()
    s = fresh()
    tok, seq = run(s, s[tab][text])
    loss(tok, seq).backward()
    assert R.rel_err(tok, rtok) < 1e-12 and R.rel_err(seq[1:], rseq[1:]) < 1e-12
    if p == 0.0 and not zero:
        assert R.rel_err(tok, fx[f"{name}_f64_token_emb"]) < 1e-12 and R.rel_err(seq, fx[f"{name}_f64_seq_emb"]) < 1e-12
        for k in pnames:
            assert R.rel_err(s[k].grad, fx[f"{name}_f64_d{k}"]) < 1e-11, k
    for k in pnames:
        assert s[k].grad.shape == s[k].shape
        e = R.rel_err(s[k].grad, rg[k])
        assert e < 1e-11, (k, e)
    # no dtok / no dseq: only one output takes part in the objective
    for use_tok, use_seq in ((False, True), (True, False)):
        _, _, og = plain(use_tok, use_seq)
        s1 = fresh()
        tok1, seq1 = run(s1, s1[tab][text])
        (loss(tok1, seq1, use_tok, False) if not use_seq else loss(tok1.detach(), seq1, False, True)).backward()
        for k in pnames:
            assert R.rel_err(s1[k].grad, og[k]) < 1e-11, (k, use_tok, use_seq)
    # frozen gates and a frozen table: nothing is returned (and no product formed) where nothing is needed
    frozen = ("conv_gru.update_gate.weight", "conv_gru.out_gate.bias")
    s2 = fresh(frozen)
    tok2, seq2 = run(s2, s2[tab][text].detach())
    loss(tok2, seq2).backward()
    assert all(s2[k].grad is None for k in frozen) and s2[tab].grad is None
    for k in R.GATE_NAMES:
        if k not in frozen:
            assert R.rel_err(s2[k].grad, rg[k]) < 1e-11, k
    s3 = fresh(tuple(R.GATE_NAMES))                        # freeze_text_encoder of everything but the table
    tok3, seq3 = run(s3, s3[tab][text])
    loss(tok3, seq3).backward()
    assert all(s3[k].grad is None for k in R.GATE_NAMES) and R.rel_err(s3[tab].grad, rg[tab]) < 1e-11


def test_operator_fake_kernels():
    import texttoaudiogrounding_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("text_intra", "text_intra_backward"):
        assert name in T.OP_NAMES
        assert str(getattr(torch.ops.tag, name).default._schema).startswith(f"tag::{name}(")
    E, R_, L, layers = 32, 6, 4, 3
    with FakeTensorMode():
        ps = [torch.empty(E, 2 * E, requires_grad=True), torch.empty(E, requires_grad=True)] * 3
        ps = [p.detach().clone().requires_grad_(True) for p in ps]
        x = torch.empty(R_, L, E, requires_grad=True)
        lens, pe = torch.empty(R_, dtype=torch.long), torch.empty(100, E)
        tok, seq, saved = torch.ops.tag.text_intra(x, lens, pe, ps, layers, 0.2, 3)
        assert tok.shape == (R_, L, E) and seq.shape == (R_, E) and tok.dtype == torch.float32
        per = [(R_ * L, E), (R_, L, L)] + [(R_ * L, E)] * 4
        assert [tuple(t.shape) for t in saved] == per * layers + [(R_ * L, E)] * (layers - 1)
        (tok.sum() + seq.sum()).backward()                       # the formula runs through the backward operator's fake kernel
        assert x.grad.shape == x.shape and all(p.grad.shape == p.shape for p in ps)
        g = torch.ops.tag.text_intra_backward(tok.detach(), None, x.detach(), lens, pe, [t.detach() for t in saved],
                                              [p.detach() for p in ps], layers, 0.2, 3, [True, False, True, False, True, False], False)
        assert len(g) == 7 and g[0].numel() == 0 and g[1].shape == ps[0].shape and g[2].numel() == 0 and g[5].shape == ps[4].shape


def test_symbols_declared_exported_and_einval():
    from texttoaudiogrounding_amd import lib, ops
    names = ("tag_text_intra_forward", "tag_text_intra_backward", "tag_convgru_gates_forward", "tag_convgru_update_forward",
             "tag_convgru_update_backward", "tag_convgru_gates_backward")
    for name in names:
        assert name in lib.declared_symbols(), name
    for name in ("TextIntraFunction", "text_intra_forward", "text_intra_backward", "text_intra_core", "text_intra_core_backward",
                 "convgru_gates_forward", "convgru_update_forward", "convgru_update_backward", "convgru_gates_backward",
                 "text_intra_dropout_seeds", "text_intra_check"):
        assert hasattr(ops, name), name
    h = lib.load()
    assert h.tag_abi_version() == 3
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tag_hip.h")).read()
    assert "models/text_encoder.py:206-237" in header and all(n in header for n in names)
    # bad arguments are refused with TAG_EINVAL and a message; nothing is launched (no GPU is touched)
    one = 16                                                      # any non-null pointer value: the checks come before any use
    ok = dict(x=one, pe=one, len=one, msg=one, attn=None, R=4, L=5, E=64, p=0.0)

    def fwd(**kw):
        a = dict(ok, **kw)
        return h.tag_text_intra_forward(a["x"], a["pe"], a["len"], a["msg"], a["attn"], a["R"], a["L"], a["E"], a["p"], 0, 1, None)
    bad_shapes = (dict(R=0), dict(L=0), dict(L=65), dict(E=0), dict(E=33), dict(E=1026), dict(p=1.0), dict(p=-0.1))
    for bad in (dict(x=None), dict(pe=None), dict(len=None), dict(msg=None)) + bad_shapes:
        assert fwd(**bad) == -1, bad
        assert b"argument check failed" in h.tag_last_error()
    okb = dict(dmsg=one, x=one, pe=one, attn=one, len=one, dx=one, R=4, L=5, E=64, p=0.0)

    def bwd(**kw):
        a = dict(okb, **kw)
        return h.tag_text_intra_backward(a["dmsg"], a["x"], a["pe"], a["attn"], a["len"], a["dx"], 0, a["R"], a["L"], a["E"], a["p"],
                                         0, 1, None)
    for bad in (dict(dmsg=None), dict(x=None), dict(pe=None), dict(attn=None), dict(len=None), dict(dx=None)) + bad_shapes:
        assert bwd(**bad) == -1, bad
        assert b"argument check failed" in h.tag_last_error()
    assert h.tag_convgru_gates_forward(None, one, one, one, 4, 8, None) == -1
    assert h.tag_convgru_gates_forward(one, one, one, one, 0, 8, None) == -1
    assert h.tag_convgru_update_forward(one, one, one, one, None, one, 2, 3, 8, None) == -1       # a mean without lengths
    assert h.tag_convgru_update_forward(one, one, one, None, None, None, 2, 3, 8, None) == -1
    assert h.tag_convgru_update_backward(None, None, one, one, one, one, one, one, one, 2, 3, 8, None) == -1
    assert h.tag_convgru_update_backward(None, one, None, one, one, one, one, one, one, 2, 3, 8, None) == -1
    assert h.tag_convgru_gates_backward(one, one, one, one, None, 4, 8, None) == -1
    assert h.tag_convgru_gates_backward(one, one, one, one, one, 4, 0, None) == -1


def test_cpu_tensors_raise():
    import texttoaudiogrounding_amd.torch_ops  # noqa: F401
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.models.text_encoder import EmbeddingAgg, EmbeddingLayer, IntraAttention
    E = 32
    ps = [torch.zeros(E, 2 * E), torch.zeros(E)] * 3
    x, lens, pe = torch.zeros(2, 3, E), torch.tensor([3, 1]), torch.zeros(100, E)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.tag.text_intra(x, lens, pe, ps, 2, 0.0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.TextIntraFunction.apply(x, lens, pe, 2, 0.0, 0, *ps)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.text_intra_core(x, pe, lens)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.text_intra_core_backward(x, x, pe, torch.zeros(2, 3, 3), lens)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.convgru_gates_forward(x.view(6, E), x.view(6, E), x.view(6, E))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.convgru_update_forward(x.view(6, E), x.view(6, E), x.view(6, E), 2, 3)
    for inner in (EmbeddingLayer(10, E), EmbeddingAgg(10, E)):
        for layers in (0, 2):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                IntraAttention(inner, layers)({"text": torch.tensor([[1, 2, 0], [3, 0, 0]]), "text_len": [2, 1]})
