"""LaionClapEncoder (the trainable LAION-CLAP text tower) on the GPU: every row kernel of csrc/text_clap.hip alone against the fp64
restatement (forward, backward, two runs bit-identical, 4-byte aligned views), the module against the fixture made from the real
transformers modules and at RoBERTa-base shape against the restatement, eval-mode agreement with the inference class, both
dropouts with the materialised masks, and BiEncoder / MultiTextBiEncoder through StrongRunner / WeakPhraseRunner (direct
gradients equal the operator path, a frozen tower launches no backward, the loss decreases).

Bounds (the rule of tests/test_gpu_text_rnn.py, unchanged): 5e-6 relative to the largest entry of the tensor on outputs and on
every gradient whose recorded fp32 deviation of the REFERENCE is below 1.25e-6; where the recorded deviation is larger the bound
is 4 x that deviation.  Cases with no recorded figure measure the deviation of the same restatement run in fp32 on the CPU inside
the test and apply the same rule.  Every measured error is printed.  (The key bias's gradient is zero up to rounding; it is
measured against the query bias's gradient scale, tests/text_clap_ref.quantity_err.)

Worst measured on an MI355X, relative to the largest entry of the fp64 tensor (CPU fp32 deviation of the same quantity in
brackets; the full table is in docs/experiments_text_clap.md):
  residual + LayerNorm alone   y 1.8e-7, xhat 1.5e-7, rstd 1.3e-7, ds 1.9e-7, dgamma 1.1e-7, dbeta 4.6e-8   [all <= 2.5e-7]
  GELU / GELU backward / tanh backward   5.8e-8 / 1.1e-7 / 5.8e-8   [5.8e-8 / 1.1e-7 / 5.7e-8]
  embedding block alone   h 1.6e-7, dword 1.4e-7, dtype0 1.2e-7, dpos 1.4e-7, dgamma 1.4e-7, dbeta 4.8e-8   [all <= 2.0e-7]
  module vs the transformers fixture   token_emb 4.8e-7, seq_emb 5.4e-7, worst gradient 1.0e-6 (word_embeddings)   [6.6e-7, 4.9e-7, 7.5e-7]
  module at RoBERTa-base shape   token_emb 4.0e-6, seq_emb 3.8e-6 [1.7e-6, 1.9e-6]; gradients 2 - 2.5 x the CPU fp32 figure, the
      closest to its bound layer.8.output.LayerNorm.weight at 0.93 of it (the GEMM chain of twelve layers, not the row kernels)
  both dropouts with materialised masks   token_emb 4.2e-7, seq_emb 8.3e-7, worst gradient 2.1e-6 (word_embeddings)   [3.7e-7, 7.9e-7, 1.4e-6]
  eval vs the inference class 4.7e-7 / 6.5e-7; direct vs operator-path gradients through both runners: bit-identical."""
import numpy as np
import pytest
import torch

from oracle import clap_text_oracle as C
from tests import text_clap_ref as R

pytestmark = pytest.mark.gpu

BOUND, DEV_LIMIT = 5e-6, 1.25e-6
CFG, FX = R.TINY, R.FIXTURE
NAMES = R.param_names(CFG["num_hidden_layers"])


def bound_for(dev32):
    return BOUND if dev32 < DEV_LIMIT else 4.0 * dev32


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(f"{golden_dir}/text_clap.npz")


def _unaligned(t):
    """The same values in a view that is only 4-byte aligned (offset 1 of a flat buffer)."""
    buf = torch.zeros(t.numel() + 1, device=t.device, dtype=t.dtype)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view_as(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _check(tag, got, ref64, ref32):
    """got (device) against the fp64 figure under the rule, the CPU fp32 figure measured here; prints; returns the error."""
    d32 = R.rel_err(ref32, ref64)
    e = R.rel_err(got.detach().cpu(), ref64)
    print(f"    {tag}: err {e:.2e} (cpu fp32 {d32:.1e}, bound {bound_for(d32):.1e})")
    assert e < bound_for(d32), (tag, e, d32)
    return e


# ---------------------------------------------------------------------------------------------- residual + LayerNorm
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("M,D", [(1, 48), (3, 64), (17, 768), (1030, 1024), (4100, 64)])
def test_resln_alone_vs_fp64(dev, M, D, with_res):
    from texttoaudiogrounding_amd import ops
    g = torch.Generator().manual_seed(100 * M + D)
    x, res, dy = (torch.randn(M, D, generator=g) for _ in range(3))
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    if not with_res:
        res = None
    eps = 1e-12
    print(f"resln M={M} D={D} res={with_res}")
    ref = {}
    for dt in (torch.float64, torch.float32):
        a = [t.to(dt) if t is not None else None for t in (x, res, gamma, beta, dy)]
        y, xhat, rstd = R.ln_forward(a[0], a[1], a[2], a[3], eps)
        ref[dt] = (y, xhat, rstd) + R.ln_backward(a[4], xhat, rstd, a[2])
    xd, rd, gd, bd, dyd = (t.to(dev) if t is not None else None for t in (x, res, gamma, beta, dy))
    y, xhat, rstd = ops.text_clap_resln_forward(xd, rd, gd, bd, eps)
    y2, xhat2, rstd2 = ops.text_clap_resln_forward(xd, rd, gd, bd, eps)
    assert torch.equal(y, y2) and torch.equal(xhat, xhat2) and torch.equal(rstd, rstd2), "two forward runs differ"
    y3, none1, none2 = ops.text_clap_resln_forward(xd, rd, gd, bd, eps, need_state=False)
    assert none1 is None and none2 is None and torch.equal(y3, y)
    ds, dg, db = ops.text_clap_resln_backward(dyd, xhat, rstd, gd)
    ds2, dg2, db2 = ops.text_clap_resln_backward(dyd, xhat, rstd, gd)
    assert torch.equal(ds, ds2) and torch.equal(dg, dg2) and torch.equal(db, db2), "two backward runs differ"
    ds3, dg3, db3 = ops.text_clap_resln_backward(dyd, xhat, rstd, gd, need_dgamma=False, need_dbeta=False)
    assert dg3 is None and db3 is None and torch.equal(ds3, ds)
    for i, (name, got) in enumerate((("y", y), ("xhat", xhat), ("rstd", rstd), ("ds", ds), ("dgamma", dg), ("dbeta", db))):
        _check(name, got, ref[torch.float64][i], ref[torch.float32][i])
    # 4-byte aligned views: the same channels per lane, read and written 4 bytes at a time: the same bits
    xu, dyu = _unaligned(xd), _unaligned(dyd)
    ru = _unaligned(rd) if rd is not None else None
    yu, xhu, rsu = ops.text_clap_resln_forward(xu, ru, _unaligned(gd), _unaligned(bd), eps)
    assert torch.equal(yu, y) and torch.equal(xhu, xhat) and torch.equal(rsu, rstd)
    dsu, dgu, dbu = ops.text_clap_resln_backward(dyu, _unaligned(xhat), rstd, _unaligned(gd))
    assert torch.equal(dsu, ds) and torch.equal(dgu, dg) and torch.equal(dbu, db)
    out = _unaligned(torch.empty_like(y))
    ops.text_clap_resln_forward(xd, rd, gd, bd, eps, out=out)
    assert torch.equal(out, y)


# ---------------------------------------------------------------------------------------------- GELU and tanh
@pytest.mark.parametrize("n", [1, 3, 160, 4099, 2 ** 20 + 1])
def test_gelu_and_tanh_alone_vs_fp64(dev, n):
    from texttoaudiogrounding_amd import ops
    g = torch.Generator().manual_seed(n)
    u = torch.linspace(-8.0, 8.0, n) if n > 1 else torch.tensor([0.7])
    u = u[torch.randperm(n, generator=g)]
    df = torch.randn(n, generator=g)
    print(f"gelu / tanh n={n}")
    ud, dfd = u.to(dev), df.to(dev)
    f, du = ops.text_clap_gelu_forward(ud), ops.text_clap_gelu_backward(ud, dfd)
    assert torch.equal(f, ops.text_clap_gelu_forward(ud)) and torch.equal(du, ops.text_clap_gelu_backward(ud, dfd))
    _check("gelu", f, R.gelu(u.double()), R.gelu(u))
    _check("gelu backward", du, R.gelu_backward(u.double(), df.double()), R.gelu_backward(u, df))
    y = torch.tanh(u)
    yd = y.to(dev)
    dx = ops.text_clap_tanh_backward(yd, dfd)
    assert torch.equal(dx, ops.text_clap_tanh_backward(yd, dfd))
    _check("tanh backward", dx, R.tanh_backward(y.double(), df.double()), R.tanh_backward(y, df))
    # 4-byte aligned views take the element-by-element form: the same bits
    uu, dfu = _unaligned(ud), _unaligned(dfd)
    assert torch.equal(ops.text_clap_gelu_forward(uu), f) and torch.equal(ops.text_clap_gelu_backward(uu, dfu), du)
    assert torch.equal(ops.text_clap_tanh_backward(_unaligned(yd), dfu), dx)


# ---------------------------------------------------------------------------------------------- embedding block
@pytest.mark.parametrize("B,L,V,D,P", [(1, 2, 120, 64, 72), (3, 3, 120, 64, 72), (17, 12, 120, 64, 72), (5, 64, 120, 64, 72),
                                       (3, 12, 50265, 768, 514)])
def test_embed_block_alone_vs_fp64(dev, B, L, V, D, P):
    from texttoaudiogrounding_amd import ops
    pad, eps = 1, 1e-12
    g = torch.Generator().manual_seed(B * 1000 + L)
    ids, _ = R.draw_inputs(B, L, seed=B + L, vocab=V, pad_id=pad)
    if B > 1:
        assert int((ids[1] != pad).sum()) == 2 and int((ids == pad).sum()) > 0
    flat = ids[ids != pad]
    assert B * L <= 4 or flat.numel() > flat.unique().numel(), "ids must repeat"
    word, pos = 0.5 * torch.randn(V, D, generator=g), 0.5 * torch.randn(P, D, generator=g)
    type0 = 0.5 * torch.randn(1, D, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dh = torch.randn(B * L, D, generator=g)
    print(f"embed block B={B} L={L} V={V} D={D}")
    ref = {}
    for dt in (torch.float64, torch.float32):
        w, t0, po, ga, be, d = (t.to(dt) for t in (word, type0, pos, gamma, beta, dh))
        h, pid, xhat, rstd = R.embed_forward(ids, w, t0, po, ga, be, eps, pad)
        ref[dt] = (h,) + tuple(R.embed_backward(d, xhat, rstd, ga, ids, pid, V, P, pad))
        ref["pos_ids"] = pid
    idd, wd, td, pd, gd, bd, dhd = (t.to(dev) for t in (ids, word, type0, pos, gamma, beta, dh))
    h, pid, xhat, rstd = ops.text_clap_embed_forward(idd, wd, td, pd, gd, bd, eps, pad)
    h2, pid2, xhat2, rstd2 = ops.text_clap_embed_forward(idd, wd, td, pd, gd, bd, eps, pad)
    assert torch.equal(h, h2) and torch.equal(xhat, xhat2) and torch.equal(rstd, rstd2), "two forward runs differ"
    assert pid.dtype == torch.long and torch.equal(pid.cpu(), ref["pos_ids"])
    grads = ops.text_clap_embed_backward(dhd, xhat, rstd, gd, idd, pid, V, P, pad)
    grads2 = ops.text_clap_embed_backward(dhd, xhat, rstd, gd, idd, pid, V, P, pad)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2)), "two backward runs differ"
    ops.check_async_errors()
    for i, (name, got) in enumerate([("h", h)] + list(zip(("dword", "dtype0", "dpos", "dgamma", "dbeta"), grads))):
        assert got.shape == ref[torch.float64][i].shape, name
        _check(name, got, ref[torch.float64][i], ref[torch.float32][i])
    dword, _, dpos, _, _ = grads
    assert float(dword[pad].abs().max()) == 0.0 and float(dpos[pad].abs().max()) == 0.0, "a pad row received gradient"
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[ids.reshape(-1)] = False
    assert float(dword[untouched.to(dev)].abs().max()) == 0.0 if untouched.any() else True
    # only what is asked for is produced, into the given destinations; the tables accumulate into zeroed rows
    sink = torch.zeros(P, D, device=dev)
    part = ops.text_clap_embed_backward(dhd, xhat, rstd, gd, idd, pid, V, P, pad, need=[False, True, True, False, True],
                                        outs=[None, None, sink, None, None])
    assert part[0] is None and part[3] is None and part[2] is sink and torch.equal(sink, dpos)
    assert torch.equal(part[1], grads[1]) and torch.equal(part[4], grads[4])
    # 4-byte aligned tables and rows: the same bits
    hu, _, xhu, _ = ops.text_clap_embed_forward(idd, _unaligned(wd), _unaligned(td), _unaligned(pd), gd, bd, eps, pad)
    assert torch.equal(hu, h) and torch.equal(xhu, xhat)


# ---------------------------------------------------------------------------------------------- the module
def _encoder(dev, cfg=CFG, state=None, train=True):
    from texttoaudiogrounding_amd.models.text_encoder import LaionClapEncoder
    enc = LaionClapEncoder(None, cfg)
    if state is not None:
        missing = enc.load_state_dict(state, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
    return enc.to(dev).train(train)


def _fixture_inputs(fx):
    return torch.from_numpy(fx["input_ids"].astype(np.int64)), torch.from_numpy(fx["attention_mask"].astype(np.int64))


def _module_results(enc, ids, mask, wt, ws):
    enc.zero_grad()
    o = enc({"input_ids": ids, "attention_mask": mask})
    R.objective(o["token_emb"], o["seq_emb"], wt.to(o["token_emb"]), ws.to(o["token_emb"])).backward()
    got = {"token_emb": o["token_emb"].detach().cpu(), "seq_emb": o["seq_emb"].detach().cpu()}
    got.update({"d" + k: p.grad.detach().cpu() for k, p in enc.named_parameters()})
    return got


@pytest.mark.parametrize("on_device", [False, True])
def test_module_vs_transformers_fixture(dev, fx, on_device):
    ids, mask = _fixture_inputs(fx)
    enc = _encoder(dev, state=R.draw_state(CFG, FX["state_seed"]))
    wt, ws = R.objective_weights(FX["R"], FX["L"], CFG["projection_dim"], FX["objective_seed"])
    got = _module_results(enc, ids.to(dev) if on_device else ids, mask.to(dev) if on_device else mask, wt, ws)
    quantities = fx["quantities"].tolist()
    ref = {k: torch.from_numpy(fx["f64_" + k]) for k in quantities}
    dev32 = dict(zip(quantities, fx["f32_dev"].tolist()))
    assert sorted(got) == quantities
    worst = {}
    print("LaionClapEncoder vs the transformers fixture (tiny config):")
    for k in quantities:
        e = R.quantity_err(got, ref, k)
        b = BOUND if k in ("token_emb", "seq_emb") else bound_for(dev32[k])
        worst[k] = e
        print(f"    {k}: err {e:.2e} (modules' fp32 {dev32[k]:.1e}, bound {b:.1e})")
        assert e < b, (k, e, b)
    pad = CFG["pad_token_id"]
    assert float(got["dmodel.embeddings.word_embeddings.weight"][pad].abs().max()) == 0.0
    assert float(got["dmodel.embeddings.position_embeddings.weight"][pad].abs().max()) == 0.0
    # two runs of the whole step are bit-identical
    again = _module_results(enc, ids, mask, wt, ws)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_module_at_roberta_base_shape_vs_fp64(dev):
    st = C.init_text_state(seed=5)
    ids, mask = C.synthetic_tokens(6, 12, seed=2)
    from texttoaudiogrounding_amd.models.hf_modeling_grounding import CLAP_TEXT_DEFAULTS
    cfg = dict(CLAP_TEXT_DEFAULTS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    enc = _encoder(dev, cfg, st)
    wt, ws = R.objective_weights(6, 12, 512, 4)
    got = _module_results(enc, ids, mask, wt, ws)
    r64 = R.results(st, ids, mask, 12, torch.float64, 1e-12, 1, wt=wt, ws=ws)
    r32 = R.results(st, ids, mask, 12, torch.float32, 1e-12, 1, wt=wt, ws=ws)
    print("LaionClapEncoder at RoBERTa-base shape, R=6 L=12:")
    worst = (0.0, None)
    for k in sorted(r64):
        d32 = R.quantity_err(r32, r64, k)
        e = R.quantity_err(got, r64, k)
        b = bound_for(d32)
        worst = max(worst, (e / b, k))
        if k in ("token_emb", "seq_emb") or "layer" not in k or e > 0.25 * b:
            print(f"    {k}: err {e:.2e} (cpu fp32 {d32:.1e}, bound {b:.1e})")
        assert e < b, (k, e, b)
    print(f"    closest to its bound: {worst[1]} at {worst[0]:.2f} of it")
    assert float(got["dmodel.embeddings.word_embeddings.weight"][1].abs().max()) == 0.0


def test_eval_agrees_with_the_inference_class(dev, fx):
    from texttoaudiogrounding_amd.models import hf_modeling_grounding as H
    ids, mask = _fixture_inputs(fx)
    st = R.draw_state(CFG, FX["state_seed"])
    enc = _encoder(dev, state=st, train=False)
    inf = H.LaionClapEncoder(None, CFG)
    inf.load_state_dict(enc.state_dict())
    inf = inf.to(dev).eval()
    with torch.no_grad():
        a = enc({"input_ids": ids, "attention_mask": mask})
    b = inf({"input_ids": ids, "attention_mask": mask})
    assert not a["token_emb"].requires_grad
    for k in ("token_emb", "seq_emb"):
        e = R.rel_err(a[k].cpu(), b[k].cpu())
        e64 = R.rel_err(a[k].cpu(), fx["f64_" + k])
        print(f"eval vs hf_modeling_grounding.LaionClapEncoder: {k} {e:.2e}; vs fp64 {e64:.2e}")
        assert e < BOUND and e64 < BOUND
    # leading shapes are flattened and restored
    o = enc({"input_ids": ids[:4].reshape(2, 2, -1), "attention_mask": mask[:4].reshape(2, 2, -1)})
    assert o["token_emb"].shape == (2, 2, FX["L"], 32) and o["seq_emb"].shape == (2, 2, 32)
    assert torch.equal(o["seq_emb"].reshape(4, 32), a["seq_emb"][:4])


def test_dropout_with_materialised_masks(dev, fx):
    from texttoaudiogrounding_amd import ops
    ids, mask = _fixture_inputs(fx)
    p_h, p_a, seed = 0.2, 0.3, 987654321
    st = R.draw_state(CFG, FX["state_seed"])
    enc = _encoder(dev, dict(CFG, hidden_dropout_prob=p_h, attention_probs_dropout_prob=p_a), st)
    Rn, L, D, H = FX["R"], FX["L"], CFG["hidden_size"], CFG["num_attention_heads"]
    s_emb, per = ops.text_clap_dropout_seeds(seed, CFG["num_hidden_layers"])
    masks = {"emb": ops.dropout_mask(s_emb, (Rn * L, D), p_h, dev).cpu()}
    for l, (s_attn, s_ao, s_out) in enumerate(per):
        masks[("attn", l)] = ops.dropout_mask(s_attn, (Rn, H, L, L), p_a, dev).cpu()
        masks[("ao", l)] = ops.dropout_mask(s_ao, (Rn * L, D), p_h, dev).cpu()
        masks[("out", l)] = ops.dropout_mask(s_out, (Rn * L, D), p_h, dev).cpu()
    assert 0.6 < float(masks["emb"].float().mean()) < 0.95
    wt, ws = R.objective_weights(Rn, L, CFG["projection_dim"], FX["objective_seed"])
    ps = enc._params()
    tok, seq, _ = torch.ops.tag.text_clap(ids.to(dev), mask.to(dev), ps, H, 1e-12, 1, p_h, p_a, seed, True)
    R.objective(tok, seq, wt.to(tok), ws.to(tok)).backward()
    got = {"token_emb": tok.detach().cpu(), "seq_emb": seq.detach().cpu(), **{"d" + k: p.grad.cpu() for k, p in zip(NAMES, ps)}}
    r64 = R.results(st, ids, mask, H, torch.float64, masks=masks, p_hidden=p_h, p_attn=p_a, wt=wt, ws=ws)
    r32 = R.results(st, ids, mask, H, torch.float32, masks=masks, p_hidden=p_h, p_attn=p_a, wt=wt, ws=ws)
    print(f"LaionClapEncoder with dropout p_hidden={p_h} p_attn={p_a} (materialised masks):")
    for k in sorted(r64):
        d32 = R.quantity_err(r32, r64, k)
        e = R.quantity_err(got, r64, k)
        if "layer.0" not in k:
            print(f"    {k}: err {e:.2e} (cpu fp32 {d32:.1e})")
        assert e < bound_for(d32), (k, e, d32)
    # the module in train mode draws a seed and drops something: two calls differ, eval does not drop
    a = enc({"input_ids": ids, "attention_mask": mask})["seq_emb"]
    b = enc({"input_ids": ids, "attention_mask": mask})["seq_emb"]
    assert not torch.equal(a, b)
    enc.eval()
    c = enc({"input_ids": ids, "attention_mask": mask})["seq_emb"]
    assert R.rel_err(c.detach().cpu(), fx["f64_seq_emb"]) < BOUND


# ---------------------------------------------------------------------------------------------- in a model
SAMPLES = 48000


def _clap_batch(B=2, L=6, seed=7):
    from oracle import tag_oracle as O
    b = O.synthetic_batch(B, SAMPLES, seed=seed, ragged=True, hop=640, vocab_size=CFG["vocab_size"])
    ids, mask = R.draw_inputs(B, L, seed=seed, vocab=CFG["vocab_size"])
    del b["text"]
    b.update(input_ids=ids, attention_mask=mask, text_len=mask.sum(-1).numpy())
    return b


def _clone_batch(b):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}


def _biencoder(freeze_text=False):
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    torch.manual_seed(3)
    enc = text_encoder.LaionClapEncoder(None, CFG)
    enc.load_state_dict(R.draw_state(CFG, FX["state_seed"]))
    model = audio_text_model.BiEncoder(audio_encoder.CrnnEncoder(32000, 256), enc, match.DotProduct(), 64, add_proj=True,
                                       freeze_text_encoder=freeze_text)
    model.audio_encoder.dropout_p = 0.0
    return model


def _count_backward(monkeypatch):
    from texttoaudiogrounding_amd import functions
    calls = []
    real = functions.text_clap_backward

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(functions, "text_clap_backward", spy)
    return calls


def test_biencoder_through_strong_runner(dev, monkeypatch):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.runner import StrongRunner
    calls = _count_backward(monkeypatch)
    batch = _clap_batch()
    runner = StrongRunner(_biencoder(), device=str(dev))
    runner.model.train()
    loss = runner.forward_backward(_clone_batch(batch))
    lv = runner.loss_value(loss)
    assert len(calls) == 1
    direct = {n: p.grad.detach().clone() for n, p in runner.model.named_parameters()}
    text = [n for n in direct if n.startswith("text_encoder.")]
    assert len(text) == len(NAMES)
    assert all(direct[n].abs().max() > 0 for n in text if "key.bias" not in n), "a text gradient is all zero"
    # the same step through the operator's registered formula (AccumulateGrad into the same flat views)
    assert not ops.DIRECT_GRADS
    runner.flat.zero_grad()
    out = runner.forward(_clone_batch(batch), training=True)
    loss2 = runner.loss_fn(out)
    loss2.backward()
    assert abs(float(loss2.item()) - lv) < 1e-6 and len(calls) == 1
    worst = 0.0
    for n, p in runner.model.named_parameters():
        scale = direct[n.replace("key.bias", "query.bias")]
        e = R.rel_err(direct[n], p.grad, p.grad if "key.bias" not in n else scale)
        worst = max(worst, e)
        assert e < 1e-6, (n, e)
    print(f"StrongRunner BiEncoder(CrnnEncoder, LaionClapEncoder): loss {lv:.6f}; direct vs operator-path gradients, worst {worst:.2e}")
    # the loss is finite and decreases over three steps on one batch
    losses = [runner.loss_value(runner.train_step(_clone_batch(batch))) for _ in range(3)]
    print("    three steps on one batch:", [f"{v:.6f}" for v in losses])
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0]
    # frozen after the flat buffers were built: no tower backward launch, the flat-gradient slice and the values stay untouched
    del calls[:]
    r1 = StrongRunner(_biencoder(), device=str(dev))
    r1.model.train()
    for p in r1.model.text_encoder.parameters():
        p.requires_grad = False
    before = {n: p.detach().clone() for n, p in r1.model.named_parameters()}
    r1.loss_value(r1.train_step(_clone_batch(batch)))
    for n, p in r1.model.named_parameters():
        if n.startswith("text_encoder."):
            assert torch.equal(before[n], p) and float(p._tag_grad_sink.abs().max()) == 0.0, n
    assert not torch.equal(before["text_proj.weight"], dict(r1.model.named_parameters())["text_proj.weight"])
    assert calls == []
    # frozen by the constructor: the tower is not in the flat buffers at all
    r2 = StrongRunner(_biencoder(freeze_text=True), device=str(dev))
    r2.model.train()
    before = {n: p.detach().clone() for n, p in r2.model.text_encoder.named_parameters()}
    r2.loss_value(r2.train_step(_clone_batch(batch)))
    assert all(torch.equal(before[n], p) and p.grad is None for n, p in r2.model.text_encoder.named_parameters())
    assert calls == []


def test_multitext_biencoder_through_weak_phrase_runner(dev, monkeypatch):
    from texttoaudiogrounding_amd import losses, ops
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import WeakPhraseRunner
    from oracle import tag_oracle as O
    calls = _count_backward(monkeypatch)
    B, N, L = 2, 3, 5
    wave = O.synthetic_batch(B, SAMPLES, seed=11, ragged=True, hop=640, vocab_size=CFG["vocab_size"])
    ids, mask = R.draw_inputs(B * N, L, seed=4, vocab=CFG["vocab_size"])
    g = torch.Generator().manual_seed(6)
    batch = {"waveform": wave["waveform"], "waveform_len": wave["waveform_len"], "input_ids": ids.view(B, N, L),
             "attention_mask": mask.view(B, N, L), "text_len": mask.sum(-1).view(B, N), "label": (torch.rand(B, N, generator=g) < 0.5).float()}

    def model(freeze=False):
        enc = text_encoder.LaionClapEncoder(None, CFG)
        enc.load_state_dict(R.draw_state(CFG, FX["state_seed"]))
        torch.manual_seed(5)
        m = audio_text_model.MultiTextBiEncoder(audio_encoder.CrnnEncoder(32000, 256), enc, match.DotProduct(), 64,
                                                ["input_ids", "attention_mask"], add_proj=True, freeze_text_encoder=freeze)
        m.audio_encoder.dropout_p = 0.0
        return m
    runner = WeakPhraseRunner(model(), loss_fn=losses.ClipBceLoss(), device=str(dev))
    runner.model.train()
    loss = runner.forward_backward(_clone_batch(batch))
    lv = float(loss.item())
    assert len(calls) == 1
    direct = {n: p.grad.detach().clone() for n, p in runner.model.named_parameters()}
    assert not ops.DIRECT_GRADS
    runner.flat.zero_grad()
    out = runner.forward(_clone_batch(batch), training=True)
    assert out["clip_sim"].shape == (B, N)
    loss2 = runner.loss_fn(out)
    loss2.backward()
    assert abs(float(loss2.item()) - lv) < 1e-6
    worst = 0.0
    for n, p in runner.model.named_parameters():
        scale = direct[n.replace("key.bias", "query.bias")]
        e = R.rel_err(direct[n], p.grad, p.grad if "key.bias" not in n else scale)
        worst = max(worst, e)
        assert e < 1e-6, (n, e)
    print(f"WeakPhraseRunner MultiTextBiEncoder(CrnnEncoder, LaionClapEncoder): loss {lv:.6f}; direct vs operator path, worst {worst:.2e}")
    losses_ = [float(runner.train_step(_clone_batch(batch)).item()) for _ in range(3)]
    print("    three steps on one batch:", [f"{v:.6f}" for v in losses_])
    assert all(np.isfinite(losses_)) and losses_[2] < losses_[1] < losses_[0]
    del calls[:]
    r2 = WeakPhraseRunner(model(freeze=True), loss_fn=losses.ClipBceLoss(), device=str(dev))
    r2.model.train()
    before = {n: p.detach().clone() for n, p in r2.model.text_encoder.named_parameters()}
    assert torch.isfinite(r2.train_step(_clone_batch(batch)))
    assert all(torch.equal(before[n], p) and p.grad is None for n, p in r2.model.text_encoder.named_parameters())
    assert calls == []
