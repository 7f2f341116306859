"""Bert / SentenceBert (the BERT text encoders on the HIP text tower) on the GPU: the kernels of csrc/text_bert.hip alone against
the fp64 restatement (forward, backward, two runs bit-identical), the modules against the fixture made from the real transformers
BertModel and at all-MiniLM-L6-v2's shape against the restatement, both dropouts with the materialised masks, Bert inside
BiEncoder / MultiTextBiEncoder through StrongRunner / WeakPhraseRunner (direct gradients equal the operator path bit for bit),
PhraseEmbedder's bucketing against single-phrase runs and RetrievalTextEncoder.

Bounds (the rule of docs/experiments_text_clap.md, unchanged): the error relative to the largest entry of the fp64 tensor is at
most 5e-6, or 4 x the CPU fp32 deviation of the same quantity (recorded in the fixture, or measured on the same restatement in
fp32 inside the test) where that deviation is above 1.25e-6.  Every measured error is printed.

Worst measured on an MI355X, relative to the largest entry of the fp64 tensor (CPU fp32 deviation of the same quantity in
brackets; the full table is in docs/experiments_text_bert.md):
  embedding block alone   h 1.8e-7, xhat 1.6e-7, rstd 1.3e-7, dword 1.6e-7, dtype 1.4e-7, dpos 1.4e-7, dgamma 1.6e-7, dbeta 4.5e-8
      [all <= 1.8e-7]
  pooling alone   seq 2.9e-7 [1.6e-7], raw 4.3e-8 [4.3e-8], dh 1.1e-7 [1.1e-7]
  modules vs the transformers fixture   outputs 6.0e-7 [9.8e-7]; worst gradient cls 1.8e-6, mean + normalize 1.8e-6, mean 1.5e-6
      (a query bias each) [fixture fp32 2.0e-6, 2.7e-6, 1.9e-6]
  SentenceBert at all-MiniLM-L6-v2's shape   token_emb 1.5e-6 [1.0e-6], seq_emb 1.4e-6 [8.3e-7], worst gradient 8.1e-6 [6.6e-6], the
      closest to its bound layer.0 query.weight at 0.84 of it (the GEMM chain of six layers, not the row kernels)
  both dropouts with materialised masks   token_emb 9.1e-7, seq_emb 4.3e-7, worst gradient 2.0e-6 [8.7e-7, 5.2e-7, 1.8e-6]
  PhraseEmbedder bucketed vs each phrase alone: identical bits; vs fp64 <= 4.1e-7 [<= 3.8e-7]
  RetrievalTextEncoder 5.7e-7 / with text_proj and normalisation 2 6.5e-7 [4.0e-7 / 3.4e-7]
  direct vs operator-path gradients through both runners: bit-identical."""
import numpy as np
import pytest
import torch

from tests import text_bert_ref as R
from texttoaudiogrounding_amd.models.text_encoder import Bert, SentenceBert  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu

BOUND, DEV_LIMIT = 5e-6, 1.25e-6
CFG, FX = R.TINY, R.FIXTURE
NAMES = R.param_names(CFG["num_hidden_layers"])


def bound_for(dev32):
    return BOUND if dev32 < DEV_LIMIT else 4.0 * dev32


@pytest.fixture(scope="module")
def fx(golden_dir):
    out = dict(np.load(f"{golden_dir}/text_bert.npz"))
    for case in ("mean_norm", "mean"):
        out.update({k: v for k, v in np.load(f"{golden_dir}/text_bert_{case}.npz").items() if k.startswith(case + "_f")})
    return out


def _check(tag, got, ref64, ref32):
    d32 = R.rel_err(ref32, ref64)
    e = R.rel_err(got.detach().cpu(), ref64)
    print(f"    {tag}: err {e:.2e} (cpu fp32 {d32:.1e}, bound {bound_for(d32):.1e})")
    assert e < bound_for(d32), (tag, e, d32)
    return e


# ---------------------------------------------------------------------------------------------- embedding block
@pytest.mark.parametrize("types", ["zero", "null", "mixed", "last"])
@pytest.mark.parametrize("B,L,V,D,P,T", [(1, 2, 120, 64, 72, 2), (3, 3, 120, 64, 72, 2), (17, 12, 120, 384, 72, 2),
                                         (5, 64, 120, 64, 64, 2), (4, 7, 120, 50, 72, 3), (2, 5, 30522, 768, 512, 2),
                                         (3, 4, 120, 1024, 72, 1)])
def test_embed_block_alone_vs_fp64(dev, B, L, V, D, P, T, types):
    from texttoaudiogrounding_amd import ops
    pad, eps = 0, 1e-12
    g = torch.Generator().manual_seed(B * 1000 + L)
    ids, mixed, _ = R.draw_inputs(B, L, seed=B + L, vocab=V, types=T, pad_id=pad)
    tps = {"zero": torch.zeros_like(ids), "null": None, "mixed": mixed, "last": torch.full_like(ids, T - 1)}[types]
    word, pos = 0.5 * torch.randn(V, D, generator=g), 0.5 * torch.randn(P, D, generator=g)
    typ = 0.5 * torch.randn(T, D, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dh = torch.randn(B * L, D, generator=g)
    print(f"bert embed block B={B} L={L} V={V} D={D} P={P} T={T} types={types}")
    ref = {}
    for dt in (torch.float64, torch.float32):
        w, ty, po, ga, be, d = (t.to(dt) for t in (word, typ, pos, gamma, beta, dh))
        h, xhat, rstd = R.embed_forward(ids, tps, w, ty, po, ga, be, eps)
        ref[dt] = (h, xhat, rstd) + tuple(R.embed_backward(d, xhat, rstd, ga, ids, tps, V, T, P, pad))
    idd, wd, td, pd, gd, bd, dhd = (t.to(dev) for t in (ids, word, typ, pos, gamma, beta, dh))
    tpd = tps.to(dev) if tps is not None else None
    h, xhat, rstd = ops.text_bert_embed_forward(idd, tpd, wd, td, pd, gd, bd, eps)
    h2, xhat2, rstd2 = ops.text_bert_embed_forward(idd, tpd, wd, td, pd, gd, bd, eps)
    assert torch.equal(h, h2) and torch.equal(xhat, xhat2) and torch.equal(rstd, rstd2), "two forward runs differ"
    h3, n1, n2 = ops.text_bert_embed_forward(idd, tpd, wd, td, pd, gd, bd, eps, need_state=False)
    assert n1 is None and n2 is None and torch.equal(h3, h)
    grads = ops.text_bert_embed_backward(dhd, xhat, rstd, gd, idd, tpd, V, T, P, pad)
    grads2 = ops.text_bert_embed_backward(dhd, xhat, rstd, gd, idd, tpd, V, T, P, pad)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2)), "two backward runs differ"
    ops.check_async_errors()
    got = [("h", h), ("xhat", xhat), ("rstd", rstd)] + list(zip(("dword", "dtype", "dpos", "dgamma", "dbeta"), grads))
    for i, (name, t) in enumerate(got):
        assert t.shape == ref[torch.float64][i].shape, name
        _check(name, t, ref[torch.float64][i], ref[torch.float32][i])
    dword, _, dpos, _, _ = grads
    assert float(dword[pad].abs().max()) == 0.0, "the pad row received gradient"
    if L < P:
        assert float(dpos[L:].abs().max()) == 0.0, "a position row >= L was touched"
    # the rows >= L of a destination are NOT written
    sink = torch.full((P, D), 7.0, device=dev)
    sink[:L] = 0.0
    part = ops.text_bert_embed_backward(dhd, xhat, rstd, gd, idd, tpd, V, T, P, pad, need=[False, True, True, False, True],
                                        outs=[None, None, sink, None, None])
    assert part[0] is None and part[3] is None and part[2] is sink and torch.equal(sink[:L], dpos[:L])
    assert L == P or bool((sink[L:] == 7.0).all())
    assert torch.equal(part[1], grads[1]) and torch.equal(part[4], grads[4])


def test_type_ids_out_of_range(dev):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.models.text_encoder import Bert
    enc = Bert(None, CFG).to(dev).eval()
    ids, tps, mask = R.draw_inputs(3, 5, seed=1)
    bad = tps.clone()
    bad[0, 1] = 2
    with pytest.raises(ValueError):
        enc({"input_ids": ids, "token_type_ids": bad, "attention_mask": mask})
    with torch.no_grad():
        a = enc({"input_ids": ids, "token_type_ids": bad.to(dev), "attention_mask": mask})   # clamped and flagged
    with pytest.raises(IndexError):
        ops.check_async_errors()
    ops.check_async_errors()
    with torch.no_grad():
        b = enc({"input_ids": ids, "token_type_ids": bad.to(dev), "attention_mask": mask})
        c = enc({"input_ids": ids, "token_type_ids": bad.clamp(max=1), "attention_mask": mask})
    with pytest.raises(IndexError):
        ops.check_async_errors()
    assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) for k in ("token_emb", "seq_emb")), "clamped to T - 1, same bits"


# ---------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("R_,L,D", [(1, 2, 48), (3, 3, 64), (17, 12, 384), (5, 64, 1024), (1030, 7, 50)])
def test_pool_alone_vs_fp64(dev, R_, L, D):
    from texttoaudiogrounding_amd import ops
    g = torch.Generator().manual_seed(R_ * 100 + L)
    h = torch.randn(R_, L, D, generator=g)
    klen = torch.randint(0, L + 1, (R_,), generator=g)
    klen[0] = L
    if R_ > 2:
        klen[1], klen[2] = 0, 1
    dseq, dtok = torch.randn(R_, D, generator=g), torch.randn(R_, L, D, generator=g)
    hd, kd, dsd, dtd = h.to(dev), klen.to(dev), dseq.to(dev), dtok.to(dev)
    print(f"bert pool R={R_} L={L} D={D}")
    for mode in (0, 1):
        for norm in (0, 1, 2):
            seq, raw = ops.text_bert_pool_forward(hd, kd, mode, norm, need_raw=True)
            seq2, _ = ops.text_bert_pool_forward(hd, kd, mode, norm)
            assert torch.equal(seq, seq2)
            r64, r32 = R.pool(h.double(), klen, mode, norm), R.pool(h, klen, mode, norm)
            _check(f"mode {mode} norm {norm} seq", seq, r64[0], r32[0])
            _check(f"mode {mode} norm {norm} raw", raw, r64[1], r32[1])
            if mode == 1 and R_ > 2:
                assert float(seq[1].abs().max()) == 0.0, "klen = 0 must give a zero row"
            if norm == 2:
                with pytest.raises(ValueError):
                    ops.text_bert_pool_backward(dsd, None, raw, kd, mode, norm, (R_, L, D))
                continue
            for with_tok in (False, True):
                dh = ops.text_bert_pool_backward(dsd, dtd if with_tok else None, raw, kd, mode, norm, (R_, L, D))
                dh2 = ops.text_bert_pool_backward(dsd, dtd if with_tok else None, raw, kd, mode, norm, (R_, L, D))
                assert torch.equal(dh, dh2)
                b64 = R.pool_backward(dseq.double(), dtok.double() if with_tok else None, h.double(), klen, mode, norm)
                b32 = R.pool_backward(dseq, dtok if with_tok else None, h, klen, mode, norm)
                _check(f"mode {mode} norm {norm} dh (dtok {with_tok})", dh, b64, b32)


# ---------------------------------------------------------------------------------------------- the modules
def _state(cfg=CFG, seed=FX["state_seed"]):
    st = R.draw_state(cfg, seed)
    st["dummy_param"] = torch.zeros(1)
    return st


def _bert(dev, cfg=CFG, train=True):
    from texttoaudiogrounding_amd.models.text_encoder import Bert
    enc = Bert(None, cfg)
    enc.load_state_dict(_state(cfg), strict=True)
    return enc.to(dev).train(train)


def _sbert(dev, pooling, normalize, cfg=CFG, seed=FX["state_seed"]):
    from texttoaudiogrounding_amd.models.text_encoder import SentenceBert
    enc = SentenceBert(None, cfg, pooling=pooling, normalize=normalize)
    enc.load_state_dict(_state(cfg, seed), strict=True)
    return enc.to(dev).train()


def _fixture_inputs(fx):
    return tuple(torch.from_numpy(fx[k].astype(np.int64)) for k in ("input_ids", "token_type_ids", "attention_mask"))


def _module_results(enc, ids, tps, mask, wt, ws):
    enc.zero_grad()
    o = enc({"input_ids": ids, "token_type_ids": tps, "attention_mask": mask})
    R.objective(o["token_emb"], o["seq_emb"], wt.to(o["token_emb"]), ws.to(o["token_emb"])).backward()
    got = {"token_emb": o["token_emb"].detach().cpu(), "seq_emb": o["seq_emb"].detach().cpu()}
    for k, p in enc.named_parameters():
        if k.startswith("model.pooler.") or k == "dummy_param":
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, f"{k} received a gradient"
        else:
            got["d" + k] = p.grad.detach().cpu()
    return got


@pytest.mark.parametrize("case,on_device", [("cls", False), ("cls", True), ("mean_norm", False), ("mean", False)])
def test_modules_vs_transformers_fixture(dev, fx, case, on_device):
    ids, tps, mask = _fixture_inputs(fx)
    enc = _bert(dev) if case == "cls" else _sbert(dev, "mean", case == "mean_norm")
    wt, ws = R.objective_weights(FX["R"], FX["L"], CFG["hidden_size"], FX["objective_seed"])
    args = [t.to(dev) if on_device else t for t in (ids, tps, mask)]
    got = _module_results(enc, *args, wt, ws)
    quantities = fx["quantities"].tolist()
    ref = {k: torch.from_numpy(fx[f"{case}_f64_{k}"]) for k in quantities}
    dev32 = dict(zip(quantities, fx[case + "_f32_dev"].tolist()))
    assert sorted(got) == quantities
    print(f"{type(enc).__name__} ({case}) vs the transformers fixture (tiny config):")
    worst = (0.0, None)
    for k in quantities:
        e = R.quantity_err(got, ref, k)
        b = bound_for(dev32[k])
        worst = max(worst, (e, k))
        if "layer" not in k:
            print(f"    {k}: err {e:.2e} (module's fp32 {dev32[k]:.1e}, bound {b:.1e})")
        assert e < b, (k, e, b)
    print(f"    worst: {worst[1]} {worst[0]:.2e}")
    assert float(got["dmodel.embeddings.word_embeddings.weight"][CFG["pad_token_id"]].abs().max()) == 0.0
    assert float(got["dmodel.embeddings.position_embeddings.weight"][FX["L"]:].abs().max()) == 0.0
    again = _module_results(enc, *args, wt, ws)
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs of the step differ"
    if case == "cls":                                       # leading shapes are flattened and restored; float inputs as staged
        with torch.no_grad():
            o = enc({"input_ids": ids[:4].reshape(2, 2, -1).float(), "token_type_ids": tps[:4].reshape(2, 2, -1).float(),
                     "attention_mask": mask[:4].reshape(2, 2, -1)})
        assert o["token_emb"].shape == (2, 2, FX["L"], 64) and o["seq_emb"].shape == (2, 2, 64)
        assert o["attention_mask"].shape == (2, 2, FX["L"])
        assert torch.equal(o["seq_emb"].reshape(4, 64).cpu(), got["seq_emb"][:4])


def test_sentence_bert_at_minilm_shape_vs_fp64(dev):
    cfg = R.MINILM
    st = R.draw_state(cfg, 9)
    ids, tps, mask = R.draw_inputs(6, 12, seed=2, vocab=cfg["vocab_size"])
    enc = _sbert(dev, "mean", True, cfg, 9)
    wt, ws = R.objective_weights(6, 12, 384, 4)
    got = _module_results(enc, ids, tps, mask, wt, ws)
    r64 = R.results(st, ids, tps, mask, 12, 1, 1, torch.float64, seed=4)
    r32 = R.results(st, ids, tps, mask, 12, 1, 1, torch.float32, seed=4)
    print("SentenceBert at all-MiniLM-L6-v2's shape, R=6 L=12:")
    worst = (0.0, None)
    for k in sorted(got):
        d32 = R.quantity_err(r32, r64, k)
        e = R.quantity_err(got, r64, k)
        b = bound_for(d32)
        worst = max(worst, (e / b, k))
        if "layer" not in k or e > 0.25 * b:
            print(f"    {k}: err {e:.2e} (cpu fp32 {d32:.1e}, bound {b:.1e})")
        assert e < b, (k, e, b)
    print(f"    closest to its bound: {worst[1]} at {worst[0]:.2f} of it")
    again = _module_results(enc, ids, tps, mask, wt, ws)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_dropout_with_materialised_masks(dev, fx):
    from texttoaudiogrounding_amd import ops
    ids, tps, mask = _fixture_inputs(fx)
    p_h, p_a, seed = 0.2, 0.3, 987654321
    st = R.draw_state(CFG, FX["state_seed"])
    enc = _bert(dev, dict(CFG, hidden_dropout_prob=p_h, attention_probs_dropout_prob=p_a))
    Rn, L, D, H = FX["R"], FX["L"], CFG["hidden_size"], CFG["num_attention_heads"]
    s_emb, per = ops.text_clap_dropout_seeds(seed, CFG["num_hidden_layers"])
    masks = {"emb": ops.dropout_mask(s_emb, (Rn * L, D), p_h, dev).cpu()}
    for l, (s_attn, s_ao, s_out) in enumerate(per):
        masks[("attn", l)] = ops.dropout_mask(s_attn, (Rn, H, L, L), p_a, dev).cpu()
        masks[("ao", l)] = ops.dropout_mask(s_ao, (Rn * L, D), p_h, dev).cpu()
        masks[("out", l)] = ops.dropout_mask(s_out, (Rn * L, D), p_h, dev).cpu()
    assert 0.6 < float(masks["emb"].float().mean()) < 0.95
    wt, ws = R.objective_weights(Rn, L, D, FX["objective_seed"])
    ps = enc._params()

    def run():
        for p in ps:
            p.grad = None
        tok, seq, _ = torch.ops.tag.text_bert(ids.to(dev), tps.to(dev), mask.to(dev), ps, H, 1e-12, 0, 1, 1, p_h, p_a, seed, True)
        R.objective(tok, seq, wt.to(tok), ws.to(tok)).backward()
        return {"token_emb": tok.detach().cpu(), "seq_emb": seq.detach().cpu(), **{"d" + k: p.grad.cpu() for k, p in zip(NAMES, ps)}}
    got = run()
    kw = dict(masks=masks, p_hidden=p_h, p_attn=p_a, seed=FX["objective_seed"])
    r64 = R.results(st, ids, tps, mask, H, 1, 1, torch.float64, **kw)
    r32 = R.results(st, ids, tps, mask, H, 1, 1, torch.float32, **kw)
    print(f"text_bert (mean + normalize) with dropout p_hidden={p_h} p_attn={p_a} (materialised masks):")
    for k in sorted(got):
        d32 = R.quantity_err(r32, r64, k)
        e = R.quantity_err(got, r64, k)
        if "layer.0" not in k:
            print(f"    {k}: err {e:.2e} (cpu fp32 {d32:.1e})")
        assert e < bound_for(d32), (k, e, d32)
    again = run()
    assert all(torch.equal(got[k], again[k]) for k in got)
    batch = {"input_ids": ids, "token_type_ids": tps, "attention_mask": mask}
    a, b = enc(batch)["seq_emb"], enc(batch)["seq_emb"]
    assert not torch.equal(a, b)
    enc.eval()
    assert R.rel_err(enc(batch)["seq_emb"].detach().cpu(), fx["cls_f64_seq_emb"]) < BOUND


# ---------------------------------------------------------------------------------------------- in a model
SAMPLES = 48000


def _clone_batch(b):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}


def _text_names(model):
    return [n for n, _ in model.named_parameters() if n.startswith("text_encoder.")]


def _grads_equal(runner, direct):
    for n, p in runner.model.named_parameters():
        a, b = direct[n], p.grad
        if n.startswith("text_encoder.model.pooler.") or n == "text_encoder.dummy_param":
            assert (a is None or float(a.abs().max()) == 0.0) and (b is None or float(b.abs().max()) == 0.0), n
        else:
            assert torch.equal(a, b), f"{n}: direct and operator-path gradients differ"


def _second_run_identical(runner, batch, lv, direct):
    """The same forward + backward again (the models' dropouts are 0): the loss and every gradient have identical bits."""
    loss = runner.forward_backward(_clone_batch(batch))
    assert float(loss.item()) == lv, "two runs give different losses"
    for n, p in runner.model.named_parameters():
        assert (p.grad is None and direct[n] is None) or torch.equal(p.grad, direct[n]), f"{n}: two runs differ"


def test_biencoder_through_strong_runner(dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import StrongRunner
    batch = O.synthetic_batch(2, SAMPLES, seed=7, ragged=True, hop=640, vocab_size=CFG["vocab_size"])
    ids, tps, mask = R.draw_inputs(2, 6, seed=7)
    del batch["text"]
    batch.update(input_ids=ids, token_type_ids=tps, attention_mask=mask, text_len=mask.sum(-1).numpy())
    torch.manual_seed(3)
    enc = text_encoder.Bert(None, CFG)
    enc.load_state_dict(_state())
    model = audio_text_model.BiEncoder(audio_encoder.CrnnEncoder(32000, 256), enc, match.DotProduct(), 64, add_proj=True)
    model.audio_encoder.dropout_p = 0.0
    runner = StrongRunner(model, device=str(dev))
    runner.model.train()
    loss = runner.forward_backward(_clone_batch(batch))
    lv = runner.loss_value(loss)
    direct = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in runner.model.named_parameters()}
    _second_run_identical(runner, batch, lv, direct)
    live = [n for n in _text_names(runner.model) if "pooler" not in n and "dummy" not in n and "key.bias" not in n]
    assert len(live) == len(NAMES) - CFG["num_hidden_layers"] and all(direct[n].abs().max() > 0 for n in live)
    assert not ops.DIRECT_GRADS
    runner.flat.zero_grad()
    loss2 = runner.loss_fn(runner.forward(_clone_batch(batch), training=True))
    loss2.backward()
    assert abs(float(loss2.item()) - lv) < 1e-6
    _grads_equal(runner, direct)
    frozen = {n: p.detach().clone() for n, p in runner.model.named_parameters() if "pooler" in n or "dummy_param" in n}
    assert len(frozen) == 3
    losses = [runner.loss_value(runner.train_step(_clone_batch(batch))) for _ in range(3)]
    print(f"StrongRunner BiEncoder(CrnnEncoder, Bert): loss {lv:.6f}; three steps:", [f"{v:.6f}" for v in losses])
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0]
    now = dict(runner.model.named_parameters())
    assert all(torch.equal(v, now[n]) for n, v in frozen.items()), "the pooler / dummy_param changed"


def test_multitext_biencoder_through_weak_phrase_runner(dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd import losses, ops
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import WeakPhraseRunner
    B, N, L = 2, 3, 5
    wave = O.synthetic_batch(B, SAMPLES, seed=11, ragged=True, hop=640, vocab_size=CFG["vocab_size"])
    ids, tps, mask = R.draw_inputs(B * N, L, seed=4)
    g = torch.Generator().manual_seed(6)
    batch = {"waveform": wave["waveform"], "waveform_len": wave["waveform_len"], "input_ids": ids.view(B, N, L),
             "token_type_ids": tps.view(B, N, L), "attention_mask": mask.view(B, N, L), "text_len": mask.sum(-1).view(B, N),
             "label": (torch.rand(B, N, generator=g) < 0.5).float()}
    enc = text_encoder.Bert(None, CFG)
    enc.load_state_dict(_state())
    torch.manual_seed(5)
    m = audio_text_model.MultiTextBiEncoder(audio_encoder.CrnnEncoder(32000, 256), enc, match.DotProduct(), 64,
                                            ["input_ids", "token_type_ids", "attention_mask"], add_proj=True)
    m.audio_encoder.dropout_p = 0.0
    runner = WeakPhraseRunner(m, loss_fn=losses.ClipBceLoss(), device=str(dev))
    runner.model.train()
    loss = runner.forward_backward(_clone_batch(batch))
    lv = float(loss.item())
    direct = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in runner.model.named_parameters()}
    _second_run_identical(runner, batch, lv, direct)
    assert not ops.DIRECT_GRADS
    runner.flat.zero_grad()
    out = runner.forward(_clone_batch(batch), training=True)
    assert out["clip_sim"].shape == (B, N)
    loss2 = runner.loss_fn(out)
    loss2.backward()
    assert abs(float(loss2.item()) - lv) < 1e-6
    _grads_equal(runner, direct)
    losses_ = [float(runner.train_step(_clone_batch(batch)).item()) for _ in range(3)]
    print(f"WeakPhraseRunner MultiTextBiEncoder(CrnnEncoder, Bert): loss {lv:.6f}; three steps:", [f"{v:.6f}" for v in losses_])
    assert all(np.isfinite(losses_)) and losses_[2] < losses_[1] < losses_[0]


# ---------------------------------------------------------------------------------------------- phrase embeddings
class _Tok:
    """A tokenizer over made-up words: [CLS]=1, [SEP]=2, word ids by hash; the call signature of a Hugging Face tokenizer."""
    pad_token_id = 0

    def __call__(self, texts, truncation=True, max_length=64, padding=False):
        rows = [([1] + [3 + (sum(map(ord, w)) % 100) for w in t.split()])[:max_length - 1] + [2] for t in texts]
        return {"input_ids": rows, "token_type_ids": [[0] * len(r) for r in rows]}


PHRASES = ["a dog barks", "rain", "a man speaks while a car passes by on a wet road", "birds", "a dog barks twice", "wind blows hard",
           "a b c d e f g h i j k l m n o p q r s t u v w x y z a b c d e f g h i j k l m n o p q r s t u v w x y z a b c d e f g h i j k l m n"]


def test_phrase_embedder_bucketed_equals_single(dev):
    from texttoaudiogrounding_amd.utils.text_embed import PhraseEmbedder
    enc = _sbert(dev, "mean", True).eval()
    emb = PhraseEmbedder(enc, _Tok(), batch_tokens=40)
    lens = [len(x) for x in emb.tokenize(PHRASES)[0]]
    assert max(lens) == 64 and len(emb.plan(lens, 40)) >= 3
    out = emb.encode(PHRASES)
    assert out.dtype == np.float32 and out.shape == (len(PHRASES), 64)
    assert np.array_equal(out, emb.encode(PHRASES)), "two runs differ"
    single = PhraseEmbedder(enc, _Tok(), batch_tokens=2)                 # one phrase per batch: no padding at all
    alone = single.encode(PHRASES)
    # the reference for the bound: the restatement on the unpadded phrase in fp64 and fp32
    st = R.draw_state(CFG, FX["state_seed"])
    ids, types = emb.tokenize(PHRASES)
    for i, p in enumerate(PHRASES):
        t = torch.tensor([ids[i]])
        z, m = torch.zeros_like(t), torch.ones_like(t)
        r64 = R.forward({k: v.double() for k, v in st.items()}, t, z, m, 4, 1, 1)[1][0]
        r32 = R.forward(st, t, z, m, 4, 1, 1)[1][0]
        d32 = R.rel_err(r32, r64)
        e_b, e_a, e_ab = R.rel_err(out[i], r64), R.rel_err(alone[i], r64), R.rel_err(out[i], alone[i])
        print(f"    {lens[i]:2d} tokens: bucketed {e_b:.2e}, alone {e_a:.2e}, bucketed vs alone {e_ab:.2e} (cpu fp32 {d32:.1e})")
        assert e_b < bound_for(d32) and e_a < bound_for(d32) and e_ab < bound_for(d32)


@pytest.mark.parametrize("with_proj", [False, True])
def test_retrieval_text_encoder(dev, with_proj):
    from texttoaudiogrounding_amd.utils.text_embed import RetrievalTextEncoder
    st = R.draw_state(CFG, FX["state_seed"])
    g = torch.Generator().manual_seed(17)
    pw, pb = torch.randn(48, 64, generator=g) / 8.0, 0.1 * torch.randn(48, generator=g)
    ckpt = {"text_encoder." + k: v for k, v in st.items()}
    ckpt.update({"text_proj.weight": pw, "text_proj.bias": pb, "audio_encoder.fc.weight": torch.zeros(3, 3),
                 "audio_proj.weight": torch.zeros(2, 2), "logit_scale": torch.zeros(())})
    enc = RetrievalTextEncoder(CFG, 48, with_proj)
    assert enc.load_retrieval_state_dict(ckpt) == 3
    enc = enc.to(dev).eval()
    ids, tps, mask = R.draw_inputs(5, 9, seed=5)
    with torch.no_grad():
        got = enc({"input_ids": ids, "token_type_ids": tps, "attention_mask": mask})["seq_emb"]
        again = enc({"input_ids": ids, "token_type_ids": tps, "attention_mask": mask})["seq_emb"]
    assert torch.equal(got, again)
    ref = {}
    for dt in (torch.float64, torch.float32):
        s = {k: v.to(dt) for k, v in st.items()}
        x = R.forward(s, ids, tps, mask, 4, 0, 0)[1]
        if with_proj:
            x = torch.nn.functional.linear(x, pw.to(dt), pb.to(dt))
            x = x.div(x.norm(p=2, dim=-1, keepdim=True) + 1e-7).clip(-1e3, 1e3)
        ref[dt] = x
    assert got.shape == ref[torch.float64].shape
    _check(f"RetrievalTextEncoder with_proj={with_proj}", got, ref[torch.float64], ref[torch.float32])
    if with_proj:
        with pytest.raises(ValueError):
            enc({"input_ids": ids, "token_type_ids": tps, "attention_mask": mask})


class _LabelEncoder:
    """What the tools read of a pickled sklearn LabelEncoder."""
    classes_ = np.array(["a dog barks loud", "rain falls", "wind blows"])


def test_tool_pickles_feed_map_phrase_to_event(dev, tmp_path):
    """tools/prepare_phrase_sbert.py (real encoder) -> pickles -> tools/map_phrase_to_event.py, as they are."""
    import importlib.util
    import json
    import os
    import pickle
    from texttoaudiogrounding_amd.utils.text_embed import PhraseEmbedder
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def tool(name):
        spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(root, "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    emb = PhraseEmbedder(_sbert(dev, "mean", True).eval(), _Tok(), batch_tokens=40)
    data = [{"audio_id": f"{i}.wav", "phrases": [{"phrase": p}]} for i, p in enumerate(PHRASES[:6])]
    paths = {k: str(tmp_path / k) for k in ("label.json", "enc.pkl", "phrase.pkl", "label.pkl", "map.tsv")}
    with open(paths["label.json"], "w") as f:
        json.dump(data, f)
    with open(paths["enc.pkl"], "wb") as f:
        pickle.dump(_LabelEncoder(), f)
    sb, mp = tool("prepare_phrase_sbert"), tool("map_phrase_to_event")
    sb.main(sb.build_parser().parse_args(["phrase", "--input", paths["label.json"], "--output", paths["phrase.pkl"]]), emb)
    sb.main(sb.build_parser().parse_args(["label", "--input", paths["enc.pkl"], "--output", paths["label.pkl"]]), emb)
    mp.main(mp.build_parser().parse_args(["--phrase_emb", paths["phrase.pkl"], "--label_emb", paths["label.pkl"], "--output",
                                          paths["map.tsv"], "--device", str(dev)]))
    rows = [line.split("\t") for line in open(paths["map.tsv"]).read().splitlines()]
    assert rows[0] == ["phrase", "index", "sim"] and [r[0] for r in rows[1:]] == PHRASES[:6]
    with open(paths["phrase.pkl"], "rb") as f:
        x = np.stack(list(pickle.load(f).values())).astype(np.float64)
    with open(paths["label.pkl"], "rb") as f:
        e = np.stack(list(pickle.load(f).values())).astype(np.float64)
    cos = (x / np.linalg.norm(x, axis=1, keepdims=True)) @ (e / np.linalg.norm(e, axis=1, keepdims=True)).T
    order = np.sort(cos, axis=1)
    assert float((order[:, -1] - order[:, -2]).min()) > 1e-4, "a near tie: choose other phrases"
    assert [int(r[1]) for r in rows[1:]] == cos.argmax(1).tolist()
    assert np.abs(np.array([float(r[2]) for r in rows[1:]]) - cos.max(1)).max() < 5e-6
