"""SelfAttention on the MI355X: the row-local attention core (csrc/text_attn.hip) alone against the fp64 restatement, the module
against the fixture made from the imported reference (tests/golden/text_selfattn.npz), lengths the reference cannot run, both
dropouts with the materialised masks, the whole-model case, StrongRunner.train_step (direct gradients, frozen text encoder, the
sticky token-id check), MultiTextBiEncoder's two paths and a token-level head on the contextual token_emb.

Bounds (the rule of tests/test_gpu_text_rnn.py, unchanged): 5e-6 relative to the largest entry of the tensor on outputs and on
every gradient whose recorded fp32 deviation of the REFERENCE is below 1.25e-6; where the recorded deviation is larger the
gradient bound is 4 x that deviation.  The kernel-alone cases have no recorded reference figure: their figure is the deviation of
the same restatement run in fp32 on the CPU, measured in the test, under the same rule.  Every measured error is printed.

Worst measured error per quantity on the MI355X: not measured yet (docs/experiments_text_selfattn.md says the same); every
case prints its figures under ``-s``."""
import numpy as np
import pytest
import torch

from tests import text_selfattn_ref as R

pytestmark = pytest.mark.gpu

BOUND, DEV_LIMIT = 5e-6, 1.25e-6


def bound_for(recorded_dev):
    return BOUND if recorded_dev < DEV_LIMIT else 4.0 * recorded_dev


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(f"{golden_dir}/text_selfattn.npz")


def _fixture_case(fx, name):
    cfg = R.CONFIGS[name]
    st = {k: torch.from_numpy(fx[f"{name}_param_{k}"]) for k in R.PARAM_NAMES}
    st["pe.pe"] = R.position_table(cfg["E"])
    return cfg, st, torch.from_numpy(fx[f"{name}_text"].astype(np.int64)), torch.from_numpy(fx[f"{name}_text_len"].astype(np.int64))


# (R, S, E, H): every S of {2, 3, 10, 32, 33, 64} (one token; the 32-key limit of the audio-over-tokens core and one past it; a
# full wave of query rows), head_dim {16, 32, 64, 128}, H {1, 4, 8}, R {1, 3, 17, 1024}
CORE_CASES = [(1, 2, 16, 1), (3, 3, 128, 4), (17, 10, 256, 4), (1024, 10, 128, 8), (17, 32, 64, 1), (3, 33, 512, 4), (17, 33, 256, 8),
              (3, 64, 128, 8), (1, 64, 128, 1), (17, 64, 64, 4), (1024, 3, 32, 1), (3, 2, 512, 8)]


def _core_case(Rn, S, E, H):
    g = torch.Generator().manual_seed(10000 * Rn + 100 * S + E + H)
    qkv = torch.randn(Rn, S, 3 * E, generator=g)
    dctx = torch.randn(Rn, S, E, generator=g)
    klen = torch.randint(1, S + 1, (Rn,), generator=g)
    klen[0] = S
    klen[-1] = 1 if Rn > 1 else S
    if Rn == 1:                                            # a single row cannot hold both ends: two launches below
        klen = torch.tensor([S])
    return qkv, dctx, klen


def _unaligned(t):
    """The same values in a view that is only 4-byte aligned (offset 1 of a flat buffer)."""
    buf = torch.zeros(t.numel() + 1, device=t.device, dtype=t.dtype)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view_as(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("Rn,S,E,H", CORE_CASES)
def test_core_alone_vs_fp64(dev, Rn, S, E, H, p):
    from texttoaudiogrounding_amd import ops
    qkv, dctx, klen = _core_case(Rn, S, E, H)
    klens = [klen] if Rn > 1 else [klen, torch.tensor([1])]       # klen includes 1 and S in every case
    for klen in klens:
        seed = 1234 + S
        qd, dd, kd = qkv.to(dev), dctx.to(dev), klen.to(dev)
        mask = ops.dropout_mask(seed, (Rn, H, S, S), p, dev).cpu() if p > 0.0 else None
        ref = R.core_results(qkv, klen, H, dctx, torch.float64, mask, p)
        f32 = R.core_results(qkv, klen, H, dctx, torch.float32, mask, p)
        ctx, attn = ops.text_selfattn_core(qd, kd, H, True, p, seed)
        ctx2, attn2 = ops.text_selfattn_core(qd, kd, H, True, p, seed)
        assert torch.equal(ctx, ctx2) and torch.equal(attn, attn2), "two forward runs differ"
        ctx3, attn3 = ops.text_selfattn_core(qd, kd, H, False, p, seed)
        assert attn3 is None and torch.equal(ctx3, ctx), "the forward without attn gives another ctx"
        dqkv = ops.text_selfattn_core_backward(qd, attn, dd, kd, H, p, seed)
        dqkv2 = ops.text_selfattn_core_backward(qd, attn, dd, kd, H, p, seed)
        assert torch.equal(dqkv, dqkv2), "two backward runs differ"
        assert dqkv.shape == qkv.shape and torch.isfinite(dqkv).all()
        # the weights: rows sum to 1 over the valid keys, exactly 0 beyond klen
        dead = (torch.arange(S)[None, :] >= klen[:, None])[:, None, None, :].expand(Rn, H, S, S)
        assert float(attn.cpu()[dead].abs().max()) == 0.0 if dead.any() else True
        assert (attn.sum(-1) - 1.0).abs().max().item() < 1e-5
        errs = {"ctx": (R.rel_err(ctx, ref["ctx"]), BOUND, R.rel_err(f32["ctx"], ref["ctx"])),
                "attn": (R.rel_err(attn, ref["attn"]), BOUND, R.rel_err(f32["attn"], ref["attn"]))}
        d32 = R.rel_err(f32["dqkv"], ref["dqkv"])
        errs["dqkv"] = (R.rel_err(dqkv, ref["dqkv"]), bound_for(d32), d32)
        print(f"text_selfattn core R={Rn} S={S} E={E} H={H} p={p} klen[{int(klen.min())}..{int(klen.max())}]: "
              + ", ".join(f"{k} {e:.2e} (cpu fp32 {d:.1e})" for k, (e, b, d) in errs.items()))
        for k, (e, b, d) in errs.items():
            assert e < b, (k, e, b)


def test_core_scalar_form_gives_the_same_bits(dev):
    """qkv (and dctx) only 4-byte aligned: the kernels take their scalar-read form, the same fmaf chain."""
    from texttoaudiogrounding_amd import ops
    Rn, S, E, H, p, seed = 17, 10, 128, 4, 0.3, 99
    qkv, dctx, klen = _core_case(Rn, S, E, H)
    qd, dd, kd = qkv.to(dev), dctx.to(dev), klen.to(dev)
    assert qd.data_ptr() % 16 == 0 and dd.data_ptr() % 16 == 0
    ctx, attn = ops.text_selfattn_core(qd, kd, H, True, p, seed)
    dqkv = ops.text_selfattn_core_backward(qd, attn, dd, kd, H, p, seed)
    qu, du = _unaligned(qd), _unaligned(dd)
    ctx_u, attn_u = ops.text_selfattn_core(qu, kd, H, True, p, seed)
    assert torch.equal(ctx_u, ctx) and torch.equal(attn_u, attn)
    for a, b in ((qu, du), (qu, dd), (qd, du)):
        assert torch.equal(ops.text_selfattn_core_backward(a, attn, b, kd, H, p, seed), dqkv)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_cls_pe_kernels(dev, p):
    from texttoaudiogrounding_amd import ops
    g = torch.Generator().manual_seed(3)
    Rn, L, E, seed = 17, 5, 48, 321
    tok, cls, pe = torch.randn(Rn, L, E, generator=g), torch.randn(1, 1, E, generator=g), torch.randn(1, 100, E, generator=g)
    dx = torch.randn(Rn, L + 1, E, generator=g)
    keep = ops.dropout_mask(seed, (Rn, L + 1, E), p, dev).cpu().double() / (1.0 - p) if p > 0.0 else 1.0
    want = (torch.cat((cls.expand(Rn, -1, -1), tok), 1).double() + pe[:, :L + 1].double()) * keep
    x = ops.text_cls_pe_forward(tok.to(dev), cls.to(dev), pe[0].to(dev), p, seed)
    dtok, dcls = ops.text_cls_pe_backward(dx.to(dev), p, seed)
    dtok2, dcls2 = ops.text_cls_pe_backward(dx.to(dev), p, seed)
    assert torch.equal(dtok, dtok2) and torch.equal(dcls, dcls2)
    gk = dx.double() * keep
    errs = dict(x=R.rel_err(x, want), dtok=R.rel_err(dtok, gk[:, 1:]), dcls=R.rel_err(dcls, gk[:, 0].sum(0)))
    print(f"text_cls_pe p={p}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    # x, dtok: at most six roundings of 2^-24 (the sum, 1 - p, its reciprocal, the product), relative to the largest entry
    assert errs["x"] < 4e-7 and errs["dtok"] < 4e-7 and errs["dcls"] < BOUND
    only_tok, none = ops.text_cls_pe_backward(dx.to(dev), p, seed, need_dcls=False)
    assert none is None and torch.equal(only_tok, dtok)
    with pytest.raises(ValueError, match="positions"):
        ops.text_cls_pe_forward(tok.to(dev), cls.to(dev), pe[0, :L].to(dev))


def _encoder(cfg, st, dev, dropout=0.0):
    from texttoaudiogrounding_amd.models.text_encoder import SelfAttention
    enc = SelfAttention(cfg["V"], cfg["E"], cfg["heads"], dropout)
    enc.load_state_dict(st, strict=True)
    return enc.to(dev)


def _module_results(enc, cfg, text, text_len, dev):
    enc.zero_grad(set_to_none=True)
    o = enc({"text": text, "text_len": text_len})
    wt, ws = R.objective_weights(cfg, torch.float32)
    R.objective(o["token_emb"], o["seq_emb"], wt.to(dev), ws.to(dev)).backward()
    got = {"token_emb": o["token_emb"].detach(), "seq_emb": o["seq_emb"].detach()}
    got.update({"d" + k: p.grad for k, p in enc.named_parameters()})
    return got


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_module_vs_reference_fixture(dev, fx, name, mode):
    cfg, st, text, text_len = _fixture_case(fx, name)
    enc = _encoder(cfg, st, dev)
    enc.train(mode == "train")
    got = _module_results(enc, cfg, text, text_len, dev)
    assert got["token_emb"].shape == (cfg["R"], cfg["L"], cfg["E"]) and got["seq_emb"].shape == (cfg["R"], cfg["E"])
    assert got["token_emb"][0, -1].abs().max() > 0, "token_emb at a padded position is not zero in the reference"
    assert got["dembedding.core.weight"][0].abs().max() > 0, "row 0 of the table (the pad id) receives gradient in the reference"
    assert got["dcls_token"].shape == (1, 1, cfg["E"])
    recorded = dict(zip(fx[f"{name}_quantities"].tolist(), fx[f"{name}_f32_dev"].tolist()))
    errs = {k: (R.rel_err(got[k], fx[f"{name}_f64_{k}"]), BOUND if k in ("token_emb", "seq_emb") else bound_for(recorded[k]))
            for k in recorded}
    print(f"SelfAttention {name} ({mode}) vs the reference's fp64: " + ", ".join(f"{k} {e:.2e}" for k, (e, _) in errs.items()))
    for k, (e, b) in errs.items():
        assert e < b, (k, e, b, recorded[k])
    # any leading shape EmbeddingLayer accepts; lengths as a list / numpy array / tensor
    L, E = cfg["L"], cfg["E"]
    with torch.no_grad():
        o2 = enc({"text": text[:8].view(2, 4, L).numpy(), "text_len": text_len[:8].view(2, 4).numpy()})
        o3 = enc({"text": text[:8], "text_len": text_len[:8].tolist()})
        o4 = enc({"text": text[:8].to(dev), "text_len": text_len[:8].to(dev)})
    assert o2["token_emb"].shape == (2, 4, L, E) and o2["seq_emb"].shape == (2, 4, E)
    assert torch.equal(o2["token_emb"].view(8, L, -1), o3["token_emb"]) and torch.equal(o2["seq_emb"].view(8, -1), o3["seq_emb"])
    assert torch.equal(o4["token_emb"], o3["token_emb"]) and torch.equal(o4["seq_emb"], o3["seq_emb"])
    assert torch.equal(o3["token_emb"], got["token_emb"][:8]) and torch.equal(o3["seq_emb"], got["seq_emb"][:8]), \
        "rows of a batch never interact"


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_lengths_the_reference_cannot_run(dev, fx, name):
    """max(text_len) < L and text_len 0 (only cls is attended): against the restatement, outputs and every gradient."""
    cfg, st, _, _ = _fixture_case(fx, name)
    text, text_len = R.draw_inputs(cfg, full=False)
    assert int(text_len.min()) == 0 and int(text_len.max()) < cfg["L"]
    got = _module_results(_encoder(cfg, st, dev).train(), cfg, text, text_len, dev)
    assert all(torch.isfinite(v).all() for v in got.values())
    ref = R.config_results(cfg, st, text, text_len, torch.float64)
    f32 = R.config_results(cfg, st, text, text_len, torch.float32)
    errs = {k: (R.rel_err(got[k], ref[k]), BOUND if k in ("token_emb", "seq_emb") else bound_for(R.rel_err(f32[k], ref[k]))) for k in ref}
    print(f"SelfAttention {name} text_len in [0, L-1]: " + ", ".join(f"{k} {e:.2e}" for k, (e, _) in errs.items()))
    for k, (e, b) in errs.items():
        assert e < b, (k, e, b)


@pytest.mark.parametrize("name", ["e64_h4", "e64_h1"])
def test_dropout(dev, fx, name):
    from texttoaudiogrounding_amd import ops
    cfg, st, text, text_len = _fixture_case(fx, name)
    p, S = 0.3, cfg["L"] + 1
    enc = _encoder(cfg, st, dev, dropout=p).train()
    torch.manual_seed(77)
    seed = ops.new_seed()                                 # what the module draws first after this manual_seed
    torch.manual_seed(77)
    got = _module_results(enc, cfg, text, text_len, dev)
    s_pe, s_attn = ops.text_selfattn_dropout_seeds(seed)
    pe_mask = ops.dropout_mask(s_pe, (cfg["R"], S, cfg["E"]), p, dev).cpu()
    attn_mask = ops.dropout_mask(s_attn, (cfg["R"], cfg["heads"], S, S), p, dev).cpu()
    kept = (float(pe_mask.float().mean()), float(attn_mask.float().mean()))
    assert abs(kept[0] - (1 - p)) < 0.05 and abs(kept[1] - (1 - p)) < 0.05, kept
    assert not torch.equal(pe_mask.view(-1)[:1000], attn_mask.view(-1)[:1000]), "the two dropouts share one mask"
    ref = R.config_results(cfg, st, text, text_len, torch.float64, pe_mask, attn_mask, p)
    f32 = R.config_results(cfg, st, text, text_len, torch.float32, pe_mask, attn_mask, p)
    errs = {}
    for k in ref:
        d32 = R.rel_err(f32[k], ref[k])
        errs[k] = (R.rel_err(got[k], ref[k]), BOUND if k in ("token_emb", "seq_emb") else bound_for(d32))
    print(f"SelfAttention {name} dropout {p}: kept {kept[0]:.3f} / {kept[1]:.3f}; " + ", ".join(f"{k} {e:.2e}" for k, (e, _) in errs.items()))
    for k, (e, b) in errs.items():
        assert e < b, (k, e, b)
    torch.manual_seed(77)
    again = _module_results(enc, cfg, text, text_len, dev)
    assert all(torch.equal(again[k], got[k]) for k in got), "the same seed must give the same step"
    torch.manual_seed(78)
    other = _module_results(enc, cfg, text, text_len, dev)
    assert not torch.equal(other["token_emb"], got["token_emb"]), "two seeds gave the same mask"
    # eval mode ignores p
    enc.eval()
    ev = _module_results(enc, cfg, text, text_len, dev)
    assert R.rel_err(ev["token_emb"], fx[f"{name}_f64_token_emb"]) < BOUND


def _biencoder(text_enc, freeze_text=False):
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match
    return audio_text_model.BiEncoder(audio_encoder.CrnnEncoder(32000, 256), text_enc, match.DotProduct(), 256,
                                      freeze_text_encoder=freeze_text)


def test_whole_model_eval_vs_reference_fixture(dev, fx):
    from texttoaudiogrounding_amd.models import text_encoder
    m = R.MODEL
    st, batch = R.model_state(), R.model_batch()
    assert np.allclose(R.state_checksum(st), fx["model_state_checksum"], rtol=1e-12, atol=0)
    assert np.allclose(R.checksum(batch["waveform"]), fx["model_waveform_checksum"], rtol=1e-12, atol=0)
    assert np.array_equal(batch["text"].numpy(), fx["model_text"]) and np.array_equal(batch["text_len"], fx["model_text_len"])
    model = _biencoder(text_encoder.SelfAttention(m["V"], m["E"], m["heads"], 0.0))
    missing = model.load_state_dict(st, strict=False)
    assert not missing.unexpected_keys and all("melspec" in k or "window" in k or "fb" in k for k in missing.missing_keys), missing
    assert [k for k in model.state_dict() if k.startswith("text_encoder.")] == fx["model_keys"].tolist()
    model = model.to(dev).eval()
    with torch.no_grad():
        o = model({"waveform": batch["waveform"].to(dev), "waveform_len": batch["waveform_len"], "text": batch["text"],
                   "text_len": batch["text_len"], "specaug": False})
    ref = torch.from_numpy(fx["model_frame_sim_f64"])
    assert o["frame_sim"].shape == ref.shape and torch.as_tensor(o["length"]).tolist() == fx["model_length"].tolist()
    e = (o["frame_sim"].cpu().double() - ref).abs().max().item()
    print(f"BiEncoder(CrnnEncoder, SelfAttention, DotProduct) eval: frame_sim err {e:.2e} (the reference's own fp32: "
          f"{float(fx['model_frame_sim_f32_dev']):.2e} relative)")
    assert e < 1e-4


def _strong_model(freeze_text=False, freeze_embedding=False):
    from texttoaudiogrounding_amd.models import text_encoder
    m = R.MODEL
    model = _biencoder(text_encoder.SelfAttention(m["V"], m["E"], m["heads"], 0.0), freeze_text)
    model.load_state_dict(R.model_state(), strict=False)
    model.audio_encoder.dropout_p = 0.0
    return model


def _clone_batch(b):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}


def _train_batch():
    """The whole-model batch at its full padded width (text_len [1, 2] in 4 columns): a batch the reference cannot run."""
    from oracle import tag_oracle as O
    return O.synthetic_batch(2, R.MODEL["samples"], seed=R.MODEL["batch_seed"], ragged=True, hop=640, vocab_size=R.MODEL["V"])


def test_strong_runner_train_step(dev):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.runner import StrongRunner
    batch = _train_batch()
    runner = StrongRunner(_strong_model(), device=str(dev))
    runner.model.train()
    names = [n for n, _ in runner.model.named_parameters()]
    assert "text_encoder.cls_token" in names
    loss = runner.forward_backward(_clone_batch(batch))
    lv = runner.loss_value(loss)
    direct = {n: p.grad.detach().clone() for n, p in runner.model.named_parameters()}
    assert all(direct[n].abs().max() > 0 for n in names if n.startswith("text_encoder.")), "a text gradient is all zero"
    # the same step through plain autograd (the operators' registered formulas, AccumulateGrad into the same flat views)
    assert not ops.DIRECT_GRADS
    runner.flat.zero_grad()
    out = runner.forward(_clone_batch(batch), training=True)
    loss2 = runner.loss_fn(out)
    loss2.backward()
    assert abs(float(loss2.item()) - lv) < 1e-6
    worst = 0.0
    for n, p in runner.model.named_parameters():
        e = R.rel_err(direct[n], p.grad)
        worst = max(worst, e)
        assert e < 1e-6, (n, e)
    print(f"StrongRunner BiEncoder(CrnnEncoder, SelfAttention): loss {lv:.6f}; direct vs plain-autograd gradients, worst {worst:.2e}")
    # a whole step moves every parameter of the text encoder, cls_token included
    before = {n: p.detach().clone() for n, p in runner.model.named_parameters()}
    runner.loss_value(runner.train_step(_clone_batch(batch)))
    assert all(not torch.equal(before[n], p) for n, p in runner.model.named_parameters() if n.startswith("text_encoder."))
    # frozen after the flat buffers were built (a fresh runner: Adam's moments are still zero): no GEMM for them, their
    # flat-gradient rows and their values stay untouched while the audio side trains
    r1 = StrongRunner(_strong_model(), device=str(dev))
    for p in r1.model.text_encoder.parameters():
        p.requires_grad = False
    before = {n: p.detach().clone() for n, p in r1.model.named_parameters()}
    r1.loss_value(r1.train_step(_clone_batch(batch)))
    for n, p in r1.model.named_parameters():
        if n.startswith("text_encoder."):
            assert torch.equal(before[n], p) and float(p._tag_grad_sink.abs().max()) == 0.0, n
    assert not torch.equal(before["audio_encoder.gru.weight_hh_l0"], dict(r1.model.named_parameters())["audio_encoder.gru.weight_hh_l0"])
    # frozen by the constructor: the text parameters are not in the flat buffers at all and a step leaves them alone
    r2 = StrongRunner(_strong_model(freeze_text=True), device=str(dev))
    before = {n: p.detach().clone() for n, p in r2.model.text_encoder.named_parameters()}
    r2.loss_value(r2.train_step(_clone_batch(batch)))
    assert all(torch.equal(before[n], p) and p.grad is None for n, p in r2.model.text_encoder.named_parameters())
    # a device-resident token id outside the table: clamped by the gather, reported by the sticky flag
    bad = _clone_batch(batch)
    bad["text"] = bad["text"].to(dev)
    bad["text"][0, 0] = R.MODEL["V"] + 5
    r3 = StrongRunner(_strong_model(), device=str(dev))
    loss = r3.forward_backward(bad)
    with pytest.raises(IndexError, match="out of range"):
        r3.loss_value(loss)


def test_multitext_biencoder_both_paths(dev):
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    m = R.MODEL
    B, N, L = 4, 5, 6
    g = torch.Generator().manual_seed(91)
    wave = 0.1 * torch.randn(B, 48000, generator=g)
    text = torch.randint(2, m["V"], (B, N, L), generator=g)
    text_len = torch.randint(1, L + 1, (B, N), generator=g)
    for b in range(B):
        for n in range(N):
            text[b, n, text_len[b, n]:] = 0
    model = audio_text_model.MultiTextBiEncoder(audio_encoder.CrnnEncoder(32000, 256),
                                                text_encoder.SelfAttention(m["V"], m["E"], m["heads"], 0.0),
                                                match.DotProduct(), 256, text_forward_keys=["text"])
    model.load_state_dict(R.model_state(), strict=False)
    model = model.to(dev).eval()
    inp = {"waveform": wave.to(dev), "waveform_len": np.full(B, 48000), "text": text, "text_len": text_len, "specaug": False}
    with torch.no_grad():
        grouped = model(dict(inp))
        general = model._forward_general(dict(inp))
    assert grouped["frame_sim"].shape == general["frame_sim"].shape == (B, 19, N)
    e_fs = (grouped["frame_sim"] - general["frame_sim"]).abs().max().item()
    e_cs = (grouped["clip_sim"] - general["clip_sim"]).abs().max().item()
    print(f"MultiTextBiEncoder(CrnnEncoder, SelfAttention) B={B} N={N}: grouped vs general frame_sim {e_fs:.2e}, clip_sim {e_cs:.2e}")
    assert e_fs < 5e-6 and e_cs < 5e-6 and grouped["clip_sim"].shape == (B, N)
    # the text side against the fp64 restatement (R = B * N rows in one launch)
    st = R.model_text_state()
    with torch.no_grad():
        te = model.text_encoder({"text": text.view(B * N, L), "text_len": text_len.view(-1)})
    tok, seq = R.encoder_forward({k: v.double() for k, v in st.items()}, text.view(B * N, L), text_len.view(-1), m["heads"])
    assert R.rel_err(te["token_emb"], tok) < BOUND and R.rel_err(te["seq_emb"], seq) < BOUND


def test_token_level_head_on_contextual_token_emb(dev, fx):
    """match.CrossAttention over SelfAttention's token_emb: the head's gradient reaches mha.in_proj_weight (and every other text
    parameter) and equals the restatement's gradient for the same d token_emb."""
    from texttoaudiogrounding_amd.models import match
    name = "e64_h4"
    cfg, st, text, text_len = _fixture_case(fx, name)
    enc = _encoder(cfg, st, dev).train()
    torch.manual_seed(5)
    head = match.CrossAttention(cfg["E"], 4, 0.0).to(dev).train()
    g = torch.Generator().manual_seed(6)
    audio = torch.randn(cfg["R"], 7, cfg["E"], generator=g).to(dev)
    o = enc({"text": text, "text_len": text_len})
    tok = o["token_emb"]
    tok.retain_grad()
    sim = head({"audio_emb": audio, "text_emb": o, "text_len": text_len.to(dev)})
    assert sim.shape == (cfg["R"], 7)
    sim.sum().backward()
    dtok = tok.grad.detach().cpu().double()
    assert dtok.abs().max() > 0
    s = {k: v.double().clone().requires_grad_(k in R.PARAM_NAMES) for k, v in st.items()}
    tok64, _ = R.encoder_forward(s, text, text_len, cfg["heads"])
    (tok64 * dtok).sum().backward()
    assert R.rel_err(tok, tok64) < BOUND
    errs = {k: R.rel_err(dict(enc.named_parameters())[k].grad, s[k].grad) for k in R.PARAM_NAMES}
    print("CrossAttention head on SelfAttention token_emb: " + ", ".join(f"d{k} {e:.2e}" for k, e in errs.items()))
    assert enc.mha.in_proj_weight.grad.abs().max() > 0
    for k, e in errs.items():
        assert e < BOUND, (k, e)
