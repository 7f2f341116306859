"""RnnEncoder on the MI355X: the two row-local recurrence kernels (csrc/text_gru.hip) alone against the fp64 restatement, the
module against the fixture made from the imported reference (tests/golden/text_rnn.npz), the whole-model case, inter-layer
dropout with the materialised mask, StrongRunner.train_step (direct gradients, frozen text encoder, the sticky token-id check)
and MultiTextBiEncoder's two paths.

Bounds: 5e-6 relative to the largest entry of the tensor (the project's bound for a head of this depth, tests/test_gpu_weak.py)
on token_emb, seq_emb and on every gradient whose recorded fp32 deviation of the REFERENCE is below 1.25e-6; where the recorded
deviation is larger the gradient bound is 4 x that deviation.  The kernel-alone cases have no recorded reference figure: their
figure is the deviation of the same restatement run in fp32 on the CPU, measured in the test, under the same rule.
Every measured error is printed.

Measured on the MI355X, worst per quantity: docs/experiments_text_rnn.md (at most 9.5e-7, the saved gates at H = 512)."""
import numpy as np
import pytest
import torch

from tests import text_rnn_ref as R

pytestmark = pytest.mark.gpu

BOUND, DEV_LIMIT = 5e-6, 1.25e-6


def bound_for(recorded_dev):
    return BOUND if recorded_dev < DEV_LIMIT else 4.0 * recorded_dev


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(f"{golden_dir}/text_rnn.npz")


def _fixture_case(fx, name):
    cfg = R.CONFIGS[name]
    st = {k: torch.from_numpy(fx[f"{name}_param_{k}"]) for k in R.param_names(cfg["layers"], cfg["dirs"])}
    return cfg, st, torch.from_numpy(fx[f"{name}_text"].astype(np.int64)), torch.from_numpy(fx[f"{name}_text_len"].astype(np.int64))


# every value of R {1, 3, 17, 64, 1024}, L {1, 2, 9, 20}, H {1, 16, 50, 128, 256, 512}, dirs {1, 2}, and (1024, 12, 256, 2)
KERNEL_CASES = [(1, 1, 1, 1), (3, 2, 16, 2), (17, 9, 50, 2), (64, 20, 128, 1), (1024, 12, 256, 2), (64, 9, 512, 2),
                (17, 20, 50, 1), (3, 9, 256, 1), (1, 2, 128, 2), (64, 1, 16, 1), (1024, 2, 1, 2), (17, 9, 20, 2)]


def _kernel_case(Rn, L, H, dirs):
    g = torch.Generator().manual_seed(1000 * Rn + 100 * L + 10 * H + dirs)
    k = 1.0 / max(H, 1) ** 0.5
    gi = torch.randn(Rn, L, dirs, 3 * H, generator=g)
    w_hh = (torch.rand(dirs, 3 * H, H, generator=g) * 2 - 1) * k
    b_hh = (torch.rand(dirs, 3 * H, generator=g) * 2 - 1) * k
    lens = torch.randint(1, L + 1, (Rn,), generator=g)
    lens[0] = L
    lens[-1] = 1
    dy = torch.randn(Rn, L, dirs * H, generator=g)
    dseq = torch.randn(Rn, dirs * H, generator=g)
    return gi, w_hh, b_hh, lens, dy, dseq


def _restated(gi, w_hh, b_hh, lens, dy, dseq, dtype):
    """Forward and backward of one launch in ``dtype`` on the CPU through plain autograd: y, gates, seq, hprev, dgi, dgh for the
    three gradient inputs (dy only, dseq only, both)."""
    out = {}
    for tag, use_dy, use_dseq in (("both", True, True), ("dy", True, False), ("dseq", False, True)):
        gi_ = gi.to(dtype).clone().requires_grad_(True)
        y, gates, seq, hprev, ghs = R.recurrence(gi_, w_hh.to(dtype), b_hh.to(dtype), lens, keep_gh=True)
        loss = 0.0
        if use_dy:
            loss = loss + (y * dy.to(dtype)).sum()
        if use_dseq:
            loss = loss + (seq * dseq.to(dtype)).sum()
        loss.backward()
        dgh = torch.zeros_like(gi_)
        for d, t, gh in ghs:
            dgh[:, t, d] = gh.grad
        out[tag] = dict(dgi=gi_.grad, dgh=dgh.detach())
        out.update(y=y.detach(), gates=gates.detach(), seq=seq.detach(), hprev=hprev.detach())
    return out


@pytest.mark.parametrize("Rn,L,H,dirs", KERNEL_CASES)
def test_kernels_alone_vs_fp64(dev, Rn, L, H, dirs):
    from texttoaudiogrounding_amd import ops
    gi, w_hh, b_hh, lens, dy, dseq = _kernel_case(Rn, L, H, dirs)
    ref = _restated(gi, w_hh, b_hh, lens, dy, dseq, torch.float64)
    f32 = _restated(gi, w_hh, b_hh, lens, dy, dseq, torch.float32)
    gd, wd, bd, ld = gi.to(dev), w_hh.to(dev), b_hh.to(dev), lens.to(dev)
    y, gates, seq = ops.text_gru_recurrence(gd, wd, bd, ld, True)
    y2, gates2, seq2 = ops.text_gru_recurrence(gd, wd, bd, ld, True)
    assert torch.equal(y, y2) and torch.equal(gates, gates2) and torch.equal(seq, seq2), "two forward runs differ"
    # nullable outputs absent: the same hidden states
    y3, g3, s3 = ops.text_gru_recurrence(gd, wd, bd, None, False)
    assert g3 is None and s3 is None and torch.equal(y3, y)
    # a W_hh that is only 4-byte aligned (a flat-parameter view) takes the scalar-read form of the kernel: same arithmetic
    buf = torch.zeros(wd.numel() + 1, device=dev)
    buf[1:].copy_(wd.reshape(-1))
    y4, g4, s4 = ops.text_gru_recurrence(gd, buf[1:].view_as(wd), bd, ld, True)
    assert torch.equal(y4, y) and torch.equal(g4, gates) and torch.equal(s4, seq)
    errs = {}
    for k, got in (("y", y), ("gates", gates), ("seq", seq)):
        errs[k] = (R.rel_err(got, ref[k]), BOUND, R.rel_err(f32[k], ref[k]))
    for tag, a_dy, a_dseq in (("both", dy, dseq), ("dy", dy, None), ("dseq", None, dseq)):
        args = (a_dy.to(dev) if a_dy is not None else None, a_dseq.to(dev) if a_dseq is not None else None, ld, y, gates, wd)
        dgi, dgh, hprev = ops.text_gru_recurrence_backward(*args)
        dgi2, dgh2, hprev2 = ops.text_gru_recurrence_backward(*args)
        assert torch.equal(dgi, dgi2) and torch.equal(dgh, dgh2) and torch.equal(hprev, hprev2), "two backward runs differ"
        for k, got in (("dgi", dgi), ("dgh", dgh)):
            dev32 = R.rel_err(f32[tag][k], ref[tag][k])
            errs[f"{k}[{tag}]"] = (R.rel_err(got, ref[tag][k]), bound_for(dev32), dev32)
        errs[f"hprev[{tag}]"] = (R.rel_err(hprev, ref["hprev"]) if L > 1 else float(hprev.abs().max()), BOUND, 0.0)
    print(f"text_gru kernels R={Rn} L={L} H={H} dirs={dirs}: " + ", ".join(f"{k} {e:.2e} (cpu fp32 {d:.1e})" for k, (e, b, d) in errs.items()))
    for k, (e, b, d) in errs.items():
        assert e < b, (k, e, b)


def _encoder(cfg, st, dev, dropout=0.0):
    from texttoaudiogrounding_amd.models.text_encoder import RnnEncoder
    enc = RnnEncoder(cfg["V"], cfg["E"], cfg["H"], cfg["layers"], dropout, cfg["dirs"] == 2, "GRU")
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
    assert got["token_emb"].shape == (cfg["R"], cfg["L"], cfg["H"] * cfg["dirs"])
    assert got["token_emb"][0, -1].abs().max() > 0, "token_emb at a padded position is not zero in the reference"
    assert got["dembedding.core.weight"][0].abs().max() > 0, "row 0 of the table (the pad id) receives gradient in the reference"
    recorded = dict(zip(fx[f"{name}_quantities"].tolist(), fx[f"{name}_f32_dev"].tolist()))
    errs = {k: (R.rel_err(got[k], fx[f"{name}_f64_{k}"]), BOUND if k in ("token_emb", "seq_emb") else bound_for(recorded[k]))
            for k in recorded}
    print(f"RnnEncoder {name} ({mode}) vs the reference's fp64: " + ", ".join(f"{k} {e:.2e}" for k, (e, _) in errs.items()))
    for k, (e, b) in errs.items():
        assert e < b, (k, e, b, recorded[k])
    # any leading shape EmbeddingLayer accepts; lengths as a list / numpy array
    R_, L = cfg["R"], cfg["L"]
    with torch.no_grad():
        o2 = enc({"text": text[:16].view(4, 4, L).numpy(), "text_len": text_len[:16].view(4, 4).numpy()})
        o3 = enc({"text": text[:16], "text_len": text_len[:16].tolist()})
    assert o2["token_emb"].shape == (4, 4, L, cfg["H"] * cfg["dirs"]) and o2["seq_emb"].shape == (4, 4, cfg["H"] * cfg["dirs"])
    assert torch.equal(o2["token_emb"].view(16, L, -1), o3["token_emb"]) and torch.equal(o2["seq_emb"].view(16, -1), o3["seq_emb"])
    assert torch.equal(o3["token_emb"], got["token_emb"][:16]), "rows of a batch never interact"


def test_whole_model_eval_vs_reference_fixture(dev, fx):
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    m = R.MODEL
    st, batch = R.model_state(), R.model_batch()
    assert np.allclose(R.state_checksum(st), fx["model_state_checksum"], rtol=1e-12, atol=0)
    assert np.allclose(R.checksum(batch["waveform"]), fx["model_waveform_checksum"], rtol=1e-12, atol=0)
    assert np.array_equal(batch["text"].numpy(), fx["model_text"]) and np.array_equal(batch["text_len"], fx["model_text_len"])
    model = audio_text_model.BiEncoder(audio_encoder.CrnnEncoder(32000, 256),
                                       text_encoder.RnnEncoder(m["V"], m["E"], m["H"], m["layers"], 0.0, m["dirs"] == 2, "GRU"),
                                       match.DotProduct(), 256)
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
    print(f"BiEncoder(CrnnEncoder, RnnEncoder, DotProduct) eval: frame_sim err {e:.2e} (the reference's own fp32: "
          f"{float(fx['model_frame_sim_f32_dev']):.2e} relative)")
    assert e < 1e-4


@pytest.mark.parametrize("name", ["l2_bi", "l2_uni"])
def test_inter_layer_dropout(dev, fx, name):
    from texttoaudiogrounding_amd import ops
    cfg, st, text, text_len = _fixture_case(fx, name)
    p, D = 0.3, cfg["H"] * cfg["dirs"]
    enc = _encoder(cfg, st, dev, dropout=p).train()
    torch.manual_seed(77)
    seed = ops.new_seed()                                 # what the module draws first after this manual_seed
    torch.manual_seed(77)
    got = _module_results(enc, cfg, text, text_len, dev)
    masks = [ops.dropout_mask(ops.text_gru_dropout_seed(seed, l), (cfg["R"], cfg["L"], D), p, dev).cpu()
             for l in range(cfg["layers"] - 1)]
    kept = float(masks[0].float().mean())
    assert abs(kept - (1 - p)) < 0.05, kept
    ref = R.config_results(cfg, st, text, text_len, torch.float64, masks, p)
    f32 = R.config_results(cfg, st, text, text_len, torch.float32, masks, p)
    errs = {}
    for k in ref:
        d32 = R.rel_err(f32[k], ref[k])
        errs[k] = (R.rel_err(got[k], ref[k]), BOUND if k in ("token_emb", "seq_emb") else bound_for(d32))
    print(f"RnnEncoder {name} dropout {p}: kept {kept:.3f}; " + ", ".join(f"{k} {e:.2e}" for k, (e, _) in errs.items()))
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


def _strong_model(freeze_text=False):
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    m = R.MODEL
    model = audio_text_model.BiEncoder(audio_encoder.CrnnEncoder(32000, 256),
                                       text_encoder.RnnEncoder(m["V"], m["E"], m["H"], 2, 0.0, True, "GRU"),
                                       match.DotProduct(), 256, freeze_text_encoder=freeze_text)
    st = R.model_state()
    st.update({"text_encoder." + k: v for k, v in R.draw_params(m["V"], m["E"], m["H"], 2, 2, 67).items()})
    model.load_state_dict(st, strict=False)
    model.audio_encoder.dropout_p = 0.0
    return model


def _clone_batch(b):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}


def test_strong_runner_train_step(dev):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.runner import StrongRunner
    batch = R.model_batch()
    runner = StrongRunner(_strong_model(), device=str(dev))
    runner.model.train()
    names = [n for n, _ in runner.model.named_parameters()]
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
    print(f"StrongRunner BiEncoder(CrnnEncoder, RnnEncoder x2 layers): loss {lv:.6f}; direct vs plain-autograd gradients, worst {worst:.2e}")
    # a whole step moves every parameter of the text encoder
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
                                                text_encoder.RnnEncoder(m["V"], m["E"], m["H"], 1, 0.0, True, "GRU"),
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
    print(f"MultiTextBiEncoder(CrnnEncoder, RnnEncoder) B={B} N={N}: grouped vs general frame_sim {e_fs:.2e}, clip_sim {e_cs:.2e}")
    assert e_fs < 5e-6 and e_cs < 5e-6 and grouped["clip_sim"].shape == (B, N)
    # the text side against the fp64 restatement (R = B * N rows in one launch)
    st = R.model_text_state()
    with torch.no_grad():
        te = model.text_encoder({"text": text.view(B * N, L), "text_len": text_len.view(-1)})
    tok, seq = R.encoder_forward({k: v.double() for k, v in st.items()}, text.view(B * N, L), text_len.view(-1), 1, 2)
    assert R.rel_err(te["token_emb"], tok) < BOUND and R.rel_err(te["seq_emb"], seq) < BOUND
