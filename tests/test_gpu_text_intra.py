"""IntraAttention on the MI355X: the row-local attention core and the ConvGRU cell kernels (csrc/text_intra.hip) alone against the
fp64 restatement, the module against the fixture made from the imported reference (tests/golden/text_intra.npz), train mode with
the materialised masks, num_layers 0 / 1 / 3, EmbeddingAgg as the inner module, leading dimensions, empty phrases, the whole-model
case, StrongRunner.train_step (direct gradients, frozen text encoder, the sticky token-id check), MultiTextBiEncoder's two paths
and a token-level head on token_emb.

Bounds (the rule of tests/test_gpu_text_rnn.py, unchanged): 5e-6 relative to the largest entry of the tensor where the recorded
fp32 deviation of the REFERENCE is below 1.25e-6; where the recorded deviation is larger the bound is 4 x that deviation.  Unlike
the self-attention core the 4 x branch also covers attn and message: the scores are unscaled and reach the hundreds, where one
fp32 ulp of a score is already about 1e-5 of an attention weight.  The kernel-alone cases have no recorded reference figure:
their figure is the deviation of the same restatement run in fp32 on the CPU on the same inputs, measured in the test, under the
same rule.  Every measured error is printed.  The core has no vector-read form (4-byte reads, contiguous over the lanes), so
there is no alignment case.

Worst measured error per quantity on the MI355X (docs/experiments_text_intra.md): core message 2.5e-6 at (17, 32, 130) p = 0.2
(cpu fp32 there 5.4e-6), attn 2.2e-6 and dx 3.2e-6 at (1024, 9, 64) p = 0.2 (cpu fp32 2.2e-6 / 3.0e-6); cell kernels 2.2e-7;
module against the reference's fp64: token_emb 1.7e-7, seq_emb 1.6e-7, gradients 6.1e-7 (recorded deviation up to 8.2e-7);
train mode with masks: token_emb 2.6e-7, gradients 5.8e-7; whole-model frame_sim 2.5e-7.  Every case prints its figures under
``-s``."""
import numpy as np
import pytest
import torch

from tests import text_intra_ref as R

pytestmark = pytest.mark.gpu

BOUND, DEV_LIMIT = 5e-6, 1.25e-6


def bound_for(recorded_dev):
    return BOUND if recorded_dev < DEV_LIMIT else 4.0 * recorded_dev


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(f"{golden_dir}/text_intra.npz")


def _fixture_case(fx, name):
    cfg = R.CONFIGS[name]
    st = {k: torch.from_numpy(fx[f"{name}_param_{k}"]) for k in R.param_names(cfg["agg"])}
    st["pe.pe"] = R.position_table(cfg["E"])
    return cfg, st, torch.from_numpy(fx[f"{name}_text"].astype(np.int64)), torch.from_numpy(fx[f"{name}_text_len"].astype(np.int64))


# (R, L, E): L of {1, 2, 9, 32, 33, 64}, E of {2, 6, 64, 130, 512, 1024} (6 and 130 are no multiple of 4, 130 and 6 leave a wave
# partly idle), R of {1, 3, 17, 1024}; (2, 64, 1024) is the LDS corner (32 KB of scores + 16 KB of keep bits in the backward)
CORE_CASES = [(1, 1, 2), (3, 2, 6), (17, 9, 64), (1024, 9, 64), (17, 32, 130), (3, 33, 512), (17, 33, 64), (2, 64, 1024), (3, 64, 6),
              (17, 1, 64), (3, 9, 1024), (1, 64, 130), (1024, 2, 2)]


def _core_lens(Rn, L):
    """Length vectors that together hold 1, L and 0."""
    if Rn >= 3:
        g = torch.Generator().manual_seed(100 * Rn + L)
        lens = torch.randint(0, L + 1, (Rn,), generator=g)
        lens[0], lens[1], lens[-1] = L, 0, 1
        return [lens]
    return [torch.full((Rn,), v) for v in sorted({L, 1, 0})]


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("Rn,L,E", CORE_CASES)
def test_core_alone_vs_fp64(dev, Rn, L, E, p):
    from texttoaudiogrounding_amd import ops
    g = torch.Generator().manual_seed(10000 * Rn + 100 * L + E)
    x = (0.2 if E >= 128 else 1.0) * torch.randn(Rn, L, E, generator=g)
    dmsg = torch.randn(Rn, L, E, generator=g)
    pe = R.position_table(E)[0]
    for lens in _core_lens(Rn, L):
        seeds = (1234 + L, 977 + E)
        xd, gd, ld, ped = x.to(dev), dmsg.to(dev), lens.to(dev), pe.to(dev)
        ma, mb = ((ops.dropout_mask(s, (Rn, L, E), p, dev).cpu() for s in seeds) if p > 0.0 else (None, None))
        ref = R.core_results(x, pe, lens, dmsg, torch.float64, ma, mb, p)
        f32 = R.core_results(x, pe, lens, dmsg, torch.float32, ma, mb, p)
        msg, attn = ops.text_intra_core(xd, ped, ld, True, p, seeds)
        msg2, attn2 = ops.text_intra_core(xd, ped, ld, True, p, seeds)
        assert torch.equal(msg, msg2) and torch.equal(attn, attn2), "two forward runs differ"
        msg3, attn3 = ops.text_intra_core(xd, ped, ld, False, p, seeds)
        assert attn3 is None and torch.equal(msg3, msg), "the forward without attn gives another message"
        dx = ops.text_intra_core_backward(gd, xd, ped, attn, ld, p, seeds)
        dx2 = ops.text_intra_core_backward(gd, xd, ped, attn, ld, p, seeds)
        assert torch.equal(dx, dx2), "two backward runs differ"
        assert dx.shape == x.shape and torch.isfinite(dx).all() and torch.isfinite(msg).all()
        acc = torch.ones_like(dx)
        assert torch.equal(ops.text_intra_core_backward(gd, xd, ped, attn, ld, p, seeds, out=acc), acc) and \
            R.rel_err(acc - 1.0, dx) < 1e-6, "the accumulating form adds something else"
        # the weights: rows sum to 1 over ALL L cells (dead cells carry weight); a padded query row is exactly uniform
        a = attn.cpu()
        assert (a.sum(-1) - 1.0).abs().max().item() < 1e-5
        pad = torch.arange(L)[None, :] >= lens[:, None]
        if pad.any():
            rows = a[pad]
            assert torch.equal(rows, rows[:, :1].expand_as(rows)) and (rows[:, 0] - 1.0 / L).abs().max().item() < 1e-7
        errs = {}
        for k, got in (("message", msg), ("attn", attn), ("dx", dx)):
            d32 = R.rel_err(f32[k], ref[k])
            errs[k] = (R.rel_err(got, ref[k]), bound_for(d32), d32)
        print(f"text_intra core R={Rn} L={L} E={E} p={p} len[{int(lens.min())}..{int(lens.max())}]: "
              + ", ".join(f"{k} {e:.2e} (cpu fp32 {d:.1e})" for k, (e, b, d) in errs.items()))
        for k, (e, b, d) in errs.items():
            assert e < b, (k, e, b)


# (R, L, E): (R*L, E) = (1, 2), (51, 6), (153, 64), (10240, 512)
CELL_CASES = [(1, 1, 2), (17, 3, 6), (17, 9, 64), (1024, 10, 512)]


@pytest.mark.parametrize("Rn,L,E", CELL_CASES)
def test_cell_kernels_alone_vs_fp64(dev, Rn, L, E):
    from texttoaudiogrounding_amd import ops
    g = torch.Generator().manual_seed(7 * Rn + L + E)
    u_pre, r_pre, o_pre, x, dnew, dxr = (torch.randn(Rn, L, E, generator=g) for _ in range(6))
    dseq = torch.randn(Rn, E, generator=g)
    full = torch.randint(1, L + 1, (Rn,), generator=g)
    full[0], full[-1] = L, 1
    vectors = [full] + ([torch.randint(1, L, (Rn,), generator=g)] if L > 1 else [])        # 1 and L; max < L
    M = Rn * L

    def restated(dtype, lens):
        t = lambda v: v.to(dtype)                                                      # noqa: E731
        u, r, xr = R.cell_elementwise(t(u_pre), t(r_pre), t(x))
        o, new = R.cell_update(t(o_pre), u, t(x))
        out = dict(u=u, r=r, xr=xr, o=o, xnew=new, seq=R.masked_mean(new, lens))
        for tag, dn, ds in (("", t(dnew), t(dseq)), ("_tok", t(dnew), None), ("_seq", None, t(dseq))):
            do_pre, du_pre, dx = R.cell_update_backward(dn, ds, lens, t(x), u, o)
            dr_pre, dx = R.cell_gates_backward(t(dxr), t(x), r, dx)
            out.update({"do_pre" + tag: do_pre, "du_pre" + tag: du_pre, "dr_pre" + tag: dr_pre, "dx" + tag: dx})
        return out

    for lens in vectors:
        ref, f32 = restated(torch.float64, lens), restated(torch.float32, lens)
        ld, xd = lens.to(dev), x.to(dev).view(M, E)
        u, r, o = u_pre.to(dev).view(M, E).clone(), r_pre.to(dev).view(M, E).clone(), o_pre.to(dev).view(M, E).clone()
        got = dict(xr=ops.convgru_gates_forward(u, r, xd), u=u, r=r)
        got["xnew"], got["seq"] = ops.convgru_update_forward(o, u, xd, Rn, L, ld)
        got["o"] = o
        o2 = o_pre.to(dev).view(M, E).clone()
        new2, none = ops.convgru_update_forward(o2, u, xd, Rn, L)
        assert none is None and torch.equal(new2, got["xnew"]) and torch.equal(o2, o), "the form without the mean differs"
        for tag, dn, ds in (("", dnew.to(dev), dseq.to(dev)), ("_tok", dnew.to(dev), None), ("_seq", None, dseq.to(dev))):
            do_pre, du_pre, dx = ops.convgru_update_backward(dn, ds, ld, xd, u, o, Rn, L)
            dr_pre = ops.convgru_gates_backward(dxr.to(dev).view(M, E), xd, r, dx)
            got.update({"do_pre" + tag: do_pre, "du_pre" + tag: du_pre, "dr_pre" + tag: dr_pre, "dx" + tag: dx})
        errs = {}
        for k in ref:
            d32 = R.rel_err(f32[k], ref[k])
            errs[k] = (R.rel_err(got[k].reshape(ref[k].shape), ref[k]), bound_for(d32), d32)
        worst = max(errs.items(), key=lambda kv: kv[1][0])
        print(f"convgru cell R={Rn} L={L} E={E} len[{int(lens.min())}..{int(lens.max())}]: worst {worst[0]} {worst[1][0]:.2e} "
              f"(cpu fp32 {worst[1][2]:.1e}); seq {errs['seq'][0]:.2e}, xnew {errs['xnew'][0]:.2e}")
        for k, (e, b, d) in errs.items():
            assert e < b, (k, e, b)


def _encoder(cfg, st, dev, layers=None):
    from texttoaudiogrounding_amd.models.text_encoder import EmbeddingAgg, EmbeddingLayer, IntraAttention
    enc = IntraAttention((EmbeddingAgg if cfg["agg"] else EmbeddingLayer)(cfg["V"], cfg["E"]), cfg["layers"] if layers is None else layers)
    enc.load_state_dict(st, strict=True)
    return enc.to(dev)


def _module_results(enc, cfg, text, text_len, dev, skip_seq_row0=False):
    enc.zero_grad(set_to_none=True)
    o = enc({"text": text, "text_len": text_len})
    wt, ws = R.objective_weights(cfg, torch.float32)
    seq = o["seq_emb"][1:] if skip_seq_row0 else o["seq_emb"]
    R.objective(o["token_emb"], seq, wt.to(dev), (ws[1:] if skip_seq_row0 else ws).to(dev)).backward()
    got = {"token_emb": o["token_emb"].detach(), "seq_emb": o["seq_emb"].detach()}
    got.update({"d" + k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in enc.named_parameters()})
    return got


def _check(tag, got, ref, recorded):
    errs = {k: (R.rel_err(got[k], ref[k]), bound_for(recorded[k])) for k in recorded}
    print(f"{tag}: " + ", ".join(f"{k} {e:.2e}" for k, (e, _) in errs.items()))
    for k, (e, b) in errs.items():
        assert e < b, (k, e, b, recorded[k])


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_module_eval_vs_reference_fixture(dev, fx, name):
    cfg, st, text, text_len = _fixture_case(fx, name)
    enc = _encoder(cfg, st, dev).eval()
    got = _module_results(enc, cfg, text, text_len, dev)
    assert got["token_emb"].shape == (cfg["R"], cfg["L"], cfg["E"]) and got["seq_emb"].shape == (cfg["R"], cfg["E"])
    assert got["token_emb"][0, -1].abs().max() > 0, "token_emb at a padded position is not zero in the reference"
    assert got["d" + R.table_name(cfg["agg"])][0].abs().max() > 0, "row 0 of the table (the pad id) receives gradient"
    recorded = dict(zip(fx[f"{name}_quantities"].tolist(), fx[f"{name}_f32_dev"].tolist()))
    _check(f"IntraAttention {name} (eval) vs the reference's fp64", got, {k: fx[f"{name}_f64_{k}"] for k in recorded}, recorded)
    again = _module_results(enc, cfg, text, text_len, dev)
    assert all(torch.equal(again[k], got[k]) for k in got), "two runs differ"
    # leading dimensions (the reference raises on a 3-D text); lengths as a list / numpy array / tensor
    L, E = cfg["L"], cfg["E"]
    with torch.no_grad():
        o2 = enc({"text": text[:6].view(2, 3, L).numpy(), "text_len": text_len[:6].view(2, 3).numpy()})
        o3 = enc({"text": text[:6], "text_len": text_len[:6].tolist()})
        o4 = enc({"text": text[:6].to(dev), "text_len": text_len[:6].to(dev)})
    assert o2["token_emb"].shape == (2, 3, L, E) and o2["seq_emb"].shape == (2, 3, E)
    assert torch.equal(o2["token_emb"].view(6, L, -1), o3["token_emb"]) and torch.equal(o2["seq_emb"].view(6, -1), o3["seq_emb"])
    assert torch.equal(o4["token_emb"], o3["token_emb"]) and torch.equal(o4["seq_emb"], o3["seq_emb"])
    assert torch.equal(o3["token_emb"], got["token_emb"][:6]) and torch.equal(o3["seq_emb"], got["seq_emb"][:6]), \
        "rows of a batch never interact"


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_module_train_with_materialised_masks(dev, fx, name):
    from texttoaudiogrounding_amd import ops
    cfg, st, text, text_len = _fixture_case(fx, name)
    p, shape = 0.2, (cfg["R"], cfg["L"], cfg["E"])
    enc = _encoder(cfg, st, dev).train()
    assert enc.pe.p == p
    torch.manual_seed(77)
    seed = ops.new_seed()                                 # what the module draws first after this manual_seed
    torch.manual_seed(77)
    got = _module_results(enc, cfg, text, text_len, dev)
    masks = [tuple(ops.dropout_mask(s, shape, p, dev).cpu() for s in pair) for pair in ops.text_intra_dropout_seeds(seed, cfg["layers"])]
    kept = [float(m.float().mean()) for pair in masks for m in pair]
    assert all(abs(k - (1 - p)) < 0.05 for k in kept), kept
    assert not torch.equal(masks[0][0], masks[0][1]), "the two dropouts of a layer share one mask"
    ref = R.config_results(cfg, st, text, text_len, torch.float64, masks, p)
    f32 = R.config_results(cfg, st, text, text_len, torch.float32, masks, p)
    _check(f"IntraAttention {name} (train, p = {p}) vs the restatement", got, ref, {k: R.rel_err(f32[k], ref[k]) for k in ref})
    torch.manual_seed(77)
    again = _module_results(enc, cfg, text, text_len, dev)
    assert all(torch.equal(again[k], got[k]) for k in got), "the same seed must give the same step"
    torch.manual_seed(78)
    other = _module_results(enc, cfg, text, text_len, dev)
    assert not torch.equal(other["token_emb"], got["token_emb"]), "two seeds gave the same masks"


@pytest.mark.parametrize("name,layers", [("e64_n2", 0), ("e16_agg", 0), ("e64_n2", 1), ("e32_n1", 3), ("e16_agg", 3)])
def test_other_layer_counts_vs_restatement(dev, fx, name, layers):
    cfg, st, text, text_len = _fixture_case(fx, name)
    got = _module_results(_encoder(cfg, st, dev, layers).eval(), cfg, text, text_len, dev)
    ref = R.config_results(cfg, st, text, text_len, torch.float64, layers=layers)
    f32 = R.config_results(cfg, st, text, text_len, torch.float32, layers=layers)
    _check(f"IntraAttention {name} num_layers = {layers}", got, ref, {k: R.rel_err(f32[k], ref[k]) for k in ref})
    if layers == 0:
        assert all(float(got["d" + k].abs().max()) == 0.0 for k in R.GATE_NAMES)


@pytest.mark.parametrize("name", ["e64_n2", "e16_agg"])
def test_empty_phrases(dev, fx, name):
    """text_len = 0: token_emb is finite and matches the restatement, seq_emb of that row is 0/0 like EmbeddingAgg's, the other
    rows and every gradient of an objective without that seq_emb row are unaffected."""
    cfg, st, _, _ = _fixture_case(fx, name)
    text, text_len = R.draw_inputs(cfg, zero=True)
    got = _module_results(_encoder(cfg, st, dev).eval(), cfg, text, text_len, dev, skip_seq_row0=True)
    assert torch.isfinite(got["token_emb"]).all() and torch.isnan(got["seq_emb"][0]).all() and torch.isfinite(got["seq_emb"][1:]).all()

    def restated(dtype):
        names = R.param_names(cfg["agg"])
        s = {k: v.to(dtype).clone().requires_grad_(k in names) for k, v in st.items()}
        tok, seq = R.encoder_forward(s, text, text_len, cfg["layers"], agg=cfg["agg"])
        wt, ws = R.objective_weights(cfg, dtype)
        R.objective(tok, R.masked_mean(tok, text_len.clamp(min=1))[1:], wt, ws[1:]).backward()
        out = {"token_emb": tok.detach(), "seq_emb": seq.detach()[1:]}
        out.update({"d" + k: s[k].grad for k in names})
        return out

    ref, f32 = restated(torch.float64), restated(torch.float32)
    got["seq_emb"] = got["seq_emb"][1:]
    assert all(torch.isfinite(v).all() for v in got.values())
    _check(f"IntraAttention {name} with an empty phrase", got, ref, {k: R.rel_err(f32[k], ref[k]) for k in ref})


def _biencoder(text_enc, freeze_text=False):
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match
    return audio_text_model.BiEncoder(audio_encoder.CrnnEncoder(32000, 256), text_enc, match.DotProduct(), 256,
                                      freeze_text_encoder=freeze_text)


def _text_encoder():
    from texttoaudiogrounding_amd.models import text_encoder
    m = R.MODEL
    return text_encoder.IntraAttention(text_encoder.EmbeddingLayer(m["V"], m["E"]), m["layers"])


def test_whole_model_eval_vs_reference_fixture(dev, fx):
    st, batch = R.model_state(), R.model_batch()
    assert np.allclose(R.state_checksum(st), fx["model_state_checksum"], rtol=1e-12, atol=0)
    assert np.allclose(R.checksum(batch["waveform"]), fx["model_waveform_checksum"], rtol=1e-12, atol=0)
    assert np.array_equal(batch["text"].numpy(), fx["model_text"]) and np.array_equal(batch["text_len"], fx["model_text_len"])
    model = _biencoder(_text_encoder())
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
    print(f"BiEncoder(CrnnEncoder, IntraAttention, DotProduct) eval: frame_sim err {e:.2e} (the reference's own fp32: "
          f"{float(fx['model_frame_sim_f32_dev']):.2e} relative)")
    assert e < 1e-4


def _strong_model(freeze_text=False):
    model = _biencoder(_text_encoder(), freeze_text)
    model.load_state_dict(R.model_state(), strict=False)
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
    assert "text_encoder.conv_gru.reset_gate.weight" in names and "text_encoder.embedding.core.weight" in names
    torch.manual_seed(5)                                  # the text encoder's dropout (p = 0.2) draws its seed here
    loss = runner.forward_backward(_clone_batch(batch))
    lv = runner.loss_value(loss)
    direct = {n: p.grad.detach().clone() for n, p in runner.model.named_parameters()}
    assert all(direct[n].abs().max() > 0 for n in names if n.startswith("text_encoder.")), "a text gradient is all zero"
    # the same step through plain autograd (the operators' registered formulas, AccumulateGrad into the same flat views)
    assert not ops.DIRECT_GRADS
    runner.flat.zero_grad()
    torch.manual_seed(5)
    out = runner.forward(_clone_batch(batch), training=True)
    loss2 = runner.loss_fn(out)
    loss2.backward()
    assert abs(float(loss2.item()) - lv) < 1e-6
    worst = 0.0
    for n, p in runner.model.named_parameters():
        e = R.rel_err(direct[n], p.grad)
        worst = max(worst, e)
        assert e < 1e-6, (n, e)
    print(f"StrongRunner BiEncoder(CrnnEncoder, IntraAttention): loss {lv:.6f}; direct vs plain-autograd gradients, worst {worst:.2e}")
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
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match
    m = R.MODEL
    B, N, L = 4, 5, 6
    g = torch.Generator().manual_seed(91)
    wave = 0.1 * torch.randn(B, 48000, generator=g)
    text = torch.randint(2, m["V"], (B, N, L), generator=g)
    text_len = torch.randint(1, L + 1, (B, N), generator=g)
    for b in range(B):
        for n in range(N):
            text[b, n, text_len[b, n]:] = 0
    model = audio_text_model.MultiTextBiEncoder(audio_encoder.CrnnEncoder(32000, 256), _text_encoder(), match.DotProduct(), 256,
                                                text_forward_keys=["text"])
    model.load_state_dict(R.model_state(), strict=False)
    model = model.to(dev).eval()
    inp = {"waveform": wave.to(dev), "waveform_len": np.full(B, 48000), "text": text, "text_len": text_len, "specaug": False}
    with torch.no_grad():
        grouped = model(dict(inp))
        general = model._forward_general(dict(inp))
    assert grouped["frame_sim"].shape == general["frame_sim"].shape == (B, 19, N)
    e_fs = (grouped["frame_sim"] - general["frame_sim"]).abs().max().item()
    e_cs = (grouped["clip_sim"] - general["clip_sim"]).abs().max().item()
    print(f"MultiTextBiEncoder(CrnnEncoder, IntraAttention) B={B} N={N}: grouped vs general frame_sim {e_fs:.2e}, clip_sim {e_cs:.2e}")
    assert e_fs < 5e-6 and e_cs < 5e-6 and grouped["clip_sim"].shape == (B, N)
    # the text side against the fp64 restatement (R = B * N rows in one launch)
    st = R.model_text_state()
    with torch.no_grad():
        te = model.text_encoder({"text": text.view(B * N, L), "text_len": text_len.view(-1)})
    tok, seq = R.encoder_forward({k: v.double() for k, v in st.items()}, text.view(B * N, L), text_len.view(-1), m["layers"])
    assert R.rel_err(te["token_emb"], tok) < BOUND and R.rel_err(te["seq_emb"], seq) < BOUND


def _float_outputs(out):
    return [v for v in out.values() if torch.is_tensor(v) and v.is_floating_point()]


def test_as_text_encoder_of_align_by_phrase_and_cross_cnn8rnn(dev):
    """IntraAttention where the weak phrase-level model and the early-fusion model take their text encoder: the forward is
    finite and the backward reaches the shared cell and the table."""
    from texttoaudiogrounding_amd.models import align, audio_encoder, audio_text_model, sim_pooling, text_encoder
    g = torch.Generator().manual_seed(12)
    B, S = 3, 48000
    wave = (0.1 * torch.randn(B, S, generator=g)).to(dev)
    nums, L = [2, 1, 3], 4
    phrases = torch.randint(2, 300, (sum(nums), L), generator=g)
    phrases_len = torch.randint(1, L + 1, (sum(nums),), generator=g)
    for r in range(sum(nums)):
        phrases[r, phrases_len[r]:] = 0

    def encoder(E):
        torch.manual_seed(3)
        return text_encoder.IntraAttention(text_encoder.EmbeddingLayer(300, E), 2)

    m1 = audio_text_model.AudioTextAlignByPhrase(audio_encoder.Cnn8Rnn(32000), encoder(512), align.DotProduct(),
                                                 sim_pooling.AudioMeanTextMean(), 512).to(dev).eval()
    o1 = m1({"waveform": wave, "waveform_len": [S] * B, "phrases": phrases, "phrases_len": phrases_len, "phrases_num": list(nums),
             "text_key": "phrases", "specaug": False})
    m2 = audio_text_model.CrossCnn8_Rnn(32000, encoder(256)).to(dev).eval()
    o2 = m2({"waveform": wave, "waveform_len": [S] * B, "text": phrases[:B].to(dev), "text_len": phrases_len[:B].to(dev),
             "specaug": False})
    for tag, model, out in (("AudioTextAlignByPhrase", m1, o1), ("CrossCnn8_Rnn", m2, o2)):
        outs = _float_outputs(out)
        assert outs and all(torch.isfinite(v).all() for v in outs), tag
        sum(v.sum() for v in outs if v.requires_grad).backward()
        te = model.text_encoder
        grads = {k: p.grad for k, p in te.named_parameters()}
        assert all(v is not None and torch.isfinite(v).all() for v in grads.values()), tag
        assert float(grads["conv_gru.out_gate.weight"].abs().max()) > 0 and float(grads["embedding.core.weight"].abs().max()) > 0, tag
        print(f"{tag}(IntraAttention): outputs {[tuple(v.shape) for v in outs]}, |d out_gate.weight| max "
              f"{float(grads['conv_gru.out_gate.weight'].abs().max()):.2e}")


def test_token_level_head_on_token_emb(dev, fx):
    """match.CrossAttention over IntraAttention's token_emb: the head's gradient reaches the shared cell (and the table) and equals
    the restatement's gradient for the same d token_emb."""
    from texttoaudiogrounding_amd.models import match
    name = "e64_n2"
    cfg, st, text, text_len = _fixture_case(fx, name)
    enc = _encoder(cfg, st, dev).eval()                   # eval: no dropout behind the positions; gradients flow all the same
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
    names = R.param_names()
    s = {k: v.double().clone().requires_grad_(k in names) for k, v in st.items()}
    tok64, _ = R.encoder_forward(s, text, text_len, cfg["layers"])
    (tok64 * dtok).sum().backward()
    assert R.rel_err(tok, tok64) < BOUND
    errs = {k: R.rel_err(dict(enc.named_parameters())[k].grad, s[k].grad) for k in names}
    print("CrossAttention head on IntraAttention token_emb: " + ", ".join(f"d{k} {e:.2e}" for k, e in errs.items()))
    assert enc.conv_gru.out_gate.weight.grad.abs().max() > 0
    for k, e in errs.items():
        assert e < BOUND, (k, e)
