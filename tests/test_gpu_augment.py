"""SpecAugment + mixup in the Cnn8Rnn training forward (csrc/augment.hip, ops.Cnn8RnnFunction, tag::cnn8rnn_encoder,
models/augmentation.py): the kernels against a float64 restatement, the identity of zero-width stripes, parity with the reference
fixtures (tests/golden/make_golden_specaug.py), the operator, the batch guard of the pairing heads and the benched size."""
import gc

import numpy as np
import pytest
import torch

from oracle import tag_oracle as O
from tests.test_gpu_path import assert_grad_close, sample_grad

pytestmark = pytest.mark.gpu

FIXTURES = ("cnn8rnn_specaug_train", "cnn8rnn_specaug_mixup_train")


# ---------------------------------------------------------------------------------------------------------------- kernels
def edge_stripes(B, F, NM, nt, nf, seed):
    """Per clip: stripes at both edges, overlapping, full width and zero width, mixed at random."""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, nt + nf, 2), np.int32)
    for b in range(B):
        for k in range(nt + nf):
            W = F if k < nt else NM
            kind = rng.integers(0, 6)
            w = int(rng.integers(0, W + 1))
            if kind == 0:
                out[b, k] = (0, w)                       # at the start
            elif kind == 1:
                out[b, k] = (W - w, w)                   # at the end
            elif kind == 2:
                out[b, k] = (0, W)                       # full width
            elif kind == 3:
                out[b, k] = (int(rng.integers(0, W + 1)), 0)   # zero width (also at bgn = W)
            else:
                bgn = int(rng.integers(0, W + 1))
                out[b, k] = (bgn, int(rng.integers(0, W - bgn + 1)))
        if nt > 1 and b % 3 == 0:
            out[b, 1] = (out[b, 0, 0], out[b, 0, 1] + (1 if out[b, 0].sum() < F else 0))   # overlapping its neighbour
    return out


def ref_mask(stripes, nt, B, F, NM):
    m = np.zeros((B, F, NM), bool)
    f, c = np.arange(F), np.arange(NM)
    for b in range(B):
        for k in range(stripes.shape[1]):
            bgn, w = stripes[b, k]
            if k < nt:
                m[b] |= ((f >= bgn) & (f < bgn + w))[:, None]
            else:
                m[b] |= ((c >= bgn) & (c < bgn + w))[None, :]
    return m


def ref_forward(lm, scale, shift, mask, lam):
    """float64 restatement, rounded where the kernel rounds: fmaf (one rounding) -> zeros -> fp32 products -> fp32 sum."""
    x = lm.astype(np.float64)
    if scale is not None:
        x = (x * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32).astype(np.float64)
    x = np.where(mask, 0.0, x)
    if lam is None:
        return x.astype(np.float32), mask
    l = lam.astype(np.float64)[:, None, None]
    p = (x * l).astype(np.float32).astype(np.float64)
    return (p[0::2] + p[1::2]).astype(np.float32), mask[0::2] & mask[1::2]


def assert_ulp(got, want, what):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    bad = err > ulp
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()))


@pytest.mark.parametrize("B,F", [(2, 1), (2, 151), (4, 151), (4, 1001), (64, 151), (64, 1001), (64, 1)])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("mixup", [False, True])
def test_kernels_against_float64_restatement(dev, B, F, affine, mixup):
    from texttoaudiogrounding_amd import ops
    NM, nt, nf = 64, 2, 2
    g = np.random.default_rng(B * 1000 + F)
    lm = (g.standard_normal((B, F, NM)) * 20 - 40).astype(np.float32)
    scale = (0.5 + g.random(NM)).astype(np.float32) if affine else None
    shift = g.standard_normal(NM).astype(np.float32) if affine else None
    stripes = edge_stripes(B, F, NM, nt, nf, seed=B + F)
    lam = g.random(B).astype(np.float32) * 2 - 0.5 if mixup else None
    mask = ref_mask(stripes, nt, B, F, NM)
    want, wmask = ref_forward(lm, scale, shift, mask, lam)
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    x0 = ops.augment_forward(t(lm), t(scale), t(shift), t(stripes), nt, t(lam)).cpu().numpy()
    assert x0.shape == want.shape
    assert (x0[wmask] == 0).all(), "masked elements must be exactly 0"
    assert_ulp(x0, want, "forward")
    # gradient: mask[b] * lam[b] * dx0[b/2]  (the VJP of the restatement; one fp32 product)
    dx0 = g.standard_normal(want.shape).astype(np.float32)
    rep = np.repeat(dx0, 2, axis=0) if mixup else dx0
    wgrad = (rep.astype(np.float64) * lam.astype(np.float64)[:, None, None]).astype(np.float32) if mixup else rep
    wgrad = np.where(mask, np.float32(0), wgrad)
    dbn0 = ops.augment_backward(t(dx0), B, t(stripes), nt, t(lam)).cpu().numpy()
    assert (dbn0[mask] == 0).all()
    assert np.array_equal(dbn0, wgrad)
    torch.cuda.synchronize()


def test_lambda_one_zero_reproduces_even_clip_bitwise(dev):
    from texttoaudiogrounding_amd import ops
    B, F, NM = 8, 151, 64
    g = torch.Generator().manual_seed(3)
    lm = (torch.randn(B, F, NM, generator=g) * 10).to(dev)
    scale, shift = (torch.rand(NM, generator=g) + 0.5).to(dev), torch.randn(NM, generator=g).to(dev)
    stripes = torch.from_numpy(edge_stripes(B, F, NM, 2, 2, seed=9)).to(dev)
    lam = torch.tensor([1.0, 0.0] * (B // 2), device=dev)
    plain = ops.augment_forward(lm, scale, shift, stripes, 2)
    mixed = ops.augment_forward(lm, scale, shift, stripes, 2, lam)
    assert torch.equal(mixed.view(torch.int32), plain[0::2].contiguous().view(torch.int32))


def test_kernel_argument_checks(dev):
    from texttoaudiogrounding_amd import ops
    lm = torch.zeros(3, 10, 64, device=dev)
    with pytest.raises(RuntimeError):
        ops.augment_forward(lm, lam=torch.ones(3, device=dev))                       # odd B with lambda
    with pytest.raises(RuntimeError):
        ops.augment_forward(torch.zeros(2, 10, 62, device=dev))                       # NM % 4 != 0
    with pytest.raises(RuntimeError):
        ops.augment_forward(lm, stripes=torch.zeros(3, 9, 2, dtype=torch.int32, device=dev), n_time=0)   # 9 > 8 stripes
    with pytest.raises(RuntimeError):
        ops.augment_forward(lm, stripes=torch.zeros(3, 2, 2, dtype=torch.int32), n_time=1)               # host table


def test_specaugmentation_module_forward_and_grad(dev):
    """models.augmentation.SpecAugmentation on a (B, C, T, F) tensor: the twin's zeros, the twin's gradient."""
    from tests import torchlibrosa_twin
    from texttoaudiogrounding_amd.models.augmentation import SpecAugmentation
    x = torch.randn(3, 2, 101, 64, generator=torch.Generator().manual_seed(1))
    twin = torchlibrosa_twin.SpecAugmentation(64, 2, 8, 2).train()
    xt = x.clone().requires_grad_(True)
    torch.manual_seed(5)
    yt = twin(xt.clone())
    yt.backward(torch.ones_like(yt))
    sa = SpecAugmentation(64, 2, 8, 2).train()
    xd = x.to(dev).requires_grad_(True)
    torch.manual_seed(5)
    y = sa(xd)
    y.backward(torch.ones_like(y))
    assert torch.equal(y.detach().cpu(), yt.detach())
    assert torch.equal(xd.grad.cpu(), xt.grad)
    assert sa.eval()(xd) is xd


# ---------------------------------------------------------------------------------------------------------------- encoder
def encoder_state():
    st = O.init_state(seed=7, text_dim=512, shared_dim=512, logit_gain=120.0)
    return {k[len("audio_encoder."):]: v for k, v in st.items() if k.startswith("audio_encoder.")}


def build_encoder(dev):
    from texttoaudiogrounding_amd.models.audio_encoder import Cnn8Rnn
    m = Cnn8Rnn(32000)
    missing = m.load_state_dict(encoder_state(), strict=False)
    assert not missing.unexpected_keys and all("melspec_extractor" in k for k in missing.missing_keys)
    m.dropout_p = (0.0, 0.0)
    return m.to(dev).train()


def fixture_inputs(gold, dev):
    lens = gold["lens"]
    B, S = lens.shape[0], 48000
    wave = O.synthetic_batch(B, S, seed=1234, ragged=False, hop=320)["waveform"].clone()
    for i in range(B):
        wave[i, lens[i]:] = 0.0
    return wave.to(dev), lens


def encoder_step(m, wave, lens, specaug, lam=None, seed=None, R_seed=31):
    d = {"waveform": wave, "waveform_len": lens, "specaug": specaug}
    if lam is not None:
        d["mixup_lambda"] = lam
    if seed is not None:
        torch.manual_seed(seed)
    out = m(d)
    emb = out["embedding"]
    R = torch.randn(emb.shape, generator=torch.Generator().manual_seed(R_seed), dtype=torch.float64).float().to(emb.device)
    loss = (emb * R).sum()
    loss.backward()
    return out, loss


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("wino", [True, False])
def test_parity_with_reference_fixture(dev, golden_dir, monkeypatch, name, wino):
    from texttoaudiogrounding_amd import ops
    monkeypatch.setattr(ops, "CONV_WINOGRAD", wino)
    gold = np.load(f"{golden_dir}/{name}.npz")
    wave, lens = fixture_inputs(gold, dev)
    lam = gold["mixup_lambda"] if "mixup_lambda" in gold.files else None
    m = build_encoder(dev)
    out, loss = encoder_step(m, wave, lens, True, lam, seed=int(gold["seed"]))
    assert np.array_equal(m._last_specaug.numpy(), gold["stripes"])
    emb = out["embedding"].detach().cpu().numpy().astype(np.float64)
    err = np.abs(emb - gold["embedding_f64_as_f32"]).max()
    print(f"{name} winograd={wino}: embedding err {err:.2e} (reference f32 {float(gold['embedding_f32_err']):.2e}), "
          f"loss {loss.item():.6f} vs {float(gold['loss_f64']):.6f}")
    assert emb.shape == gold["embedding_f64_as_f32"].shape and err < 1e-4
    assert str(out["length"].dtype) == str(gold["length_dtype"])
    assert np.array_equal(out["length"].cpu().numpy(), gold["length"])
    for pname, p in m.named_parameters():
        want, ref32 = gold[f"grad_f64/{pname}"], gold[f"grad_f32/{pname}"]
        got = sample_grad(p.grad)
        scale = want[1] + 1e-30
        e = np.abs(got[2:] - want[2:]).max() / scale
        e32 = np.abs(ref32[2:] - want[2:]).max() / scale
        print(f"  {pname:40s} hip {e:.2e}  reference-f32 {e32:.2e}")
        assert_grad_close(pname, e, e32)
    sd = m.state_dict()
    for k in gold.files:
        if k.startswith("after/"):
            assert np.allclose(sd[k[len("after/"):]].cpu().numpy(), gold[k], rtol=2e-4, atol=1e-5), k


@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_mode_step_with_augmentation(dev, golden_dir, monkeypatch, name):
    """TAG_ACT_DTYPE=bf16 TAG_CONV_MATH=bf16: the augmented step runs and its gradient norms stay within the bf16 budget of
    test_gpu_path.py::test_bf16_mode_train_step_budget (per tensor |norm error| <= the budget's bias + 2 x noise bound: 11 % for
    conv blocks / bn0, 5 % for the rest).  The budget's cosine bounds were set on 1024 sampled entries of a B = 64, 10 s step;
    here the step has 4 (2 after mixup) clips of 1.5 s and the fixture keeps 16 entries per tensor, whose cosine is one noisy
    sample (measured on the MI355X: 0.916 for bn0.bias under mixup, 0.9974 for fc1.bias), so direction is checked loosely:
    >= 0.9 for conv blocks / bn0, >= 0.99 for the rest."""
    from texttoaudiogrounding_amd import ops
    monkeypatch.setattr(ops, "CONV_MATH", "bf16")
    monkeypatch.setattr(ops, "ACT_DTYPE", "bf16")
    gold = np.load(f"{golden_dir}/{name}.npz")
    wave, lens = fixture_inputs(gold, dev)
    lam = gold["mixup_lambda"] if "mixup_lambda" in gold.files else None
    m = build_encoder(dev)
    out, loss = encoder_step(m, wave, lens, True, lam, seed=int(gold["seed"]))
    emb = out["embedding"].detach().cpu().numpy().astype(np.float64)
    ref = gold["embedding_f64_as_f32"].astype(np.float64)
    eerr = np.abs(emb - ref).max()
    print(f"{name} bf16: embedding err {eerr:.2e}, loss {loss.item():.4f} vs {float(gold['loss_f64']):.4f}")
    assert np.isfinite(emb).all() and 1e-6 < eerr < 6e-2
    bad = []
    for pname, p in m.named_parameters():
        want = gold[f"grad_f64/{pname}"]
        got = sample_grad(p.grad)
        deep = "conv_block" in pname or "bn0" in pname
        nerr = abs(got[0] - want[0]) / (want[0] + 1e-300)
        cos = float(np.dot(got[2:], want[2:]) / (np.linalg.norm(got[2:]) * np.linalg.norm(want[2:]) + 1e-300))
        print(f"  {pname:40s} norm err {nerr:.2e} cosine {cos:.6f}")
        if nerr > (0.06 + 2 * 0.025 if deep else 0.03 + 2 * 0.01) or cos < (0.9 if deep else 0.99):
            bad.append((pname, nerr, cos))
    assert not bad, bad


def test_zero_width_stripes_are_the_identity(dev):
    """Zero-width stripes and no lambda, through the operator: embedding, every parameter gradient and every running statistic
    bitwise equal to specaug=False on the same inputs (dropout off) -- x0 is the value the Cin = 1 convolution forms itself."""
    from texttoaudiogrounding_amd.models.augmentation import DropStripes
    wave = (0.1 * torch.randn(4, 48000, generator=torch.Generator().manual_seed(2))).to(dev)
    lens = np.array([48000, 41000, 30000, 48000])
    res = []
    for specaug in (False, True):
        m = build_encoder(dev)
        m.spec_augmenter.time_dropper = DropStripes(2, 1, 2)          # drop_width 1: every width is 0
        m.spec_augmenter.freq_dropper = DropStripes(3, 1, 2)
        out, _ = encoder_step(m, wave, lens, specaug)
        if specaug:
            assert m._last_specaug is not None and (m._last_specaug[..., 1] == 0).all()
        res.append((out["embedding"].detach(), {n: p.grad.clone() for n, p in m.named_parameters()},
                    {n: b.clone() for n, b in m.named_buffers()}))
    (e0, g0, b0), (e1, g1, b1) = res
    assert torch.equal(e0, e1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    for n in b0:
        assert torch.equal(b0[n], b1[n]), n


def test_eval_mode_ignores_both_keys(dev):
    wave = (0.1 * torch.randn(4, 32000, generator=torch.Generator().manual_seed(4))).to(dev)
    m = build_encoder(dev).eval()
    with torch.no_grad():
        a = m({"waveform": wave, "waveform_len": [32000] * 4, "specaug": False})
        b = m({"waveform": wave, "waveform_len": [32000] * 4, "specaug": True, "mixup_lambda": [0.3, 0.7, 0.1, 0.9]})
    assert torch.equal(a["embedding"], b["embedding"]) and torch.equal(a["length"], b["length"])


def test_operator_opcheck_with_augmentation(dev):
    import texttoaudiogrounding_amd.torch_ops as T
    m = build_encoder(dev)
    B = 4
    wave = (0.1 * torch.randn(B, 48000, generator=torch.Generator().manual_seed(5))).to(dev)   # 151 frames > time_drop_width
    frames = 48000 // m.hop_length + 1
    torch.manual_seed(0)
    stripes = m.spec_augmenter.draw(B, frames, 64).to(dev)
    lam = torch.tensor([0.3, 0.7, 0.6, 0.4], device=dev)
    op = torch.ops.tag.cnn8rnn_encoder
    tok = T.encoder_token(m)
    params = list(m._flat_params())
    for extra, rows in (((stripes, None), B), ((None, lam), B // 2), ((stripes, lam), B // 2)):
        torch.library.opcheck(op, (wave, params, tok, False, *extra), test_utils=("test_schema", "test_faketensor"))
        torch.library.opcheck(op, (wave, params, tok, True, *extra), test_utils=("test_autograd_registration",))
        assert op(wave, params, tok, False, *extra).shape == (rows, frames // 4, 512)
    # the old positional call: unchanged
    assert op(wave, params, tok, False).shape == (B, frames // 4, 512)


# ---------------------------------------------------------------------------------------------------------------- guard
def test_pairing_heads_refuse_mismatched_batches(dev):
    from texttoaudiogrounding_amd.models import audio_text_model, match as match_mod, text_encoder
    a4, t2 = torch.randn(4, 9, 64, device=dev), torch.randn(2, 64, device=dev)
    a2, t4 = torch.randn(2, 9, 64, device=dev), torch.randn(4, 64, device=dev)
    for a, t in ((a4, t2), (a2, t4)):
        for kind in (0, 1):
            with pytest.raises(RuntimeError, match="batch"):
                torch.ops.tag.frame_match(a, t, kind, False, True)
        with pytest.raises(RuntimeError, match="batch"):
            torch.ops.tag.align_dot(a, t.view(t.shape[0], 1, 64).contiguous(), False, False)
    # BiEncoder: mixup halves the audio batch, the text batch stays -> the match head refuses (the reference's broadcast fails)
    st = O.init_state(seed=7, text_dim=512, shared_dim=512, logit_gain=120.0)
    model = audio_text_model.BiEncoder(build_encoder("cpu"), text_encoder.EmbeddingAgg(5221, 512), match_mod.DotProduct(), 512)
    model.load_state_dict(st, strict=False)
    model = model.to(dev).train()
    model.audio_encoder.dropout_p = (0.0, 0.0)
    b = O.synthetic_batch(4, 32000, seed=1)
    d = {"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"], "text": b["text"].to(dev),
         "text_len": torch.as_tensor(b["text_len"]).to(dev), "specaug": True, "mixup_lambda": [0.2, 0.8, 0.5, 0.5]}
    with pytest.raises(RuntimeError, match="batch"):
        model(d)


# ---------------------------------------------------------------------------------------------------------------- benched size
@pytest.mark.parametrize("mixup", [False, True])
def test_benched_size_steps(dev, mixup):
    """B = 64 x 10 s training steps of the encoder with SpecAugment (and mixup): finite, (32, 250, 512) under mixup, and no
    allocator growth over 5 steps."""
    m = build_encoder(dev)
    m.dropout_p = (0.2, 0.5)
    b = O.synthetic_batch(64, 320000, seed=99, ragged=True)
    wave = b["waveform"].to(dev)
    lam = np.tile([0.3, 0.7], 32) if mixup else None
    # Earlier tests leave device tensors in reference cycles (the BiEncoder that test_pairing_heads_refuse_mismatched_batches makes
    # refuse stays alive through the traceback of its exception): the cyclic collector frees them whenever its counters say so, which
    # may be in the middle of the steps measured here.  Collect them first, so that the figures below are the steps' own.
    held = torch.cuda.memory_allocated()
    gc.collect()
    print(f"device memory held by garbage of earlier tests: {(held - torch.cuda.memory_allocated()) >> 20} MiB")
    mem = []
    for step in range(5):
        m.zero_grad(set_to_none=False)
        out, loss = encoder_step(m, wave, b["waveform_len"], True, lam)
        emb = out["embedding"]
        assert emb.shape == ((32 if mixup else 64), 250, 512)
        assert torch.isfinite(emb).all() and torch.isfinite(loss)
        assert all(torch.isfinite(p.grad).all() for p in m.parameters())
        del out, loss, emb
        torch.cuda.synchronize()
        mem.append((torch.cuda.memory_allocated(), torch.cuda.memory_reserved()))
    print(f"mixup={mixup}: allocated / reserved per step {[(a >> 20, r >> 20) for a, r in mem]} MiB")
    assert mem[1] == mem[4], mem
