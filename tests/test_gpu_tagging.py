"""The class-mapping baseline AudioTagging on the MI355X: the head, its class-innermost passes (csrc/tagging.hip), the
masked frame BCE, the whole model over both encoders, segments through the class helper, ClassMappingRunner and the two
operators -- against the fixture made from the imported reference (tests/golden/audio_tagging.npz) and the fp64
restatement tests/tagging_ref.py.

Bounds are the project's own for heads of this depth (tests/test_gpu_weak.py): 5e-6 relative (and absolute for a loss)
against the fixture's fp64 arrays and for each pass alone, 2e-5 at the benched sizes, and for whole-model runs 1e-4 on
frame_sim / clip_sim, 2e-5 on the loss, 1e-4 relative on gradients."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import tag_oracle as O
from tests import tagging_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_tagging.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _modes():
    from texttoaudiogrounding_amd import ops
    return ops.POOL_MODES


def _lengths(B, T, g):
    length = torch.randint(1, T + 1, (B,), generator=g)
    length[0] = T
    length[-1] = 1 if B > 1 else T
    return length


def _device_head(case, pooling, dev, frame_weight):
    """TaggingHeadFunction + the three loss modules on the device -> same keys as R.head_case_results."""
    from texttoaudiogrounding_amd import losses, ops
    x = case["embedding"].to(dev).requires_grad_(True)
    w = case["weight"].to(dev).requires_grad_(True)
    b = case["bias"].to(dev).requires_grad_(True)
    length = case["length"].to(dev)
    prob, clip = ops.TaggingHeadFunction.apply(x, w, b, length, _modes()[pooling])
    out = {"frame_sim": prob, "clip_sim": clip, "length": length, "label": case["weak_label"].to(dev),
           "weak_label": case["weak_label"].to(dev), "strong_label": case["strong_label"].to(dev),
           "strong_label_mask": case["strong_label_mask"].to(dev)}
    l_clip = losses.ClipBceLoss()(out)
    l_frame = losses.MaskedFrameBceLoss()(out)
    l_mix = losses.ClipMaskedFrameBceLoss(frame_weight)(out)
    l_mix.backward()
    return {"frame_sim": prob, "clip_sim": clip, "loss_clip": l_clip, "loss_frame": l_frame, "loss_mix": l_mix,
            "dembedding": x.grad, "dweight": w.grad, "dbias": b.grad}


# ------------------------------------------------------------------------------------------------ 1. fixture
@pytest.mark.parametrize("pooling", R.POOLINGS)
def test_head_and_losses_match_the_reference_fixture(dev, fx, pooling):
    case = R.draw_head_case()
    got = _device_head(case, pooling, dev, R.FRAME_WEIGHT)
    for k, v in got.items():
        want = torch.as_tensor(fx[f"head_{pooling}_{k}_f64"])
        e = rel(v, want)
        print(f"{pooling} {k}: rel err {e:.2e}")
        assert e < 5e-6, (pooling, k, e)
        if k.startswith("loss"):
            assert abs(v.item() - want.item()) < 5e-6, (pooling, k)


# ------------------------------------------------------------------------------------------------ 2. each pass alone
SHAPES = [(B, T, C) for B in (1, 3, 64) for T in (1, 37, 250) for C in (1, 24, 65, 527)]


def _pool_case(B, T, C, seed):
    g = torch.Generator().manual_seed(seed)
    prob = torch.sigmoid(1.5 * torch.randn(B, T, C, generator=g))
    return prob, _lengths(B, T, g), torch.randn(B, T, C, generator=g), torch.randn(B, C, generator=g)


@pytest.mark.parametrize("pooling", R.POOLINGS)
def test_class_pool_and_head_backward_alone(dev, pooling):
    """tag_class_pool_forward and tag_tagging_head_backward on every (B, T, C) of the grid against fp64 (the fp32 input is
    exact in fp64, so `max` takes the same frame); dprob null, dclip null and dlogit aliasing dprob on a rotating subset;
    two runs of each pass are bit-identical."""
    from texttoaudiogrounding_amd import ops
    mode = _modes()[pooling]
    worst = [0.0, 0.0]
    for i, (B, T, C) in enumerate(SHAPES):
        prob, length, dprob, dclip = _pool_case(B, T, C, 100 + i)
        variant = i % 4                                      # 0 both, 1 dprob null, 2 dclip null, 3 dlogit aliases dprob
        p64 = prob.double()
        logit = torch.logit(p64).requires_grad_(True)
        pr = torch.sigmoid(logit)
        cl = R.pool(pr, length, pooling)
        obj = 0.0
        if variant != 1:
            obj = obj + (pr * dprob.double()).sum()
        if variant != 2:
            obj = obj + (cl * dclip.double()).sum()
        obj.backward()
        # d/d logit through sigmoid(logit(p)) = p (1 - p) up to fp64 rounding
        pd, ld = prob.to(dev), length.to(dev)
        clip, aux = ops.class_pool_forward(pd, ld, mode)
        clip2, aux2 = ops.class_pool_forward(pd, ld, mode)
        assert torch.equal(clip, clip2) and torch.equal(aux, aux2)
        e = rel(clip, cl)
        assert e < 5e-6, (pooling, B, T, C, e)
        if pooling == "max":
            m = R.length_mask(length, T).unsqueeze(-1)
            want_idx = p64.masked_fill(~m, -1.0).argmax(1)            # torch.argmax: the first maximal value, as the kernel
            assert torch.equal(aux.cpu().long(), want_idx), (B, T, C)
        dp = dprob.to(dev) if variant != 1 else None
        dc = dclip.to(dev) if variant != 2 else None
        d1 = ops.tagging_head_dlogit(pd, dp, dc, clip, aux, ld, mode)
        d2 = ops.tagging_head_dlogit(pd, dp, dc, clip, aux, ld, mode)
        assert torch.equal(d1, d2)
        if variant == 3:
            buf = dp.clone()
            d3 = ops.tagging_head_dlogit(pd, buf, dc, clip, aux, ld, mode, out=buf)
            assert d3.data_ptr() == buf.data_ptr() and torch.equal(d3, d1)
        e2 = rel(d1, logit.grad)
        assert e2 < 5e-6, (pooling, B, T, C, variant, e2)
        worst = [max(worst[0], e), max(worst[1], e2)]
    print(f"{pooling}: worst rel err over {len(SHAPES)} shapes: clip {worst[0]:.2e}, dlogit {worst[1]:.2e}")


def test_masked_frame_bce_alone(dev):
    """tag_masked_frame_bce_forward / _backward on every (B, T, C) of the grid against fp64: class mask null / with an
    all-zero row / mixed, the label (and the scores) as views of wider buffers, lengths including 1 and T; two runs are
    bit-identical; masked entries of the gradient are exactly zero."""
    from texttoaudiogrounding_amd import ops
    worst = [0.0, 0.0]
    for i, (B, T, C) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(300 + i)
        pad_p, pad_y = (0, 3)[i % 2], (5, 0, 2)[i % 3]
        prob_buf = torch.sigmoid(2.0 * torch.randn(B, T + pad_p, C, generator=g))
        label_buf = (torch.rand(B, T + pad_y, C, generator=g) < 0.3).float()
        length = _lengths(B, T, g)
        if i % 5 == 0:
            length[B // 2] = T + 4                                     # beyond Tt: clamped
        variant = i % 3                                                # 0 null, 1 mixed with an all-zero row, 2 mixed
        mask = None
        if variant:
            mask = (torch.rand(B, C, generator=g) < 0.5).float()
            mask[0, 0] = 1.0                                           # never all zero overall
            if variant == 1 and B > 1:
                mask[B - 1] = 0.0
        p64 = prob_buf[:, :T].double().requires_grad_(True)
        want = R.masked_frame_bce(p64, label_buf[:, :T].double(), length, mask)
        want.backward()
        pd, yd, ld = prob_buf.to(dev)[:, :T], label_buf.to(dev)[:, :T], length.to(dev)
        md = mask.to(dev) if mask is not None else None
        loss = ops.masked_frame_bce_forward(pd, yd, ld, md)
        assert torch.equal(loss, ops.masked_frame_bce_forward(pd, yd, ld, md))
        # the same numbers from contiguous copies: the views were read in place, not misread
        assert torch.equal(loss, ops.masked_frame_bce_forward(pd.contiguous(), yd.contiguous(), ld, md))
        e = abs(loss.item() - want.item())
        assert e < 5e-6 and e < 5e-6 * abs(want.item()) + 1e-12, (B, T, C, variant, loss.item(), want.item())
        one = torch.ones((), device=dev)
        dp = ops.masked_frame_bce_backward(pd, yd, ld, md, one)
        assert dp.shape == (B, T, C) and dp.is_contiguous()
        assert torch.equal(dp, ops.masked_frame_bce_backward(pd, yd, ld, md, one))
        e2 = rel(dp, p64.grad)
        assert e2 < 5e-6, (B, T, C, variant, e2)
        assert bool((dp.cpu()[p64.grad == 0] == 0).all())                # exactly zero wherever the reference masks
        worst = [max(worst[0], e), max(worst[1], e2)]
    print(f"masked frame BCE: worst over {len(SHAPES)} shapes: loss abs err {worst[0]:.2e}, dprob rel err {worst[1]:.2e}")


# ------------------------------------------------------------------------------------------------ 3. benched sizes
@pytest.mark.parametrize("shape", [(64, 250, 512, 527), (64, 125, 256, 300)])
@pytest.mark.parametrize("pooling", R.POOLINGS)
def test_head_at_the_benched_sizes(dev, shape, pooling):
    """Forward, ClipMaskedFrameBceLoss(0.5) and every gradient against the fp64 restatement, bound 2e-5.  `max`: near-ties
    among the frames flip the arg-max between any two arithmetics (the reference's own fp32 run disagrees with its fp64
    run by 1.8e-1 on the embedding gradient at this size), so the device's decision is imposed on the fp64 side -- after
    asserting, for EVERY (clip, class), that the fp64 probability at the device's index is within 4e-5 of the fp64
    maximum (twice the frame_sim bound: two scores each right to 2e-5 cannot be ordered more wrongly)."""
    from texttoaudiogrounding_amd import ops
    case = R.draw_head_case(seed=7000 + shape[1], shape=shape)
    got = _device_head(case, pooling, dev, 0.5)
    argmax = None
    if pooling == "max":
        _, aux = ops.class_pool_forward(got["frame_sim"].detach(), case["length"].to(dev), _modes()["max"])
        argmax = aux.cpu().long()
        p64, c64 = R.head(case["embedding"].double(), case["weight"].double(), case["bias"].double(), case["length"], "max")
        at_idx = p64.gather(1, argmax.view(shape[0], 1, shape[3])).squeeze(1)
        gap = (c64 - at_idx).max().item()
        print(f"max: fp64 maximum minus fp64 probability at the device's index: at most {gap:.2e}")
        assert (at_idx <= c64).all() and gap < 4e-5
        assert bool((argmax < case["length"].view(-1, 1)).all())
    want = R.head_case_results(case, pooling, torch.float64, frame_weight=0.5, argmax=argmax)
    for k, v in got.items():
        e = rel(v, want[k])
        print(f"{shape} {pooling} {k}: rel err {e:.2e}")
        assert e < 2e-5, (shape, pooling, k, e)
        if k.startswith("loss"):
            assert abs(v.item() - want[k].item()) < 2e-5


# ------------------------------------------------------------------------------------------------ 4. whole model
def _build(kind, dev):
    from texttoaudiogrounding_amd.models import audio_encoder
    from texttoaudiogrounding_amd.models.audio_text_model import AudioTagging
    enc = audio_encoder.Cnn8Rnn(32000) if kind == "cnn8rnn" else audio_encoder.CrnnEncoder(32000, 256)
    model = AudioTagging(enc, R.MODELS[kind]["classes"])
    st = R.model_state(kind)
    missing = model.load_state_dict(st, strict=False)
    assert not missing.unexpected_keys and all("melspec" in k for k in missing.missing_keys)
    return model.to(dev), st


def _labels(kind, T, seed=9):
    C = R.MODELS[kind]["classes"]
    g = torch.Generator().manual_seed(seed)
    return {"strong_label": (torch.rand(2, T, C, generator=g) < 0.3).float(),
            "weak_label": (torch.rand(2, C, generator=g) < 0.3).float(),
            "strong_label_mask": (torch.rand(2, C, generator=g) < 0.5).float()}


@pytest.mark.parametrize("kind", ["cnn8rnn", "crnn"])
def test_whole_model_against_the_reference_and_the_oracle(dev, fx, kind):
    from texttoaudiogrounding_amd.losses import ClipMaskedFrameBceLoss
    model, st = _build(kind, dev)
    model.eval()
    batch = R.model_batch(kind)
    out = model({"waveform": batch["waveform"].to(dev), "waveform_len": batch["waveform_len"], "specaug": False})
    assert set(out) == {"frame_sim", "clip_sim", "length"}
    assert torch.as_tensor(out["length"]).cpu().long().tolist() == fx[f"{kind}_length"].tolist()
    e_fs = (out["frame_sim"].detach().cpu().double() - torch.as_tensor(fx[f"{kind}_frame_sim"]).double()).abs().max().item()
    e_cs = (out["clip_sim"].detach().cpu().double() - torch.as_tensor(fx[f"{kind}_clip_sim"]).double()).abs().max().item()
    print(f"{kind}: vs the reference's fp32 run: frame_sim err {e_fs:.1e}, clip_sim err {e_cs:.1e}")
    assert out["frame_sim"].shape == fx[f"{kind}_frame_sim"].shape and e_fs < 1e-4 and e_cs < 1e-4
    T = out["frame_sim"].shape[1]
    lab = _labels(kind, T)
    o = dict(out)
    o.update({k: v.to(dev) for k, v in lab.items()})
    loss = ClipMaskedFrameBceLoss(0.5)(o)
    loss.backward()
    s64 = O.state_to(st, torch.float64, requires_grad=True)
    ao = R.encoder_forward(kind, s64, batch["waveform"].double(), batch["waveform_len"])
    fo, co = R.head(ao["embedding"], s64["fc_output.weight"], s64["fc_output.bias"], ao["length"], "linear_softmax")
    lo = R.clip_masked_frame_bce(fo, co, lab["weak_label"].double(), lab["strong_label"].double(), ao["length"],
                                 lab["strong_label_mask"].double(), 0.5)
    lo.backward()
    e_fs, e_cs = rel(out["frame_sim"], fo) * fo.abs().max().item(), rel(out["clip_sim"], co) * co.abs().max().item()
    print(f"{kind}: vs the fp64 oracle: frame_sim err {e_fs:.1e}, clip_sim err {e_cs:.1e}, loss {loss.item():.6f} vs {lo.item():.6f}")
    assert e_fs < 1e-4 and e_cs < 1e-4 and abs(loss.item() - lo.item()) < 2e-5
    names = ["fc_output.weight", "fc_output.bias"]
    names += ["backbone.fc1.weight", "backbone.rnn.weight_ih_l0"] if kind == "cnn8rnn" else ["backbone.gru.weight_ih_l0"]
    params = dict(model.named_parameters())
    for name in names:
        e = rel(params[name].grad, s64[name].grad)
        print(f"{kind}: grad {name}: rel err {e:.1e}")
        assert e < 1e-4, (name, e)


# ------------------------------------------------------------------------------------------------ 5. segments
def test_segments_of_every_class_column(dev, fx):
    """The device's frame_sim of the head-level fixture case, every class column through eval_util.class_frame_sim, 50
    thresholds, median windows 1 and 5: the segment lists equal those O.segments computes from the REFERENCE's fp64 scores
    for every (clip, class, threshold) case in which no valid frame of the reference lies within 1e-4 of the threshold; at
    most 2 % of the cases may be left out."""
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils import eval_util
    case = R.draw_head_case()
    B, T, E, C = R.HEAD_SHAPE
    with torch.no_grad():
        prob, _ = ops.TaggingHeadFunction.apply(case["embedding"].to(dev), case["weight"].to(dev), case["bias"].to(dev),
                                                case["length"].to(dev), _modes()["linear_softmax"])
    ref = fx["head_linear_softmax_frame_sim_f64"]
    th = eval_util.eval_thresholds(50)
    assert np.array_equal(th, O.eval_thresholds())
    n_connect = eval_util.n_connect_for(0.04)
    total = left_out = 0
    for b in range(B):
        n = int(case["length"][b])
        rows = prob[b:b + 1, :n].expand(C, n, C)
        mat = eval_util.class_frame_sim(rows, torch.arange(C))
        assert mat.shape == (C, n) and mat.is_contiguous() and torch.equal(mat, prob[b, :n].t())
        for window in (1, 5):
            got = eval_util.segments_for_thresholds(mat, th, window, n_connect)
            for c in range(C):
                for ti, tt in enumerate(th):
                    total += 1
                    if np.abs(ref[b, :n, c] - tt).min() < 1e-4:
                        left_out += 1
                        continue
                    assert np.array_equal(got[c][ti], O.segments(ref[b, :n, c], tt, window, n_connect)), (b, c, tt, window)
    print(f"segments: {total} (clip, class, threshold, window) cases, {left_out} left out ({100.0 * left_out / total:.2f} %)")
    assert left_out <= 0.02 * total


# ------------------------------------------------------------------------------------------------ 6. runner
def _train_batch(kind, T_label, seed=9):
    b = R.model_batch(kind)
    batch = {"waveform": b["waveform"].clone(), "waveform_len": b["waveform_len"].copy()}
    batch.update(_labels(kind, T_label, seed))
    return batch


def _train_model(dev):
    model, _ = _build("cnn8rnn", dev)
    model.backbone.dropout_p = (0.0, 0.0)
    return model


@pytest.mark.parametrize("T_label", [40, 30])
def test_runner_direct_gradients_equal_plain_autograd(dev, T_label):
    """One forward_backward with direct gradients against loss.backward() through the same modules (T_label = 40: the label
    is truncated to the model's 37 frames as a view; 30: frame_sim is)."""
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.losses import ClipMaskedFrameBceLoss
    from texttoaudiogrounding_amd.runner import ClassMappingRunner
    model = _train_model(dev)
    plain = copy.deepcopy(model).train()
    runner = ClassMappingRunner(model, loss_fn=ClipMaskedFrameBceLoss(0.5), device=dev)
    runner.model.train()
    loss = runner.forward_backward(_train_batch("cnn8rnn", T_label))
    b = {k: (torch.as_tensor(v).to(dev) if k != "waveform_len" else v) for k, v in _train_batch("cnn8rnn", T_label).items()}
    assert not ops.DIRECT_GRADS
    out = plain({"waveform": b["waveform"], "waveform_len": b["waveform_len"], "specaug": False})
    tt = min(out["frame_sim"].size(1), T_label)
    assert out["frame_sim"].size(1) == 37
    out.update({"frame_sim": out["frame_sim"][:, :tt], "strong_label": b["strong_label"][:, :tt],
                "length": torch.clamp(out["length"], 1, tt), "weak_label": b["weak_label"],
                "strong_label_mask": b["strong_label_mask"]})
    loss2 = ClipMaskedFrameBceLoss(0.5)(out)
    loss2.backward()
    assert abs(loss.item() - loss2.item()) < 5e-6
    got, want = dict(runner.model.named_parameters()), dict(plain.named_parameters())
    for name in ("fc_output.weight", "fc_output.bias"):
        e = rel(got[name].grad, want[name].grad)
        print(f"T_label {T_label}: {name}: direct vs plain rel err {e:.1e}")
        assert e < 5e-6, (name, e)
    has = lambda p: p.grad is not None and bool((p.grad != 0).any())
    assert {n for n, p in got.items() if has(p)} == {n for n, p in want.items() if has(p)}
    assert has(got["fc_output.weight"]) and has(got["backbone.conv_block1.conv1.weight"])


def test_runner_frozen_parts_loss_descent_and_weak_batches(dev):
    from texttoaudiogrounding_amd.losses import ClipBceLoss
    from texttoaudiogrounding_amd.runner import ClassMappingRunner
    # fc_output frozen: the head still hands the embedding its gradient, nothing frozen moves
    model = _train_model(dev)
    for p in model.fc_output.parameters():
        p.requires_grad = False
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    runner = ClassMappingRunner(model, device=dev)
    runner.train_step(_train_batch("cnn8rnn", 40))
    after = dict(runner.model.named_parameters())
    assert torch.equal(after["fc_output.weight"], before["fc_output.weight"]) and after["fc_output.weight"].grad is None
    assert torch.equal(after["fc_output.bias"], before["fc_output.bias"]) and after["fc_output.bias"].grad is None
    assert not torch.equal(after["backbone.fc1.weight"], before["backbone.fc1.weight"])
    # backbone frozen: only the head trains
    model = _train_model(dev)
    for p in model.backbone.parameters():
        p.requires_grad = False
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    runner = ClassMappingRunner(model, device=dev)
    assert len(runner.flat.params) == 2
    runner.train_step(_train_batch("cnn8rnn", 40))
    for n, p in runner.model.named_parameters():
        if n.startswith("backbone."):
            assert torch.equal(p, before[n]) and p.grad is None, n
        else:
            assert not torch.equal(p, before[n]), n
    # the loss falls over 5 steps on one batch (default loss: ClipMaskedFrameBceLoss(0.5))
    runner = ClassMappingRunner(_train_model(dev), device=dev)
    losses = [runner.loss_value(runner.train_step(_train_batch("cnn8rnn", 40))) for _ in range(5)]
    print("ClassMappingRunner: loss over 5 steps on one batch:", [round(v, 5) for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    # run_weak.py: ClipBceLoss on a label-only batch
    runner = ClassMappingRunner(_train_model(dev), loss_fn=ClipBceLoss(), device=dev)
    b = R.model_batch("cnn8rnn")
    weak = {"waveform": b["waveform"].clone(), "waveform_len": b["waveform_len"].copy(), "label": _labels("cnn8rnn", 1)["weak_label"]}
    l0 = runner.loss_value(runner.train_step(weak))
    assert np.isfinite(l0) and bool((runner.model.fc_output.weight.grad != 0).any())


# ------------------------------------------------------------------------------------------------ 7. operators
def test_operators_match_the_node_and_pass_opcheck(dev):
    import texttoaudiogrounding_amd.torch_ops  # noqa: F401
    from texttoaudiogrounding_amd import ops
    case = R.draw_head_case(seed=11, shape=(3, 11, 32, 7))
    x, w, b = (case[k].to(dev).requires_grad_(True) for k in ("embedding", "weight", "bias"))
    length, lab, mask = case["length"].to(dev), case["strong_label"].to(dev), case["strong_label_mask"].to(dev)
    prob, clip, _aux = torch.ops.tag.tagging_head(x, w, b, length, 3)
    loss = torch.ops.tag.masked_frame_bce(prob, lab, length, mask) + clip.square().sum()
    loss.backward()
    g1 = [t.grad.clone() for t in (x, w, b)]
    for t in (x, w, b):
        t.grad = None
    prob2, clip2 = ops.TaggingHeadFunction.apply(x, w, b, length, 3)
    loss2 = torch.ops.tag.masked_frame_bce(prob2, lab, length, mask) + clip2.square().sum()
    loss2.backward()
    assert torch.equal(loss, loss2) and all(torch.equal(a, t.grad) for a, t in zip(g1, (x, w, b)))
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.tag.tagging_head, (x.detach().requires_grad_(True), w.detach().requires_grad_(True),
                                                       b.detach().requires_grad_(True), length, 2), test_utils=utils)
    torch.library.opcheck(torch.ops.tag.masked_frame_bce, (prob.detach().requires_grad_(True), lab, length, mask),
                          test_utils=utils)
    torch.library.opcheck(torch.ops.tag.masked_frame_bce, (prob.detach().requires_grad_(True), lab, length, None),
                          test_utils=utils)
