"""GPU: the early-fusion CrossCDur (models/audio_text_model.py:461-568 in the reference) -- the biased conv kernels against
float64, the frame head at N = 256, the whole model against the fixture made from the imported reference
(tests/golden/cross_cdur.npz: eval with segments and upsampling, one training step), the dropout-on step against a float64
restatement of the reference forward built from the model's own weights, the benched size, StrongRunner, requires_grad=False,
the operator's registration and CDurTextBlock on its own."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tag_oracle as O
from tests import cross_cdur_state as CS
from tests.test_gpu_kernels import nchw, nhwc, relerr
from tests.test_gpu_path import assert_crnn_grad_close

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ kernels
def _prologue(v, pro, s, t):
    sc, sh = s.view(1, -1, 1, 1).double(), t.view(1, -1, 1, 1).double()
    return (F.leaky_relu(v, 0.1) if pro == 2 else v) * sc + sh


@pytest.mark.parametrize("B,H,W,Cin,Cout,pro", [(3, 5, 16, 32, 128, 3), (3, 7, 16, 128, 128, 2), (2, 9, 4, 128, 128, 2),
                                                (2, 9, 4, 128, 128, 3), (1, 1, 16, 32, 128, 3), (1, 1, 16, 128, 128, 2)])
def test_biased_conv_vs_fp64_and_zero_bias_bit_identical(dev, B, H, W, Cin, Cout, pro):
    """y = conv(prologue(x)) + t[b, cout] of the halo-tile kernel's bias epilogue: odd heights, so the last row tile of a clip
    is partial and the next workgroup belongs to another clip.  Bound of test_conv3x3_forward_dgrad_wgrad."""
    from texttoaudiogrounding_amd import dispatch
    g = torch.Generator().manual_seed(B * 1000 + H + Cin)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    s, t = torch.rand(Cin, generator=g) + 0.5, 0.3 * torch.randn(Cin, generator=g)
    bias = torch.randn(B, Cout, generator=g)
    ref = F.conv2d(_prologue(x.double(), pro, s, t), w.double(), None, 1, 1) + bias.double()[:, :, None, None]
    wf, _ = dispatch.pack_conv_weight(w.to(dev), want_dgrad=False)
    xd, sd, td = nhwc(x).to(dev), s.to(dev), t.to(dev)
    y = dispatch.conv3x3_bias(xd, wf, Cout, pro, sd, td, bias.to(dev))
    e = relerr(nchw(y), ref)
    print(f"biased conv ({B},{H},{W},{Cin}->{Cout}, prologue {pro}): {e:.2e} of the range")
    assert e < 5e-6
    y0 = dispatch.conv3x3_bias(xd, wf, Cout, pro, sd, td, torch.zeros(B, Cout, device=dev))
    assert torch.equal(y0, dispatch.conv3x3(xd, wf, Cout, pro, sd, td))


def test_biased_c1_conv_vs_fp64_and_zero_bias_bit_identical(dev):
    """The Cin = 1 kernel at (B 3, H 11, W 64, -> 32): its pixel groups run over the whole batch, so a workgroup holds rows of
    two clips.  Bound of test_conv3x3_c1."""
    from texttoaudiogrounding_amd import dispatch
    g = torch.Generator().manual_seed(7)
    B, H, W, Cout = 3, 11, 64, 32
    x = torch.randn(B, H, W, generator=g) * 10 - 30
    cs, ct = torch.rand(W, generator=g) * 0.1 + 0.05, torch.randn(W, generator=g)
    w = torch.randn(Cout, 1, 3, 3, generator=g) / 3
    bias = torch.randn(B, Cout, generator=g)
    xin = (x.double() * cs.double() + ct.double()).unsqueeze(1)
    ref = F.conv2d(xin, w.double(), None, 1, 1) + bias.double()[:, :, None, None]
    y = dispatch.conv3x3_c1_bias(x.to(dev), w.to(dev), cs.to(dev), ct.to(dev), bias.to(dev))
    e = relerr(nchw(y), ref)
    print(f"biased Cin = 1 conv: {e:.2e} of the range")
    assert e < 2e-6
    y0 = dispatch.conv3x3_c1_bias(x.to(dev), w.to(dev), cs.to(dev), ct.to(dev), torch.zeros(B, Cout, device=dev))
    assert torch.equal(y0, dispatch.conv3x3_c1(x.to(dev), w.to(dev), cs.to(dev), ct.to(dev)))


@pytest.mark.parametrize("B,H,W,Cin,Cout,pro", [(2, 5, 8, 32, 128, 3), (2, 5, 16, 64, 128, 2), (2, 5, 16, 32, 64, 3),
                                                (2, 5, 16, 32, 128, 1), (2, 5, 16, 32, 128, 0)])
def test_biased_conv_unserved_shape_is_einval_not_a_launch(dev, B, H, W, Cin, Cout, pro):
    from texttoaudiogrounding_amd import dispatch
    x = torch.zeros(B, H, W, Cin, device=dev)
    wf = torch.zeros(9, Cin, Cout, device=dev)
    s = torch.ones(Cin, device=dev)
    with pytest.raises(RuntimeError, match=r"tag_conv3x3_forward_bias failed \(rc=-1\)"):
        dispatch.conv3x3_bias(x, wf, Cout, pro, s, s, torch.zeros(B, Cout, device=dev))
    with pytest.raises(RuntimeError, match=r"tag_conv3x3_c1_forward_bias failed \(rc=-1\)"):
        dispatch.conv3x3_c1_bias(torch.zeros(2, 5, 62, device=dev), torch.zeros(32, 1, 3, 3, device=dev), None, None,
                                 torch.zeros(2, 32, device=dev))
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,H,W,C,ph,pw,drop", [(3, 7, 8, 128, 2, 4, 0.0), (2, 5, 64, 32, 2, 4, 0.0), (3, 9, 4, 128, 1, 4, 0.3),
                                                (1, 1, 4, 128, 1, 4, 0.0)])
def test_lppool_backward_clip_sums_vs_fp64_bitwise_dz_and_repeatable(dev, B, H, W, C, ph, pw, drop):
    """tag_lppool_leaky_backward_clip (blocks 1, 3, 5): dt = per-clip sums of dz against float64 autograd, equal to
    rowgroup_colsum over dz within the same bound, dz bit-identical to tag_lppool_leaky_backward's, all outputs bitwise
    equal on a second run."""
    from texttoaudiogrounding_amd import dispatch, functions
    g = torch.Generator().manual_seed(3 + H)
    z = torch.randn(B, H, W, C, generator=g)
    t = 0.5 * torch.randn(B, C, generator=g)
    seed = 777 if drop > 0 else 0
    # the conv output is z - t, so that t's gradient is the clip sum of dz
    z64, t64 = (z - t[:, None, None, :]).double().requires_grad_(True), t.double().requires_grad_(True)
    a = F.lp_pool2d(F.leaky_relu(z64 + t64[:, None, None, :], 0.1).permute(0, 3, 1, 2), 4.0, (ph, pw))
    if drop > 0:
        keep = dispatch.dropout_mask(seed, (B, H // ph, W // pw, C), drop, dev, pooled=True).cpu().permute(0, 3, 1, 2)
        a = a * keep.double() / (1 - drop)
    da = torch.randn(a.shape, generator=g)
    a.backward(da.double())
    zd, dad = z.to(dev), nhwc(da).to(dev)
    runs = [dispatch.lppool_leaky_backward_clip(zd, dad, ph, pw, drop, seed) for _ in range(2)]
    dz, dt = runs[0]
    bound = lambda r: 1e-4 * (1 + r.abs().max().item())
    assert (dz.cpu().double() - z64.grad).abs().max().item() <= bound(z64.grad)
    assert (dt.cpu().double() - t64.grad).abs().max().item() <= bound(t64.grad)
    plain = dispatch.lppool_leaky_backward(zd, dad, ph, pw, drop, seed)
    assert torch.equal(dz, plain)
    sep = functions._clip_sums(plain)
    assert (dt.cpu().double() - sep.cpu().double()).abs().max().item() <= bound(t64.grad)
    assert (sep.cpu().double() - t64.grad).abs().max().item() <= bound(t64.grad)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(sep, functions._clip_sums(plain))


@pytest.mark.parametrize("B,H,W,C,train", [(3, 7, 8, 128, True), (2, 5, 16, 128, False), (1, 3, 4, 128, True), (5, 125, 4, 128, True)])
def test_bn_act_backward_clip_sums_vs_fp64_bitwise_dz_and_repeatable(dev, B, H, W, C, train):
    """tag_bn_act_backward_clip (blocks 2, 4: u = bn(leaky(conv + t))): the same checks."""
    from texttoaudiogrounding_amd import dispatch, functions
    g = torch.Generator().manual_seed(5 + H)
    z = torch.randn(B, H, W, C, generator=g)
    t = 0.5 * torch.randn(B, C, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    rm, rv = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    z64, t64 = (z - t[:, None, None, :]).double().requires_grad_(True), t.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    v = F.leaky_relu(z64 + t64[:, None, None, :], 0.1).permute(0, 3, 1, 2)
    u = F.batch_norm(v, rm.double().clone(), rv.double().clone(), g64, b64, train, 0.1, 1e-5)
    du = torch.randn(u.shape, generator=g)
    u.backward(du.double())
    zd, dud, gd = z.to(dev), nhwc(du).to(dev), gamma.to(dev)
    st = dispatch.bn_stats(zd.view(-1, C), gd, beta.to(dev), rm.to(dev), rv.to(dev), train, pre_op=1)
    runs = [dispatch.bn_act_backward_clip(zd, 1, st, gd, dud) for _ in range(2)]
    dz, dg, db, dt = runs[0]
    bound = lambda r: 1e-4 * (1 + r.abs().max().item())
    assert (dz.cpu().double() - z64.grad).abs().max().item() <= bound(z64.grad)
    assert (dt.cpu().double() - t64.grad).abs().max().item() <= bound(t64.grad)
    assert (dg.cpu().double() - g64.grad).abs().max().item() <= bound(g64.grad)
    assert (db.cpu().double() - b64.grad).abs().max().item() <= bound(b64.grad)
    plain = dispatch.bn_act_backward(zd, 1, st, gd, dud)
    assert torch.equal(dz, plain[0]) and torch.equal(dg, plain[1]) and torch.equal(db, plain[2])
    sep = functions._clip_sums(plain[0])
    assert (dt.cpu().double() - sep.cpu().double()).abs().max().item() <= bound(t64.grad)
    assert (sep.cpu().double() - t64.grad).abs().max().item() <= bound(t64.grad)
    for x0, x1 in zip(runs[0], runs[1]):
        assert torch.equal(x0, x1)


def test_frame_head_n256_with_clamp(dev):
    """The frame head at N = 256 (2 x GRU(128)) with a row driven far below the clamp: prob = 1e-7 exactly, zero gradient."""
    from texttoaudiogrounding_amd import dispatch
    g = torch.Generator().manual_seed(11)
    B, T, N = 3, 13, 256
    y = torch.randn(B * T, N, generator=g).to(dev)
    r = torch.randn(B, N, generator=g).to(dev)
    w = (torch.randn(N, generator=g) / 8).to(dev)
    b0 = torch.tensor([0.1]).to(dev)
    y[5] = -40 * w / (w * w).sum() - r[0]                    # (y + r) . w = -40: sigmoid < 1e-7
    prob, sig = dispatch.frame_head_forward(y, r, w, b0, T)
    y64 = y.cpu().double().requires_grad_(True)
    r64, w64, b64 = (v.cpu().double().requires_grad_(True) for v in (r, w, b0))
    p64 = torch.sigmoid(((y64.view(B, T, N) + r64[:, None]) @ w64) + b64).clamp(1e-7, 1.0).view(-1)
    assert prob[5].item() == np.float32(1e-7) and p64[5].item() == 1e-7
    assert (prob.cpu().double() - p64).abs().max().item() <= 1e-6
    dp = torch.randn(B * T, generator=g)
    p64.backward(dp.double())
    dy, dw, db0, dr = dispatch.frame_head_backward(y, r, w, sig, dp.to(dev), T)
    assert dy[5].abs().max().item() == 0.0 and y64.grad[5].abs().max().item() == 0.0
    for got, want in ((dy, y64.grad), (dw, w64.grad), (db0, b64.grad), (dr, r64.grad)):
        assert (got.cpu().double() - want).abs().max().item() <= 1e-5 * (1 + want.abs().max().item())


# ------------------------------------------------------------------------------------------------------------ whole model
def build(dev, gold, **kw):
    from texttoaudiogrounding_amd.models import audio_text_model as M, text_encoder as TE
    torch.manual_seed(0)
    m = M.CrossCDur(32000, TE.EmbeddingAgg(CS.VOCAB, CS.D_TEXT), **kw)
    st = CS.draw_state(gold["block1_bn_running"])
    assert np.allclose(CS.state_checksum(st), gold["state_checksum"], rtol=1e-9), "seeded weights drifted from the fixture"
    res = m.load_state_dict(st, strict=False)
    assert len(res.missing_keys) == 2 and not res.unexpected_keys
    return m.to(dev)


def to_dev(b, dev):
    """No ``specaug`` / ``mixup_lambda`` keys: the forward reads neither."""
    return {"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"], "text": b["text"].to(dev),
            "text_len": torch.as_tensor(b["text_len"]).to(dev)}


def ref_forward(st, b, training, mask=None, p_drop=0.3, upsample=False):
    """The reference CrossCDur.forward in float64 on the CPU; st: the model's state dict (requires_grad leaves), running statistics
    updated in place; mask: keep mask (B, 128, T', 1) of the dropout, or None (dropout off)."""
    e = O.embedding_agg_mean(st, b["text"].cpu(), torch.as_tensor(b["text_len"]).cpu(), prefix="text_encoder.")["seq_emb"]
    x = O.logmel(b["waveform"].cpu().to(e.dtype), "crnn").transpose(1, 2).unsqueeze(1)            # (B, 1, F, 64)

    def block(x, i):
        p = f"block{i}."
        x = F.conv2d(O._bn(x, st, p + "bn.", training), st[p + "conv.weight"], None, 1, 1)
        return F.leaky_relu(x + F.linear(e, st[p + "fc_text.weight"], st[p + "fc_text.bias"])[:, :, None, None], 0.1)

    x = F.lp_pool2d(block(x, 1), 4.0, (2, 4))
    x = F.lp_pool2d(block(block(x, 2), 3), 4.0, (2, 4))
    x = F.lp_pool2d(block(block(x, 4), 5), 4.0, (1, 4))
    if mask is not None:
        x = x * mask.to(x.dtype) / (1.0 - p_drop)
    x = x.transpose(1, 2).contiguous().flatten(-2)
    x = O.gru_bidir(x, st, "gru.") + F.linear(e, st["fc_text.weight"], st["fc_text.bias"])[:, None]
    prob = torch.sigmoid(F.linear(x, st["fc_output.weight"], st["fc_output.bias"])).squeeze(-1).clamp(1e-7, 1.0)
    if upsample:
        prob = F.interpolate(prob.unsqueeze(1), prob.shape[1] * 4, mode="linear", align_corners=False).squeeze(1)
    return prob


def _state(m, dtype):
    st = {k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu() for k, v in m.state_dict().items()}
    for k, _ in m.named_parameters():
        st[k].requires_grad_(True)
    return st


def test_eval_vs_reference_fixture_with_segments_and_upsample(dev, golden_dir):
    from texttoaudiogrounding_amd.utils import eval_util
    gold = np.load(f"{golden_dir}/cross_cdur.npz")
    b = CS.eval_batch()
    m = build(dev, gold).eval()
    with torch.no_grad():
        out = m(to_dev(b, dev))
    fs = out["frame_sim"]
    assert fs.shape == (2, 125) and np.array_equal(out["length"].cpu().numpy(), gold["length"])
    err = float(np.abs(fs.cpu().double().numpy() - gold["frame_sim_f64"]).max())
    ref_err = float(gold["frame_sim_ref_err"])
    print(f"eval: frame_sim {err:.2e} from the fp64 twin (the fp32 reference: {ref_err:.2e})")
    assert err < 1e-4
    thresholds = gold["thresholds"]
    regions = eval_util.segments_for_thresholds(fs, thresholds, 1, int(gold["n_connect"]))
    want = {}
    for bi, ti, on, off in gold["segments"]:
        want.setdefault((int(bi), int(ti)), []).append((int(on), int(off)))
    checked = 0
    for bi in range(2):
        for ti in range(len(thresholds)):
            if gold["margin"][bi, ti] <= 2 * (err + ref_err):
                continue
            got = [(int(a), int(c)) for a, c in np.asarray(regions[bi][ti]).reshape(-1, 2)]
            assert got == want.get((bi, ti), []), (bi, ti)
            checked += 1
    print(f"eval: segments identical to the reference's at {checked} of 100 (clip, threshold) pairs")
    assert checked >= 95
    mu = build(dev, gold, upsample=True).eval()
    with torch.no_grad():
        ou = mu(to_dev(b, dev))
    assert ou["frame_sim"].shape == (2, 500) and np.array_equal(ou["length"].cpu().numpy(), gold["length_up"])
    assert np.array_equal(ou["length"].cpu().numpy(), 4 * gold["length"])
    eu = float(np.abs(ou["frame_sim"].cpu().double().numpy() - gold["frame_sim_up_f64"]).max())
    print(f"eval, upsample: {eu:.2e} from the fp64 twin")
    assert eu < 1e-4


def _check_grads(named, want_of, floor_of, text):
    worst = 0.0
    for name, p in named:
        want, floor = want_of(name), floor_of(name)
        assert p.grad is not None, name
        g = p.grad.detach().double().flatten().cpu()
        idx = CS.sample_index(name, tuple(p.shape), text)
        err = np.abs(g[idx].numpy() - want[2:]).max() / (want[1] + 1e-300)
        nerr = abs(g.norm().item() - want[0]) / (want[0] + 1e-300)
        worst = max(worst, max(err, nerr) / (4.0 * max(floor, 1e-6)))
        print(f"  {name:40s} hip {err:.2e} (norm {nerr:.2e})  fp32 floor {floor:.2e}")
        assert_crnn_grad_close(name, err, nerr, floor)
    return worst


def test_train_step_vs_reference_fixture(dev, golden_dir):
    """Fixture (c): dropout off, FrameBceLoss: loss within 2e-5, every parameter's gradient by assert_crnn_grad_close (embedding
    table and the six fc_text linears included), BatchNorm buffers and num_batches_tracked after the step."""
    from texttoaudiogrounding_amd.runner import StrongRunner
    gold = np.load(f"{golden_dir}/cross_cdur.npz")
    b = CS.train_batch()
    assert np.allclose(CS.checksum(b["waveform"]) + CS.checksum(b["label"]), gold["train_input_checksum"], rtol=1e-9)
    m = build(dev, gold).train()
    m.dropout_p = 0.0
    runner = StrongRunner(m, device=str(dev))
    loss = runner.forward_backward({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
    lv = runner.loss_value(loss)
    print(f"train: loss {lv:.7f} vs fp64 {float(gold['loss_f64']):.7f} (fp32 reference {float(gold['loss_f32']):.7f})")
    assert abs(lv - float(gold["loss_f64"])) < 2e-5
    names = [n for n, _ in m.named_parameters()]
    assert len(names) == 38 and all(f"grad/{n}" in gold.files for n in names)
    worst = _check_grads(m.named_parameters(), lambda n: gold[f"grad/{n}"], lambda n: float(gold[f"floor/{n}"].max()), b["text"])
    print(f"train: worst gradient tensor at {worst:.2f} of its 4 x floor bound")
    sd = m.state_dict()
    after = [k for k in gold.files if k.startswith("after/")]
    assert len(after) == 15
    for k in after:
        got = sd[k[len("after/"):]].cpu().numpy()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(gold[k]) == 4, k
        else:
            assert np.allclose(got, gold[k], rtol=2e-4, atol=1e-5), k


def test_train_step_with_dropout_vs_fp64_restatement(dev, golden_dir):
    """Dropout on: the step against the float64 restatement above from the model's own weights, the keep mask replayed from
    ``_last_dropout``; the floor of each tensor is the restatement's own fp32 distance from fp64.  Same bounds as fixture (c)."""
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.runner import StrongRunner
    gold = np.load(f"{golden_dir}/cross_cdur.npz")
    b = CS.train_batch()
    m = build(dev, gold).train()
    assert m.dropout_p == 0.3
    st64, st32 = _state(m, torch.float64), _state(m, torch.float32)
    runner = StrongRunner(m, device=str(dev))
    loss = runner.forward_backward({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
    lv = runner.loss_value(loss)
    info = m._last_dropout
    assert info["p"] == 0.3 and len(info["seeds"]) == 1 and info["seeds"][0] != 0
    keep = ops.dropout_mask(info["seeds"][0], (2, 25, 1, 128), 0.3, dev, pooled=True).cpu().permute(0, 3, 1, 2)
    assert 0.6 < keep.float().mean().item() < 0.8
    length = torch.clamp(O.output_length(b["waveform_len"], CS.HOP), 1, 25)
    res = {}
    for st, dtype in ((st64, torch.float64), (st32, torch.float32)):
        prob = ref_forward(st, b, True, mask=keep.to(dtype))
        ls = O.frame_bce_loss(prob, b["label"].to(dtype), length)
        ls.backward()
        res[dtype] = (float(ls.detach()), {k: st[k].grad.detach().double() for k, _ in m.named_parameters()})
    l64, g64 = res[torch.float64]
    g32 = res[torch.float32][1]
    print(f"train + dropout: loss {lv:.7f} vs fp64 {l64:.7f} (fp32 restatement {res[torch.float32][0]:.7f})")
    assert abs(lv - l64) < 2e-5

    def want_of(n):
        flat = g64[n].flatten()
        return np.concatenate([[flat.norm().item(), flat.abs().max().item()],
                               flat[CS.sample_index(n, tuple(g64[n].shape), b["text"])].numpy()])

    def floor_of(n):
        flat, f32 = g64[n].flatten(), g32[n].flatten()
        return max((f32 - flat).abs().max().item() / (flat.abs().max().item() + 1e-300),
                   abs(f32.norm().item() - flat.norm().item()) / (flat.norm().item() + 1e-300))

    _check_grads(m.named_parameters(), want_of, floor_of, b["text"])
    sd = m.state_dict()
    for k, v in st64.items():
        if "running_" in k:
            assert np.allclose(sd[k].cpu().numpy(), v.detach().numpy(), rtol=2e-4, atol=1e-5), k


def _b64_batch(dev):
    b = O.synthetic_batch(64, 320000, seed=99, ragged=True, hop=CS.HOP)
    return b, to_dev(b, dev)


def test_eval_b64_clips_are_independent(dev, golden_dir):
    """Eval at B = 64 x 10 s: finite, and its first two clips equal a B = 2 run of the same clips within 1e-6 (clips are
    independent in eval: the tile-straddling check at the benched size)."""
    gold = np.load(f"{golden_dir}/cross_cdur.npz")
    m = build(dev, gold).eval()
    _, inp = _b64_batch(dev)
    with torch.no_grad():
        big = m(inp)["frame_sim"]
        two = {k: (v[:2] if torch.is_tensor(v) else v[:2]) for k, v in inp.items()}
        small = m(two)["frame_sim"]
    assert big.shape == (64, 125) and bool(torch.isfinite(big).all())
    d = (big[:2] - small).abs().max().item()
    print(f"eval B = 64 vs B = 2 on the same clips: {d:.2e}")
    assert d <= 1e-6


def test_b64_strong_runner_step_bitwise_and_frozen_parameter(dev, golden_dir, monkeypatch):
    """One B = 64 x 10 s training step through StrongRunner.train_step runs; its gradients equal those of a hand-driven forward /
    loss / backward bit for bit (same dropout seed); a parameter with requires_grad=False gets none and the others do not
    change."""
    from texttoaudiogrounding_amd import functions
    from texttoaudiogrounding_amd.losses import FrameBceLoss
    from texttoaudiogrounding_amd.runner import StrongRunner
    gold = np.load(f"{golden_dir}/cross_cdur.npz")
    b, inp = _b64_batch(dev)
    monkeypatch.setattr(functions, "new_seed", lambda: 6000011)
    label = b["label"].to(dev)
    length = torch.clamp(O.output_length(b["waveform_len"], CS.HOP), 1, 125).to(dev)

    def by_hand(m):
        m.train()
        out = m(dict(inp))
        loss = FrameBceLoss()({"frame_sim": out["frame_sim"], "label": label, "length": length})
        loss.backward()
        return {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in m.named_parameters()}

    hand = by_hand(build(dev, gold))
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in hand.values())
    m = build(dev, gold)
    runner = StrongRunner(m, device=str(dev))
    loss = runner.forward_backward({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
    assert np.isfinite(runner.loss_value(loss))
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, hand[k]), k
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    loss = runner.train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
    assert np.isfinite(runner.loss_value(loss))
    assert all(not torch.equal(p.detach(), before[k]) for k, p in m.named_parameters())
    # a frozen conv weight, a frozen BatchNorm affine and a frozen text linear
    frozen = ["block3.conv.weight", "block2.bn.weight", "block4.fc_text.weight", "gru.weight_hh_l0"]
    mf = build(dev, gold)
    for k, p in mf.named_parameters():
        if k in frozen:
            p.requires_grad_(False)
    got = by_hand(mf)
    for k, g in got.items():
        if k in frozen:
            assert g is None, k
        else:
            assert g is not None and torch.equal(g, hand[k]), k


def test_frozen_conv_weight_launches_no_weight_gradient_conv(dev, golden_dir, monkeypatch):
    from texttoaudiogrounding_amd import functions
    gold = np.load(f"{golden_dir}/cross_cdur.npz")
    calls = []
    real = functions.conv3x3_wgrad
    monkeypatch.setattr(functions, "conv3x3_wgrad", lambda x, dy, **kw: calls.append(tuple(x.shape)) or real(x, dy, **kw))
    b = CS.train_batch()
    for freeze, n in ((False, 4), (True, 3)):
        m = build(dev, gold).train()
        m.block3.conv.weight.requires_grad_(not freeze)
        del calls[:]
        m(to_dev(b, dev))["frame_sim"].sum().backward()
        assert len(calls) == n, (freeze, calls)
        assert (m.block3.conv.weight.grad is None) == freeze


def test_operator_registration_and_real_call_matches_the_module(dev, golden_dir):
    import texttoaudiogrounding_amd.torch_ops as T
    from texttoaudiogrounding_amd import ops
    gold = np.load(f"{golden_dir}/cross_cdur.npz")
    assert "cross_cdur" in T.OP_NAMES
    m = build(dev, gold).eval()
    b = to_dev(CS.train_batch(), dev)
    with torch.no_grad():
        want = m(b)["frame_sim"]
        e = m.text_encoder(b)["seq_emb"]
    texts = [ops.LinearFunction.apply(e, blk.fc_text.weight, blk.fc_text.bias) for blk in m._blocks()]
    texts.append(ops.LinearFunction.apply(e, m.fc_text.weight, m.fc_text.bias))
    texts = [t.detach().requires_grad_(True) for t in texts]
    op = torch.ops.tag.cross_cdur
    tok = T.encoder_token(m)
    params = list(m._flat_params())
    got = op(b["waveform"], texts, params, tok, False)
    assert got.shape == (2, 25) and torch.equal(got, want)
    torch.library.opcheck(op, (b["waveform"], texts, params, tok, False), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(op, (b["waveform"], texts, params, tok, True), test_utils=("test_autograd_registration",))


@pytest.mark.parametrize("cin,cout,W", [(1, 32, 64), (32, 128, 16), (128, 128, 4)])
def test_cdur_text_block_standalone_vs_fp64(dev, cin, cout, W):
    from texttoaudiogrounding_amd.models.audio_text_model import CDurTextBlock
    g = torch.Generator().manual_seed(cin + W)
    torch.manual_seed(1)
    blk = CDurTextBlock(cin, cout, 48)
    with torch.no_grad():
        blk.bn.weight.uniform_(0.5, 1.5)
        blk.bn.bias.uniform_(-0.2, 0.2)
        blk.fc_text.bias.uniform_(-0.2, 0.2)
    blk = blk.to(dev).train()
    B, H = 3, 7
    x = torch.randn(B, cin, H, W, generator=g)
    text = torch.randn(B, 48, generator=g)
    st = _state(blk, torch.float64)
    x64, t64 = x.double().requires_grad_(cin > 1), text.double().requires_grad_(True)
    tb = F.linear(t64, st["fc_text.weight"], st["fc_text.bias"])[:, :, None, None]
    ref = F.leaky_relu(F.conv2d(O._bn(x64, st, "bn.", True), st["conv.weight"], None, 1, 1) + tb, 0.1)
    dout = torch.randn(ref.shape, generator=g)
    ref.backward(dout.double())
    xd, td = x.to(dev).requires_grad_(cin > 1), text.to(dev).requires_grad_(True)
    out = blk(xd, td)
    assert out.shape == ref.shape
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() <= 1e-5 * (1 + ref.abs().max().item())
    out.backward(dout.to(dev))
    bound = lambda r: 1e-4 * (1 + r.abs().max().item())
    pairs = [(td.grad, t64.grad)] + [(p.grad, st[k].grad) for k, p in blk.named_parameters()]
    if cin > 1:
        pairs.append((xd.grad, x64.grad))
    for got, want in pairs:
        assert (got.cpu().double() - want).abs().max().item() <= bound(want)
    assert int(blk.bn.num_batches_tracked) == 1
    assert np.allclose(blk.bn.running_var.cpu().numpy(), st["bn.running_var"].numpy(), rtol=2e-4, atol=1e-5)
