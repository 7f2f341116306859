"""GPU: the early-fusion CrossCnn8_Rnn (models/audio_text_model.py:571-840 in the reference) -- its per-clip bias kernels and heads
against float64 restatements, the whole model (train, SpecAugment, eval; three conv paths) against a float64 restatement of the
reference forward built from the model's own weights, freeze_cnn, StrongRunner, the operator's registration, the benched size,
the precision refusals and ConvTextBlock on its own."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tag_oracle as O
from tests.test_gpu_path import assert_grad_close

pytestmark = pytest.mark.gpu

POOLS = [(2, 2), (2, 2), (1, 2), (1, 2)]


def _bnstat(dispatch, y, gamma, beta, train):
    C = y.shape[-1]
    rm = torch.randn(C, device=y.device) * 0.1
    rv = torch.rand(C, device=y.device) + 0.5
    return dispatch.bn_stats(y.view(-1, C), gamma, beta, rm.clone(), rv.clone(), train), rm, rv


def _ref_bn(y64, gamma, beta, rm, rv, train):
    return F.batch_norm(y64.permute(0, 3, 1, 2), rm.double().clone(), rv.double().clone(), gamma.double(), beta.double(), train,
                        0.1, 1e-5).permute(0, 2, 3, 1)


def _ref_pool(a, ph, pw, pool):
    an = a.permute(0, 3, 1, 2)
    if pool == 2:
        o = F.avg_pool2d(an, (ph, pw))
    elif pool == 3:
        o = F.max_pool2d(an, (ph, pw))
    else:
        o = F.avg_pool2d(an, (ph, pw)) + F.max_pool2d(an, (ph, pw))
    return o.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("B,H,W,C,ph,pw,pool,train,drop", [
    (1, 7, 9, 64, 2, 2, 0, True, 0.0),
    (3, 5, 5, 128, 2, 2, 0, True, 0.2),
    (3, 9, 1, 512, 1, 1, 2, False, 0.0),
    (1, 1, 7, 64, 1, 2, 3, True, 0.2),
    (3, 11, 3, 512, 1, 2, 0, False, 0.2),
])
def test_bias_bnrelu_pool_site_vs_fp64(dev, B, H, W, C, ph, pw, pool, train, drop):
    """dropout(pool(relu(bn(y) + t))) and its backward (dy, dgamma, dbeta, per-clip sums) against float64 autograd."""
    from texttoaudiogrounding_amd import dispatch
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C)
    y = torch.randn(B, H, W, C, generator=g).to(dev)
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)).to(dev), (0.2 * torch.randn(C, generator=g)).to(dev)
    t = (0.5 * torch.randn(B, C, generator=g)).to(dev)
    st, rm, rv = _bnstat(dispatch, y, gamma, beta, train)
    seed = 1234
    out = dispatch.bias_bnrelu_pool(y, st, t, ph, pw, pool=pool, drop_p=drop, seed=seed)
    y64 = y.double().cpu().requires_grad_(True)
    t64 = t.double().cpu().requires_grad_(True)
    g64, b64 = gamma.double().cpu().requires_grad_(True), beta.double().cpu().requires_grad_(True)
    z = _ref_bn(y64, g64, b64, rm.cpu(), rv.cpu(), train) + t64[:, None, None, :]
    ref = _ref_pool(F.relu(z), ph, pw, pool)
    if drop > 0:
        m = dispatch.dropout_mask(seed, ref.shape, drop, dev, pooled=True).cpu().double()
        ref = ref * m / (1 - drop)
    assert out.shape == ref.shape
    assert (out.cpu().double() - ref).abs().max().item() <= 1e-5 * (1 + ref.abs().max().item())
    dout = torch.randn(ref.shape, generator=g)
    ref.backward(dout.double())
    dy, dg, db, clip = dispatch.bias_bnrelu_pool_backward(y, st, gamma, t, dout.to(dev), ph, pw, pool=pool, drop_p=drop, seed=seed)
    scale = lambda r: 1e-4 * (1 + r.abs().max().item())
    assert (dy.cpu().double() - y64.grad).abs().max().item() <= scale(y64.grad)
    assert (db.cpu().double() - b64.grad).abs().max().item() <= scale(b64.grad)
    assert (dg.cpu().double() - g64.grad).abs().max().item() <= scale(g64.grad)
    assert (clip[:, 0].cpu() - t64.grad).abs().max().item() <= scale(t64.grad)


@pytest.mark.parametrize("B,H,W,C,train", [(1, 5, 7, 64, True), (3, 3, 1, 128, False), (3, 7, 5, 512, True)])
def test_bias_bnrelu_site_vs_fp64_and_dt_deterministic(dev, B, H, W, C, train):
    """relu(bn(y) + t) written out, its backward, and dt = both sites' per-clip sums from one fold: against float64, and
    bitwise equal on a second run."""
    from texttoaudiogrounding_amd import dispatch
    g = torch.Generator().manual_seed(7 + C)
    y = torch.randn(B, H, W, C, generator=g).to(dev)
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)).to(dev), (0.2 * torch.randn(C, generator=g)).to(dev)
    t = (0.5 * torch.randn(B, C, generator=g)).to(dev)
    st, rm, rv = _bnstat(dispatch, y, gamma, beta, train)
    a = dispatch.bias_bnrelu_forward(y, st, t)
    y64 = y.double().cpu().requires_grad_(True)
    t64 = t.double().cpu().requires_grad_(True)
    g64, b64 = gamma.double().cpu().requires_grad_(True), beta.double().cpu().requires_grad_(True)
    ref = F.relu(_ref_bn(y64, g64, b64, rm.cpu(), rv.cpu(), train) + t64[:, None, None, :])
    assert (a.cpu().double() - ref).abs().max().item() <= 1e-5 * (1 + ref.abs().max().item())
    da = torch.randn(ref.shape, generator=g)
    ref.backward(da.double())
    prev = torch.randn(B, 2, C, generator=g, dtype=torch.float64).to(dev)
    runs = [dispatch.bias_bnrelu_backward(y, st, gamma, t, da.to(dev), prev=prev) for _ in range(2)]
    dy, dg, db, dt = runs[0]
    scale = lambda r: 1e-4 * (1 + r.abs().max().item())
    assert (dy.cpu().double() - y64.grad).abs().max().item() <= scale(y64.grad)
    assert (db.cpu().double() - b64.grad).abs().max().item() <= scale(b64.grad)
    assert (dg.cpu().double() - g64.grad).abs().max().item() <= scale(g64.grad)
    want = t64.grad + prev[:, 0].cpu()
    assert (dt.cpu().double() - want).abs().max().item() <= scale(want)
    for x0, x1 in zip(runs[0], runs[1]):
        assert torch.equal(x0, x1)


def test_heads_vs_fp64_with_clamp(dev):
    """fc1's row-group bias + ReLU and per-clip column sums; the frame head with logits far below the clamp (prob = 1e-7
    exactly, zero gradient there)."""
    from texttoaudiogrounding_amd import dispatch
    g = torch.Generator().manual_seed(11)
    B, T, N = 3, 13, 512
    x = torch.randn(B * T, N, generator=g).to(dev)
    u = torch.randn(B, N, generator=g).to(dev)
    h = dispatch.rowgroup_bias_relu(x, u, T)
    ref = F.relu(x.cpu().double().view(B, T, N) + u.cpu().double()[:, None]).view(B * T, N)
    assert (h.cpu().double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    grp, tot = dispatch.rowgroup_colsum(x, T)
    rg = x.cpu().double().view(B, T, N).sum(1)
    assert (grp.cpu().double() - rg).abs().max().item() <= 1e-5 and (tot.cpu().double() - rg.sum(0)).abs().max().item() <= 1e-5

    y = torch.randn(B * T, N, generator=g).to(dev)
    r = torch.randn(B, N, generator=g).to(dev)
    w = (torch.randn(N, generator=g) / 8).to(dev)
    b0 = torch.tensor([0.1]).to(dev)
    y[5] = -40 * w / (w * w).sum() * N / 8 - r[0]           # (y + r) . w far below -16: sigmoid < 1e-7
    prob, sig = dispatch.frame_head_forward(y, r, w, b0, T)
    y64 = y.cpu().double().requires_grad_(True)
    r64, w64, b64 = (v.cpu().double().requires_grad_(True) for v in (r, w, b0))
    logit = ((y64.view(B, T, N) + r64[:, None]) @ w64) + b64
    p64 = torch.sigmoid(logit).clamp(1e-7, 1.0).view(-1)
    assert prob[5].item() == np.float32(1e-7) and p64[5].item() == 1e-7
    assert (prob.cpu().double() - p64).abs().max().item() <= 1e-6
    dp = torch.randn(B * T, generator=g)
    p64.backward(dp.double())
    dy, dw, db0, dr = dispatch.frame_head_backward(y, r, w, sig, dp.to(dev), T)
    assert dy[5].abs().max().item() == 0.0 and y64.grad[5].abs().max().item() == 0.0
    for got, want in ((dy, y64.grad), (dw, w64.grad), (db0, b64.grad), (dr, r64.grad)):
        assert (got.cpu().double() - want).abs().max().item() <= 1e-5 * (1 + want.abs().max().item())


# ------------------------------------------------------------------------------------------------------------ whole model
def build(dev, seed=0, text_dim=256, vocab=300, **kw):
    from texttoaudiogrounding_amd.models import audio_text_model as M, text_encoder as TE
    torch.manual_seed(seed)
    m = M.CrossCnn8_Rnn(32000, TE.EmbeddingAgg(vocab, text_dim), **kw)
    with torch.no_grad():                                   # keep prob away from saturation
        m.fc_output.weight.mul_(0.3)
        m.rnn_text.weight.mul_(0.3)
        for i in range(1, 5):
            getattr(m, f"conv_block{i}").bn2.weight.uniform_(0.5, 1.5)
            getattr(m, f"conv_block{i}").bn2.bias.uniform_(-0.2, 0.2)
    m.dropout_p = (0.0, 0.0)
    return m.to(dev)


def batch(dev, B=4, seconds=1.5, vocab=300, seed=3):
    g = torch.Generator().manual_seed(seed)
    S = int(32000 * seconds)
    wave = 0.1 * torch.randn(B, S, generator=g)
    lens = [S - 4000 * i for i in range(B)]
    for i, n in enumerate(lens):
        wave[i, n:] = 0
    L = 6
    text = torch.randint(1, vocab, (B, L), generator=g)
    text_len = torch.tensor([L - i % 3 for i in range(B)])
    return {"waveform": wave.to(dev), "waveform_len": lens, "text": text.to(dev), "text_len": text_len.to(dev),
            "specaug": False}


def ref_forward(st, b, training, stripes=None, upsample=False):
    """The reference CrossCnn8_Rnn.forward (dropout off) in float64 on the CPU; st: the model's state dict (requires_grad
    leaves), running statistics updated in place."""
    e = O.embedding_agg_mean(st, b["text"].cpu(), b["text_len"].cpu(), prefix="text_encoder.")["seq_emb"]
    x = O.logmel(b["waveform"].cpu().to(e.dtype), "cnn8rnn")              # (B, 64, F)
    x = x.transpose(1, 2).unsqueeze(1).transpose(1, 3)
    x = O._bn(x, st, "bn0.", training).transpose(1, 3)                     # (B, 1, F, 64)
    if stripes is not None:
        keep = torch.ones_like(x)
        for bi in range(x.shape[0]):
            for k, (bgn, wd) in enumerate(stripes[bi].tolist()):
                if k < 2:
                    keep[bi, :, bgn:bgn + wd, :] = 0
                else:
                    keep[bi, :, :, bgn:bgn + wd] = 0
        x = x * keep
    for i, ps in enumerate(POOLS, start=1):
        p = f"conv_block{i}."
        t = F.linear(e, st[p + "fc_text.weight"], st[p + "fc_text.bias"])[:, :, None, None]
        x = F.relu(O._bn(F.conv2d(x, st[p + "conv1.weight"], None, 1, 1), st, p + "bn1.", training) + t)
        x = F.relu(O._bn(F.conv2d(x, st[p + "conv2.weight"], None, 1, 1), st, p + "bn2.", training) + t)
        x = F.avg_pool2d(x, ps) + F.max_pool2d(x, ps)
    x = x.mean(3).transpose(1, 2)
    x = F.relu(F.linear(x, st["fc1.weight"], st["fc1.bias"]) + F.linear(e, st["fc1_text.weight"], st["fc1_text.bias"])[:, None])
    x = O.gru_bidir(x, st, "rnn.") + F.linear(e, st["rnn_text.weight"], st["rnn_text.bias"])[:, None]
    prob = torch.sigmoid(F.linear(x, st["fc_output.weight"], st["fc_output.bias"])).clamp(1e-7, 1.0)
    if upsample:
        prob = F.interpolate(prob.transpose(1, 2), prob.shape[1] * 4, mode="linear", align_corners=False).transpose(1, 2)
    return prob


def _state(m, dtype):
    st = {k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu() for k, v in m.state_dict().items()}
    for k, _ in m.named_parameters():
        st[k].requires_grad_(True)
    return st


CONV_PATHS = ["default", "direct", "winograd"]


def _conv_path(ops, path):
    if path == "direct":
        return {"CONV_WINOGRAD": False}
    if path == "winograd":
        return {"WINO_MIN_WORK": 1}
    return {}


@pytest.mark.parametrize("path", CONV_PATHS)
@pytest.mark.parametrize("specaug", [False, True])
def test_train_step_vs_fp64(dev, path, specaug):
    from texttoaudiogrounding_amd import ops
    m = build(dev)
    m.train()
    b = batch(dev)
    b["specaug"] = specaug
    st64, st32 = _state(m, torch.float64), _state(m, torch.float32)
    old = {k: getattr(ops, k) for k in _conv_path(ops, path)}
    try:
        for k, v in _conv_path(ops, path).items():
            setattr(ops, k, v)
        torch.manual_seed(5)
        out = m(b)
        prob = out["frame_sim"]
        T = prob.shape[1]
        dprob = torch.randn(prob.shape, generator=torch.Generator().manual_seed(9))
        prob.backward(dprob.to(dev))
        torch.cuda.synchronize()
    finally:
        for k, v in old.items():
            setattr(ops, k, v)
    stripes = m._last_specaug if specaug else None
    ref = ref_forward(st64, b, True, stripes)
    ref32 = ref_forward(st32, b, True, stripes)
    assert prob.shape == ref.shape == (4, T, 1)
    assert (prob.cpu().double() - ref).abs().max().item() <= 1e-4
    assert torch.equal(out["length"], O.output_length(b["waveform_len"], 320))
    ref.backward(dprob.double())
    ref32.backward(dprob)
    for k, p in m.named_parameters():
        want = st64[k].grad
        scale = want.abs().max().item() + 1e-30
        err = (p.grad.cpu().double() - want).abs().max().item() / scale
        floor = (st32[k].grad.double() - want).abs().max().item() / scale
        if specaug and "conv_block" in k:
            # the zeroed stripes make runs of exactly equal activations: max-pool ties that any two fp32 convolutions (their
            # accumulation orders differ by tile position) break differently, each flip moving O(1e-2) of a gradient here
            assert err <= max(4.0 * floor, 3e-2), (k, err, floor)
        else:
            assert_grad_close(k, err, floor)
    for k, v in m.state_dict().items():
        if "running" in k:
            assert torch.allclose(v.cpu().double(), st64[k], rtol=2e-4, atol=1e-5), k


@pytest.mark.parametrize("path", CONV_PATHS)
def test_eval_vs_fp64_with_upsample_and_segments(dev, path):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils import eval_util
    m = build(dev, seed=1, upsample=True)
    b = batch(dev, seed=4)
    st64 = _state(m, torch.float64)
    m.eval()
    old = {k: getattr(ops, k) for k in _conv_path(ops, path)}
    try:
        for k, v in _conv_path(ops, path).items():
            setattr(ops, k, v)
        with torch.no_grad():
            out = m(b)
    finally:
        for k, v in old.items():
            setattr(ops, k, v)
    with torch.no_grad():
        ref = ref_forward(st64, b, False, upsample=True)
    prob = out["frame_sim"]
    assert prob.shape == ref.shape
    assert (prob.cpu().double() - ref).abs().max().item() <= 1e-4
    assert torch.equal(out["length"], O.output_length(b["waveform_len"], 320) * 4)
    lo, hi = float(ref.min()), float(ref.max())
    assert 1e-3 < lo and hi < 1 - 1e-3, (lo, hi)                     # not saturated
    # the binarised frames (hence every segment) agree at each of 50 thresholds whose margin to every reference frame is at
    # least the parity tolerance
    p = prob.squeeze(2).cpu().numpy()
    r = ref.squeeze(2).numpy()
    checked = 0
    for thr in np.linspace(0.01, 0.99, 50):
        if np.abs(r - thr).min() < 1e-4:
            continue
        assert ((p > thr) == (r > thr)).all(), thr
        checked += 1
    assert checked > 25


def test_freeze_cnn_only_rnn_gets_gradients(dev):
    b = batch(dev)
    grads = {}
    for freeze in (False, True):
        m = build(dev, freeze_cnn=freeze)
        m.train()
        prob = m(b)["frame_sim"]
        prob.backward(torch.randn(prob.shape, generator=torch.Generator().manual_seed(2)).to(dev))
        grads[freeze] = {k: (p.grad.clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    for k, g in grads[True].items():
        if k.startswith("rnn."):
            assert g is not None and torch.allclose(g, grads[False][k], rtol=1e-5, atol=1e-7), k
        else:
            assert g is None, k


def test_strong_runner_train_step_moves_every_parameter(dev):
    from texttoaudiogrounding_amd.runner import StrongRunner
    m = build(dev)
    m.dropout_p = (0.2, 0.5)
    b = batch(dev)
    T = (b["waveform"].shape[1] // 320 + 1) // 4
    b["label"] = (torch.rand(4, T, generator=torch.Generator().manual_seed(1)) > 0.5).float()
    b.pop("specaug")
    runner = StrongRunner(m, device=dev)
    before = {k: p.detach().clone() for k, p in runner.model.named_parameters()}
    loss = runner.train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
    assert np.isfinite(runner.loss_value(loss))
    for k, p in runner.model.named_parameters():
        assert p.requires_grad and not torch.equal(p.detach(), before[k]), k


def test_operator_opcheck(dev):
    import texttoaudiogrounding_amd.torch_ops as T
    from texttoaudiogrounding_amd import ops
    m = build(dev)
    m.train()
    B = 4
    wave = (0.1 * torch.randn(B, 48000, generator=torch.Generator().manual_seed(5))).to(dev)
    frames = 48000 // m.hop_length + 1
    e = torch.randn(B, 256, device=dev)
    texts = [ops.LinearFunction.apply(e, blk.fc_text.weight, blk.fc_text.bias) for blk in m._blocks()]
    texts += [ops.LinearFunction.apply(e, m.fc1_text.weight, m.fc1_text.bias),
              ops.LinearFunction.apply(e, m.rnn_text.weight, m.rnn_text.bias)]
    texts = [t.detach().requires_grad_(True) for t in texts]
    torch.manual_seed(0)
    stripes = m.spec_augmenter.draw(B, frames, 64).to(dev)
    op = torch.ops.tag.cross_cnn8rnn
    tok = T.encoder_token(m)
    params = list(m._flat_params())
    for extra in ((), (stripes,)):
        torch.library.opcheck(op, (wave, texts, params, tok, False, *extra), test_utils=("test_schema", "test_faketensor"))
        torch.library.opcheck(op, (wave, texts, params, tok, True, *extra), test_utils=("test_autograd_registration",))
        assert op(wave, texts, params, tok, False, *extra).shape == (B, frames // 4, 1)


def test_benched_size_steps(dev):
    """B = 64 x 10 s with EmbeddingAgg(5221, 512) and dropout on: finite (64, 250, 1) and no allocator growth over 5 steps."""
    m = build(dev, text_dim=512, vocab=5221)
    m.dropout_p = (0.2, 0.5)
    m.train()
    b = O.synthetic_batch(64, 320000, seed=99, ragged=True)
    inp = {"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"], "text": b["text"].to(dev),
           "text_len": torch.as_tensor(b["text_len"]).to(dev), "specaug": False}
    mem = []
    for step in range(5):
        m.zero_grad(set_to_none=False)
        prob = m(inp)["frame_sim"]
        assert prob.shape == (64, 250, 1)
        loss = prob.log().mean()
        loss.backward()
        assert torch.isfinite(prob).all() and torch.isfinite(loss)
        assert all(torch.isfinite(p.grad).all() for p in m.parameters())
        del prob, loss
        torch.cuda.synchronize()
        mem.append((torch.cuda.memory_allocated(), torch.cuda.memory_reserved()))
    print(f"allocated / reserved per step {[(a >> 20, r >> 20) for a, r in mem]} MiB")
    assert mem[1][1] == mem[4][1], mem


@pytest.mark.parametrize("setting", [("CONV_MATH", "x3"), ("ACT_DTYPE", "bf16")])
def test_precision_refusals(dev, setting):
    from texttoaudiogrounding_amd import ops
    m = build(dev)
    m.train()
    b = batch(dev)
    name, value = setting
    extra = {"CONV_MATH": "bf16"} if name == "ACT_DTYPE" else {}
    old = {k: getattr(ops, k) for k in [name, *extra]}
    try:
        for k, v in {name: value, **extra}.items():
            setattr(ops, k, v)
        with pytest.raises(RuntimeError, match="fp32"):
            m(b)
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


@pytest.mark.parametrize("cin,cout,ps,pool_type", [(1, 64, (2, 2), "avg+max"), (64, 128, (1, 2), "max"), (128, 64, (2, 2), "avg")])
def test_conv_text_block_standalone_vs_fp64(dev, cin, cout, ps, pool_type):
    from texttoaudiogrounding_amd.models.audio_text_model import ConvTextBlock
    torch.manual_seed(cin)
    blk = ConvTextBlock(cin, cout, 48).to(dev)
    blk.train()
    g = torch.Generator().manual_seed(cout)
    W = 64 if cin == 1 else 12
    x = torch.randn(3, cin, 9, W, generator=g).to(dev).requires_grad_(True)
    text = torch.randn(3, 48, generator=g).to(dev).requires_grad_(True)
    st = {k: v.detach().cpu().double().requires_grad_(v.requires_grad) for k, v in blk.named_parameters()}
    st.update({k: v.detach().cpu().double() for k, v in blk.named_buffers()})
    out = blk(x, text, pool_size=ps, pool_type=pool_type)
    x64, t64 = x.detach().cpu().double().requires_grad_(True), text.detach().cpu().double().requires_grad_(True)
    t = F.linear(t64, st["fc_text.weight"], st["fc_text.bias"])[:, :, None, None]
    a = F.relu(O._bn(F.conv2d(x64, st["conv1.weight"], None, 1, 1), st, "bn1.", True) + t)
    a = F.relu(O._bn(F.conv2d(a, st["conv2.weight"], None, 1, 1), st, "bn2.", True) + t)
    ref = {"avg+max": lambda v: F.avg_pool2d(v, ps) + F.max_pool2d(v, ps), "avg": lambda v: F.avg_pool2d(v, ps),
           "max": lambda v: F.max_pool2d(v, ps)}[pool_type](a)
    assert out.shape == ref.shape
    assert (out.detach().cpu().double() - ref).abs().max().item() <= 1e-4 * (1 + ref.abs().max().item())
    dout = torch.randn(ref.shape, generator=g)
    out.backward(dout.to(dev))
    ref.backward(dout.double())
    for got, want, name in [(x.grad, x64.grad, "x"), (text.grad, t64.grad, "text")] + [
            (p.grad, st[k].grad, k) for k, p in blk.named_parameters()]:
        err = (got.cpu().double() - want).abs().max().item() / (want.abs().max().item() + 1e-30)
        assert err <= 1e-3, (name, err)
    for k in ("bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var"):
        assert torch.allclose(getattr(blk, k.split(".")[0]).__getattr__(k.split(".")[1]).cpu().double(), st[k], rtol=2e-4,
                              atol=1e-5), k
