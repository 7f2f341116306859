"""The CPU helpers of the bn_pool.hip sweep (tests/bnpool_ref.py) against torch itself: a reference that is wrong would make
the GPU sweep assert the wrong thing."""
import pytest
import torch
import torch.nn.functional as F

from tests import bnpool_ref as R


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / (b.double().abs().max().item() + 1e-30)


@pytest.mark.parametrize("P,C,big", [(1, 4, 0), (63, 20, 0), (65, 64, 0), (16385, 4, 8)])
def test_partial_rows_and_chan_merge_reproduce_the_moments(P, C, big):
    """synth_partials + chan_merge == the direct fp64 mean and variance of the tensor, with channel means up to 50 sigma, empty
    rows full of garbage and a fp32-rounded pivot per tile (the merge is exact algebra; what remains is the fp32 storage of r, q)"""
    cnt = R.tile_counts(P, seed=P + C, big_every=big)
    assert int(cnt[0]) > 0 and (P < 16 or int((cnt == 0).sum()) > 0) and int(cnt.max()) <= 64
    N = int(cnt.sum())
    g = torch.Generator().manual_seed(P)
    sigma = torch.rand(C, generator=g) + 0.5
    x = torch.randn(N, C, generator=g) * sigma + torch.linspace(-50, 50, C) * sigma
    flat = R.synth_partials(x, cnt, seed=3)
    assert flat.dtype == torch.float32 and flat.numel() == P * 3 * C + P and torch.isfinite(flat).all()
    mean, var, n = R.chan_merge(flat, P, C)
    m, v, _ = R.bn_moments(x.double())
    assert n == N
    assert rel(mean, m) < 1e-9
    if N > 1:
        assert ((var - v).abs() / v.clamp_min(1e-30)).max().item() < 1e-6       # per channel, not max-normalised


@pytest.mark.parametrize("rows", [2, 9, 130])
def test_written_out_batchnorm_is_torchs(rows):
    g = torch.Generator().manual_seed(rows)
    C = 8
    x = (torch.randn(rows, C, generator=g) * 2 - 3).double()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).double(), torch.randn(C, generator=g).double()
    rm, rv = torch.randn(C, generator=g).double(), (torch.rand(C, generator=g) + 0.5).double()
    xa, ga, ba = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    xb, gb, bb = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    rm_t, rv_t = rm.clone(), rv.clone()
    want = F.batch_norm(xa, rm_t, rv_t, ga, ba, True, 0.1, R.EPS)
    got = R.bn_train(xb, gb, bb)
    dout = torch.randn(rows, C, generator=g).double()
    want.backward(dout)
    got.backward(dout)
    assert rel(got, want) < 1e-12 and rel(xb.grad, xa.grad) < 1e-10 and rel(gb.grad, ga.grad) < 1e-12 and rel(bb.grad, ba.grad) < 1e-12
    st = R.stats_outputs(x, gamma, beta, rm, rv)
    assert rel(st["rm"], rm_t) < 1e-12 and rel(st["rv"], rv_t) < 1e-12
    inv = 1 / torch.sqrt(x.var(0, unbiased=False) + R.EPS)
    assert rel(st["invstd"], inv) < 1e-12 and rel(st["scale"], gamma * inv) < 1e-12
    assert rel(st["shift"], beta - x.mean(0) * gamma * inv) < 1e-12
    ev = F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, R.EPS)
    assert rel(R.bn_eval(x, rm, 1 / torch.sqrt(rv + R.EPS), gamma, beta), ev) < 1e-12


def test_one_row_batchnorm_reference():
    """rows = 1 (torch raises): var 0, invstd = eps^-1/2, the output is beta, running_var takes the BIASED value (0), and the
    gradient with respect to the input vanishes"""
    x = torch.tensor([[1.5, -2.0, 0.25, 7.0]], dtype=torch.float64, requires_grad=True)
    gamma, beta = torch.full((4,), 2.0, dtype=torch.float64), torch.arange(4.0, dtype=torch.float64)
    with pytest.raises(ValueError):
        F.batch_norm(x.detach().view(1, 4), None, None, gamma, beta, True, 0.1, R.EPS)
    st = R.stats_outputs(x.detach(), gamma, beta, torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64))
    assert torch.equal(st["mean"], x.detach()[0]) and rel(st["invstd"], torch.full((4,), R.EPS ** -0.5, dtype=torch.float64)) < 1e-12
    assert rel(st["rv"], torch.full((4,), 0.9, dtype=torch.float64)) < 1e-15 and rel(st["rm"], 0.1 * x.detach()[0]) < 1e-15
    out = R.bn_train(x, gamma, beta)
    out.backward(torch.ones(1, 4, dtype=torch.float64))
    assert torch.equal(out.detach()[0], beta) and (x.grad == 0).all()
    m, var, inv = R.stats_one_pass_fp32_squares(x.detach().float())
    assert (var == 0).all() and rel(m, x.detach()[0]) < 1e-12


@pytest.mark.parametrize("ph,pw,H,W", [(2, 4, 5, 7), (1, 4, 3, 8), (2, 2, 4, 5)])
def test_written_out_lppool_gradient_is_torchs_where_torch_defines_it(ph, pw, H, W):
    g = torch.Generator().manual_seed(H * W)
    y = torch.randn(2, 3, H, W, generator=g).double()
    dout = torch.randn(2, 3, H // ph, W // pw, generator=g).double()
    ya = y.clone().requires_grad_(True)
    F.lp_pool2d(F.leaky_relu(ya, 0.1), 4.0, (ph, pw)).backward(dout)
    assert rel(R.lppool_leaky_backward_ref(y, dout, ph, pw), ya.grad) < 1e-8      # torch's own pow(1/4) rounds differently
    assert rel(R.pool_ref(F.leaky_relu(y, 0.1), ph, pw, 1), R.windows(F.leaky_relu(y, 0.1), ph, pw).pow(4).sum(-1).pow(0.25)) < 1e-12
    # an all-zero window: torch's gradient is NaN or zero there (by version), the written-out one is zero; the other windows agree
    y[0, 1, :ph, :pw] = 0.0
    ya = y.clone().requires_grad_(True)
    F.lp_pool2d(F.leaky_relu(ya, 0.1), 4.0, (ph, pw)).backward(dout)
    ref = R.lppool_leaky_backward_ref(y, dout, ph, pw)
    g0 = ya.grad[0, 1, :ph, :pw]
    assert (torch.isnan(g0) | (g0 == 0)).all() and (ref[0, 1, :ph, :pw] == 0).all() and torch.isfinite(ref).all()
    ok = torch.isfinite(ya.grad)
    assert rel(ref[ok], ya.grad[ok]) < 1e-8
    assert (ref[:, :, (H // ph) * ph:] == 0).all() and (ref[:, :, :, (W // pw) * pw:] == 0).all()


def test_frame_head_reference_is_autograd_of_the_clamped_sigmoid():
    """with sig = sigmoid(logit) stored in fp64 the written-out gate is torch's clamp gradient"""
    g = torch.Generator().manual_seed(1)
    B, T, N = 2, 5, 4
    y, rb = torch.randn(B, T, N, generator=g).double(), torch.randn(B, N, generator=g).double()
    w, dprob = torch.randn(N, generator=g).double(), torch.randn(B, T, generator=g).double()
    ya, ra, wa, b0 = y.clone().requires_grad_(True), rb.clone().requires_grad_(True), w.clone().requires_grad_(True), \
        torch.zeros((), dtype=torch.float64, requires_grad=True)
    sig = torch.sigmoid(((ya + ra.unsqueeze(1)) * wa).sum(-1) + b0)
    sig.clamp(1e-7, 1.0).backward(dprob)
    dy, dw, db0, drb, clip = R.frame_head_backward_ref(y, rb, w, sig.detach(), dprob)
    assert rel(dy, ya.grad) < 1e-12 and rel(dw, wa.grad) < 1e-12 and rel(drb, ra.grad) < 1e-12
    assert abs(db0.item() - b0.grad.item()) < 1e-12 and rel(clip[:, 0].sum(0), wa.grad) < 1e-12
    # the gate: below float32(1e-7) and above 1 nothing passes; at exactly 1 the factor (1 - sig) is zero
    s = torch.tensor([[5e-8, 2e-7, 1.0, 0.5, float(torch.tensor(1e-7, dtype=torch.float32))]], dtype=torch.float64)
    dl = R.frame_head_backward_ref(torch.zeros(1, 5, 4, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64),
                                   torch.ones(4, dtype=torch.float64), s, torch.ones(1, 5, dtype=torch.float64))[0][0, :, 0]
    assert dl[0] == 0 and dl[1] > 0 and dl[2] == 0 and dl[3] == 0.25 and dl[4] > 0


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("ph,pw", [(2, 2), (1, 2), (2, 1), (1, 1)])
def test_repair_leaves_no_decision_within_the_margin(ph, pw, bf16):
    """random draws DO contain violations (asserted), the repaired tensor has none, stays bf16-representable when asked, and
    differs from the draw only at a handful of elements"""
    g = torch.Generator().manual_seed(10 * ph + pw)
    B, C, H, W = 3, 64, 3 * ph + (ph - 1), 5 * pw + (pw - 1)
    y = torch.randn(B, C, H, W, generator=g).double()
    if ph * pw > 1:
        y[1, 2, 0, 0] = 2.0
        y[1, 2, ph - 1, pw - 1] = 2.0                        # planted: an exact tie of a window maximum
    if bf16:
        y = R.bf16r(y)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).double().view(1, C, 1, 1), (0.2 * torch.randn(C, generator=g)).double().view(1, C, 1, 1)

    def affine(t):                                           # training BatchNorm: the statistics move with the repair
        m = t.mean((0, 2, 3), keepdim=True)
        inv = 1 / torch.sqrt(t.var((0, 2, 3), unbiased=False, keepdim=True) + R.EPS)
        return (t - m) * inv * gamma + beta, gamma * inv

    for _ in range(8):                                       # planted: a pre-activation at zero (the statistics move with it)
        a, slope = affine(y)
        y[0, 0, 0, 0] -= (a / slope.expand_as(a))[0, 0, 0, 0]
        if bf16:
            y = R.bf16r(y)
    near, run = R.decision_violations(affine(y)[0], ph, pw)
    assert (bf16 or near.any()) and (ph * pw == 1 or run.any())      # (a bf16 step of y is wider than the margin)
    fixed = R.repair(y, affine, ph, pw, bf16=bf16)
    near, run = R.decision_violations(affine(fixed)[0], ph, pw)
    assert not near.any() and not run.any()
    assert (fixed != y).sum().item() < y.numel() // 100
    if bf16:
        assert torch.equal(R.bf16r(fixed), fixed)


def test_bf16_bounds_accept_correct_rounding_and_refuse_a_neighbour():
    g = torch.Generator().manual_seed(2)
    ref = torch.randn(4096, generator=g).double() * torch.logspace(-1, 0, 4096, dtype=torch.float64)
    one, half, safe = R.bf16_bounds(ref)
    good = ref.float().bfloat16().double()
    err = (good - ref).abs()
    assert (err <= one).all() and (err[safe] <= half[safe]).all() and safe.float().mean() > 0.9
    assert torch.equal(R.bf16_ulp(torch.tensor([1.0, 1.5, 2.0, 0.75])), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]))
    big = ref.abs() > 1e-2 * ref.abs().max()                  # where the delta floor is far below an ulp
    worse = good + R.bf16_ulp(good) * torch.where(good >= ref, 1.0, -1.0)          # one bf16 step further from the reference
    assert ((worse - ref).abs()[big & safe] > half[big & safe]).all()
    assert ((worse + R.bf16_ulp(good) * torch.where(good >= ref, 1.0, -1.0) - ref).abs()[big] > one[big]).all()
