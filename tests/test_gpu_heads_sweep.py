"""csrc/heads.hip over its edge shapes: the seq-level match heads, the grouped weak-supervision head, every similarity reducer,
attention pooling, MaxMargin, FrameBceLoss, grad-norm / Adam and segment extraction, each against the fp64 statement of the same
operation in oracle/tag_oracle.py on the same seeded CPU inputs.  The shapes are the smallest that reach each branch of the
kernels: a D tail and every register slot, both match_bwd_kernel widths, the multi-chunk forward grid, all six
match_group_bwd_kernel instantiations (two of them at the 160 KiB LDS limit), T below / at / above one wave, one row, length 1,
lengths the kernels clamp, row counts that do not fill the last block, separate leading dimensions, and the second grid-stride
trip of the optimiser kernels.

Tolerances are the ones the project already asserts for these kernels with the max-normalised ``relerr``: 2e-6 forward (5e-6 for
the pooling outputs), 2e-5 gradients, exact for integers and for the determinism checks.  Every comparison also evaluates the
SAME oracle function in fp32 on the CPU and prints its distance from fp64 (the ``floor``) beside the measured error: the rule of
tests/test_gpu_path.py::assert_crnn_grad_close (bound = 4 x max(floor, 1e-6)) was kept ready for a case that the summation
order alone would push past its bound, and no case needed it -- the largest error measured is 2.5e-6 on a gradient (floor
2.1e-6), see docs/experiments_heads_sweep.md -- so every comparison asserts the plain bound.  Nothing is calibrated on the
kernels."""
import math

import numpy as np
import pytest
import torch

from oracle import tag_oracle as O

pytestmark = pytest.mark.gpu

FWD, POOL, GRAD = 2e-6, 5e-6, 2e-5


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


@pytest.fixture(scope="module")
def ops(dev):
    from texttoaudiogrounding_amd import ops as _ops
    from texttoaudiogrounding_amd import torch_ops  # noqa: F401  (registers torch.ops.tag.*)
    return _ops


def close(name, got, ref64, ref32, bound):
    """got (HIP) against ref64 within ``bound``; floor = the fp32 CPU oracle's own distance from ref64, printed for comparison.
    A reference that is zero to fp64 rounding (a gradient that vanishes identically, e.g. through F.normalize at D = 1) has no
    scale to normalise by: the same bound then holds for the absolute values (the inputs are of order one)."""
    got, ref64, ref32 = (torch.as_tensor(v).detach().double().cpu() for v in (got, ref64, ref32))
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    if ref64.abs().max().item() < 1e-12:
        err, floor, how = got.abs().max().item(), ref32.abs().max().item(), "abs (zero reference)"
    else:
        err, floor, how = relerr(got, ref64), relerr(ref32, ref64), "rel"
    print(f"  {name:58s} err {err:.2e}  fp32-oracle floor {floor:.2e}  bound {bound:.2e}  {how}")
    assert err <= bound, (name, err, floor, bound)


def leaf(t, dtype):
    """a fresh autograd leaf holding t's values (a copy: the shared inputs never start to require grad themselves)"""
    return t.detach().to(dtype, copy=True).requires_grad_(True)


# ------------------------------------------------------------------------------------------------ 1. seq-level match heads
# (B, T, D).  register slots = ceil(D / 64) of 16; D % 64 != 0 runs the `d < D` tail; T >= 32 takes match_bwd_kernel<8>, below
# that <4>; T > 16 gives the forward a grid of more than one frame chunk (B * chunks < 1024 here):
#   (1, 1, 1)       one lane of slot 0, <4>, 1 chunk, three of the four waves idle
#   (2, 5, 63)      slot 0 with a tail, <4>
#   (3, 17, 64)     slot 0 exactly full, <4>, 2 chunks (first multi-chunk forward)
#   (2, 31, 65)     slot 1 holds one lane, <4> at its largest T, 2 chunks
#   (2, 32, 300)    5 slots with a tail, <8> at its smallest T, 2 chunks
#   (5, 33, 512)    8 slots exactly, <8>, 4 chunks, T % 8 != 0
#   (2, 70, 1023)   all 16 slots with a one-lane tail, <8>, 8 chunks
#   (1, 250, 1024)  all 16 slots full (the D <= 1024 bound), <8>, 16 chunks (the cap), the runner's T
MATCH_SHAPES = [(1, 1, 1), (2, 5, 63), (3, 17, 64), (2, 31, 65), (2, 32, 300), (5, 33, 512), (2, 70, 1023), (1, 250, 1024)]
# (kind, l2norm, scale): kind 0 = DotProduct, 1 = ExpNegL2 (which has no scale)
MATCH_MODES = [(0, False, True), (0, True, False), (0, True, True), (0, False, False), (1, True, False), (1, False, False)]
# seed of a case = 100 * shape index + mode index, except where that draw misses the precondition below: at D = 1 F.normalize
# makes a scalar +-1, so ExpNegL2 is exactly 1 unless audio and text differ in sign (then e^-2)
MATCH_SEED = {(0, 4): 1007}


def match_inputs(B, T, D, kind, l2norm, scale, seed):
    """Conditioned so that a max-normalised error means something: every similarity in [0.02, 0.98] (asserted on the reference).
    ExpNegL2: audio = text + noise / sqrt(D) (distance about 1; plain randn would give e^-45 at D = 1024).  DotProduct: audio
    0.5 randn (logits about N(0, 1/4): no similarity near the clamp among thousands), and both operands times D^-1/4 where nothing
    else divides the logit by sqrt(D)."""
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(B, D, generator=g)
    noise = torch.randn(B, T, D, generator=g)
    if kind == 1:
        audio = text[:, None, :] + noise / math.sqrt(D)
    else:
        audio = 0.5 * noise
        if not scale and not l2norm:
            audio, text = audio * D ** -0.25, text * D ** -0.25
    return audio, text, torch.randn(B, T, generator=g)


def match_ref(audio, text, dsim, kind, l2norm, scale, dtype):
    a, t = leaf(audio, dtype), leaf(text, dtype)
    sim = O.match_dot_product(a, t, l2norm, scale) if kind == 0 else O.match_exp_neg_l2(a, t, l2norm)
    sim.backward(dsim.to(dtype))
    return sim.detach(), a.grad, t.grad


def match_case(si, mi):
    (B, T, D), (kind, l2norm, scale) = MATCH_SHAPES[si], MATCH_MODES[mi]
    seed = MATCH_SEED.get((si, mi), 100 * si + mi)
    return (B, T, D, kind, l2norm, scale), match_inputs(B, T, D, kind, l2norm, scale, seed)


@pytest.mark.parametrize("mi", range(len(MATCH_MODES)), ids=[f"kind{k}-l2{int(n)}-scale{int(s)}" for k, n, s in MATCH_MODES])
@pytest.mark.parametrize("si", range(len(MATCH_SHAPES)), ids=["x".join(map(str, s)) for s in MATCH_SHAPES])
def test_match_heads_sweep(ops, dev, si, mi):
    (B, T, D, kind, l2norm, scale), (audio, text, dsim) = match_case(si, mi)
    ref = match_ref(audio, text, dsim, kind, l2norm, scale, torch.float64)
    assert 0.02 <= ref[0].min().item() and ref[0].max().item() <= 0.98, "input precondition (not the kernel)"
    r32 = match_ref(audio, text, dsim, kind, l2norm, scale, torch.float32)
    a, t = leaf(audio.to(dev), torch.float32), leaf(text.to(dev), torch.float32)
    sim = torch.ops.tag.frame_match(a, t, kind, l2norm, scale)
    sim.backward(dsim.to(dev))
    tag = f"match ({B},{T},{D}) kind {kind} l2norm {int(l2norm)} scale {int(scale)}"
    close(tag + " sim", sim, ref[0], r32[0], FWD)
    close(tag + " daudio", a.grad, ref[1], r32[1], GRAD)
    close(tag + " dtext", t.grad, ref[2], r32[2], GRAD)


def test_match_dot_saturated_clamp_and_its_backward(ops, dev):
    """Logits of -30 / +30 / about N(0, 1/4) in turn along T: sigmoid(-30) = 9.4e-14 is clamped to 1e-7f and passes no gradient,
    sigmoid(+30) rounds to 1.0f.  (2, 33, 65): match_bwd_kernel<8>, a D tail."""
    B, T, D = 2, 33, 65
    g = torch.Generator().manual_seed(7)
    text = torch.randn(B, D, generator=g)
    unit = text / (text * text).sum(-1, keepdim=True) * math.sqrt(D)          # unit . text / sqrt(D) = 1
    audio = 0.5 * torch.randn(B, T, D, generator=g)
    low, high = torch.arange(T) % 3 == 0, torch.arange(T) % 3 == 1
    audio[:, low] = -30.0 * unit[:, None, :]
    audio[:, high] = 30.0 * unit[:, None, :]
    dsim = torch.randn(B, T, generator=g)
    ad, td = leaf(audio, torch.float64), leaf(text, torch.float64)
    prob = torch.sigmoid(O.match_dot_product(ad, td, False, True, return_logit=True)).detach()
    assert not ((prob >= 5e-8) & (prob <= 2e-7)).any(), "input precondition: no probability beside the clamp threshold"
    assert (prob[:, low] < 5e-8).all() and (prob[:, high] > 1 - 1e-9).all() and (prob[:, ~(low | high)] > 0.02).all()
    ref = O.match_dot_product(ad, td, False, True)
    ref.backward(dsim.double())
    r32 = match_ref(audio, text, dsim, 0, False, True, torch.float32)
    a, t = leaf(audio.to(dev), torch.float32), leaf(text.to(dev), torch.float32)
    sim = torch.ops.tag.frame_match(a, t, 0, False, True)
    sim.backward(dsim.to(dev))
    s = sim.detach().cpu()
    assert torch.equal(s[:, low], torch.full_like(s[:, low], 1e-7)) and torch.equal(s[:, high], torch.ones_like(s[:, high]))
    assert (a.grad.cpu()[prob < 5e-8] == 0).all()
    close("saturated sim", sim, ref, r32[0], FWD)
    close("saturated daudio", a.grad, ad.grad, r32[1], GRAD)
    close("saturated dtext", t.grad, td.grad, r32[2], GRAD)


@pytest.mark.parametrize("kind,l2norm", [(0, True), (1, False)])
def test_match_backward_is_deterministic(ops, dev, kind, l2norm):
    """The dtext reduction claims a fixed order (per-wave registers, then LDS rows 0..NW-1): two runs are bit-equal.  T = 70: <8>."""
    audio, text, dsim = (v.to(dev) for v in match_inputs(2, 70, 1023, kind, l2norm, True, 11))
    sim = ops.match_forward(audio, text, kind, l2norm, True)
    first = ops.match_backward(audio, text, sim, dsim, kind, l2norm, True)
    again = ops.match_backward(audio, text, sim, dsim, kind, l2norm, True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_match_rejects_d_above_1024(ops, dev):
    """tag_match_forward checks D <= 64 * 16 before its launch."""
    with pytest.raises(RuntimeError, match="argument check failed"):
        torch.ops.tag.frame_match(torch.zeros(1, 2, 1025, device=dev), torch.zeros(1, 1025, device=dev), 0, False, True)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. grouped head
# (B, N, T, D) -> match_group_bwd_kernel<NG, ND>: NG = 4 / 8 / 16 by N <= 4 / <= 8 / <= 16, ND = 8 / 16 by D <= 512 / > 512
#   (2, 1, 5, 64)     <4,8>    one phrase, D = one slot
#   (1, 4, 33, 65)    <4,8>    N at the top of its class, a D tail, T % 4 != 0
#   (1, 3, 9, 520)    <4,16>   first D above 512
#   (2, 5, 17, 512)   <8,8>    D at the top of its class
#   (1, 8, 9, 1024)   <8,16>   dynamic LDS 5 * 8 * 1024 * 4 = 163,840 B: exactly the 160 KiB a workgroup may have
#   (2, 9, 250, 300)  <16,8>   the runner's T
#   (1, 16, 9, 512)   <16,8>   N = MAXG, LDS exactly 160 KiB again
#   (1, 10, 7, 576)   <16,16>
GROUP_SHAPES = [(2, 1, 5, 64), (1, 4, 33, 65), (1, 3, 9, 520), (2, 5, 17, 512), (1, 8, 9, 1024), (2, 9, 250, 300), (1, 16, 9, 512),
                (1, 10, 7, 576)]


def group_inputs(B, N, T, D, scale, seed):
    g = torch.Generator().manual_seed(seed)
    audio, text = 0.5 * torch.randn(B, T, D, generator=g), torch.randn(B * N, D, generator=g)
    if not scale:
        audio, text = audio * D ** -0.25, text * D ** -0.25
    return audio, text, torch.randn(B * N, T, generator=g)


def group_ref(audio, text, dsim, N, scale, dtype):
    a, t = leaf(audio, dtype), leaf(text, dtype)
    B, T, D = a.shape
    sim = O.match_dot_product(a.unsqueeze(1).expand(-1, N, -1, -1).reshape(B * N, T, D), t, False, scale)   # as O.multitext_head
    sim.backward(dsim.to(dtype))
    return sim.detach(), a.grad, t.grad


@pytest.mark.parametrize("scale", [True, False])
@pytest.mark.parametrize("shape", GROUP_SHAPES, ids=["x".join(map(str, s)) for s in GROUP_SHAPES])
def test_match_group_sweep(ops, dev, shape, scale):
    B, N, T, D = shape
    audio, text, dsim = group_inputs(B, N, T, D, scale, 17 * D + N)
    ref = group_ref(audio, text, dsim, N, scale, torch.float64)
    assert 0.02 <= ref[0].min().item() and ref[0].max().item() <= 0.98, "input precondition (not the kernel)"
    r32 = group_ref(audio, text, dsim, N, scale, torch.float32)
    a, t = leaf(audio.to(dev), torch.float32), leaf(text.to(dev), torch.float32)
    sim = ops.MatchGroupFunction.apply(a, t, N, scale)
    sim.backward(dsim.to(dev))
    torch.cuda.synchronize()                                  # a launch the device refuses (LDS) shows here, in this case
    tag = f"group ({B},{N},{T},{D}) scale {int(scale)}"
    close(tag + " sim", sim, ref[0], r32[0], FWD)
    close(tag + " daudio", a.grad, ref[1], r32[1], GRAD)
    close(tag + " dtext", t.grad, ref[2], r32[2], GRAD)


@pytest.mark.parametrize("N,D", [(17, 64), (16, 520)])
def test_match_group_backward_rejects_before_launch(ops, dev, N, D):
    """tag_match_group_backward checks N <= MAXG = 16 and 5 * N * D * 4 <= 160 KiB ((16, 520): 166,400 B) before its launch; the
    forward has neither limit."""
    audio, text, dsim = group_inputs(1, N, 3, D, True, 3)
    a, t = leaf(audio.to(dev), torch.float32), leaf(text.to(dev), torch.float32)
    sim = ops.MatchGroupFunction.apply(a, t, N, True)
    with pytest.raises(RuntimeError, match="argument check failed"):
        sim.backward(dsim.to(dev))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. reducers
AMODES = ["mean", "max", "linear_softmax", "exp_softmax"]
TMODES = [None, "mean", "sum", "max", "mean_sum"]
# pair layout (B, B, T, N) -> R = B * B rows of one wave each, 4 rows per block, a_div = t_mod = B.  B = 4: whole blocks;
# B = 5: 25 rows, the last block has one.  T: 1 (one lane), 7, 64 (one full wave trip), 65 (a second trip of one lane), 130
# (three trips).  N = 1 and 5.  Lengths hold 1, T / N, a value above T / N (the kernels clamp) and one in between.
POOL_SHAPES = [(4, T, N) for T in (1, 7, 64, 65, 130) for N in (1, 5)] + [(5, 65, 5), (5, 7, 1)]


def pool_lens(B, T, N):
    al = torch.tensor([T, 1, T + 3, max(1, (T + 1) // 2), T][:B])
    tl = torch.tensor([1, N, N + 2, max(1, N // 2), N][:B])
    return al, tl


def _top2_gap(x, lens, dim):
    """smallest gap between the two largest valid entries along ``dim`` (valid: index < lens, lens per leading row)"""
    n = x.shape[dim]
    if n < 2:
        return float("inf")
    shape = [1] * x.ndim
    shape[dim] = n
    valid = torch.arange(n).view(shape) < lens.view([-1] + [1] * (x.ndim - 1))
    top = x.masked_fill(~valid, float("-inf")).topk(2, dim=dim).values
    gap = top.select(dim, 0) - top.select(dim, 1)
    return gap.min().item()


def pool_min_gap(sim, al, tl, am, tm):
    """The max reducers pick an argument: fp32 picks the reference's as long as its top two differ by more than fp32 rounding."""
    B, _, T, N = sim.shape
    x = sim.double().reshape(B * B, T, N)
    alr = al.clamp(max=T).repeat_interleave(B)
    gap = _top2_gap(x, alr, 1) if am == "max" else float("inf")
    if tm == "max":
        gap = min(gap, _top2_gap(O.SEQ_POOL[am](x, alr), tl.clamp(max=N).repeat(B), 1))
    return gap


def pool_inputs(B, T, N, am, tm, seed):
    """rand * 0.98 + 0.01; the draw is repeated with the next seed until the max reducers' top-two gap exceeds 1e-4"""
    al, tl = pool_lens(B, T, N)
    for s in range(seed, seed + 64):
        g = torch.Generator().manual_seed(s)
        sim = torch.rand(B, B, T, N, generator=g) * 0.98 + 0.01
        if pool_min_gap(sim, al, tl, am, tm) > 1e-4:
            break
    dout = torch.randn(B * B, N, generator=g) if tm is None else torch.randn(B, B, generator=g)
    return sim, al, tl, dout


def pool_ref(sim, al, tl, dout, am, tm, dtype):
    """The oracle takes the lengths as its callers pass them, never above the axis: the kernels' clamp is applied here."""
    B, _, T, N = sim.shape
    s = leaf(sim, dtype)
    alc, tlc = al.clamp(max=T), tl.clamp(max=N)
    if tm is None:
        out = O.SEQ_POOL[am](s.reshape(B * B, T, N), alc.repeat_interleave(B))
    else:
        out = O.sim_pooling(s, alc, tlc, am, tm)
    out.backward(dout.to(dtype))
    return out.detach(), s.grad.reshape(B * B, T, N)


@pytest.mark.parametrize("tm", TMODES, ids=[f"text-{m}" for m in TMODES])
@pytest.mark.parametrize("am", AMODES)
def test_sim_pool_sweep(ops, dev, am, tm):
    for B, T, N in POOL_SHAPES:
        sim, al, tl, dout = pool_inputs(B, T, N, am, tm, 1000 * T + 10 * N + B)
        assert pool_min_gap(sim, al, tl, am, tm) > 1e-4, "input precondition (not the kernel)"
        ref, r32 = pool_ref(sim, al, tl, dout, am, tm, torch.float64), pool_ref(sim, al, tl, dout, am, tm, torch.float32)
        s = leaf(sim.reshape(B * B, T, N).to(dev), torch.float32)
        if tm is None:
            out = ops.SimPoolFunction.apply(s, al.to(dev), None, B, 1, ops.POOL_MODES[am], -1)
        else:
            out = ops.SimPoolFunction.apply(s, al.to(dev), tl.to(dev), B, B, ops.POOL_MODES[am], ops.TEXT_MODES[tm]).view(B, B)
        out.backward(dout.to(dev))
        tag = f"sim_pool {am}/{tm} B {B} T {T} N {N}"
        close(tag + " out", out, ref[0], r32[0], POOL)
        close(tag + " dsim (whole tensor)", s.grad, ref[1], r32[1], GRAD)


@pytest.mark.parametrize("group", [1, 3])
def test_linear_softmax_pool_sweep(ops, dev, group):
    for T in (1, 63, 64, 65):
        g = torch.Generator().manual_seed(40 + T)
        length = torch.tensor([1, T, T + 5])
        fs = torch.rand(3 * group, T, generator=g) * 0.98 + 0.01
        dclip = torch.randn(3 * group, generator=g)
        refs = []
        for dtype in (torch.float64, torch.float32):
            f = leaf(fs, dtype)
            clip = O.linear_softmax_with_lens(f, length.repeat_interleave(group))
            clip.backward(dclip.to(dtype))
            refs.append((clip.detach(), f.grad))
        f = leaf(fs.to(dev), torch.float32)
        clip = ops.LinearSoftmaxPoolFunction.apply(f, length.to(dev), group)
        clip.backward(dclip.to(dev))
        close(f"linsoftmax group {group} T {T} clip", clip, refs[0][0], refs[1][0], POOL)
        close(f"linsoftmax group {group} T {T} dfs (whole tensor)", f.grad, refs[0][1], refs[1][1], GRAD)


@pytest.mark.parametrize("B", [1, 5])
def test_meanmean_pool_sweep(ops, dev, B):
    for T, N in ((1, 1), (13, 1), (65, 6)):
        g = torch.Generator().manual_seed(60 + T + B)
        sim = torch.rand(B, B, T, N, generator=g) * 0.98 + 0.01
        dout = torch.randn(B, B, generator=g)
        al, tl = (torch.tensor([T], dtype=torch.long), torch.tensor([N], dtype=torch.long)) if B == 1 else pool_lens(B, T, N)
        refs = []
        for dtype in (torch.float64, torch.float32):
            s = leaf(sim, dtype)
            out = O.audio_mean_text_mean(s, al.clamp(max=T), tl.clamp(max=N))         # the kernel clamps, the oracle's callers do
            out.backward(dout.to(dtype))
            refs.append((out.detach(), s.grad))
        s = leaf(sim.to(dev), torch.float32)
        out = ops.MeanMeanPoolFunction.apply(s, al.to(dev), tl.to(dev))
        out.backward(dout.to(dev))
        close(f"meanmean B {B} T {T} N {N} out", out, refs[0][0], refs[1][0], POOL)
        close(f"meanmean B {B} T {T} N {N} dsim (whole tensor)", s.grad, refs[0][1], refs[1][1], GRAD)


@pytest.mark.parametrize("B,L,D,lens", [(1, 1, 1, [1]), (5, 4, 65, [4, 1, 2, 3, 4]), (6, 7, 300, [7, 1, 3, 5, 2, 7]),
                                        (3, 2, 1024, [2, 1, 2])])
def test_attention_pooling_sweep(ops, dev, B, L, D, lens):
    """One wave per phrase, 4 per block: B = 1, 5, 6, 3 leave the last block part-filled; D = 1024 fills all 16 register slots.
    db vanishes identically (softmax ignores a common shift), so it is compared in absolute terms as the golden test does."""
    g = torch.Generator().manual_seed(80 + D)
    x, w, b = torch.randn(B, L, D, generator=g), torch.randn(1, D, generator=g) / math.sqrt(D), torch.randn(1, generator=g)
    dout, lens = torch.randn(B, D, generator=g), torch.tensor(lens)
    refs = []
    for dtype in (torch.float64, torch.float32):
        xs, ws, bs = leaf(x, dtype), leaf(w, dtype), leaf(b, dtype)
        out = O.attention_pooling(xs, lens, ws, bs)
        out.backward(dout.to(dtype))
        refs.append((out.detach(), xs.grad, ws.grad, bs.grad))
    xs, ws, bs = (leaf(v.to(dev), torch.float32) for v in (x, w, b))
    out = ops.AttnPoolFunction.apply(xs, lens.to(dev), ws, bs)
    out.backward(dout.to(dev))
    tag = f"attnpool ({B},{L},{D})"
    close(tag + " out", out, refs[0][0], refs[1][0], POOL)
    close(tag + " dx", xs.grad, refs[0][1], refs[1][1], GRAD)
    close(tag + " dw", ws.grad, refs[0][2], refs[1][2], GRAD)
    db, db_ref = bs.grad.reshape(-1)[0].item(), refs[0][3].reshape(-1)[0].item()
    print(f"  {tag} db {db:.2e} (reference {db_ref:.2e})")
    assert abs(db - db_ref) < 1e-5


def maxmargin_min_hinge(x, margin, lam, fix_norm):
    n = x.shape[0]
    x = x.double()
    d = torch.diag(x).view(-1, 1)
    keep = ~torch.eye(n, dtype=torch.bool) if fix_norm else torch.ones(n, n, dtype=torch.bool)
    return min((margin - (d - x))[keep].abs().min().item(), (margin - (d - lam * x.t()))[keep].abs().min().item())


@pytest.mark.parametrize("n", [2, 3, 64, 65, 257])
def test_maxmargin_sweep(ops, dev, n):
    """n = 2 (the smallest the entry point takes), 3, 64 / 65 (one wave trip / a second of one lane; 16 and 17 blocks of 4 rows),
    257 (more elements than the forward's 256 threads visit in 256 trips; 65 blocks, the last with one row).  0.7 randn puts
    hinges on both sides of zero; the draw is repeated with the next seed until no hinge argument is within 1e-5 of it."""
    for fix_norm in (True, False):
        for margin, lam in ((1.0, 1.0), (1.0, 0.5), (0.2, 1.0), (0.2, 0.5)):
            for seed in range(n, n + 64):
                x = 0.7 * torch.randn(n, n, generator=torch.Generator().manual_seed(seed))
                if maxmargin_min_hinge(x, margin, lam, fix_norm) > 1e-5:
                    break
            assert maxmargin_min_hinge(x, margin, lam, fix_norm) > 1e-5, "input precondition (not the kernel)"
            refs = []
            for dtype in (torch.float64, torch.float32):
                xs = leaf(x, dtype)
                loss = O.max_margin_ranking_loss(xs, margin, lam, fix_norm)
                (1.3 * loss).backward()
                refs.append((loss.detach(), xs.grad))
            xs = leaf(x.to(dev), torch.float32)
            loss = ops.MaxMarginFunction.apply(xs, margin, lam, fix_norm)
            (1.3 * loss).backward()
            tag = f"maxmargin n {n} fix_norm {int(fix_norm)} margin {margin} lamda1 {lam}"
            close(tag + " loss", loss, refs[0][0], refs[1][0], FWD)
            close(tag + " dx", xs.grad, refs[0][1], refs[1][1], GRAD)


# ------------------------------------------------------------------------------------------------ 4. frame_bce
# (B, ld_sim, ld_label, Tt, first length of the cycle): the three extents differ; ld_sim > Tt leaves columns the backward must
# zero; B = 300 makes the backward's 256-thread `den` loop take a second trip; (64, 250, 251, 250) is the runner's shape with
# the label one frame longer.  Lengths cycle through 0 and Tt + 3 (clamped to 1 and Tt), 1, Tt and a value in between.
BCE_SHAPES = [(1, 1, 1, 1, 0), (3, 13, 11, 11, 0), (3, 11, 13, 11, 2), (300, 9, 8, 7, 0), (64, 250, 251, 250, 0)]


@pytest.mark.parametrize("B,ld_sim,ld_label,Tt,first", BCE_SHAPES, ids=["x".join(map(str, s[:4])) for s in BCE_SHAPES])
def test_frame_bce_separate_extents(ops, dev, B, ld_sim, ld_label, Tt, first):
    g = torch.Generator().manual_seed(100 + B + Tt)
    sim = torch.rand(B, ld_sim, generator=g) * 0.98 + 0.01
    label = (torch.rand(B, ld_label, generator=g) > 0.5).float()
    cycle = [0, Tt + 3, 1, Tt, max(1, Tt // 2)]
    length = torch.tensor([cycle[(first + i) % 5] for i in range(B)])
    dloss = 0.7
    refs = []
    for dtype in (torch.float64, torch.float32):
        s = leaf(sim, dtype)
        loss = O.frame_bce_loss(s[:, :Tt], label[:, :Tt].to(dtype), length.clamp(1, Tt))
        (dloss * loss).backward()
        refs.append((loss.detach(), s.grad))                                     # zero in the columns Tt .. ld_sim - 1
    s, lab, ln = sim.to(dev), label.to(dev), length.to(dev)
    loss = ops.frame_bce_forward(s, lab, ln, Tt)
    ds = ops.frame_bce_backward(s, lab, ln, Tt, torch.tensor(dloss, device=dev))
    tag = f"frame_bce ({B},{ld_sim},{ld_label},{Tt})"
    close(tag + " loss", loss, refs[0][0], refs[1][0], FWD)
    close(tag + " dsim (full width)", ds, refs[0][1], refs[1][1], 1e-5)          # 1e-5: what test_frame_bce asserts for it


# ------------------------------------------------------------------------------------------------ 5. optimiser
@pytest.mark.parametrize("n", [1, 255, 257, 4097, 1024 * 16 * 256 + 1001])
def test_grad_sumsq_sizes(ops, dev, n):
    """1 element; one block short of / past 256 threads; a second block (4096 elements each); 1001 past the 1024 x 16 x 256
    elements the capped grid covers in 16 trips, so some threads take a 17th."""
    gr = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
    want = float((gr.double() ** 2).sum())
    got = ops.grad_sumsq(gr.to(dev)).item()
    print(f"  grad_sumsq n {n}: rel err {abs(got - want) / want:.2e}")
    assert abs(got - want) / want < 1e-10


def _adam_reference(p0, grads, max_norm, grad_scale):
    pr = p0.clone().double().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3)
    for gr in grads:
        pr.grad = gr.double() * grad_scale
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pr], max_norm)
        opt.step()
    return pr.detach()


def _adam_inputs(n, gain, seed):
    """Parameters uniform in (-1, 1): their fp32 storage rounds by at most 6e-8 per step, so the 1e-6 bound on the difference
    from the fp64 optimiser measures the update arithmetic and not the width of a float at |p| > 4."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) * 2 - 1, [torch.randn(n, generator=g) * gain * (i + 1) for i in range(3)]


def test_adam_three_steps_past_the_grid_cap(ops, dev):
    """n = 4096 * 256 + 777: the grid is capped at 4096 blocks, 777 threads take a second trip.  Gradient norms 10 .. 30: clipped."""
    n = 4096 * 256 + 777
    p0, grads = _adam_inputs(n, 0.01, 5)
    want = _adam_reference(p0, grads, 1.0, 1.0)
    p, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for i, gr in enumerate(grads):
        gd = gr.to(dev)
        ops.adam_step(p, gd, m, v, 1e-3, 0.9, 0.999, 1e-8, i + 1, ops.grad_sumsq(gd), 1.0, 1.0)
    err = (p.cpu().double() - want).abs().max().item()
    print(f"  adam n {n}: max abs parameter difference {err:.2e}")
    assert err < 1e-6


@pytest.mark.parametrize("case", ["max_norm_0", "no_gnorm", "grad_scale"])
def test_adam_clip_switches(ops, dev, case):
    """max_norm = 0 and gnorm_sq = None both mean no clipping (the reference: no clip_grad_norm_); grad_scale = 0.125 is the
    data-parallel average, and the clip then acts on the scaled gradient (norms 4 .. 12 after scaling: clipped)."""
    n = 1000
    p0, grads = _adam_inputs(n, 1.0, 6)
    max_norm, grad_scale, with_gnorm, ref_norm = {"max_norm_0": (0.0, 1.0, True, 0.0), "no_gnorm": (1.0, 1.0, False, 0.0),
                                                  "grad_scale": (1.0, 0.125, True, 1.0)}[case]
    want = _adam_reference(p0, grads, ref_norm, grad_scale)
    p, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for i, gr in enumerate(grads):
        gd = gr.to(dev)
        ops.adam_step(p, gd, m, v, 1e-3, 0.9, 0.999, 1e-8, i + 1, ops.grad_sumsq(gd) if with_gnorm else None, max_norm, grad_scale)
    err = (p.cpu().double() - want).abs().max().item()
    print(f"  adam {case}: max abs parameter difference {err:.2e}")
    assert err < 1e-6


# ------------------------------------------------------------------------------------------------ 6. segments
@pytest.mark.parametrize("T", [1, 2, 3, 5, 64, 65])
def test_segments_tiny_rows_and_ties(ops, dev, T):
    """Rows shorter than the median window (window // 2 > T: the reflection wraps more than once), n_connect = 0, and two
    thresholds that test the strict `>` in double: one EQUAL to a float32 score of every row (not above it) and the double just
    below that score (above it in double, equal after rounding to float).  B * NT = 35 work items: one part-filled block."""
    B = 5
    x = torch.rand(B, T, generator=torch.Generator().manual_seed(200 + T))
    x[:, T // 2] = x[0, T // 2]
    tie = float(x[0, T // 2].item())
    th = np.array([0.05, 0.25, np.nextafter(tie, 0.0), tie, 0.55, 0.75, 0.95], dtype=np.float64)
    xd, xn = x.to(dev), x.numpy()
    for window in (1, 2, 3, 4, 5, 9, 25):
        for n_connect in (0, 1, 13):
            regions, counts = ops.segments(xd, th, window, n_connect)
            regions, counts = regions.cpu().numpy(), counts.cpu().numpy()
            for b in range(B):
                for ti in range(len(th)):
                    want = O.segments(xn[b], th[ti], window, n_connect)
                    assert np.array_equal(regions[b, ti, :counts[b, ti]], want), (T, window, n_connect, b, ti)
