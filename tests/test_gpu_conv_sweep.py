"""csrc/conv.hip and csrc/conv_c1.hip over their edge shapes, every entry point called through the C ABI (ops.call / ops.query / ops.ptr) so that the
kernel a row reaches is the one its table in tests/conv_ref.py claims (the claims are re-derived from the launchers' formulas in
tests/test_conv_ref_cpu.py; the split counts are asserted here through tag_conv3x3_wgrad_ws_bytes, the statistics rows through
tag_conv3x3_stats_rows): the weight packs, the halo-tile forward / dgrad with and without fused statistics, the tap-by-tap forward
at every other width, the bias epilogue, the three fused epilogue entries, the all-taps, row-ring and per-tap weight gradients --
the last with the tiny images whose 32-pixel chunks span two image boundaries --, and the Cin = 1 family, each against the fp64
statements of tests/conv_ref.py on the same seeded CPU inputs.

Staging: every operand sits in a device buffer with at least (W + 2) C NaN floats in front of and behind it and must be
bit-unchanged afterwards; every output, statistics buffer and workspace starts as NaN between guards of a sentinel that must be
bit-unchanged; a refused call must leave its outputs untouched.

Bounds are the ones tests/test_gpu_kernels.py asserts for the same quantities with the max-normalised ``relerr``: 5e-6 for forward,
dgrad and weight gradient (test_conv3x3_forward_dgrad_wgrad, ``tol = 5e-6``) and the fused pool output
(test_conv_fused_bnrelu_pool_eval); 1e-6 for the folded mean and 2e-6 per channel for the folded invstd, both of the KERNEL'S OWN
output as there (test_conv3x3_fused_bn_stats); 1e-5 for the sums of the two backward epilogues (test_conv_dgrad_fused_bnrelu_backward,
test_conv_dgrad_fused_pool_backward_sums); 2e-6 for the Cin = 1 results (test_conv3x3_c1).  Every comparison prints the fp32 CPU
floor beside its error.  FLOOR_RULE names the comparisons whose bound is 4 x max(floor, 1e-6) instead
(docs/experiments_conv_sweep.md lists them); nothing is calibrated on the kernels.  Masks, counts, bit-identities and second runs
are exact.

The option conv_impl is read once per process: test_conv_impl_1_child_process repeats the forward and weight-gradient tables in
a child process with TAG_CONV_IMPL=1, where they all run on the per-tap kernels, at widths 4 .. 64 too."""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import conv_ref as R

pytestmark = pytest.mark.gpu

IMPL = int(os.environ.get("TAG_CONV_IMPL", "0"))        # what lib.load() forwards to the library's conv_impl option
SENT = -1234.5
F64, F32 = torch.float64, torch.float32
#: names (of close()) whose bound is 4 x max(floor, 1e-6) instead of the plain one: none
FLOOR_RULE = re.compile(r"(?!)")
COUNT = {"comparisons": 0}


@pytest.fixture(scope="module")
def ops(dev):
    from texttoaudiogrounding_amd import ops as _ops
    yield _ops
    for f in (fwd_case, wgrad_case, c1_case):
        f.cache_clear()
    torch.cuda.empty_cache()
    print(f"\n  conv sweep: {COUNT['comparisons']} tensor comparisons in this process (conv_impl {IMPL})")


def close(name, got, ref64, ref32, bound):
    ref64 = torch.as_tensor(ref64).detach()
    got = torch.as_tensor(got).detach().cpu().double()
    assert ref64.dtype == F64 and got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), f"{name}: NaN or sentinel left inside the logical extent"
    err = R.relerr(got, ref64)
    floor = ref32 if isinstance(ref32, float) else R.relerr(ref32, ref64)
    how = ""
    if FLOOR_RULE.match(name):
        bound, how = 4 * max(floor, 1e-6), "  floor rule"
    COUNT["comparisons"] += 1
    print(f"  {name:70s} err {err:.2e}  fp32-cpu floor {floor:.2e}  bound {bound:.2e}{how}")
    assert err <= bound, (name, err, floor, bound)


# ------------------------------------------------------------------------------------------------ staging
class Staged:
    """A flat device buffer [guard | logical extent | guard].  Operands: the tensor between NaN guards, all of it bit-unchanged
    afterwards.  Outputs: NaN between SENT guards; the guards bit-unchanged afterwards, the extent too after a refused call."""

    def __init__(self, dev, guard, src=None, shape=None, dtype=torch.float32):
        guard = max(64, (guard + 3) // 4 * 4)
        self.shape = tuple(src.shape) if src is not None else tuple(shape)
        n = 1
        for d in self.shape:
            n *= d
        self.n, self.guard, self.is_input = n, guard, src is not None
        self.flat = torch.full((2 * guard + n,), float("nan") if self.is_input else SENT, device=dev, dtype=dtype)
        self.t = self.flat[guard:guard + n].view(self.shape)
        if self.is_input:
            self.t.copy_(src.to(dev))
        else:
            self.t.fill_(float("nan"))
        assert self.t.data_ptr() % 16 == 0
        self.before = self._bits().clone()

    def _bits(self):
        return self.flat.view(torch.int64 if self.flat.dtype == F64 else torch.int32)

    def check(self, name, untouched=False):
        """operands and refused outputs: every bit as before; outputs: both guards as before"""
        now = self._bits()
        if self.is_input or untouched:
            assert torch.equal(now, self.before), f"{name}: buffer modified"
        else:
            g = self.guard
            assert torch.equal(now[:g], self.before[:g]) and torch.equal(now[g + self.n:], self.before[g + self.n:]), \
                f"{name}: wrote outside the logical extent"


def refused(ops, name, *args):
    with pytest.raises(RuntimeError, match=r"rc=-1"):
        ops.call(name, *args)
    torch.cuda.synchronize()


def checked(name, *bufs, untouched=()):
    torch.cuda.synchronize()
    for b in bufs:
        b.check(name)
    for b in untouched:
        b.check(name, untouched=True)


# ------------------------------------------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def fwd_case(B, H, W, Cin, Cout, pro):
    x, w, dy, s, t = R.conv_inputs(B, H, W, Cin, Cout, 100 + W + H)
    return x, w, s, t, R.conv_fwd(x, w, pro, s, t), R.conv_fwd(x, w, pro, s, t, F32)


@functools.lru_cache(maxsize=None)
def wgrad_case(B, H, W, Cin, Cout, pro):
    x, w, dy, s, t = R.conv_inputs(B, H, W, Cin, Cout, 100 + W + H)
    return x, dy, s, t, R.conv_wgrad(x, dy, pro, s, t), R.conv_wgrad(x, dy, pro, s, t, F32)


@functools.lru_cache(maxsize=None)
def c1_case(B, H, W, Cout):
    return R.c1_inputs(B, H, W, Cout, 7)


def pack(ops, dev, w, dgrad=False):
    """the pack from the CPU statement (bit-exact with tag_pack_conv_weight: test_pack_conv_weight), staged between NaN guards"""
    wp = R.pack_dgrad(w) if dgrad else R.pack_fwd(w)
    return Staged(dev, wp.shape[2] * 4, src=wp)


def run_forward(ops, dev, name, x, wp, pro, s, t, Cout, stats=False):
    """one tag_conv3x3_forward call on staged buffers; returns (y, stats buffer or None, P)"""
    B, H, W, Cin = x.shape
    g = (W + 2) * max(Cin, Cout)
    xs, y = Staged(dev, g, src=x), Staged(dev, g, shape=(B, H, W, Cout))
    ss, ts = (Staged(dev, 64, src=s), Staged(dev, 64, src=t)) if pro else (None, None)
    P = ops.query("tag_conv3x3_stats_rows", B, H, W, Cout) if stats else 0
    st = Staged(dev, 3 * Cout + 1, shape=(P * (3 * Cout + 1),)) if stats else None
    ops.call("tag_conv3x3_forward", ops.ptr(xs.t), ops.ptr(wp.t), pro, ops.ptr(ss.t if ss else None), ops.ptr(ts.t if ts else None),
             ops.ptr(y.t), ops.ptr(st.t if st else None), B, H, W, Cin, Cout)
    checked(name, *[b for b in (xs, wp, y, ss, ts, st) if b is not None])
    return y.t, (st.t if st else None), P


def pid(c, n=6):
    return "-".join(map(str, c[:n]))


# ------------------------------------------------------------------------------------------------ 1. weight packs
@pytest.mark.parametrize("Cin,Cout", R.PACK_CASES, ids=lambda v: str(v))
def test_pack_conv_weight(ops, dev, Cin, Cout):
    """both packs are exact permutations; with and without the dgrad pack; (256, 260) takes a second grid-stride trip"""
    w = torch.randn(Cout, Cin, 3, 3, generator=torch.Generator().manual_seed(Cin + Cout))
    ws = Staged(dev, 64, src=w)
    for want_dgrad in (True, False):
        pf, pd = Staged(dev, 64, shape=(9, Cin, Cout)), Staged(dev, 64, shape=(9, Cout, Cin))
        ops.call("tag_pack_conv_weight", ops.ptr(ws.t), ops.ptr(pf.t), ops.ptr(pd.t if want_dgrad else None), Cin, Cout)
        checked("pack", ws, pf, pd, untouched=() if want_dgrad else (pd,))
        assert torch.equal(pf.t.cpu(), R.pack_fwd(w))
        if want_dgrad:
            assert torch.equal(pd.t.cpu(), R.pack_dgrad(w))
    pf = Staged(dev, 64, shape=(9, Cin, Cout))
    refused(ops, "tag_pack_conv_weight", ops.ptr(ws.t), ops.ptr(pf.t), None, 0, Cout)
    refused(ops, "tag_pack_conv_weight", None, ops.ptr(pf.t), None, Cin, Cout)
    checked("pack refused", untouched=(pf,))


# ------------------------------------------------------------------------------------------------ 2. forward / dgrad
@pytest.mark.parametrize("case", R.HALO_CASES, ids=pid)
def test_forward_sweep_halo_table(ops, dev, case):
    """The halo-tile kernel (conv_impl 0; the tap-by-tap kernel in the child process): y against fp64; with statistics the same y
    bit for bit, every pixel counted once, the folded mean / invstd; the same entry on the dgrad pack is the data gradient."""
    B, H, W, Cin, Cout, pro, claim = case
    x, w, s, t, ref64, ref32 = fwd_case(B, H, W, Cin, Cout, pro)
    name = f"fwd {pid(case)} {R.fwd_kernel(W, Cout, IMPL)}"
    y, _, _ = run_forward(ops, dev, name, x, pack(ops, dev, w), pro, s, t, Cout)
    close(name + " y", y, ref64, ref32, R.FWD)
    P = ops.query("tag_conv3x3_stats_rows", B, H, W, Cout)
    if IMPL == 0:
        assert P == R.stats_rows(B, H, W) == B * claim[2] * 2
        y2, st, _ = run_forward(ops, dev, name + " stats", x, pack(ops, dev, w), pro, s, t, Cout, stats=True)
        assert torch.equal(y, y2), "the statistics epilogue changed y"
        assert bool(torch.isfinite(st).all())
        mean, invstd, n = R.fold_stats_partials(st.cpu(), P, Cout)
        assert n == B * H * W
        m_ref, i_ref = R.bn_fold(y.cpu().double())
        m_f32, i_f32 = R.bn_fold(y.cpu())
        close(name + " mean", mean, m_ref, m_f32.double(), R.STAT_MEAN)
        e = ((invstd - i_ref).abs() / i_ref).max().item()
        print(f"  {name + ' invstd':70s} err {e:.2e}  (per channel)  bound {R.STAT_INVSTD:.2e}")
        COUNT["comparisons"] += 1
        assert e <= R.STAT_INVSTD
    else:
        assert P == 0
    # the data gradient: the forward entry on the dgrad pack, channels Cout -> Cin (needs Cout % 32 == 0 as its Cin)
    if Cout % 32 == 0 and Cout <= 512:
        dy = R.conv_inputs(B, H, W, Cin, Cout, 100 + W + H)[2]
        da, _, _ = run_forward(ops, dev, name + " dgrad", dy, pack(ops, dev, w, dgrad=True), 0, None, None, Cin)
        close(name + " dgrad", da, R.conv_dgrad(dy, w), R.conv_dgrad(dy, w, F32), R.FWD)


@pytest.mark.parametrize("case", R.HALO256_CASES + R.HALO_INST_CASES, ids=pid)
def test_forward_halo_256_cout_tile_with_statistics(ops, dev, case):
    """Cout 256 / 512 at W <= 16: with statistics the launch takes the 256-cout tile, without them the 128-cout one -- same bits.
    The tiny rows of HALO_INST_CASES put one launch with statistics on every <BN, PRO, TW> a default launch can select."""
    B, H, W, Cin, Cout, pro = case
    x, w, s, t, ref64, ref32 = fwd_case(B, H, W, Cin, Cout, pro)
    name = f"fwd256 {pid(case)}"
    y, _, _ = run_forward(ops, dev, name, x, pack(ops, dev, w), pro, s, t, Cout)
    y2, st, P = run_forward(ops, dev, name + " stats", x, pack(ops, dev, w), pro, s, t, Cout, stats=True)
    close(name + " y", y2, ref64, ref32, R.FWD)
    assert torch.equal(y, y2) and P == R.stats_rows(B, H, W)
    mean, invstd, n = R.fold_stats_partials(st.cpu(), P, Cout)
    m_ref, i_ref = R.bn_fold(y.cpu().double())
    assert n == B * H * W
    close(name + " mean", mean, m_ref, R.bn_fold(y.cpu())[0].double(), R.STAT_MEAN)
    assert ((invstd - i_ref).abs() / i_ref).max().item() <= R.STAT_INVSTD


@pytest.mark.parametrize("case", R.TAP_FWD_CASES, ids=pid)
def test_forward_sweep_tap_table(ops, dev, case):
    """conv3x3_fwd_kernel<64 | 128, PRO> at the widths no halo tile serves; statistics are refused there, outputs untouched"""
    B, H, W, Cin, Cout, pro, M = case
    x, w, s, t, ref64, ref32 = fwd_case(B, H, W, Cin, Cout, pro)
    name = f"fwd {pid(case)} {R.fwd_kernel(W, Cout, IMPL)}"
    wp = pack(ops, dev, w)
    y, _, _ = run_forward(ops, dev, name, x, wp, pro, s, t, Cout)
    close(name + " y", y, ref64, ref32, R.FWD)
    assert ops.query("tag_conv3x3_stats_rows", B, H, W, Cout) == 0
    xs, yo, st = Staged(dev, (W + 2) * Cin, src=x), Staged(dev, 64, shape=(B, H, W, Cout)), Staged(dev, 64, shape=(3 * Cout + 1,))
    ss, ts = Staged(dev, 64, src=s), Staged(dev, 64, src=t)
    refused(ops, "tag_conv3x3_forward", ops.ptr(xs.t), ops.ptr(wp.t), pro, ops.ptr(ss.t), ops.ptr(ts.t), ops.ptr(yo.t), ops.ptr(st.t),
            B, H, W, Cin, Cout)
    checked(name + " refused", xs, untouched=(yo, st))


def test_forward_refusals_leave_outputs_untouched(ops, dev):
    x, w, s, t, _, _ = fwd_case(1, 1, 8, 32, 36, 1)
    xs, wp, y = Staged(dev, 320, src=x), pack(ops, dev, w), Staged(dev, 64, shape=(1, 1, 8, 36))
    ss, ts = Staged(dev, 64, src=s), Staged(dev, 64, src=t)
    P = lambda b: ops.ptr(b.t)
    for args in [(P(xs), P(wp), 4, P(ss), P(ts), P(y), None, 1, 1, 8, 32, 36), (P(xs), P(wp), 1, None, P(ts), P(y), None, 1, 1, 8, 32, 36),
                 (P(xs), P(wp), 0, None, None, P(y), None, 1, 1, 8, 48, 36), (P(xs), P(wp), 0, None, None, P(y), None, 1, 1, 8, 32, 38),
                 (P(xs), P(wp), 0, None, None, P(y), None, 1, 0, 8, 32, 36), (P(xs), P(wp), 0, None, None, P(y), None, 1, 1, 8, 544, 36),
                 (None, P(wp), 0, None, None, P(y), None, 1, 1, 8, 32, 36)]:
        refused(ops, "tag_conv3x3_forward", *args)
    checked("forward refused", xs, wp, untouched=(y,))


# ------------------------------------------------------------------------------------------------ 3. bias epilogue
def _bias_call(ops, xs, wp, pro, ss, ts, bs, y, B, H, W, Cin, Cout):
    ops.call("tag_conv3x3_forward_bias", ops.ptr(xs.t), ops.ptr(wp.t), pro, ops.ptr(ss.t), ops.ptr(ts.t), ops.ptr(bs.t), ops.ptr(y.t),
             B, H, W, Cin, Cout)


@pytest.mark.parametrize("case", R.BIAS_CASES, ids=lambda c: pid(c, 5))
def test_forward_bias(ops, dev, case):
    """y = conv(prologue(x)) + bias[clip]: a zero table gives tag_conv3x3_forward's bits; distinct rows per clip against fp64"""
    if IMPL:
        pytest.skip("the bias epilogue lives in the halo-tile kernel")
    B, H, W, Cin, pro = case
    Cout = 128
    x, w, s, t, _, _ = fwd_case(B, H, W, Cin, Cout, pro)
    bias = torch.randn(B, Cout, generator=torch.Generator().manual_seed(H)) * 2 + torch.arange(B).view(B, 1) * 3.0
    name = f"bias {pid(case, 5)}"
    g = (W + 2) * Cout
    xs, wp, ss, ts = Staged(dev, g, src=x), pack(ops, dev, w), Staged(dev, 64, src=s), Staged(dev, 64, src=t)
    y0, _, _ = run_forward(ops, dev, name, x, wp, pro, s, t, Cout)
    for b, tag in ((torch.zeros(B, Cout), "zero"), (bias, "rows")):
        bs, y = Staged(dev, Cout, src=b), Staged(dev, g, shape=(B, H, W, Cout))
        _bias_call(ops, xs, wp, pro, ss, ts, bs, y, B, H, W, Cin, Cout)
        checked(name, xs, wp, ss, ts, bs, y)
        if tag == "zero":
            assert torch.equal(y.t, y0), "a zero bias must give tag_conv3x3_forward's output bit for bit"
        else:
            close(name + " y", y.t, R.conv_fwd(x, w, pro, s, t, bias=b), R.conv_fwd(x, w, pro, s, t, F32, bias=b), R.FWD)
    # every unserved argument is refused with y untouched
    y = Staged(dev, g, shape=(B, H, W, Cout))
    for a in [(pro, B, H, 8, Cin, Cout), (pro, B, H, W, 64, Cout), (pro, B, H, W, Cin, 64), (0, B, H, W, Cin, Cout), (1, B, H, W, Cin, Cout),
              (pro, 0, H, W, Cin, Cout), (pro, B, 0, W, Cin, Cout)]:
        refused(ops, "tag_conv3x3_forward_bias", ops.ptr(xs.t), ops.ptr(wp.t), a[0], ops.ptr(ss.t), ops.ptr(ts.t), ops.ptr(bs.t),
                ops.ptr(y.t), *a[1:])
    refused(ops, "tag_conv3x3_forward_bias", ops.ptr(xs.t), ops.ptr(wp.t), pro, ops.ptr(ss.t), ops.ptr(ts.t), None, ops.ptr(y.t),
            B, H, W, Cin, Cout)
    checked(name + " refused", untouched=(y,))


# ------------------------------------------------------------------------------------------------ 4. fused epilogue entries
def _bn_tables(C, seed):
    g = torch.Generator().manual_seed(seed)
    gamma, beta = torch.rand(C, generator=g) + 0.5, 0.2 * torch.randn(C, generator=g)
    mean, var = 0.3 + 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    return gamma * invstd, beta - mean * gamma * invstd, mean, invstd


@pytest.mark.parametrize("case", R.BNSUMS_CASES, ids=lambda c: pid(c, 5))
def test_dgrad_bnsums(ops, dev, case):
    """da = conv(dy) with the plain entry's bits, and (sum dz, sum dz xhat) folded over the partial rows, at H below one tile,
    Cout 68 / 132 and W = 64 as two tile columns; W = 4 is refused"""
    if IMPL:
        pytest.skip("the epilogues live in the halo-tile kernel")
    B, H, W, Cin, Cout = case
    x, w, _, _, ref64, ref32 = fwd_case(B, H, W, Cin, Cout, 0)                 # x plays dy, ref = da
    yref = torch.randn(B, H, W, Cout, generator=torch.Generator().manual_seed(W)) * 2 + 0.3
    sc, sh, mu, isd = _bn_tables(Cout, H)
    name = f"bnsums {pid(case, 5)}"
    g = (W + 2) * max(Cin, Cout)
    P = ops.query("tag_conv3x3_stats_rows", B, H, W, Cout)
    assert P == R.stats_rows(B, H, W)
    xs, wp, ys = Staged(dev, g, src=x), pack(ops, dev, w), Staged(dev, g, src=yref)
    tb = [Staged(dev, 64, src=v) for v in (sc, sh, mu, isd)]
    da, part = Staged(dev, g, shape=(B, H, W, Cout)), Staged(dev, 2 * Cout, shape=(P, 2, Cout))
    ops.call("tag_conv3x3_dgrad_bnsums", ops.ptr(xs.t), ops.ptr(wp.t), ops.ptr(da.t), ops.ptr(ys.t), *[ops.ptr(b.t) for b in tb],
             ops.ptr(part.t), B, H, W, Cin, Cout)
    checked(name, xs, wp, ys, da, part, *tb)
    y0, _, _ = run_forward(ops, dev, name, x, wp, 0, None, None, Cout)
    assert torch.equal(da.t, y0)
    close(name + " da", da.t, ref64, ref32, R.FWD)
    s1, s2 = R.bn_bwd_sums(ref64, yref, sc, sh, mu, isd)
    f1, f2 = R.bn_bwd_sums(ref32, yref, sc, sh, mu, isd, F32)
    assert bool(torch.isfinite(part.t).all())
    close(name + " sum dz", part.t.cpu().double().sum(0)[0], s1, f1, R.SUMS)
    close(name + " sum dz xhat", part.t.cpu().double().sum(0)[1], s2, f2, R.SUMS)
    da4, p4 = Staged(dev, 64, shape=(B, H, 4, Cout)), Staged(dev, 64, shape=(P, 2, Cout))
    refused(ops, "tag_conv3x3_dgrad_bnsums", ops.ptr(xs.t), ops.ptr(wp.t), ops.ptr(da4.t), ops.ptr(ys.t), *[ops.ptr(b.t) for b in tb],
            ops.ptr(p4.t), B, H, 4, Cin, Cout)
    checked(name + " refused", untouched=(da4, p4))


@pytest.mark.parametrize("case", R.POOLSUMS_CASES, ids=lambda c: pid(c, 7))
def test_dgrad_poolsums(ops, dev, case):
    """dx = conv(dy) with the plain entry's bits and the sums of relu(bn(yref)) -> pool -> dropout's backward: H below one tile, odd Hf
    with ph = 2 (a floor-dropped row), Cout 68 / 132, W = 64 as two tile columns, the three pool kinds, drop_p 0 and 0.3 with two seeds"""
    if IMPL:
        pytest.skip("the epilogues live in the halo-tile kernel")
    B, Hf, Wf, Cin, Cout, ph, pool = case
    H, W = Hf // ph, Wf // 2
    x, w, _, _, ref64, ref32 = fwd_case(B, H, W, Cin, Cout, 0)
    yref = torch.randn(B, Hf, Wf, Cout, generator=torch.Generator().manual_seed(Wf)) * 2 + 0.3
    sc, sh, mu, isd = _bn_tables(Cout, Hf)
    name = f"poolsums {pid(case, 7)}"
    g = (Wf + 2) * max(Cin, Cout)
    P = ops.query("tag_conv3x3_stats_rows", B, H, W, Cout)
    xs, wp, ys = Staged(dev, g, src=x), pack(ops, dev, w), Staged(dev, g, src=yref)
    tb = [Staged(dev, 64, src=v) for v in (sc, sh, mu, isd)]
    y0, _, _ = run_forward(ops, dev, name, x, wp, 0, None, None, Cout)
    masks = []
    for p, seed in ((0.0, 0), (0.3, 11), (0.3, 12)):
        dx, part = Staged(dev, g, shape=(B, H, W, Cout)), Staged(dev, 2 * Cout, shape=(P, 2, Cout))
        ops.call("tag_conv3x3_dgrad_poolsums", ops.ptr(xs.t), ops.ptr(wp.t), ops.ptr(dx.t), ops.ptr(ys.t), *[ops.ptr(b.t) for b in tb],
                 ops.ptr(part.t), B, H, W, Cin, Cout, Hf, Wf, ph, 2, pool, p, seed)
        checked(name, xs, wp, ys, dx, part, *tb)
        assert torch.equal(dx.t, y0)
        keep = ops.dropout_mask(seed, (B, H, W, Cout), p, dev, pooled=True).cpu() if p > 0 else None
        masks.append(keep)
        s1, s2 = R.pool_bwd_sums(ref64, yref, sc, sh, mu, isd, ph, pool, keep, p)
        f1, f2 = R.pool_bwd_sums(ref32, yref, sc, sh, mu, isd, ph, pool, keep, p, F32)
        assert bool(torch.isfinite(part.t).all()) and bool((part.t[1::2] == 0).all()), "odd rows of the layout stay zero"
        close(f"{name} p {p} seed {seed} sum dz", part.t.cpu().double().sum(0)[0], s1, f1, R.SUMS)
        close(f"{name} p {p} seed {seed} sum dz xhat", part.t.cpu().double().sum(0)[1], s2, f2, R.SUMS)
    assert not torch.equal(masks[1], masks[2]) and 0.6 < masks[1].float().mean().item() < 0.8
    dx, part = Staged(dev, 64, shape=(B, H, 4, Cout)), Staged(dev, 64, shape=(P, 2, Cout))
    for a in [(B, H, 4, Cin, Cout, Hf, 8, ph, 2, pool, 0.0, 0), (B, H, W, Cin, Cout, Hf, Wf, 3, 2, pool, 0.0, 0),
              (B, H, W, Cin, Cout, Hf, Wf, ph, 2, 1, 0.0, 0), (B, H, W, Cin, Cout, Hf, Wf, ph, 2, pool, 1.0, 0)]:
        refused(ops, "tag_conv3x3_dgrad_poolsums", ops.ptr(xs.t), ops.ptr(wp.t), ops.ptr(dx.t), ops.ptr(ys.t), *[ops.ptr(b.t) for b in tb],
                ops.ptr(part.t), *a)
    checked(name + " refused", untouched=(dx, part))


@pytest.mark.parametrize("case", R.POOLEVAL_CASES, ids=lambda c: pid(c, 8))
def test_forward_bnrelu_pool_eval(ops, dev, case):
    """pool(relu(bn(conv))) with floor windows against fp64, and bit-identical to tag_conv3x3_forward + tag_bnact_pool_forward at
    the channel counts that entry serves"""
    if IMPL:
        pytest.skip("the epilogues live in the halo-tile kernel")
    B, H, W, Cin, Cout, ph, pro, pool = case
    x, w, s, t, ref64, ref32 = fwd_case(B, H, W, Cin, Cout, pro)
    sc, sh, _, _ = _bn_tables(Cout, H + W)
    name = f"pooleval {pid(case, 8)}"
    g = (W + 2) * max(Cin, Cout)
    xs, wp = Staged(dev, g, src=x), pack(ops, dev, w)
    ss, ts = (Staged(dev, 64, src=s), Staged(dev, 64, src=t)) if pro else (None, None)
    bsc, bsh = Staged(dev, 64, src=sc), Staged(dev, 64, src=sh)
    out = Staged(dev, g, shape=(B, H // ph, W // 2, Cout))
    ops.call("tag_conv3x3_forward_bnrelu_pool_eval", ops.ptr(xs.t), ops.ptr(wp.t), pro, ops.ptr(ss.t if ss else None),
             ops.ptr(ts.t if ts else None), ops.ptr(out.t), ops.ptr(bsc.t), ops.ptr(bsh.t), B, H, W, Cin, Cout, ph, 2, pool)
    checked(name, xs, wp, bsc, bsh, out, *[b for b in (ss, ts) if b])
    close(name, out.t, R.bnrelu_pool(ref64, sc, sh, ph, pool), R.bnrelu_pool(ref32, sc, sh, ph, pool, F32), R.FWD)
    if 256 % (Cout // 4) == 0:        # the channel counts tag_bnact_pool_forward serves (Cout / 4 divides 256): 64 and 128 here, not 68 / 132
        y0, _, _ = run_forward(ops, dev, name, x, wp, pro, s, t, Cout)
        two = Staged(dev, g, shape=(B, H // ph, W // 2, Cout))
        ops.call("tag_bnact_pool_forward", ops.ptr(y0), ops.ptr(bsc.t), ops.ptr(bsh.t), ops.ptr(two.t), B, H, W, Cout, ph, 2, 1, pool, 0.0, 0)
        torch.cuda.synchronize()
        assert torch.equal(out.t, two.t), "the one-kernel form must be bit-identical to conv + bnact_pool"
    o4 = Staged(dev, 64, shape=(B, H // ph, 2, Cout))
    for a in [(0, B, H, 4, Cin, Cout, ph, 2, pool), (2, B, H, W, Cin, Cout, ph, 2, pool), (0, B, H, W, Cin, Cout, 3, 2, pool),
              (0, B, H, W, Cin, Cout, ph, 2, 1)]:
        refused(ops, "tag_conv3x3_forward_bnrelu_pool_eval", ops.ptr(xs.t), ops.ptr(wp.t), a[0], ops.ptr(bsc.t), ops.ptr(bsh.t),
                ops.ptr(o4.t), ops.ptr(bsc.t), ops.ptr(bsh.t), *a[1:])
    checked(name + " refused", untouched=(o4,))


def test_conv_impl_switch_and_the_epilogue_entries(ops, dev):
    """conv_impl 0: the halo widths have statistics rows.  conv_impl 1 (the child process): none, and the four epilogue entries
    refuse with untouched outputs."""
    if IMPL == 0:
        assert all(ops.query("tag_conv3x3_stats_rows", 2, 9, W, 64) > 0 for W in R.HALO_W)
        return
    assert all(ops.query("tag_conv3x3_stats_rows", 2, 9, W, 64) == 0 for W in R.HALO_W)
    B, H, W, Cin, Cout = 3, 9, 16, 32, 128
    x, w, s, t, _, _ = fwd_case(B, H, W, Cin, Cout, 3)
    xs, wp, ss, ts = Staged(dev, 4096, src=x), pack(ops, dev, w), Staged(dev, 64, src=s), Staged(dev, 64, src=t)
    tb = [Staged(dev, 64, src=v) for v in _bn_tables(Cout, 1)]
    yr = Staged(dev, 4096, src=torch.randn(B, 2 * H, 2 * W, Cout))
    out, part = Staged(dev, 64, shape=(B, H, W, Cout)), Staged(dev, 64, shape=(B * 8, 2, Cout))
    bs = Staged(dev, 64, src=torch.zeros(B, Cout))
    P = lambda b: ops.ptr(b.t)
    refused(ops, "tag_conv3x3_forward_bias", P(xs), P(wp), 3, P(ss), P(ts), P(bs), P(out), B, H, W, Cin, Cout)
    refused(ops, "tag_conv3x3_dgrad_bnsums", P(xs), P(wp), P(out), P(yr), *[P(b) for b in tb], P(part), B, H, W, Cin, Cout)
    refused(ops, "tag_conv3x3_dgrad_poolsums", P(xs), P(wp), P(out), P(yr), *[P(b) for b in tb], P(part), B, H, W, Cin, Cout,
            2 * H, 2 * W, 2, 2, 0, 0.0, 0)
    refused(ops, "tag_conv3x3_forward_bnrelu_pool_eval", P(xs), P(wp), 0, None, None, P(out), P(tb[0]), P(tb[1]), B, H, W, Cin, Cout, 1, 2, 0)
    checked("conv_impl 1 refusals", xs, wp, untouched=(out, part))


# ------------------------------------------------------------------------------------------------ 5. weight gradients
def run_wgrad(ops, dev, name, x, dy, pro, s, t, expect_ws_bytes):
    """tag_conv3x3_wgrad twice on fresh NaN workspaces: (dw, second run's dw)"""
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    nbytes = ops.query("tag_conv3x3_wgrad_ws_bytes", B, H, W, Cin, Cout)
    assert nbytes == expect_ws_bytes, (name, nbytes, expect_ws_bytes)
    xs, ds = Staged(dev, (W + 2) * Cin, src=x), Staged(dev, (W + 2) * Cout, src=dy)
    ss, ts = (Staged(dev, 64, src=s), Staged(dev, 64, src=t)) if pro else (None, None)
    outs = []
    for _ in range(2):
        dw, ws = Staged(dev, 64, shape=(Cout, Cin, 3, 3)), Staged(dev, 64, shape=(nbytes // 4,))
        ops.call("tag_conv3x3_wgrad", ops.ptr(xs.t), pro, ops.ptr(ss.t if ss else None), ops.ptr(ts.t if ts else None), ops.ptr(ds.t),
                 ops.ptr(dw.t), B, H, W, Cin, Cout, ops.ptr(ws.t))
        checked(name, xs, ds, dw, ws, *[b for b in (ss, ts) if b])
        assert bool(torch.isfinite(ws.t).all()), f"{name}: a partial of the workspace was never written"
        outs.append(dw.t)
    assert torch.equal(outs[0], outs[1]), f"{name}: two runs differ"
    return outs[0]


@pytest.mark.parametrize("case", R.ALLTAPS_CASES, ids=pid)
def test_wgrad_sweep_alltaps_table(ops, dev, case):
    """all-taps (W 4 / 8) and row-ring (W 16 / 32 / 64) kernels: images shorter than the ring, splits of whole images and splits
    across images, partial ci / co tiles, the four prologues (the per-tap kernel in the child process)"""
    B, H, W, Cin, Cout, pro, (splits, cps, crosses) = case
    x, dy, s, t, ref64, ref32 = wgrad_case(B, H, W, Cin, Cout, pro)
    name = f"wgrad {pid(case)} {R.wgrad_kernel(W, Cin, Cout, IMPL)}"
    if IMPL == 0:
        assert R.wgrad_ws_bytes(B, H, W, Cin, Cout) == splits * 9 * Cin * Cout * 4
    dw = run_wgrad(ops, dev, name, x, dy, pro, s, t, R.wgrad_ws_bytes(B, H, W, Cin, Cout, IMPL))
    close(name, dw, ref64, ref32, R.FWD)


@pytest.mark.parametrize("case", R.TAP_WGRAD_CASES, ids=pid)
def test_wgrad_sweep_tap_table(ops, dev, case):
    """conv3x3_wgrad_kernel<64 | 128, PRO>: every width without an all-taps form, M % 32 != 0, two splits with a ragged last chunk"""
    B, H, W, Cin, Cout, pro, (TC, splits, chunk) = case
    x, dy, s, t, ref64, ref32 = wgrad_case(B, H, W, Cin, Cout, pro)
    name = f"wgrad {pid(case)} ('tap', {TC})"
    dw = run_wgrad(ops, dev, name, x, dy, pro, s, t, splits * 9 * Cin * Cout * 4)
    close(name, dw, ref64, ref32, R.FWD)


@pytest.mark.parametrize("B,H,W", R.TINY_WGRAD + R.TINY_CONTROLS, ids=lambda v: str(v))
@pytest.mark.parametrize("pro", [0, 1])
def test_wgrad_sweep_tiny_images(ops, dev, B, H, W, pro):
    """Images so small that a 32-pixel chunk of the per-tap kernel spans two image boundaries (H W < 32 + W): the row index wraps by
    a true modulo.  (3, 7, 5) and (5, 7) are the controls: one wrap was enough there and the fix changes no bit (the two formulas
    give the same row for every pixel slot: tests/test_conv_ref_cpu.py)."""
    Cin, Cout = 32, 64
    x, dy, s, t, ref64, ref32 = wgrad_case(B, H, W, Cin, Cout, pro)
    name = f"wgrad tiny ({B}, {H}, {W}) pro {pro}"
    dw = run_wgrad(ops, dev, name, x, dy, pro, s, t, R.wgrad_ws_bytes(B, H, W, Cin, Cout, 1))
    close(name, dw, ref64, ref32, R.FWD)


def test_wgrad_refusals_leave_outputs_untouched(ops, dev):
    x, dy, s, t, _, _ = wgrad_case(3, 2, 8, 36, 64, 1)
    xs, ds = Staged(dev, 4096, src=x), Staged(dev, 4096, src=dy)
    dw, ws = Staged(dev, 64, shape=(64, 36, 3, 3)), Staged(dev, 64, shape=(9 * 36 * 64,))
    P = lambda b: ops.ptr(b.t)
    for a in [(0, None, None, 1, 1, 65, 36, 64), (0, None, None, 3, 2, 8, 38, 64), (0, None, None, 3, 2, 8, 36, 66), (4, None, None, 3, 2, 8, 36, 64),
              (1, None, None, 3, 2, 8, 36, 64), (0, None, None, 0, 2, 8, 36, 64), (0, None, None, 3, 0, 8, 36, 64)]:
        refused(ops, "tag_conv3x3_wgrad", P(xs), a[0], a[1], a[2], P(ds), P(dw), *a[3:], P(ws))
    refused(ops, "tag_conv3x3_wgrad", P(xs), 0, None, None, P(ds), P(dw), 3, 2, 8, 36, 64, None)
    checked("wgrad refused", xs, ds, untouched=(dw, ws))


# ------------------------------------------------------------------------------------------------ 6. the Cin = 1 family
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("case", R.C1_FWD_CASES, ids=lambda c: pid(c, 5))
def test_c1_forward(ops, dev, case, affine):
    if IMPL:
        pytest.skip("the Cin = 1 kernels have no conv_impl switch")
    B, H, W, Cout, kernel = case
    x, cs, ct, w, dy = c1_case(B, H, W, Cout)
    if not affine:
        cs = ct = None
    name = f"c1 fwd {pid(case, 5)} {'affine' if affine else 'plain'}"
    xs, wsb, y = Staged(dev, W + 2, src=x), Staged(dev, 64, src=w), Staged(dev, (W + 2) * Cout, shape=(B, H, W, Cout))
    cb = [Staged(dev, 64, src=v) for v in (cs, ct)] if affine else []
    cp = [ops.ptr(b.t) for b in cb] if affine else [None, None]
    ops.call("tag_conv3x3_c1_forward", ops.ptr(xs.t), *cp, ops.ptr(wsb.t), ops.ptr(y.t), B, H, W, Cout)
    checked(name, xs, wsb, y, *cb)
    ref64, ref32 = R.c1_fwd(x, w, cs, ct), R.c1_fwd(x, w, cs, ct, F32)
    close(name, y.t, ref64, ref32, R.C1)
    if kernel == "rows":                                   # the same kernel with its fused statistics: same y, every pixel once
        P = ops.query("tag_conv3x3_c1_stats_rows", B, H, W, Cout)
        assert P == B * R.c1_bwd_geom(B, H)[0] * 16
        y2, st = Staged(dev, (W + 2) * Cout, shape=(B, H, W, Cout)), Staged(dev, 256, shape=(P * (3 * Cout + 1),))
        ops.call("tag_conv3x3_c1_forward_stats", ops.ptr(xs.t), *cp, ops.ptr(wsb.t), ops.ptr(y2.t), ops.ptr(st.t), B, H, W, Cout)
        checked(name + " stats", xs, wsb, y2, st, *cb)
        assert torch.equal(y.t, y2.t)
        mean, invstd, n = R.fold_stats_partials(st.t.cpu(), P, Cout)
        m_ref, i_ref = R.bn_fold(y.t.cpu().double())
        assert n == B * H * W
        close(name + " mean", mean, m_ref, R.bn_fold(y.t.cpu())[0].double(), R.STAT_MEAN)
        assert ((invstd - i_ref).abs() / i_ref).max().item() <= R.STAT_INVSTD
    else:
        assert ops.query("tag_conv3x3_c1_stats_rows", B, H, W, Cout) == 0


@pytest.mark.parametrize("case", R.C1_BIAS_CASES, ids=lambda c: pid(c, 4))
def test_c1_forward_bias(ops, dev, case):
    """two clips inside one workgroup: each pixel group takes its own clip's bias row; a zero table gives the plain entry's bits"""
    if IMPL:
        pytest.skip("the Cin = 1 kernels have no conv_impl switch")
    B, H, W, Cout = case
    x, cs, ct, w, dy = c1_case(B, H, W, Cout)
    bias = torch.randn(B, Cout, generator=torch.Generator().manual_seed(W)) + torch.arange(B).view(B, 1) * 5.0
    name = f"c1 bias {pid(case, 4)}"
    xs, wsb, cb = Staged(dev, W + 2, src=x), Staged(dev, 64, src=w), [Staged(dev, 64, src=v) for v in (cs, ct)]
    y0 = Staged(dev, (W + 2) * Cout, shape=(B, H, W, Cout))
    ops.call("tag_conv3x3_c1_forward", ops.ptr(xs.t), ops.ptr(cb[0].t), ops.ptr(cb[1].t), ops.ptr(wsb.t), ops.ptr(y0.t), B, H, W, Cout)
    for b, tag in ((torch.zeros(B, Cout), "zero"), (bias, "rows")):
        bs, y = Staged(dev, Cout, src=b), Staged(dev, (W + 2) * Cout, shape=(B, H, W, Cout))
        ops.call("tag_conv3x3_c1_forward_bias", ops.ptr(xs.t), ops.ptr(cb[0].t), ops.ptr(cb[1].t), ops.ptr(wsb.t), ops.ptr(bs.t),
                 ops.ptr(y.t), B, H, W, Cout)
        checked(name, xs, wsb, bs, y, *cb)
        if tag == "zero":
            assert torch.equal(y.t, y0.t)
        else:
            close(name, y.t, R.c1_fwd(x, w, cs, ct, bias=b), R.c1_fwd(x, w, cs, ct, F32, bias=b), R.C1)
    y = Staged(dev, 64, shape=(B, H, W, Cout))
    for a in [(B, H, 6, Cout), (B, H, W, 12), (B, H, W, 0), (0, H, W, Cout), (B, 0, W, Cout), (B, H, 0, Cout)]:
        refused(ops, "tag_conv3x3_c1_forward_bias", ops.ptr(xs.t), ops.ptr(cb[0].t), ops.ptr(cb[1].t), ops.ptr(wsb.t), ops.ptr(bs.t),
                ops.ptr(y.t), *a)
    checked(name + " refused", untouched=(y,))


def _c1_big(case):
    return case[0] * case[1] * case[2] * case[3] > (1 << 24)


#: the two 2^26-element rows run once, with the affine
C1_WGRAD_PARAMS = [(c, a) for c in R.C1_WGRAD_CASES for a in (True, False) if a or not _c1_big(c)]


@pytest.mark.parametrize("case,affine", C1_WGRAD_PARAMS, ids=lambda v: pid(v, 4) if isinstance(v, tuple) else ("affine" if v else "plain"))
def test_c1_wgrad_dgrad(ops, dev, case, affine):
    """conv_c1_wgrad_kernel<4> (W % 4 == 0) and conv_c1_wgrad_kernel<1>, Cout 4 .. 256, M below one block's first trip and above
    1024 rpi 64 (a second grid-stride trip); tag_conv3x3_c1_dgrad on the same dy"""
    if IMPL:
        pytest.skip("the Cin = 1 kernels have no conv_impl switch")
    B, H, W, Cout, (kernel, blocks) = case
    big = _c1_big(case)
    x, cs, ct, w, dy = c1_case(B, H, W, Cout)
    if not affine:
        cs = ct = None
    name = f"c1 wgrad {case[:4]} {'affine' if affine else 'plain'}"
    xs, ds = Staged(dev, W + 2, src=x), Staged(dev, (W + 2) * Cout, src=dy)
    cb = [Staged(dev, 64, src=v) for v in (cs, ct)] if affine else []
    cp = [ops.ptr(b.t) for b in cb] if affine else [None, None]
    nbytes = ops.query("tag_conv3x3_c1_wgrad_ws_bytes", B, H, W, Cout)
    assert nbytes == 1024 * Cout * 9 * 8
    outs = []
    for _ in range(2):
        dw, ws = Staged(dev, 64, shape=(Cout, 1, 3, 3)), Staged(dev, 64, shape=(nbytes // 8,), dtype=F64)
        ops.call("tag_conv3x3_c1_wgrad", ops.ptr(xs.t), *cp, ops.ptr(ds.t), ops.ptr(dw.t), B, H, W, Cout, ops.ptr(ws.t))
        checked(name, xs, ds, dw, ws, *cb)
        assert bool(torch.isfinite(ws.t[:blocks * Cout * 9]).all()) and bool(torch.isnan(ws.t[blocks * Cout * 9:]).all()), \
            f"{name}: the launch did not write exactly {blocks} partial rows"
        outs.append(dw.t)
    assert torch.equal(outs[0], outs[1])
    close(name, outs[0], R.c1_wgrad(x, dy, cs, ct), R.c1_wgrad(x, dy, cs, ct, F32), R.C1)
    if affine and not big:
        wsb, dx = Staged(dev, 64, src=w), Staged(dev, W + 2, shape=(B, H, W))
        ops.call("tag_conv3x3_c1_dgrad", ops.ptr(ds.t), ops.ptr(wsb.t), ops.ptr(dx.t), B, H, W, Cout)
        checked(name + " dgrad", ds, wsb, dx)
        close(f"c1 dgrad {case[:4]}", dx.t, R.c1_dgrad(dy, w), R.c1_dgrad(dy, w, F32), R.C1)


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("B,H", R.C1_BWD_CASES, ids=lambda v: str(v))
def test_c1_fused_backward(ops, dev, B, H, affine):
    """tag_conv3x3_c1_backward (W = Cout = 64) around the 8-row strip minimum: one strip shorter than 8 rows, exactly 8, and a second
    strip of one row; B = 300 puts two strips per image at nine rows too (2048 / B = 6 < 8)"""
    if IMPL:
        pytest.skip("the Cin = 1 kernels have no conv_impl switch")
    W = Cout = 64
    x, cs, ct, w, dy = c1_case(B, H, W, Cout)
    if not affine:
        cs = ct = None
    name = f"c1 bwd ({B}, {H}) {'affine' if affine else 'plain'}"
    strips, rows = R.c1_bwd_geom(B, H)
    nbytes = ops.query("tag_conv3x3_c1_backward_ws_bytes", B, H, W, Cout)
    assert nbytes == B * strips * Cout * 9 * 8
    xs, ds, wsb = Staged(dev, W + 2, src=x), Staged(dev, (W + 2) * Cout, src=dy), Staged(dev, 64, src=w)
    cb = [Staged(dev, 64, src=v) for v in (cs, ct)] if affine else []
    cp = [ops.ptr(b.t) for b in cb] if affine else [None, None]
    dw, dx, ws = Staged(dev, 64, shape=(Cout, 1, 3, 3)), Staged(dev, W + 2, shape=(B, H, W)), Staged(dev, 64, shape=(nbytes // 8,), dtype=F64)
    ops.call("tag_conv3x3_c1_backward", ops.ptr(xs.t), *cp, ops.ptr(ds.t), ops.ptr(wsb.t), ops.ptr(dw.t), ops.ptr(dx.t), B, H, W, Cout,
             ops.ptr(ws.t))
    checked(name, xs, ds, wsb, dw, dx, ws, *cb)
    assert bool(torch.isfinite(ws.t).all())
    close(name + " dw", dw.t, R.c1_wgrad(x, dy, cs, ct), R.c1_wgrad(x, dy, cs, ct, F32), R.C1)
    close(name + " dx", dx.t, R.c1_dgrad(dy, w), R.c1_dgrad(dy, w, F32), R.C1)


def test_c1_refusals_leave_outputs_untouched(ops, dev):
    """B, H, W, Cout > 0 are checked before Cout / 4 divides anything; an unserved Cout and half an affine pair are refused"""
    if IMPL:
        pytest.skip("the Cin = 1 kernels have no conv_impl switch")
    x, cs, ct, w, dy = c1_case(3, 5, 8, 4)
    xs, ds, wsb, cb = Staged(dev, 64, src=x), Staged(dev, 64, src=dy), Staged(dev, 64, src=w), Staged(dev, 64, src=cs)
    y, dw, dx, ws = (Staged(dev, 64, shape=(3, 5, 8, 4)), Staged(dev, 64, shape=(4, 1, 3, 3)), Staged(dev, 64, shape=(3, 5, 8)),
                     Staged(dev, 64, shape=(1024 * 4 * 9,), dtype=F64))
    P = lambda b: ops.ptr(b.t)
    for a in [(3, 5, 8, 0), (0, 5, 8, 4), (3, 0, 8, 4), (3, 5, 0, 4), (3, 5, 8, -4), (3, 5, 8, 6)]:
        refused(ops, "tag_conv3x3_c1_forward", P(xs), None, None, P(wsb), P(y), *a)
        refused(ops, "tag_conv3x3_c1_wgrad", P(xs), None, None, P(ds), P(dw), *a, P(ws))
        refused(ops, "tag_conv3x3_c1_dgrad", P(ds), P(wsb), P(dx), *a)
    refused(ops, "tag_conv3x3_c1_forward", P(xs), P(cb), None, P(wsb), P(y), 3, 5, 8, 4)
    refused(ops, "tag_conv3x3_c1_wgrad", P(xs), None, None, P(ds), P(dw), 3, 5, 8, 12, P(ws))
    refused(ops, "tag_conv3x3_c1_dgrad", P(ds), P(wsb), P(dx), 3, 5, 8, 260)
    refused(ops, "tag_conv3x3_c1_backward", P(xs), None, None, P(ds), P(wsb), P(dw), P(dx), 3, 5, 8, 4, P(ws))
    checked("c1 refused", xs, ds, wsb, untouched=(y, dw, dx, ws))


# ------------------------------------------------------------------------------------------------ 7. the per-tap kernels everywhere
def test_conv_impl_1_child_process(dev):
    """TAG_CONV_IMPL=1 puts every forward and weight-gradient launch on the per-tap kernels, at widths 4 .. 64 too; the option is read
    once per process, so the forward and weight-gradient tables (and the switch test) run again in a child process with it set."""
    if IMPL:
        pytest.skip("this IS the child process")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TAG_CONV_IMPL="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k",
                        "forward_sweep or wgrad_sweep or conv_impl_switch"], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "conv_impl 1" in r.stdout
