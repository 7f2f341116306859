"""csrc/conv_x3.hip, csrc/conv_rows.hip and csrc/conv_wgrad_dma.hip over their edge shapes: the split-bf16 (x3 / x9), one-product and
bf16-storage convolutions, every entry point called through the C ABI (ops.call / ops.query / ops.ptr) so that the kernel a row
reaches is the one its table in tests/conv_x3_ref.py claims (the claims are re-derived from the launchers' formulas in
tests/test_conv_x3_ref_cpu.py; partial-row and split counts are asserted here against the library's queries and against what the
launch actually wrote).  tag_conv_rows_enable / tag_wgrad_dma_enable choose between the kernels behind one entry point; they are
set and restored in try / finally.

Staging (tests/test_gpu_conv_sweep.py::Staged): operands between NaN guards of at least (W + 2) max(Cin, Cout) elements, bit-unchanged
afterwards; outputs, partial buffers and workspaces NaN between sentinel guards; finiteness inside the extent is asserted before
any comparison, so a read of a guard or an unwritten partial row is a failure and not a tolerance question.

References: fp64 statements on the CPU.  x3 / x9 on fp32 tensors: the plain convolution.  One product: the convolution of the
RNE-bf16-rounded operands, the operand after a prologue restated BIT FOR BIT (conv_x3_ref.operand; no case has a double rounding:
CPU test), so prologue cases hold the no-prologue bounds.  Bounds, all from tests/test_gpu_kernels.py: 5e-6 max-normalised for
x3 / x9 / one-product on fp32 tensors; 1.01 half-ulps of bf16 for bf16-stored outputs; 1e-5 for the bf16 weight gradient; 2e-5 for
the folded mean and variance against the fp64 statistics of the fp64 y; 1e-5 for the EPI 1 sums (fp64 da, restated mask) and the
EPI 2 sums (fp64 statement on the kernel's own bf16 dx).  The fp32-CPU floor is printed beside every error; no comparison needs
the floor rule of tests/test_gpu_conv_sweep.py (its FLOOR_RULE matches nothing; docs/experiments_x3_sweep.md has the figures).
Packs, counts, bit-identities and second runs are exact -- and so is the operand: with an identity weight (forward) or a one-pixel
dy (weight gradient) the output IS the operand of the prologue, compared bit for bit on inputs that carry values at which a
multiply-then-add in place of fmaf rounds the bf16 operand the other way."""
import functools

import pytest
import torch

from tests import conv_ref as R
from tests import conv_x3_ref as X
from tests.test_gpu_conv_sweep import COUNT, checked, close, refused
from tests.test_gpu_conv_sweep import Staged as _Staged

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def ops(dev):
    from texttoaudiogrounding_amd import ops as _ops
    n0 = COUNT["comparisons"]
    yield _ops
    for f in (fwd_refs, dgrad_refs, wgrad_refs):
        f.cache_clear()
    torch.cuda.empty_cache()
    print(f"\n  x3 sweep: {COUNT['comparisons'] - n0} tensor comparisons")


class Staged(_Staged):
    """tests/test_gpu_conv_sweep.py::Staged for bf16 tensors too: their bits are compared element by element (16 bits each)"""

    def _bits(self):
        return self.flat.view(torch.int16) if self.flat.dtype == BF16 else super()._bits()


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault(dev):
    """a launch that faulted leaves a context every later call fails on: end the module there instead of launching on"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU context is lost ({e}): nothing more is launched", returncode=3)


class switches:
    """tag_conv_rows_enable / tag_wgrad_dma_enable for the duration of a block"""

    def __init__(self, ops, rows=None, dma=None):
        self.ops, self.want, self.was = ops, dict(tag_conv_rows_enable=rows, tag_wgrad_dma_enable=dma), {}

    def __enter__(self):
        for k, v in self.want.items():
            if v is not None:
                self.was[k] = self.ops.query(k, v)

    def __exit__(self, *exc):
        for k, v in self.was.items():
            self.ops.query(k, v)
        return False


def close_ulp(name, got, ref64, ref32):
    """a bf16-stored output against fp64 in half-ulps of bf16 (the expression of _bf16_storage_case); the floor is the bf16 rounding
    of the fp32-CPU result"""
    assert got.dtype == BF16 and ref64.dtype == F64 and tuple(got.shape) == tuple(ref64.shape), (name, got.dtype, got.shape, ref64.shape)
    got = got.detach().float().cpu()
    assert torch.isfinite(got).all(), f"{name}: NaN or sentinel left inside the logical extent"
    err, floor = X.half_ulps(got, ref64), X.half_ulps(ref32.bfloat16().float(), ref64)
    COUNT["comparisons"] += 1
    print(f"  {name:70s} err {err:.3f}  fp32-cpu floor {floor:.3f}  bound {X.HALF_ULPS:.2f}  (half-ulps of bf16)")
    assert err <= X.HALF_ULPS, (name, err, floor)


def pid(c, n=6):
    return "-".join(map(str, c[:n]))


# ------------------------------------------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def fwd_refs(B, H, W, Cin, Cout, pro, products, bf16):
    x, w, dy, s, t = X.case(B, H, W, Cin, Cout, bf16)
    return X.fwd_ref(x, w, pro, s, t, products), X.fwd_ref(x, w, pro, s, t, products, F32)


@functools.lru_cache(maxsize=None)
def dgrad_refs(B, H, W, Cin, Cout, products, bf16):
    x, w, dy, s, t = X.case(B, H, W, Cin, Cout, bf16)
    return X.dgrad_ref(dy, w, products), X.dgrad_ref(dy, w, products, F32)


@functools.lru_cache(maxsize=None)
def wgrad_refs(B, H, W, Cin, Cout, pro, products, bf16):
    x, w, dy, s, t = X.case(B, H, W, Cin, Cout, bf16)
    return X.wgrad_ref(x, dy, pro, s, t, products), X.wgrad_ref(x, dy, pro, s, t, products, F32)


def dev_pack(ops, dev, w, products):
    """both packs made by tag_pack_conv_weight_x3 (bit-exact with the CPU statement: test_pack_x3), then frozen as operands"""
    Cout, Cin = w.shape[:2]
    n = X.pack_bytes(Cin, Cout) // 4
    ws, pf, pd = Staged(dev, 64, src=w), Staged(dev, 256, shape=(n,)), Staged(dev, 256, shape=(n,))
    ops.call("tag_pack_conv_weight_x3", ops.ptr(ws.t), ops.ptr(pf.t), ops.ptr(pd.t), Cin, Cout, products)
    checked("pack", ws, pf, pd)
    for b in (pf, pd):
        b.before, b.is_input = b._bits().clone(), True
    return pf, pd


def run_fwd(ops, dev, name, x, wp, pro, s, t, Cout, products, stats=False):
    """one tag_conv3x3_forward_x3[_bf16] call on staged buffers: (y, statistics buffer or None, P)"""
    B, H, W, Cin = x.shape
    bf16 = x.dtype == BF16
    g = (W + 2) * max(Cin, Cout)
    xs, y = Staged(dev, g, src=x, dtype=x.dtype), Staged(dev, g, shape=(B, H, W, Cout), dtype=x.dtype)
    ss, ts = (Staged(dev, 64, src=s), Staged(dev, 64, src=t)) if pro else (None, None)
    P = 0
    if stats:
        P = (ops.query("tag_conv3x3_x3_bf16_stats_rows", B, H, W, Cin, Cout, pro) if bf16
             else ops.query("tag_conv3x3_x3_stats_rows", B, H, W, Cout))
        assert P > 0
    st = Staged(dev, 3 * Cout + 1, shape=(P * (3 * Cout + 1),)) if stats else None
    args = [ops.ptr(xs.t), ops.ptr(wp.t), pro, ops.ptr(ss.t if ss else None), ops.ptr(ts.t if ts else None), ops.ptr(y.t),
            ops.ptr(st.t if st else None), B, H, W, Cin, Cout]
    if bf16:
        ops.call("tag_conv3x3_forward_x3_bf16", *args)
    else:
        ops.call("tag_conv3x3_forward_x3", *args, products)
    checked(name, *[b for b in (xs, wp, y, ss, ts, st) if b is not None])
    return y.t, (st.t if st else None), P


def check_stats(name, st, P, Cout, count, y_own=None, y_ref64=None):
    """every partial row written, every pixel counted once, the folded statistics.  fp32 tensors: against the kernel's own y (1e-6
    mean, 2e-6 invstd per channel: test_conv3x3_fused_bn_stats); bf16 storage: mean and variance against the fp64 y (2e-5)"""
    assert bool(torch.isfinite(st).all()), f"{name}: a partial statistics row was never written"
    mean, invstd, n = R.fold_stats_partials(st.cpu(), P, Cout)
    assert n == count, (name, n, count)
    if y_own is not None:
        m_ref, i_ref = R.bn_fold(y_own.cpu().double())
        close(name + " mean", mean, m_ref, R.bn_fold(y_own.cpu())[0].double(), R.STAT_MEAN)
        e = ((invstd - i_ref).abs() / i_ref).max().item()
        print(f"  {name + ' invstd':70s} err {e:.2e}  (per channel)  bound {R.STAT_INVSTD:.2e}")
        COUNT["comparisons"] += 1
        assert e <= R.STAT_INVSTD
    else:
        v = y_ref64.reshape(-1, Cout)
        v32 = v.float()
        close(name + " mean", mean, v.mean(0), v32.mean(0).double(), X.STATS16)
        close(name + " var", 1.0 / invstd ** 2, v.var(0, unbiased=False) + 1e-5, (v32.var(0, unbiased=False) + 1e-5).double(), X.STATS16)


def cu_count(ops):
    n = ops.query("tag_device_cu_count")
    return n if n > 0 else 256


# ------------------------------------------------------------------------------------------------ 1. the packs
@pytest.mark.parametrize("rne", [False, True], ids=["split", "rne"])
@pytest.mark.parametrize("Cin,Cout", X.PACK_CASES, ids=lambda v: str(v))
def test_pack_x3(ops, dev, Cin, Cout, rne):
    """tag_pack_conv_weight_x3 bit for bit: the truncating three-way split (products 6 and 9 give the same image), the RNE one-product
    pack with zero mid / lo planes, the dgrad pack with mirrored taps and K, N swapped"""
    w = torch.randn(Cout, Cin, 3, 3, generator=torch.Generator().manual_seed(Cin + Cout))
    n = X.pack_bytes(Cin, Cout) // 4
    assert ops.query("tag_conv3x3_x3_pack_bytes", Cin, Cout) == 4 * n
    ws = Staged(dev, 64, src=w)
    for products in ((1,) if rne else (6, 9)):
        pf, pd = Staged(dev, 256, shape=(n,)), Staged(dev, 256, shape=(n,))
        ops.call("tag_pack_conv_weight_x3", ops.ptr(ws.t), ops.ptr(pf.t), ops.ptr(pd.t), Cin, Cout, products)
        checked("pack x3", ws, pf, pd)
        assert torch.equal(pf.t.view(torch.int32).cpu(), X.pack_x3(w, False, rne).reshape(-1)), "forward pack"
        assert torch.equal(pd.t.view(torch.int32).cpu(), X.pack_x3(w, True, rne).reshape(-1)), "dgrad pack"
    pf, pd = Staged(dev, 256, shape=(n,)), Staged(dev, 256, shape=(n,))
    refused(ops, "tag_pack_conv_weight_x3", ops.ptr(ws.t), ops.ptr(pf.t), None, Cin, Cout, 6)
    refused(ops, "tag_pack_conv_weight_x3", ops.ptr(ws.t), ops.ptr(pf.t), ops.ptr(pd.t), Cin + 16, Cout, 6)
    refused(ops, "tag_pack_conv_weight_x3", ops.ptr(ws.t), ops.ptr(pf.t), ops.ptr(pd.t), Cin, Cout + 16, 6)
    checked("pack x3 refused", ws, untouched=(pf, pd))


# ------------------------------------------------------------------------------------------------ 2. one launch per tile instantiation
def _fp32_launches(ops, dev, name, case, pro, kind, dgrad=True):
    B, H, W, Cin, Cout = case
    products = X.PRODUCTS[kind]
    x, w, dy, s, t = X.case(B, H, W, Cin, Cout)
    pf, pd = dev_pack(ops, dev, w, products)
    ref64, ref32 = fwd_refs(B, H, W, Cin, Cout, pro, products, False)
    y, _, _ = run_fwd(ops, dev, name, x, pf, pro, s, t, Cout, products)
    close(name + " y", y, ref64, ref32, X.X3)
    y2, st, P = run_fwd(ops, dev, name + " stats", x, pf, pro, s, t, Cout, products, stats=True)
    assert torch.equal(y, y2), f"{name}: the statistics epilogue changed y"
    assert P == X.x3_stats_rows(B, H, W, Cout)
    check_stats(name, st, P, Cout, B * H * W, y_own=y)
    if dgrad and Cin % 64 == 0:
        d64, d32 = dgrad_refs(B, H, W, Cin, Cout, products, False)
        da, _, _ = run_fwd(ops, dev, name + " dgrad", dy, pd, 0, None, None, Cin, products)
        close(name + " dgrad", da, d64, d32, X.X3)


def _bf16_launches(ops, dev, name, case, pro, dgrad=True, expect_P=None):
    """forward without and with statistics (same bits), the statistics, the dgrad on the mirrored pack"""
    B, H, W, Cin, Cout = case
    x, w, dy, s, t = X.case(B, H, W, Cin, Cout, True)
    pf, pd = dev_pack(ops, dev, w, 1)
    ref64, ref32 = fwd_refs(B, H, W, Cin, Cout, pro, 1, True)
    y, _, _ = run_fwd(ops, dev, name, x, pf, pro, s, t, Cout, 1)
    close_ulp(name + " y", y, ref64, ref32)
    y2, st, P = run_fwd(ops, dev, name + " stats", x, pf, pro, s, t, Cout, 1, stats=True)
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), f"{name}: the statistics epilogue changed y"
    if expect_P is not None:
        assert P == expect_P, (name, P, expect_P)
    check_stats(name, st, P, Cout, B * H * W, y_ref64=ref64)
    if dgrad and Cin % 64 == 0:
        d64, d32 = dgrad_refs(B, H, W, Cin, Cout, 1, True)
        da, _, _ = run_fwd(ops, dev, name + " dgrad", dy, pd, 0, None, None, Cin, 1)
        close_ulp(name + " dgrad", da, d64, d32)
    return y


@pytest.mark.parametrize("kind", ["x3", "x9", "np1"])
@pytest.mark.parametrize("case", X.INST_TILE_CASES, ids=lambda c: pid(c, 5))
def test_tile_instantiations_fp32(ops, dev, case, kind):
    """conv3x3_x3_kernel<MB, PRO, TW, NP, float>: every prologue at every width and both tile widths, 6 / 9 / 1 products"""
    for pro in range(4):
        _fp32_launches(ops, dev, f"x3 inst {pid(case, 5)} {kind} pro {pro}", case, pro, kind, dgrad=False)


@pytest.mark.parametrize("case", X.INST_TILE_CASES, ids=lambda c: pid(c, 5))
def test_tile_instantiations_bf16(ops, dev, case):
    """conv3x3_x3_kernel<MB, PRO, TW, 1, bf16_t, EPI 0> at every prologue, the row kernel switched off (it would take W = 64, 64 -> 64 and
    W = 32, 64 -> 128 at prologue 0 / 1); prologues 2 and 3 on bf16 storage hold the no-prologue bounds"""
    B, H, W, Cin, Cout = case
    with switches(ops, rows=0):
        for pro in range(4):
            _bf16_launches(ops, dev, f"bf16 inst {pid(case, 5)} pro {pro}", case, pro, dgrad=False,
                           expect_P=X.bf16_stats_rows(B, H, W, Cin, Cout, pro, 256, rows_on=False))


# ------------------------------------------------------------------------------------------------ 3. tile-kernel edges
@pytest.mark.parametrize("case", X.TILE_CASES, ids=pid)
def test_tile_edges_x3_fp32(ops, dev, case):
    """x3 on fp32 tensors: H around the tile height of every width, Cin of 1, 3, 5 and 16 chunks, 3 and 5 tiles of 64 couts, 3 of 128,
    B = 3 with an odd number of row tiles; dgrad where the mirrored convolution is served (Cin % 64 == 0)"""
    B, H, W, Cin, Cout, pro, (MB, row_tiles, n_tiles) = case
    assert ops.query("tag_conv3x3_x3_stats_rows", B, H, W, Cout) == B * row_tiles * (1 if MB == 4 else 2)
    _fp32_launches(ops, dev, f"x3 tile {pid(case)} MB {MB}", case[:5], pro, "x3")


@pytest.mark.parametrize("case", X.TILE_CASES + X.TILE256_CASES, ids=pid)
def test_tile_edges_bf16(ops, dev, case):
    """the same table (and H around 256 / W on the 64-cout tile) on bf16 storage, the row kernel switched off"""
    B, H, W, Cin, Cout, pro, (MB, row_tiles, n_tiles) = case
    with switches(ops, rows=0):
        _bf16_launches(ops, dev, f"bf16 tile {pid(case)} MB {MB}", case[:5], pro, expect_P=B * row_tiles * (1 if MB == 4 else 2))


@pytest.mark.parametrize("case", X.H1_CASES, ids=lambda c: pid(c, 5))
def test_one_row_images_stay_on_the_tile_kernel(ops, dev, case):
    """H = 1 at the row kernel's own (W, Cin, Cout), default switches: it refuses (H < 2), the tile kernel serves"""
    B, H, W, Cin, Cout = case
    with switches(ops, rows=1):
        for pro in (0, 1):
            P = X.bf16_stats_rows(B, H, W, Cin, Cout, pro, cu_count(ops))
            assert P == B * (1 if Cout % 128 == 0 else 2)
            _bf16_launches(ops, dev, f"bf16 H=1 {pid(case, 5)} pro {pro}", case, pro, expect_P=P)
        assert ops.query("tag_conv3x3_dgrad_poolsums_bf16_rows", B, H, W, Cin, Cout) == B


# ------------------------------------------------------------------------------------------------ 4. the row-streaming kernel
def _bnsums_launch(ops, dev, name, case, expect_P):
    """tag_conv3x3_dgrad_bnsums_bf16 with x as the incoming gradient on the forward pack: da bit-identical to the plain launch and
    within 1.01 half-ulps, the sums folded over the partial rows against fp64 sums over the fp64 da with the restated mask"""
    B, H, W, Cin, Cout = case
    x, w, dy, s, t = X.case(B, H, W, Cin, Cout, True)
    yref, sc, sh, mu, isd = X.epi_case(B, H, W, Cout)
    pf, _ = dev_pack(ops, dev, w, 1)
    ref64, ref32 = fwd_refs(B, H, W, Cin, Cout, 0, 1, True)
    g = (W + 2) * max(Cin, Cout)
    P = ops.query("tag_conv3x3_x3_bf16_stats_rows", B, H, W, Cin, Cout, 0)
    assert P == expect_P, (name, P, expect_P)
    xs, ys = Staged(dev, g, src=x, dtype=BF16), Staged(dev, g, src=yref, dtype=BF16)
    tb = [Staged(dev, 64, src=v) for v in (sc, sh, mu, isd)]
    da, part = Staged(dev, g, shape=(B, H, W, Cout), dtype=BF16), Staged(dev, 2 * Cout, shape=(P, 2, Cout))
    ops.call("tag_conv3x3_dgrad_bnsums_bf16", ops.ptr(xs.t), ops.ptr(pf.t), ops.ptr(da.t), ops.ptr(ys.t), *[ops.ptr(b.t) for b in tb],
             ops.ptr(part.t), B, H, W, Cin, Cout)
    checked(name, xs, pf, ys, da, part, *tb)
    y0, _, _ = run_fwd(ops, dev, name + " plain", x, pf, 0, None, None, Cout, 1)
    assert torch.equal(da.t.view(torch.int16), y0.view(torch.int16)), f"{name}: the epilogue changed da"
    close_ulp(name + " da", da.t, ref64, ref32)
    assert bool(torch.isfinite(part.t).all()), f"{name}: a partial row was never written"
    s1, s2 = X.bn_bwd_sums_x(ref64, yref, sc, sh, mu, isd)
    f1, f2 = X.bn_bwd_sums_x(ref32, yref, sc, sh, mu, isd, F32)
    close(name + " sum dz", part.t.cpu().double().sum(0)[0], s1, f1.double(), X.SUMS)
    close(name + " sum dz xhat", part.t.cpu().double().sum(0)[1], s2, f2.double(), X.SUMS)


@pytest.mark.parametrize("case", X.ROWS_CASES, ids=lambda c: pid(c, 5))
def test_rows_kernel(ops, dev, case):
    """conv3x3_rows_kernel<64, 64, 2> and <32, 64, 4>, its five (prologue, epilogue) launches per shape: H around rows_strips' H / 16
    rule, strips of odd length (group 1 owns one row fewer), 1 to 3 n-tiles; the partial-row count against the restated formula
    with the device's CU count"""
    B, H, W, Cin, Cout, (wn, ns, odd) = case
    cus = cu_count(ops)
    with switches(ops, rows=1):
        P = X.rows_partial_rows(B, H, W, Cin, Cout, cus)
        assert P == B * ns * 2 * (4 // wn), (P, cus)
        for pro in (0, 1):
            assert ops.query("tag_conv3x3_x3_bf16_stats_rows", B, H, W, Cin, Cout, pro) == P
            _bf16_launches(ops, dev, f"rows {pid(case, 5)} WN {wn} pro {pro}", case[:5], pro, dgrad=False, expect_P=P)
        assert ops.query("tag_conv3x3_x3_bf16_stats_rows", B, H, W, Cin, Cout, 2) == X.bf16_stats_rows(B, H, W, Cin, Cout, 2, cus)
        _bnsums_launch(ops, dev, f"rows {pid(case, 5)} WN {wn} bnsums", case[:5], P)


def test_rows_kernel_cu_cap_binds(ops, dev):
    """B = 128, H = 48: ceil(cus / B) = 2 strips per image where H / 16 allows 3.  Two distinct images repeated alternately: images 0
    and 1 against fp64, every other image bit-identical to them; the statistics of the whole batch are those of the pair"""
    B, H, W, Cin, Cout = X.ROWS_CAP_CASE
    cus = cu_count(ops)
    ns = X.rows_strips(B, H, 1, cus)
    assert -(-cus // B) < H // 16 and ns == -(-cus // B), f"the cap does not bind on a part with {cus} CUs"
    x2, w, dy, s, t = X.case(2, H, W, Cin, Cout, True)
    x = x2.repeat(B // 2, 1, 1, 1)
    pf, _ = dev_pack(ops, dev, w, 1)
    ref64, ref32 = fwd_refs(2, H, W, Cin, Cout, 1, 1, True)
    with switches(ops, rows=1):
        P = ops.query("tag_conv3x3_x3_bf16_stats_rows", B, H, W, Cin, Cout, 1)
        assert P == B * ns * 2 * 2 == X.rows_partial_rows(B, H, W, Cin, Cout, cus)
        y, st, _ = run_fwd(ops, dev, "rows cap", x, pf, 1, s, t, Cout, 1, stats=True)
    close_ulp("rows cap y[0:2]", y[:2], ref64, ref32)
    yb = y.view(torch.int16).view(B // 2, 2, H, W, Cout)
    assert torch.equal(yb, yb[:1].expand_as(yb)), "an image differs from its twin"
    check_stats("rows cap", st, P, Cout, B * H * W, y_ref64=ref64)


# ------------------------------------------------------------------------------------------------ 5. weight gradients
def run_wgrad(ops, dev, name, kind, case, pro, tensors=None):
    """the weight gradient of ``kind`` twice on fresh NaN workspaces: exactly the claimed number of partials written, two runs
    bit-identical; returns dw.  tensors: (x, dy, s, t) instead of the case's own"""
    B, H, W, Cin, Cout = case
    bf16 = kind in ("bf16", "dma")
    x, w, dy, s, t = X.case(B, H, W, Cin, Cout, bf16)
    if tensors is not None:
        x, dy, s, t = tensors
    c = X.wgrad_claim(kind, B, H, W, Cin, Cout)
    nbytes = ops.query("tag_conv3x3_wgrad_x3_ws_bytes", B, H, W, Cin, Cout)
    assert nbytes == X.wgrad_x3_ws_bytes(B, H, W, Cin, Cout) >= c["splits"] * 9 * Cin * Cout * 4
    if not bf16:
        assert nbytes == c["splits"] * 9 * Cin * Cout * 4, "the workspace query determines the split count of the 32-pixel kernels"
    dt = BF16 if bf16 else F32
    xs, ds = Staged(dev, (W + 2) * Cin, src=x, dtype=dt), Staged(dev, (W + 2) * Cout, src=dy, dtype=dt)
    ss, ts = (Staged(dev, 64, src=s), Staged(dev, 64, src=t)) if pro else (None, None)
    outs = []
    with switches(ops, dma={"bf16": 0, "dma": 2 if pro else 1}.get(kind)):
        for _ in range(2):
            dw, ws = Staged(dev, 64, shape=(Cout, Cin, 3, 3)), Staged(dev, 64, shape=(nbytes // 4,))
            args = [ops.ptr(xs.t), pro, ops.ptr(ss.t if ss else None), ops.ptr(ts.t if ts else None), ops.ptr(ds.t), ops.ptr(dw.t),
                    B, H, W, Cin, Cout]
            if bf16:
                ops.call("tag_conv3x3_wgrad_x3_bf16", *args, ops.ptr(ws.t))
            else:
                ops.call("tag_conv3x3_wgrad_x3", *args, X.PRODUCTS[kind], ops.ptr(ws.t))
            checked(name, xs, ds, dw, ws, *[b for b in (ss, ts) if b])
            used = c["splits"] * 9 * Cin * Cout
            assert bool(torch.isfinite(ws.t[:used]).all()), f"{name}: a partial of the workspace was never written"
            assert bool(torch.isnan(ws.t[used:]).all()), f"{name}: more than {c['splits']} partials written"
            outs.append(dw.t)
    assert torch.equal(outs[0], outs[1]), f"{name}: two runs differ"
    return outs[0]


def _wgrad_case(ops, dev, tag, kind, case, pro):
    products = 1 if kind in ("bf16", "dma") else X.PRODUCTS[kind]
    name = f"wgrad {tag} {kind} {pid(case, 5)} pro {pro}"
    dw = run_wgrad(ops, dev, name, kind, case, pro)
    ref64, ref32 = wgrad_refs(*case, pro, products, kind in ("bf16", "dma"))
    close(name, dw, ref64, ref32, X.WGRAD16 if kind in ("bf16", "dma") else X.X3)


@pytest.mark.parametrize("case", X.WGRAD_H_CASES, ids=lambda c: pid(c, 7))
def test_wgrad_h_sweep(ops, dev, case):
    """H over {1, CH - 1, CH, CH + 1, 2 CH + 1} of every width for the x3 (32-pixel chunks), register-staged bf16 and DMA kernels
    (64-pixel chunks): images shorter than one chunk, a ragged last row block, one and two chunks per launch"""
    _wgrad_case(ops, dev, "H", case[0], case[1:6], case[6])


@pytest.mark.parametrize("case", X.WGRAD_SPLIT_CASES, ids=lambda c: pid(c, 7) + "-" + c[7][3])
def test_wgrad_splits(ops, dev, case):
    """two and more splits: a short last split, last splits of one and of two chunks (shorter than the DMA prefetch depth), splits
    that start on the last row block of a strip and on the first of the next, the two column strips of W = 64"""
    kind, B, H, W, Cin, Cout, pro, (splits, cps, last, tag) = case
    assert X.wgrad_claim(kind, B, H, W, Cin, Cout)["splits"] == splits
    _wgrad_case(ops, dev, tag, kind, case[1:6], pro)


@pytest.mark.parametrize("case", X.WGRAD_PRO_CASES + X.WGRAD_INST_CASES, ids=lambda c: pid(c, 7))
def test_wgrad_prologues_and_tiles(ops, dev, case):
    """every prologue on one shape per width, nine 64 x 64 tiles (Cin, Cout in {64, 192}), and one launch per instantiation of the
    x9 and one-product-on-fp32 weight gradients"""
    _wgrad_case(ops, dev, "pro", case[0], case[1:6], case[6])


# ------------------------------------------------------------------------------------------------ 6. fused epilogues on bf16
@pytest.mark.parametrize("case", X.BNSUMS_CASES + [c + ("tile",) for c in X.INST_TILE_CASES], ids=lambda c: pid(c, 6))
def test_dgrad_bnsums_bf16(ops, dev, case):
    """EPI 1 on the tile kernel (both tile widths at every width, H below one tile, 3 tiles of 64 and of 128 couts) and epi_kind 2
    on the row kernel"""
    B, H, W, Cin, Cout, path = case
    with switches(ops, rows=1 if path == "rows" else 0):
        P = X.bf16_stats_rows(B, H, W, Cin, Cout, 0, cu_count(ops), rows_on=path == "rows")
        _bnsums_launch(ops, dev, f"bnsums16 {pid(case, 6)}", case[:5], P)


@pytest.mark.parametrize("case", X.POOLSUMS_CASES + [(1, 6, 2 * c[2], 64, c[4], 2, (0, 2, 3)[i % 3]) for i, c in enumerate(X.INST_TILE_CASES)],
                         ids=lambda c: pid(c, 7))
def test_dgrad_poolsums_bf16(ops, dev, case):
    """EPI 2: dx bit-identical to the plain launch; the sums of relu(bn(yref)) -> pool (ph x 2, floor) -> dropout's backward against
    the fp64 statement evaluated on the kernel's OWN bf16 dx (it sums the staged bf16 tile), the dropout mask from
    tag_dropout_mask_pooled; one partial row per m-tile; both tile widths at every width"""
    B, Hf, Wf, Cin, Cout, ph, pool = case
    H, W = Hf // ph, Wf // 2
    x, w, dy, s, t = X.case(B, H, W, Cin, Cout, True)
    yref, sc, sh, mu, isd = X.epi_case(B, Hf, Wf, Cout)
    name = f"poolsums16 {pid(case, 7)}"
    g = (Wf + 2) * max(Cin, Cout)
    with switches(ops, rows=0):
        P = ops.query("tag_conv3x3_dgrad_poolsums_bf16_rows", B, H, W, Cin, Cout)
        assert P == X.poolsums_bf16_rows(B, H, W, Cin, Cout, rows_on=False) == B * X.tile_geom(H, W, Cout)["row_tiles"]
        pf, _ = dev_pack(ops, dev, w, 1)
        xs, ys = Staged(dev, g, src=x, dtype=BF16), Staged(dev, g, src=yref, dtype=BF16)
        tb = [Staged(dev, 64, src=v) for v in (sc, sh, mu, isd)]
        y0, _, _ = run_fwd(ops, dev, name + " plain", x, pf, 0, None, None, Cout, 1)
        ref64, ref32 = fwd_refs(B, H, W, Cin, Cout, 0, 1, True)
        close_ulp(name + " dx", y0, ref64, ref32)
        own = y0.float().cpu()
        for p, seed in ((0.0, 0), (0.3, 11)):
            dx, part = Staged(dev, g, shape=(B, H, W, Cout), dtype=BF16), Staged(dev, 2 * Cout, shape=(P, 2, Cout))
            ops.call("tag_conv3x3_dgrad_poolsums_bf16", ops.ptr(xs.t), ops.ptr(pf.t), ops.ptr(dx.t), ops.ptr(ys.t),
                     *[ops.ptr(b.t) for b in tb], ops.ptr(part.t), B, H, W, Cin, Cout, Hf, Wf, ph, 2, pool, p, seed)
            checked(name, xs, pf, ys, dx, part, *tb)
            assert torch.equal(dx.t.view(torch.int16), y0.view(torch.int16)), f"{name}: the epilogue changed dx"
            assert bool(torch.isfinite(part.t).all()), f"{name}: a partial row was never written"
            keep = ops.dropout_mask(seed, (B, H, W, Cout), p, dev, pooled=True).cpu() if p > 0 else None
            s1, s2 = X.pool_bwd_sums_x(own, yref, sc, sh, mu, isd, ph, pool, keep, p)
            f1, f2 = X.pool_bwd_sums_x(own, yref, sc, sh, mu, isd, ph, pool, keep, p, F32)
            close(f"{name} p {p} sum dz", part.t.cpu().double().sum(0)[0], s1, f1.double(), X.SUMS)
            close(f"{name} p {p} sum dz xhat", part.t.cpu().double().sum(0)[1], s2, f2.double(), X.SUMS)
        # what the entry refuses: ph = 3, an unknown pool kind, drop_p = 1, pw != 2 -- outputs untouched
        dx, part = Staged(dev, 64, shape=(B, H, W, Cout), dtype=BF16), Staged(dev, 64, shape=(P, 2, Cout))
        for a in [(B, H, W, Cin, Cout, Hf, Wf, 3, 2, pool, 0.0, 0), (B, H, W, Cin, Cout, Hf, Wf, ph, 2, 1, 0.0, 0),
                  (B, H, W, Cin, Cout, Hf, Wf, ph, 2, pool, 1.0, 0), (B, H, W, Cin, Cout, Hf, Wf, ph, 4, pool, 0.0, 0)]:
            refused(ops, "tag_conv3x3_dgrad_poolsums_bf16", ops.ptr(xs.t), ops.ptr(pf.t), ops.ptr(dx.t), ops.ptr(ys.t),
                    *[ops.ptr(b.t) for b in tb], ops.ptr(part.t), *a)
        checked(name + " refused", xs, pf, ys, untouched=(dx, part))


# ------------------------------------------------------------------------------------------------ 7. the operand, bit for bit
@pytest.mark.parametrize("case", X.PROBE_CASES, ids=lambda c: pid(c, 5))
def test_operand_probe_forward(ops, dev, case):
    """An identity weight makes y the operand itself: prologues 1..3 of the tile kernel on fp32 tensors (6, 9 and 1 products) and on
    bf16 storage, and prologue 1 of the row kernel where it takes the shape, must give conv_x3_ref.operand BIT FOR BIT.  The inputs
    carry planted values at which a multiply-then-add in place of fmaf changes the bf16 operand (CPU test); on fp32 operands every
    tenth element and more tells the two apart."""
    B, H, W, Cin, Cout = case
    w = X.identity_weight(Cout, Cin)
    packs = {products: dev_pack(ops, dev, w, products)[0] for products in (6, 9, 1)}
    for pro in (1, 2, 3):
        for kind, bf16, rows in [("x3", False, 0), ("x9", False, 0), ("np1", False, 0), ("bf16 tile", True, 0), ("bf16 rows", True, 1)]:
            if rows and not X.rows_takes(H, W, Cin, Cout, pro):
                continue
            products = X.PRODUCTS.get(kind, 1)
            x, s, t, planted = X.probe_inputs(B, H, W, Cin, pro, bf16=bf16)
            with switches(ops, rows=rows):
                y, _, _ = run_fwd(ops, dev, f"probe {pid(case, 5)} {kind} pro {pro}", x, packs[products], pro, s, t, Cout, products)
            want = X.probe_expected(x, pro, s, t, products, Cout)
            got = y.float().cpu()
            bad = int((got != want).sum())
            COUNT["comparisons"] += 1
            print(f"  probe {pid(case, 5)} {kind:9s} pro {pro}: {bad} of {want.numel()} elements differ from the operand ({planted} planted)")
            assert bad == 0


@pytest.mark.parametrize("kind", ["x3", "bf16", "dma"])
@pytest.mark.parametrize("W", X.WIDTHS)
def test_operand_probe_wgrad(ops, dev, W, kind):
    """dy = 1 at one pixel makes dw[co, ci, ky, kx] the operand of its 3 x 3 neighbourhood: the prologues of the register-staged weight
    gradients (1..3) and of the DMA kernel (1, applied in place in LDS) bit for bit, discriminators planted in that neighbourhood"""
    B, H, Cin, Cout = 2, 5, 64, 64
    b0, h0, w0 = X.PROBE_PIXEL
    pixels = [(b0 * H + h0 + dy) * W + w0 + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    bf16 = kind != "x3"
    for pro in ((1,) if kind == "dma" else (1, 2, 3)):
        x, s, t, planted = X.probe_inputs(B, H, W, Cin, pro, pixels=pixels, bf16=bf16)
        dy = torch.zeros(B, H, W, Cout, dtype=BF16 if bf16 else F32)
        dy[b0, h0, w0] = 1.0
        dw = run_wgrad(ops, dev, f"probe wgrad {kind} W {W} pro {pro}", kind, (B, H, W, Cin, Cout), pro, tensors=(x, dy, s, t))
        a = X.operand(x, pro, s, t)
        a = a.bfloat16().float() if bf16 else a
        want = a[b0, h0 - 1:h0 + 2, w0 - 1:w0 + 2].permute(2, 0, 1).expand(Cout, Cin, 3, 3)
        bad = int((dw.cpu() != want).sum())
        COUNT["comparisons"] += 1
        print(f"  probe wgrad {kind} W {W} pro {pro}: {bad} of {want.numel()} elements differ from the operand ({planted} planted)")
        assert bad == 0


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_outputs_untouched(ops, dev):
    """rc = -1 and nothing written: W in {4, 12}, Cin = 48, Cout = 96, Cin = 576 on the forward, prologue 4, a prologue without its
    table, Cin = 32 on the weight gradients, the pool-sums entry on a shape the row kernel takes"""
    B, H, W, Cin, Cout = 1, 2, 8, 64, 64
    x, w, dy, s, t = X.case(B, H, W, Cin, Cout)
    pf, pd = dev_pack(ops, dev, w, 6)
    P = lambda b: ops.ptr(b.t)
    for dt in (F32, BF16):
        xs, ds = Staged(dev, 4096, src=x.to(dt), dtype=dt), Staged(dev, 4096, src=dy.to(dt), dtype=dt)
        y, st = Staged(dev, 64, shape=(B, H, W, Cout), dtype=dt), Staged(dev, 64, shape=(4 * (3 * Cout + 1),))
        ss, ts = Staged(dev, 64, src=s), Staged(dev, 64, src=t)
        dw, ws = Staged(dev, 64, shape=(Cout, Cin, 3, 3)), Staged(dev, 64, shape=(9 * Cin * Cout,))
        fwd, wg, tail = (("tag_conv3x3_forward_x3", "tag_conv3x3_wgrad_x3", (6,)) if dt == F32
                         else ("tag_conv3x3_forward_x3_bf16", "tag_conv3x3_wgrad_x3_bf16", ()))
        for a in [(0, None, None, B, H, 4, Cin, Cout), (0, None, None, B, H, 12, Cin, Cout), (0, None, None, B, H, W, 48, Cout),
                  (0, None, None, B, H, W, Cin, 96), (0, None, None, B, H, W, 576, Cout), (4, P(ss), P(ts), B, H, W, Cin, Cout),
                  (1, None, P(ts), B, H, W, Cin, Cout), (2, P(ss), None, B, H, W, Cin, Cout), (0, None, None, 0, H, W, Cin, Cout)]:
            refused(ops, fwd, P(xs), P(pf), a[0], a[1], a[2], P(y), P(st), *a[3:], *tail)
        for a in [(0, None, None, B, H, W, 32, Cout), (0, None, None, B, H, W, Cin, 96), (0, None, None, B, H, 4, Cin, Cout),
                  (0, None, None, B, H, 12, Cin, Cout), (4, P(ss), P(ts), B, H, W, Cin, Cout), (3, None, None, B, H, W, Cin, Cout)]:
            refused(ops, wg, P(xs), a[0], a[1], a[2], P(ds), P(dw), *a[3:], *tail, P(ws))
        refused(ops, wg, P(xs), 0, None, None, P(ds), P(dw), B, H, W, Cin, Cout, *tail, None)
        checked("x3 refused", xs, ds, pf, ss, ts, untouched=(y, st, dw, ws))
    # the bf16 epilogue entries
    B, Hf, Wf, Cin, Cout, ph = X.POOLSUMS_ROWS_REFUSED
    H, W = Hf // ph, Wf // 2
    x, w, dy, s, t = X.case(B, H, W, Cin, Cout, True)
    yref, sc, sh, mu, isd = X.epi_case(B, Hf, Wf, Cout)
    pf, _ = dev_pack(ops, dev, w, 1)
    xs, ys = Staged(dev, 8192, src=x, dtype=BF16), Staged(dev, 8192, src=yref, dtype=BF16)
    tb = [Staged(dev, 64, src=v) for v in (sc, sh, mu, isd)]
    dx, part = Staged(dev, 64, shape=(B, H, W, Cout), dtype=BF16), Staged(dev, 64, shape=(B * H, 2, Cout))
    with switches(ops, rows=1):
        assert ops.query("tag_conv3x3_dgrad_poolsums_bf16_rows", B, H, W, Cin, Cout) == 0
        refused(ops, "tag_conv3x3_dgrad_poolsums_bf16", P(xs), P(pf), P(dx), P(ys), *[P(b) for b in tb], P(part),
                B, H, W, Cin, Cout, Hf, Wf, ph, 2, 0, 0.0, 0)
    for a in [(B, H, 4, Cin, Cout), (B, H, W, 48, Cout), (B, H, W, Cin, 96), (B, H, W, 576, Cout)]:
        refused(ops, "tag_conv3x3_dgrad_bnsums_bf16", P(xs), P(pf), P(dx), P(ys), *[P(b) for b in tb], P(part), *a)
    refused(ops, "tag_conv3x3_dgrad_bnsums_bf16", P(xs), P(pf), P(dx), None, *[P(b) for b in tb], P(part), B, H, W, Cin, Cout)
    checked("bf16 epilogues refused", xs, ys, pf, untouched=(dx, part))
