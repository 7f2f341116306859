"""csrc/conv_wino_fused.hip and csrc/conv_wino.hip over their edge shapes, every entry point called through the C ABI (ops.call /
ops.query / ops.ptr) so that the kernels a row reaches are the ones its table in tests/wino_ref.py claims (the claims are derived
again from the launchers' formulas in tests/test_wino_ref_cpu.py; partial rows, workspace bytes and slice counts are asserted here
through the library's queries): the forward with every producer prologue and its statistics rows (EPI 0), the inference pooling
(EPI 3), the two gradient epilogues (EPI 1 / EPI 2, every pool kind), the 64 x 64 x 16, row-split and plane-form weight gradients,
the kept input planes (v_keep / v_saved), the weight pack bit for bit, and the refusals -- each against the fp64 statements of
tests/wino_ref.py (tests/conv_ref.py, tests/conv_x3_ref.py) on the same seeded CPU inputs.

Staging (Staged / close / refused / checked of tests/test_gpu_conv_sweep.py, shared): every operand -- x, scale, shift, U, dy, yref,
the BatchNorm tables -- sits between NaN guards and must be bit-unchanged afterwards; every output, partial-row buffer and workspace
starts as NaN between sentinel guards, the workspace with exactly the queried size; a refused call leaves its outputs untouched; the
error word is read after every launch; every forward and weight-gradient launch of the tables runs twice and repeats bit for bit.

Bounds are the ones tests/test_gpu_wino.py asserts for the same quantities: 5e-6 max-normalised for y, da, dx, the pooled outputs
and the folded epilogue sums, 1e-5 for dw, 2e-6 of (max |mean| + max std) for the folded mean and 5e-6 for the folded invstd, both
of the kernel's OWN y.  Every comparison prints the fp32 CPU floor (the oracle's Winograd restatement in fp32) beside its error.
FLOOR_RULE (shared, empty) would name comparisons whose bound is 4 x max(floor, 1e-6); none needs it
(docs/experiments_wino_sweep.md).  Nothing is calibrated on the kernels.  Counts, pivots, masks, bit-identities and second runs are exact."""
import pytest
import torch

from tests import conv_ref as R
from tests import conv_x3_ref as X
from tests import wino_ref as WR
from tests.test_gpu_conv_sweep import COUNT, FLOOR_RULE, Staged, checked, close, refused

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
assert FLOOR_RULE.pattern == r"(?!)", "no comparison of this module takes the floor rule"


@pytest.fixture(scope="module")
def ops(dev):
    from texttoaudiogrounding_amd import ops as _ops
    n0 = COUNT["comparisons"]
    yield _ops
    for f in (WR.fwd_case, WR.dgrad_case, WR.wgrad_case):
        f.cache_clear()
    torch.cuda.empty_cache()
    print(f"\n  wino sweep: {COUNT['comparisons'] - n0} tensor comparisons in this process")


def pid(c, n=6):
    return "-".join(map(str, c[:n]))


def done(ops, name, *bufs, untouched=()):
    """after every launch: synchronise, guards and operands intact, the error word clean"""
    checked(name, *[b for b in bufs if b is not None], untouched=untouched)
    ops.check_async_errors()


def P(ops, b):
    return ops.ptr(b.t) if b is not None else None


def bits(t):
    return t.contiguous().view(torch.int32)


def pack_u(dev, w, dgrad=False):
    """U from the CPU statement (bit-exact with tag_pack_conv_weight_wino: test_pack), in the layout the launch's form reads"""
    Cout, Cin = w.shape[:2]
    K, N = (Cout, Cin) if dgrad else (Cin, Cout)
    return Staged(dev, 512, src=WR.pack_wino(w, dgrad, WR.wino_fused_ok(K, N)))


def workspace(ops, dev, B, H, W, Cin, Cout):
    nbytes = ops.query("tag_conv3x3_wino_ws_bytes", B, H, W, Cin, Cout)
    assert nbytes == WR.ws_bytes(B, H, W, Cin, Cout) and nbytes % 4 == 0
    return Staged(dev, 64, shape=(nbytes // 4,))


def check_workspace(name, ws, Cin, Cout):
    """fused form: ws is ignored (every float still NaN); plane form: V and M planes, every float written"""
    if WR.wino_fused_ok(Cin, Cout):
        ws.check(name, untouched=True)
    else:
        assert bool(torch.isfinite(ws.t).all()), f"{name}: a plane of the workspace was never written"


def run_forward(ops, dev, name, xs, us, pro, ss, ts, Cout, stats=True, v_keep=None):
    """one tag_conv3x3_wino_forward on staged operands: (y, statistics buffer or None, P)"""
    B, H, W, Cin = xs.shape
    g = (W + 2) * max(Cin, Cout)
    y = Staged(dev, g, shape=(B, H, W, Cout))
    rows = ops.query("tag_conv3x3_wino_stats_rows", B, H, W, Cout)
    st = Staged(dev, 3 * Cout + 1, shape=(rows * (3 * Cout + 1),)) if stats else None
    ws = workspace(ops, dev, B, H, W, Cin, Cout)
    ops.call("tag_conv3x3_wino_forward", P(ops, xs), P(ops, us), pro, P(ops, ss), P(ops, ts), P(ops, y), P(ops, st), B, H, W, Cin, Cout,
             P(ops, ws), P(ops, v_keep))
    done(ops, name, xs, us, ss, ts, y, st, ws, v_keep)
    if v_keep is None:
        check_workspace(name, ws, Cin, Cout)
    return y, st, rows


def stage_x(dev, x, s, t, pro, Cout):
    B, H, W, Cin = x.shape
    xs = Staged(dev, (W + 2) * max(Cin, Cout), src=x)
    ss, ts = (Staged(dev, 64, src=s), Staged(dev, 64, src=t)) if pro else (None, None)
    return xs, ss, ts


# ------------------------------------------------------------------------------------------------ 1. the weight pack
@pytest.mark.parametrize("Cin,Cout,tf,td", WR.PACK_CASES, ids=lambda v: str(v))
def test_pack(ops, dev, Cin, Cout, tf, td):
    """tag_pack_conv_weight_wino bit for bit in the layout each side's form reads (tiled where the fused kernel takes that side);
    with only one destination the other buffer is untouched"""
    w = torch.randn(Cout, Cin, 3, 3, generator=torch.Generator().manual_seed(Cin + 3 * Cout))
    ws = Staged(dev, 64, src=w)
    ref_f, ref_d = WR.pack_wino(w, False, bool(tf)), WR.pack_wino(w, True, bool(td))
    for want_f, want_d in ((True, True), (True, False), (False, True)):
        uf, ud = Staged(dev, 64, shape=(16 * Cin * Cout,)), Staged(dev, 64, shape=(16 * Cin * Cout,))
        ops.call("tag_pack_conv_weight_wino", P(ops, ws), P(ops, uf) if want_f else None, P(ops, ud) if want_d else None, Cin, Cout)
        done(ops, f"pack {Cin}->{Cout}", ws, uf, ud, untouched=[b for b, want in ((uf, want_f), (ud, want_d)) if not want])
        if want_f:
            assert torch.equal(bits(uf.t.cpu()), bits(ref_f)), "forward pack"
        if want_d:
            assert torch.equal(bits(ud.t.cpu()), bits(ref_d)), "dgrad pack"
    # (the two layouts of a side differ, so a pack that takes the other side's flag shows above)
    assert not tf or not torch.equal(ref_f, WR.pack_wino(w, False, False))
    assert not td or not torch.equal(ref_d, WR.pack_wino(w, True, False))


# ------------------------------------------------------------------------------------------------ 2. forward, EPI 0
def check_statistics(ops, dev, name, y, st, rows, case):
    """the partial rows of the kernel's own y: exact counts and pivots, empty rows zero, the fold against fp64"""
    B, H, W, Cout = y.shape
    yc, buf = y.cpu(), st.t.cpu()
    assert bool(torch.isfinite(buf).all()), f"{name}: not exactly P 3 Cout + P floats written"
    part, cnt = buf[:rows * 3 * Cout].view(rows, 3, Cout), buf[rows * 3 * Cout:]
    counts = WR.block_counts(B, H, W, Cout)
    assert len(counts) == rows and cnt.tolist() == [float(c) for c in counts], (name, cnt.tolist(), counts)
    for r, px in enumerate(WR.pivot_pixels(B, H, W, Cout)):
        if px is None:
            assert bool((part[r] == 0).all()), f"{name}: row {r} of an empty slot is not zero"
        else:
            assert torch.equal(bits(part[r, 0]), bits(yc[px[0], px[1], px[2]])), f"{name}: pivot of row {r}"
    mean, invstd, scale, shift = (torch.full((Cout,), float("nan"), device=dev) for _ in range(4))
    gam, bet = torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev)
    wsb = torch.empty(max(16, ops.query("tag_bn_stats_from_partials_ws_bytes", rows, Cout)) // 4 + 4, device=dev)
    ops.call("tag_bn_stats_from_partials", ops.ptr(st.t), rows, Cout, ops.ptr(gam), ops.ptr(bet), 1e-5, 0.1, None, None, ops.ptr(mean),
             ops.ptr(invstd), ops.ptr(scale), ops.ptr(shift), ops.ptr(wsb))
    done(ops, name + " fold", st)
    y64 = yc.double().view(-1, Cout)
    m64, v64 = y64.mean(0), y64.var(0, unbiased=False)
    y32 = yc.view(-1, Cout)
    norm = m64.abs().max().item() + v64.sqrt().max().item()
    e_m = (mean.cpu().double() - m64).abs().max().item() / norm
    f_m = (y32.mean(0).double() - m64).abs().max().item() / norm
    e_i = (invstd.cpu().double() * torch.sqrt(v64 + 1e-5) - 1.0).abs().max().item()
    f_i = ((1.0 / torch.sqrt(y32.var(0, unbiased=False) + 1e-5)).double() * torch.sqrt(v64 + 1e-5) - 1.0).abs().max().item()
    COUNT["comparisons"] += 2
    print(f"  {name + ' mean':70s} err {e_m:.2e}  fp32-cpu floor {f_m:.2e}  bound {WR.STAT_MEAN:.2e}")
    print(f"  {name + ' invstd':70s} err {e_i:.2e}  fp32-cpu floor {f_i:.2e}  bound {WR.STAT_INVSTD:.2e}")
    assert e_m <= WR.STAT_MEAN and e_i <= WR.STAT_INVSTD, (name, e_m, e_i)


@pytest.mark.parametrize("case", WR.FWD_CASES, ids=pid)
def test_forward_and_statistics_rows(ops, dev, case):
    """y against fp64; the statistics rows; the same y bits without a statistics buffer and on a second run"""
    B, H, W, Cin, Cout, pro, (kind, rows_claim, _) = case
    x, w, s, t, ref64, ref32 = WR.fwd_case(B, H, W, Cin, Cout, pro)
    name = f"fwd {kind} {pid(case)}"
    xs, ss, ts = stage_x(dev, x, s, t, pro, Cout)
    us = pack_u(dev, w)
    y, st, rows = run_forward(ops, dev, name, xs, us, pro, ss, ts, Cout)
    assert rows == rows_claim
    close(name + " y", y.t, ref64, ref32, WR.FWD)
    check_statistics(ops, dev, name, y.t, st, rows, case)
    y2, st2, _ = run_forward(ops, dev, name + " again", xs, us, pro, ss, ts, Cout)
    assert torch.equal(bits(y.t), bits(y2.t)) and torch.equal(bits(st.t), bits(st2.t)), f"{name}: two runs differ"
    y3, _, _ = run_forward(ops, dev, name + " no stats", xs, us, pro, ss, ts, Cout, stats=False)
    assert torch.equal(bits(y.t), bits(y3.t)), f"{name}: the statistics epilogue changed y"


@pytest.mark.parametrize("case", WR.BATCH_CASES, ids=pid)
def test_forward_rows_do_not_depend_on_the_batch(ops, dev, case):
    """rows 0..1 of the B = 3 launch are bit-equal to a B = 2 launch (the third image shares tile blocks with the second)"""
    B, H, W, Cin, Cout, pro = case
    x, w, s, t, _, _ = WR.fwd_case(B, H, W, Cin, Cout, pro)
    us = pack_u(dev, w)
    xs, ss, ts = stage_x(dev, x, s, t, pro, Cout)
    y3, _, _ = run_forward(ops, dev, f"batch {pid(case)}", xs, us, pro, ss, ts, Cout, stats=False)
    x2, _, _ = stage_x(dev, x[:2].contiguous(), s, t, pro, Cout)
    y2, _, _ = run_forward(ops, dev, f"batch {pid(case)} B 2", x2, us, pro, ss, ts, Cout, stats=False)
    assert torch.equal(bits(y3.t[:2]), bits(y2.t))


# ------------------------------------------------------------------------------------------------ 3. inference pooling, EPI 3
@pytest.mark.parametrize("case", WR.POOL_CASES, ids=lambda c: pid(c, 8))
def test_forward_bnrelu_pool_eval(ops, dev, case):
    """out = pool(relu(conv(prologue(x)) scale + shift)), floor windows, against fp64; bit-identical to the plain forward followed
    by tag_bnact_pool_forward (at the channel counts that entry serves: C / 4 divides 256) and on a second run"""
    B, H, W, Cin, Cout, pro, ph, pool, kind = case
    x, w, s, t, ref64, ref32 = WR.fwd_case(B, H, W, Cin, Cout, pro)
    sc, sh, _, _ = WR.bn_tables(Cout, H + W)
    name = f"pool {kind} {pid(case, 8)}"
    xs, ss, ts = stage_x(dev, x, s, t, pro, Cout)
    us, bsc, bsh = pack_u(dev, w), Staged(dev, 64, src=sc), Staged(dev, 64, src=sh)
    outs = []
    for _ in range(2):
        out, ws = Staged(dev, (W + 2) * Cout, shape=(B, H // ph, W // 2, Cout)), workspace(ops, dev, B, H, W, Cin, Cout)
        ops.call("tag_conv3x3_wino_forward_bnrelu_pool_eval", P(ops, xs), P(ops, us), pro, P(ops, ss), P(ops, ts), P(ops, out), P(ops, bsc),
                 P(ops, bsh), B, H, W, Cin, Cout, ph, 2, pool, P(ops, ws))
        done(ops, name, xs, us, ss, ts, out, bsc, bsh, ws)
        check_workspace(name, ws, Cin, Cout)
        outs.append(out.t)
    assert torch.equal(bits(outs[0]), bits(outs[1])), f"{name}: two runs differ"
    close(name, outs[0], R.bnrelu_pool(ref64, sc, sh, ph, pool), R.bnrelu_pool(ref32, sc, sh, ph, pool, F32), WR.FWD)
    if 256 % (Cout // 4) == 0:
        y, _, _ = run_forward(ops, dev, name + " plain", xs, us, pro, ss, ts, Cout, stats=False)
        two = Staged(dev, 64, shape=(B, H // ph, W // 2, Cout))
        ops.call("tag_bnact_pool_forward", P(ops, y), P(ops, bsc), P(ops, bsh), P(ops, two), B, H, W, Cout, ph, 2, 1, pool, 0.0, 0)
        done(ops, name + " two-pass", two, bsc, bsh)
        assert torch.equal(bits(outs[0]), bits(two.t)), "the one-kernel form must be bit-identical to conv + bnact_pool"


# ------------------------------------------------------------------------------------------------ 4. gradient epilogues, EPI 1 / 2
@pytest.mark.parametrize("case", WR.GRAD_CASES, ids=lambda c: pid(c, 11))
def test_dgrad_with_epilogue_sums(ops, dev, case):
    """da / dx against fp64 and bit-equal to the plain forward on the dgrad planes; (sum dz, sum dz xhat) through
    tag_bn_grad_from_partials against the fp64 statement on the kernel's OWN gradient with the exact masks (the fmaf of the ReLU
    mask and the first arg-max restated in fp32, the dropout keep mask from tag_dropout_mask_pooled); rows of empty slots are zero"""
    B, H, W, K, C, ph, pool, p, hx, wx, kind = case
    dy, w, ref64, ref32 = WR.dgrad_case(B, H, W, K, C)
    yref, sc, sh, mu, isd = WR.epi_inputs(B, H, W, C, ph, hx, wx)
    Hf, Wf = yref.shape[1:3]
    name = f"grad epi{2 if ph else 1} {kind} {pid(case, 10)}"
    g = (Wf + 2) * max(K, C)
    ds, us, ys = Staged(dev, g, src=dy), pack_u(dev, w, dgrad=True), Staged(dev, g, src=yref)
    tb = [Staged(dev, 64, src=v) for v in (sc, sh, mu, isd)]
    rows = ops.query("tag_conv3x3_wino_stats_rows", B, H, W, C)
    assert rows == WR.stats_rows(B, H, W, C)
    da, part, ws = Staged(dev, g, shape=(B, H, W, C)), Staged(dev, 2 * C, shape=(rows, 2, C)), workspace(ops, dev, B, H, W, K, C)
    if ph == 0:
        ops.call("tag_conv3x3_wino_dgrad_bnsums", P(ops, ds), P(ops, us), P(ops, da), P(ops, ys), *[P(ops, b) for b in tb], P(ops, part),
                 B, H, W, K, C, P(ops, ws))
    else:
        ops.call("tag_conv3x3_wino_dgrad_poolsums", P(ops, ds), P(ops, us), P(ops, da), P(ops, ys), *[P(ops, b) for b in tb], P(ops, part),
                 B, H, W, K, C, Hf, Wf, ph, 2, pool, float(p), WR.DROP_SEED, P(ops, ws))
    done(ops, name, ds, us, ys, da, part, ws, *tb)
    check_workspace(name, ws, K, C)
    close(name + " da", da.t, ref64, ref32, WR.FWD)
    plain, _, _ = run_forward(ops, dev, name + " plain", ds, us, 0, None, None, C, stats=False)
    assert torch.equal(bits(da.t), bits(plain.t)), f"{name}: the epilogue changed the gradient"
    pc = part.t.cpu()
    assert bool(torch.isfinite(pc).all()), f"{name}: not exactly P rows written"
    for r, tl in enumerate(WR.row_tiles(B, H, W, C)):
        if not tl:
            assert bool((pc[r] == 0).all()), f"{name}: row {r} of an empty slot is not zero"
    dg, db = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
    wsb = torch.empty(max(16, ops.query("tag_bn_grad_from_partials_ws_bytes", rows, C)) // 4 + 4, device=dev)
    ops.call("tag_bn_grad_from_partials", P(ops, part), rows, C, ops.ptr(dg), ops.ptr(db), ops.ptr(wsb))
    done(ops, name + " fold", part)
    own = da.t.cpu()
    if ph == 0:
        s64, s32 = X.bn_bwd_sums_x(own, yref, sc, sh, mu, isd), X.bn_bwd_sums_x(own, yref, sc, sh, mu, isd, F32)
    else:
        keep = ops.dropout_mask(WR.DROP_SEED, (B, H, W, C), p, dev, pooled=True).cpu() if p > 0 else None
        s64 = X.pool_bwd_sums_x(own, yref, sc, sh, mu, isd, ph, pool, keep, p)
        s32 = X.pool_bwd_sums_x(own, yref, sc, sh, mu, isd, ph, pool, keep, p, F32)
        if keep is not None:
            assert 0.6 < keep.float().mean().item() < 0.95
    # (dbeta = sum dz, dgamma = sum dz xhat; both of the larger of the two, as tests/test_gpu_wino.py normalises them)
    close(name + " sums", torch.cat([db.cpu(), dg.cpu()]), torch.cat(s64), torch.cat(s32), WR.SUMS)


# ------------------------------------------------------------------------------------------------ 5. weight gradients
def run_wgrad(ops, dev, name, xs, ss, ts, ds, pro, claim, v_saved=None):
    """tag_conv3x3_wino_wgrad twice on fresh NaN workspaces of exactly the queried size: dw"""
    B, H, W, Cin = xs.shape
    Cout = ds.shape[3]
    nbytes = ops.query("tag_conv3x3_wino_wgrad_ws_bytes", B, H, W, Cin, Cout)
    assert nbytes == WR.wgrad_ws_bytes(B, H, W, Cin, Cout), (name, nbytes)
    if claim[0] != "plane":
        assert nbytes == 2 * claim[1] * Cin * Cout * 9 * 4, f"{name}: S read back from the workspace size"
    outs = []
    for _ in range(2):
        dw, ws = Staged(dev, 64, shape=(Cout, Cin, 3, 3)), Staged(dev, 64, shape=(nbytes // 4,))
        ops.call("tag_conv3x3_wino_wgrad", None if v_saved is not None else P(ops, xs), pro, P(ops, ss), P(ops, ts), P(ops, ds), P(ops, dw),
                 B, H, W, Cin, Cout, P(ops, ws), P(ops, v_saved))
        done(ops, name, xs, ss, ts, ds, dw, ws, v_saved)
        # the row-split kernel writes 16 S raw products per (co, ci) of the 18 S floats the common formula reserves
        n_written = 16 * claim[1] * Cin * Cout if claim[0] == "rows" else nbytes // 4
        if v_saved is not None:                             # ws = [gradient planes | products]; the room of the input planes stays unused
            n_written = 16 * claim[3] * Cout + 16 * claim[1] * Cin * Cout
        assert bool(torch.isfinite(ws.t[:n_written]).all()), f"{name}: a partial of the workspace was never written"
        assert bool(torch.isnan(ws.t[n_written:]).all()), f"{name}: wrote more of the workspace than its form needs"
        outs.append(dw.t)
    assert torch.equal(bits(outs[0]), bits(outs[1])), f"{name}: two runs differ"
    return outs[0]


@pytest.mark.parametrize("case", WR.WGRAD_CASES, ids=pid)
def test_wgrad(ops, dev, case):
    """dw against fp64; the slice count through the workspace query; the second run bit-equal; the workspace guards intact"""
    B, H, W, Cin, Cout, pro, claim = case
    x, dy, s, t, ref64, ref32 = WR.wgrad_case(B, H, W, Cin, Cout, pro)
    name = f"wgrad {claim[0]} {pid(case)}"
    xs, ss, ts = stage_x(dev, x, s, t, pro, Cout)
    ds = Staged(dev, (W + 2) * max(Cin, Cout), src=dy)
    dw = run_wgrad(ops, dev, name, xs, ss, ts, ds, pro, claim)
    close(name, dw, ref64, ref32, WR.DW)


# ------------------------------------------------------------------------------------------------ 6. kept planes
@pytest.mark.parametrize("case", WR.KEEP_CASES, ids=pid)
def test_keep_planes(ops, dev, case):
    """v_keep: the forward -- fused or plane -- leaves B^T d B of the prologued input in the caller's buffer, bit for bit the
    statement, and y has the bits of the launch without; v_saved: the plane weight gradient on those planes (x = NULL) is
    bit-equal to the one that transforms x itself, and refused where the K slices need zero rows or the gradient is fused"""
    B, H, W, Cin, Cout, pro, _, reuse = case
    x, w, s, t, ref64, ref32 = WR.fwd_case(B, H, W, Cin, Cout, pro)
    name = f"keep {pid(case)}"
    T = WR.tiles(B, H, W)[2]
    xs, ss, ts = stage_x(dev, x, s, t, pro, Cout)
    us = pack_u(dev, w)
    vk = Staged(dev, 4 * Cin, shape=(16, T, Cin))
    y, _, _ = run_forward(ops, dev, name, xs, us, pro, ss, ts, Cout, stats=False, v_keep=vk)
    assert torch.equal(bits(vk.t.cpu()), bits(WR.input_planes(x, pro, s, t))), f"{name}: the kept planes"
    y0, _, _ = run_forward(ops, dev, name + " without", xs, us, pro, ss, ts, Cout, stats=False)
    assert torch.equal(bits(y.t), bits(y0.t))
    close(name + " y", y.t, ref64, ref32, WR.FWD)
    assert ops.query("tag_conv3x3_wino_wgrad_can_reuse_v", B, H, W, Cin, Cout) == reuse
    dy = WR.wgrad_case(B, H, W, Cin, Cout, pro)[1]
    ds = Staged(dev, (W + 2) * max(Cin, Cout), src=dy)
    if reuse:
        claim = ("plane", *WR.wino_wg_geom(B, H, W, Cin, Cout))
        dw = run_wgrad(ops, dev, name + " wgrad", xs, ss, ts, ds, pro, claim)
        vs = Staged(dev, 4 * Cin, src=vk.t.cpu())
        dw_kept = run_wgrad(ops, dev, name + " wgrad v_saved", xs, ss, ts, ds, pro, claim, v_saved=vs)
        assert torch.equal(bits(dw), bits(dw_kept))
        close(name + " dw", dw, WR.wgrad_case(B, H, W, Cin, Cout, pro)[4], WR.wgrad_case(B, H, W, Cin, Cout, pro)[5], WR.DW)
    else:
        nbytes = ops.query("tag_conv3x3_wino_wgrad_ws_bytes", B, H, W, Cin, Cout)
        dw, ws = Staged(dev, 64, shape=(Cout, Cin, 3, 3)), Staged(dev, 64, shape=(nbytes // 4,))
        for xp in (None, P(ops, xs)):
            refused(ops, "tag_conv3x3_wino_wgrad", xp, pro, P(ops, ss), P(ops, ts), P(ops, ds), P(ops, dw), B, H, W, Cin, Cout, P(ops, ws),
                    P(ops, vk))
        done(ops, name + " v_saved refused", xs, ds, vk, untouched=(dw, ws))


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_outputs_untouched(ops, dev):
    """Every entry point with one argument wrong on an otherwise valid call: rc = -1 before any launch, every output untouched"""
    B, H, W, Cin, Cout = 2, 4, 6, 64, 64
    x, w, s, t, _, _ = WR.fwd_case(B, H, W, Cin, Cout, 1)
    yref, sc, sh, mu, isd = WR.epi_inputs(B, H, W, Cout, 2, 1, 1)
    xs, ss, ts = stage_x(dev, x, s, t, 1, Cout)
    us, ys = pack_u(dev, w), Staged(dev, 64, src=yref)
    tb = [Staged(dev, 64, src=v) for v in (sc, sh, mu, isd)]
    y, out, dw = Staged(dev, 64, shape=(B, H, W, Cout)), Staged(dev, 64, shape=(B, H, W // 2, Cout)), Staged(dev, 64, shape=(Cout, Cin, 3, 3))
    part = Staged(dev, 64, shape=(4, 3 * Cout + 1))
    ws = Staged(dev, 64, shape=(ops.query("tag_conv3x3_wino_wgrad_ws_bytes", B, H, W, Cin, Cout) // 4,))
    vk = Staged(dev, 64, shape=(16, WR.tiles(B, H, W)[2], Cin))
    X_, U_, S_, T_, Y_, O_, D_, PT, WS, YR = (P(ops, b) for b in (xs, us, ss, ts, y, out, dw, part, ws, ys))
    TB = [P(ops, b) for b in tb]
    Hf, Wf = 2 * H + 1, 2 * W + 1
    dims = {"ok": (B, H, W, Cin, Cout), "Cin 48": (B, H, W, 48, Cout), "Cout 96": (B, H, W, Cin, 96), "Cout 2048": (B, H, W, Cin, 2048),
            "B 0": (0, H, W, Cin, Cout)}
    n = 0
    for tag, d in dims.items():
        if tag == "ok":
            continue
        refused(ops, "tag_conv3x3_wino_forward", X_, U_, 1, S_, T_, Y_, PT, *d, WS, None)
        refused(ops, "tag_conv3x3_wino_forward_bnrelu_pool_eval", X_, U_, 1, S_, T_, O_, TB[0], TB[1], *d, 2, 2, 0, WS)
        refused(ops, "tag_conv3x3_wino_dgrad_bnsums", X_, U_, Y_, YR, *TB, PT, *d, WS)
        refused(ops, "tag_conv3x3_wino_dgrad_poolsums", X_, U_, Y_, YR, *TB, PT, *d, Hf, Wf, 2, 2, 0, 0.0, 0, WS)
        refused(ops, "tag_conv3x3_wino_wgrad", X_, 1, S_, T_, X_, D_, *d, WS, None)
        n += 5
    ok = dims["ok"]
    for pro, sp in ((4, S_), (1, None), (-1, S_)):
        refused(ops, "tag_conv3x3_wino_forward", X_, U_, pro, sp, T_, Y_, PT, *ok, WS, None)
        refused(ops, "tag_conv3x3_wino_forward_bnrelu_pool_eval", X_, U_, pro, sp, T_, O_, TB[0], TB[1], *ok, 2, 2, 0, WS)
        refused(ops, "tag_conv3x3_wino_wgrad", X_, pro, sp, T_, X_, D_, *ok, WS, None)
        n += 3
    for ph, pw, pool in ((2, 1, 0), (3, 2, 0), (2, 2, 1)):
        refused(ops, "tag_conv3x3_wino_forward_bnrelu_pool_eval", X_, U_, 1, S_, T_, O_, TB[0], TB[1], *ok, ph, pw, pool, WS)
        refused(ops, "tag_conv3x3_wino_dgrad_poolsums", X_, U_, Y_, YR, *TB, PT, *ok, Hf, Wf, ph, pw, pool, 0.0, 0, WS)
        n += 2
    refused(ops, "tag_conv3x3_wino_dgrad_poolsums", X_, U_, Y_, YR, *TB, PT, *ok, Hf, Wf, 2, 2, 0, 1.0, 0, WS)                 # drop_p = 1
    refused(ops, "tag_conv3x3_wino_dgrad_poolsums", X_, U_, Y_, YR, *TB, PT, *ok, Hf + 1, Wf, 2, 2, 0, 0.0, 0, WS)             # H != Hf / ph
    refused(ops, "tag_conv3x3_wino_dgrad_poolsums", X_, U_, Y_, YR, *TB, PT, *ok, H + 1, Wf, 1, 2, 0, 0.0, 0, WS)              # ph = 1: no row over
    refused(ops, "tag_conv3x3_wino_forward_bnrelu_pool_eval", X_, U_, 1, S_, T_, O_, TB[0], TB[1], B, 1, W, Cin, Cout, 2, 2, 0, WS)   # H = 1, ph = 2
    refused(ops, "tag_conv3x3_wino_forward_bnrelu_pool_eval", X_, U_, 1, S_, T_, O_, TB[0], TB[1], B, H, 1, Cin, Cout, 1, 2, 0, WS)   # W = 1
    refused(ops, "tag_conv3x3_wino_wgrad", X_, 1, S_, T_, X_, D_, *ok, WS, P(ops, vk))                                         # v_saved, fused shape
    refused(ops, "tag_conv3x3_wino_wgrad", None, 1, S_, T_, X_, D_, *ok, WS, None)                                             # neither x nor v_saved
    refused(ops, "tag_conv3x3_wino_forward", X_, U_, 1, S_, T_, None, PT, *ok, WS, None)
    wsrc = Staged(dev, 64, src=w)
    refused(ops, "tag_pack_conv_weight_wino", P(ops, wsrc), None, None, Cin, Cout)                                             # both NULL
    refused(ops, "tag_pack_conv_weight_wino", P(ops, wsrc), Y_, None, 0, Cout)
    n += 10
    done(ops, f"{n} refused calls", xs, us, ss, ts, ys, wsrc, *tb, untouched=(y, out, dw, part, ws, vk))
