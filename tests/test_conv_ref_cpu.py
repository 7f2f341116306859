"""No GPU: the fp64 statements of tests/conv_ref.py against F.conv2d, autograd, F.batch_norm and the torch pools (1e-12); every
claim of the case tables of tests/test_gpu_conv_sweep.py re-derived from the launchers' formulas restated in Python; the input
condition of the cases (the fp32 floor is at most a quarter of the bound); the index arithmetic of the per-tap weight gradient's
chunk loader, fixed and as the parent commit had it; and the calls the entry points refuse before any HIP call."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

F64, F32 = torch.float64, torch.float32


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def torch_pro(v, p, s, t):
    s, t = s.double().view(1, -1, 1, 1), t.double().view(1, -1, 1, 1)
    return {0: lambda: v, 1: lambda: F.relu(v * s + t), 2: lambda: F.leaky_relu(v, 0.1) * s + t, 3: lambda: v * s + t}[p]()


# ------------------------------------------------------------------------------------------------ statements
@pytest.mark.parametrize("pro", [0, 1, 2, 3])
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 5, 3, 8, 12), (3, 1, 1, 4, 4), (1, 1, 7, 4, 8), (2, 6, 1, 8, 4)])
def test_conv_statements_against_torch(B, H, W, Cin, Cout, pro):
    x, w, dy, s, t = R.conv_inputs(B, H, W, Cin, Cout, 11 + pro)
    xd, wd = nchw(x).double().requires_grad_(True), w.double().requires_grad_(True)
    a = torch_pro(xd, pro, s, t)
    a.retain_grad()
    y = F.conv2d(a, wd, None, 1, 1)
    y.backward(nchw(dy).double())
    assert R.relerr(R.conv_fwd(x, w, pro, s, t), nhwc(y)) < 1e-12
    assert R.relerr(R.conv_dgrad(dy, w), nhwc(a.grad)) < 1e-12
    assert R.relerr(R.conv_wgrad(x, dy, pro, s, t), wd.grad) < 1e-12
    # the packs: the forward entry on the forward pack is the convolution, on the dgrad pack the data gradient
    assert torch.equal(R.unpack(R.pack_fwd(w)), w)
    assert R.pack_dgrad(w).shape == (9, Cout, Cin) and R.pack_dgrad(w)[0, 1, 2] == w[1, 2, 2, 2]
    # zero padding AFTER the prologue: padding first differs wherever the shift is non-zero
    if pro and H * W > 1:
        before = nhwc(F.conv2d(F.pad(torch_pro(F.pad(nchw(x).double(), (1, 1, 1, 1)), pro, s, t), (0, 0, 0, 0)), w.double()))
        assert R.relerr(before, nhwc(y)) > 1e-3
    bias = torch.randn(B, Cout, generator=torch.Generator().manual_seed(1))
    assert R.relerr(R.conv_fwd(x, w, pro, s, t, bias=bias), nhwc(y) + bias.double()[:, None, None, :]) < 1e-12


def test_statistics_and_epilogue_statements_against_torch():
    g = torch.Generator().manual_seed(5)
    B, Hf, Wf, C = 3, 7, 6, 8
    y = torch.randn(B, Hf, Wf, C, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    mean, invstd = R.bn_fold(y.double())
    yn = nchw(y).double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a = F.relu(F.batch_norm(yn, None, None, gd, bd, True, 0.1, 1e-5))
    assert R.relerr(torch.relu((y.double() - mean) * invstd * gamma.double() + beta.double()), nhwc(a)) < 1e-12
    scale, shift = gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd
    # BatchNorm+ReLU backward: dbeta = sum dz, dgamma = sum dz xhat
    da = torch.randn(B, Hf, Wf, C, generator=g)
    a.backward(nchw(da).double())
    s1, s2 = R.bn_bwd_sums(da, y, scale, shift, mean, invstd)
    assert R.relerr(s1, bd.grad) < 1e-12 and R.relerr(s2, gd.grad) < 1e-12
    # the partial-statistics fold: two ragged parts with pivots
    v = y.double().reshape(-1, C)
    parts = [v[:50], v[50:]]
    rows = torch.stack([torch.stack([p.mean(0).float().double(), (p - p.mean(0).float().double()).sum(0),
                                     ((p - p.mean(0).float().double()) ** 2).sum(0)]) for p in parts])
    buf = torch.cat([rows.reshape(-1), torch.tensor([50.0, v.shape[0] - 50.0], dtype=F64)])
    m2, i2, n = R.fold_stats_partials(buf, 2, C)
    assert n == v.shape[0] and R.relerr(m2, mean) < 1e-12 and R.relerr(i2, invstd) < 1e-12
    # pool(relu(bn(.))) with floor windows, the three kinds, and its backward sums (odd Hf with ph = 2 drops a row)
    for ph in (1, 2):
        for pool in (0, 2, 3):
            yn = nchw(y).double().requires_grad_(True)
            gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
            z = F.relu(F.batch_norm(yn, None, None, gd, bd, True, 0.1, 1e-5))
            ref = {0: F.avg_pool2d(z, (ph, 2)) + F.max_pool2d(z, (ph, 2)), 2: F.avg_pool2d(z, (ph, 2)), 3: F.max_pool2d(z, (ph, 2))}[pool]
            assert R.relerr(R.bnrelu_pool(y, scale, shift, ph, pool), nhwc(ref)) < 1e-12
            dx = torch.randn(B, Hf // ph, Wf // 2, C, generator=g)
            keep = (torch.rand(dx.shape, generator=g) > 0.3).double()
            (ref * nchw(keep) / 0.7).backward(nchw(dx).double())
            s1, s2 = R.pool_bwd_sums(dx, y, scale, shift, mean, invstd, ph, pool, keep, 0.3)
            assert R.relerr(s1, bd.grad) < 1e-12 and R.relerr(s2, gd.grad) < 1e-12


@pytest.mark.parametrize("affine", [True, False])
def test_c1_statements_against_torch(affine):
    B, H, W, Cout = 2, 5, 6, 8
    x, cs, ct, w, dy = R.c1_inputs(B, H, W, Cout, 3)
    if not affine:
        cs = ct = None
    xin = (x.double() * cs.double() + ct.double() if affine else x.double()).unsqueeze(1).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    y = F.conv2d(xin, wd, None, 1, 1)
    y.backward(nchw(dy).double())
    assert R.relerr(R.c1_fwd(x, w, cs, ct), nhwc(y)) < 1e-12
    assert R.relerr(R.c1_wgrad(x, dy, cs, ct), wd.grad) < 1e-12
    assert R.relerr(R.c1_dgrad(dy, w), xin.grad[:, 0]) < 1e-12
    bias = torch.randn(B, Cout, generator=torch.Generator().manual_seed(2))
    assert R.relerr(R.c1_fwd(x, w, cs, ct, bias=bias), nhwc(y) + bias.double()[:, None, None, :]) < 1e-12


# ------------------------------------------------------------------------------------------------ claims of the tables
def test_pack_cases_reach_the_second_grid_stride_trip():
    assert {c[0] for c in R.PACK_CASES} >= {32, 96} and {c[1] for c in R.PACK_CASES} >= {4, 68}
    assert any(9 * ci * co > R.PACK_GRID_ELEMS for ci, co in R.PACK_CASES)


def test_halo_case_claims():
    seen_rt, seen_nt, hs = set(), set(), {w: set() for w in R.HALO_W}
    for B, H, W, Cin, Cout, pro, claim in R.HALO_CASES:
        g = R.halo_geom(H, W, Cout)
        assert R.fwd_kernel(W, Cout)[0] == "halo" and Cin % 32 == 0 and Cout % 4 == 0
        assert (g["BN"], g["TW"], g["row_tiles"], g["n_tiles"]) == claim, ((B, H, W, Cin, Cout), g)
        assert R.stats_rows(B, H, W) == B * g["row_tiles"] * 2
        hs[W].add(H)
        if B == 3:
            seen_rt.add(g["row_tiles"])
        seen_nt.add(g["n_tiles"])
        # the multiply-shift division the kernel uses gives L / n_tiles and mt / row_tiles over the whole grid
        for L in range(B * g["row_tiles"] * g["n_tiles"]):
            assert R.magic_div(L, g["n_tiles"]) == L // g["n_tiles"]
            assert R.magic_div(L // g["n_tiles"], g["row_tiles"]) == (L // g["n_tiles"]) // g["row_tiles"]
    for W in R.HALO_W:
        TH = R.halo_geom(1, W, 64)["TH"]
        assert hs[W] >= {1, TH - 1, TH, TH + 1, 2 * TH + 1}, (W, hs[W])
    assert seen_rt >= {3, 5, 7} and seen_nt >= {1, 2, 3}
    cases = R.HALO_CASES
    assert {c[3] for c in cases} >= {32, 96, 512} and {c[4] for c in cases} >= {4, 36, 64, 68, 128, 132, 320}
    assert {c[5] for c in cases} == {0, 1, 2, 3} and {c[0] for c in cases} == {1, 3}
    for B, H, W, Cin, Cout, pro in R.HALO256_CASES:
        assert R.halo_geom(H, W, Cout, stats_or_epi=True)["BN"] == 256 and R.halo_geom(H, W, Cout)["BN"] == 128
    assert {(c[2], c[4]) for c in R.HALO256_CASES} >= {(8, 256), (16, 512)}


def test_every_selectable_instantiation_is_in_a_table():
    """<BN, PRO, TW, EPI> of the halo-tile kernel, <BN, PRO> of the tap-by-tap forward, <TC, PRO> of the per-tap weight gradient and
    <TW, PRO> of the all-taps and row-ring kernels: whatever a launcher can select with the default options is launched by the
    default process of the sweep (the kernel trace in docs/experiments_conv_sweep.md shows the same from the GPU's side)"""
    want, have = R.selectable_instantiations(), R.table_instantiations()
    for k in want:
        assert want[k] <= have[k], (k, sorted(want[k] - have[k]))
        assert have[k] <= want[k], (k, sorted(have[k] - want[k]))
    assert len(want["halo"]) == 44 + 8 + 8 + 12 + 4
    for B, H, W, Cin, Cout, pro in R.HALO_INST_CASES:
        assert R.halo_geom(H, W, Cout, stats_or_epi=True)["BN"] == Cout


def test_magic_division_is_exact_for_every_divisor_a_launch_can_have():
    for d in range(1, 300):
        for n in list(range(0, 4 * d + 3)) + [2 ** 20 + 7, 2 ** 31 - 1]:
            assert R.magic_div(n, d) == n // d, (n, d)


def test_tap_forward_case_claims():
    for B, H, W, Cin, Cout, pro, M in R.TAP_FWD_CASES:
        assert R.fwd_kernel(W, Cout) == ("tap", 128 if Cout >= 128 else 64) and B * H * W == M
    cases = R.TAP_FWD_CASES
    assert {c[2] for c in cases} >= {1, 2, 3, 5, 12, 20, 40, 65, 128}
    ms = {c[6] for c in cases}
    assert any(m < 128 for m in ms) and 128 in ms and any(128 < m <= 132 for m in ms) and any(c[1] == 1 for c in cases)
    assert {c[4] for c in cases} >= {36, 64, 128, 132} and {c[5] for c in cases} == {0, 1, 2, 3}
    # with TAG_CONV_IMPL=1 the halo rows run here too
    assert all(R.fwd_kernel(c[2], c[4], conv_impl=1)[0] == "tap" for c in R.HALO_CASES)


def test_bias_cases_are_the_served_pairs():
    assert {(c[2], c[3]) for c in R.BIAS_CASES} == {(16, 32), (16, 128), (4, 32), (4, 128)}
    assert {c[4] for c in R.BIAS_CASES} == {2, 3} and all(c[0] == 3 for c in R.BIAS_CASES)


def test_alltaps_case_claims():
    for B, H, W, Cin, Cout, pro, (splits, cps, crosses) in R.ALLTAPS_CASES:
        s, c, per_image = R.alltaps_splits(B, H, W, Cin, Cout)
        assert R.wgrad_kernel(W, Cin, Cout) == ("ring" if W >= 16 else "alltaps", W)
        assert (s, c) == (splits, cps), ((B, H, W, Cin, Cout), s, c)
        # a split crosses an image when one of its chunk ranges [i cps, (i + 1) cps) holds a multiple of per_image inside it
        cross = any((i * c) // per_image != (min((i + 1) * c, B * per_image) - 1) // per_image for i in range(s))
        assert cross == crosses, ((B, H, W, Cin, Cout), cross)
        assert R.wgrad_ws_bytes(B, H, W, Cin, Cout) == s * 9 * Cin * Cout * 4
    cases = R.ALLTAPS_CASES
    assert {c[2] for c in cases} == set(R.HALO_W) and {c[1] for c in cases} >= {1, 2, 3, 5, 37, 41}
    assert {c[3] for c in cases} | {c[4] for c in cases} >= {4, 36, 64, 96, 132} and {c[5] for c in cases} == {0, 1, 2, 3}
    # the issue's two examples: (3, 37, 8) splits into whole images, (3, 41, 8) into 9 + 9 + 9 + 6 chunks across images
    s, c, per = R.alltaps_splits(3, 37, 8, 96, 132)
    assert per == 10 and c == per and s == 3
    s, c, per = R.alltaps_splits(3, 41, 8, 36, 4)
    assert (s, c, per) == (4, 9, 11) and 3 * per - 3 * c == 6


def test_tap_wgrad_case_claims():
    for B, H, W, Cin, Cout, pro, (TC, splits, chunk) in R.TAP_WGRAD_CASES:
        assert R.wgrad_kernel(W, Cin, Cout) == ("tap", TC)
        assert R.wgrad_splits(B * H * W, Cin, Cout) == (splits, chunk), ((B, H, W, Cin, Cout), R.wgrad_splits(B * H * W, Cin, Cout))
    cases = R.TAP_WGRAD_CASES
    assert {c[2] for c in cases} >= {1, 3, 5, 7, 12, 20, 40} and {c[6][0] for c in cases} == {64, 128}
    assert any((c[0] * c[1] * c[2]) % 32 for c in cases) and {c[5] for c in cases} == {0, 1, 2, 3}
    ragged = [c for c in cases if c[6][1] == 2 and (c[0] * c[1] * c[2]) % c[6][2]]
    assert (3, 41, 5) in {c[:3] for c in ragged}
    # with TAG_CONV_IMPL=1 the all-taps rows run on the per-tap kernel, in both tile sizes
    assert {R.wgrad_kernel(c[2], c[3], c[4], conv_impl=1) for c in R.ALLTAPS_CASES} == {("tap", 64), ("tap", 128)}


def test_tap_wgrad_chunk_loader_index_arithmetic():
    """The fixed row wrap locates every pixel of every chunk on (m % (H W)) / W, m % W -- for the tiny images and everywhere else;
    the parent's single subtraction mis-locates pixels exactly where a chunk spans two image boundaries."""
    B = 3
    for H in range(1, 9):
        for W in list(range(1, 33)) + [40, 63]:
            assert R.tap_mislocated(B, H, W, "mod") == 0, (H, W)
            assert (R.tap_mislocated(B, H, W, "once") > 0) == R.spans_two_boundaries(B, H, W), (H, W)
    bad = {(H, W) for H in range(1, 9) for W in range(1, 33) if R.tap_mislocated(B, H, W, "once")}
    assert {(1, w) for w in range(1, 13)} <= bad and {(2, w) for w in range(1, 8)} <= bad and {(3, w) for w in range(1, 6)} <= bad
    assert {(4, 1), (4, 2), (4, 3), (5, 1), (5, 2), (5, 3), (7, 1), (7, 2)} <= bad
    assert not bad & {(7, 5), (5, 7)} and not any(w >= 20 for _, w in bad)
    for B_, H, W in R.TINY_WGRAD:
        assert R.spans_two_boundaries(B_, H, W) and R.tap_mislocated(B_, H, W, "once") > 0 and R.tap_mislocated(B_, H, W, "mod") == 0
        assert R.wgrad_kernel(W, 32, 64)[0] == "tap"
    for B_, H, W in R.TINY_CONTROLS:
        assert not R.spans_two_boundaries(B_, H, W) and R.tap_mislocated(B_, H, W, "once") == 0
        # bit-identity of the fix there: the two formulas give the same (row, column) for every pixel slot, masked ones included
        for kb in range(0, B_ * H * W, 32):
            assert R.tap_chunk_rows(B_, H, W, kb, "mod") == R.tap_chunk_rows(B_, H, W, kb, "once")


def test_c1_case_claims():
    for B, H, W, Cout, kernel in R.C1_FWD_CASES:
        assert R.c1_fwd_kernel(W, Cout) == kernel, (W, Cout)
    assert {c[4] for c in R.C1_FWD_CASES} == {"rows", "fwd4", "generic"}
    assert {(c[2], c[3]) for c in R.C1_FWD_CASES} >= {(62, 64), (8, 12)} and {c[3] for c in R.C1_FWD_CASES} >= {4, 32, 128}
    for B, H, W, Cout in R.C1_BIAS_CASES:
        assert R.c1_fwd_kernel(W, Cout) in ("fwd4", "rows") and W % 4 == 0 and 256 % (Cout // 4) == 0
        assert H * W // 4 < 256 // (Cout // 4) and B >= 2            # a workgroup's first trip holds pixel groups of two clips
    for B, H, W, Cout, (kernel, blocks) in R.C1_WGRAD_CASES:
        nblk, rpi = R.c1_wgrad_blocks(B * H * W, Cout)
        assert ("wgrad4" if W % 4 == 0 else "generic") == kernel and nblk == blocks, ((B, H, W, Cout), nblk)
    assert {c[3] for c in R.C1_WGRAD_CASES} >= {4, 256}
    assert {k for *_, (k, n) in R.C1_WGRAD_CASES if n == 1} == {"wgrad4", "generic"}     # M below one block's first trip
    big = [c for c in R.C1_WGRAD_CASES if c[0] * c[1] * c[2] > 1024 * R.c1_wgrad_blocks(1, c[3])[1] * 64]
    assert {c[4][0] for c in big} == {"wgrad4", "generic"}
    assert {h for _, h in R.C1_BWD_CASES} >= {1, 7, 8, 9}
    assert R.c1_bwd_geom(2, 1) == (1, 8) and R.c1_bwd_geom(3, 9) == (2, 8) and R.c1_bwd_geom(300, 9) == (2, 8)


def test_c1_entries_live_in_conv_c1():
    """the Cin = 1 convolution is its own translation unit: built with the library, every tag_conv3x3_c1_* entry of the
    signature table defined there and none left behind in conv.hip (whose private builds then no longer compile them)"""
    from texttoaudiogrounding_amd import lib
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "texttoaudiogrounding_amd", "csrc")
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert "conv_c1.hip" in srcs and "conv.hip" in srcs
    names = [s for s in lib.declared_symbols() if s.startswith("tag_conv3x3_c1_")]
    assert len(names) == 13
    defined = lambda f: set(re.findall(r'^extern "C" \w+ (tag_\w+)\(', open(os.path.join(csrc, f)).read(), re.M))
    assert set(names) <= defined("conv_c1.hip") and not any("_c1_" in s for s in defined("conv.hip"))
    assert defined("conv.hip") >= {"tag_conv3x3_forward", "tag_conv3x3_wgrad"}


def test_epilogue_case_claims():
    for B, H, W, Cin, Cout in R.BNSUMS_CASES:
        assert W in (8, 16, 32, 64) and Cin % 32 == 0 and Cout % 4 == 0
    assert {c[4] for c in R.BNSUMS_CASES} >= {68, 132} <= {c[4] for c in R.POOLSUMS_CASES}
    assert any(c[1] < R.halo_geom(1, c[2], 64)["TH"] for c in R.BNSUMS_CASES) and any(c[2] == 64 for c in R.BNSUMS_CASES)
    for B, Hf, Wf, Cin, Cout, ph, pool in R.POOLSUMS_CASES:
        assert Wf // 2 in (8, 16, 32, 64) and Cin % 32 == 0 and Cout % 4 == 0
    assert any(c[1] % 2 and c[5] == 2 for c in R.POOLSUMS_CASES) and any(c[2] == 128 for c in R.POOLSUMS_CASES)
    assert {c[6] for c in R.POOLSUMS_CASES} == {0, 2, 3} == {c[7] for c in R.POOLEVAL_CASES}
    assert any(c[1] % 2 and c[5] == 2 for c in R.POOLEVAL_CASES) and any(c[2] == 64 for c in R.POOLEVAL_CASES)


# ------------------------------------------------------------------------------------------------ input condition
def _floor_ok(ref64, ref32, bound, name):
    floor = R.relerr(ref32, ref64)
    assert floor <= bound / 4, (name, floor, bound)


@pytest.mark.parametrize("case", R.HALO_CASES + [c + (None,) for c in R.HALO256_CASES + R.HALO_INST_CASES] + R.TAP_FWD_CASES,
                         ids=lambda c: "-".join(map(str, c[:6])))
def test_forward_input_condition(case):
    B, H, W, Cin, Cout, pro = case[:6]
    x, w, dy, s, t = R.conv_inputs(B, H, W, Cin, Cout, 100 + W + H)
    _floor_ok(R.conv_fwd(x, w, pro, s, t), R.conv_fwd(x, w, pro, s, t, F32), R.FWD, case)


@pytest.mark.parametrize("case", R.ALLTAPS_CASES + R.TAP_WGRAD_CASES + [c + (32, 64, 1, None) for c in R.TINY_WGRAD + R.TINY_CONTROLS],
                         ids=lambda c: "-".join(map(str, c[:6])))
def test_wgrad_input_condition(case):
    B, H, W, Cin, Cout, pro = case[:6]
    x, w, dy, s, t = R.conv_inputs(B, H, W, Cin, Cout, 100 + W + H)
    _floor_ok(R.conv_wgrad(x, dy, pro, s, t), R.conv_wgrad(x, dy, pro, s, t, F32), R.FWD, case)


@pytest.mark.parametrize("case", [c for c in R.C1_FWD_CASES] + [c for c in R.C1_WGRAD_CASES if c[0] * c[1] * c[2] < 10000],
                         ids=lambda c: "-".join(map(str, c[:4])))
def test_c1_input_condition(case):
    B, H, W, Cout = case[:4]
    x, cs, ct, w, dy = R.c1_inputs(B, H, W, Cout, 7)
    _floor_ok(R.c1_fwd(x, w, cs, ct), R.c1_fwd(x, w, cs, ct, F32), R.C1, case)
    _floor_ok(R.c1_dgrad(dy, w), R.c1_dgrad(dy, w, F32), R.C1, case)


# ------------------------------------------------------------------------------------------------ refused calls (no HIP call)
TAG_EINVAL = -1


@pytest.fixture(scope="module")
def handle():
    from texttoaudiogrounding_amd import lib
    return lib.load()


def _buf(n=64):
    return (ctypes.c_float * n)()


def test_c1_entries_refuse_empty_shapes_before_dividing(handle):
    """Cout = 0 used to be a host division by zero (256 % (Cout / 4), 64 % (Cout / 4)); B, H, W were not checked at all"""
    x, w, y, ws = _buf(), _buf(), _buf(), _buf()
    p = lambda b: ctypes.addressof(b)
    for B, H, W, Cout in [(1, 1, 4, 0), (0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, -4), (-1, 1, 4, 4)]:
        assert handle.tag_conv3x3_c1_forward(p(x), None, None, p(w), p(y), B, H, W, Cout, None) == TAG_EINVAL
        assert handle.tag_conv3x3_c1_wgrad(p(x), None, None, p(y), p(w), B, H, W, Cout, p(ws), None) == TAG_EINVAL
        assert handle.tag_conv3x3_c1_dgrad(p(y), p(w), p(x), B, H, W, Cout, None) == TAG_EINVAL
        assert handle.tag_conv3x3_c1_forward_bias(p(x), None, None, p(w), p(w), p(y), B, H, W, Cout, None) == TAG_EINVAL
        assert b"check failed" in handle.tag_last_error() or b"unserved" in handle.tag_last_error()
    # and what the weight gradient and dgrad do not serve: Cout / 4 must divide 64
    assert handle.tag_conv3x3_c1_wgrad(p(x), None, None, p(y), p(w), 1, 1, 4, 12, p(ws), None) == TAG_EINVAL
    assert handle.tag_conv3x3_c1_dgrad(p(y), p(w), p(x), 1, 1, 4, 260, None) == TAG_EINVAL
    # one of the affine pair alone
    assert handle.tag_conv3x3_c1_forward(p(x), p(w), None, p(w), p(y), 1, 1, 4, 4, None) == TAG_EINVAL
    assert all(v == 0.0 for v in y) and all(v == 0.0 for v in x)


def test_conv_entries_refuse_unserved_arguments(handle):
    x, w, y, ws = _buf(), _buf(), _buf(), _buf()
    p = lambda b: ctypes.addressof(b)
    fwd = lambda *a: handle.tag_conv3x3_forward(p(x), p(w), *a, None)
    assert fwd(0, None, None, p(y), p(ws), 1, 1, 5, 32, 64) == TAG_EINVAL            # statistics where no halo tile serves the width
    assert fwd(0, None, None, p(y), None, 1, 1, 8, 48, 64) == TAG_EINVAL             # Cin % 32
    assert fwd(0, None, None, p(y), None, 1, 1, 8, 32, 6) == TAG_EINVAL              # Cout % 4
    assert fwd(0, None, None, p(y), None, 1, 1, 8, 544, 64) == TAG_EINVAL            # Cin > 512
    assert fwd(4, p(w), p(w), p(y), None, 1, 1, 8, 32, 64) == TAG_EINVAL             # prologue 4
    assert fwd(1, None, None, p(y), None, 1, 1, 8, 32, 64) == TAG_EINVAL             # prologue without its table
    assert fwd(0, None, None, p(y), None, 0, 1, 8, 32, 64) == TAG_EINVAL
    wg = lambda *a: handle.tag_conv3x3_wgrad(p(x), 0, None, None, p(y), p(w), *a, p(ws), None)
    assert wg(1, 1, 65, 32, 64) == TAG_EINVAL and wg(1, 1, 8, 6, 64) == TAG_EINVAL and wg(1, 0, 8, 32, 64) == TAG_EINVAL
    bias = lambda pro, B, H, W, Cin, Cout: handle.tag_conv3x3_forward_bias(p(x), p(w), pro, p(w), p(w), p(w), p(y), B, H, W, Cin, Cout, None)
    for args in [(2, 1, 1, 8, 32, 128), (2, 1, 1, 16, 64, 128), (2, 1, 1, 16, 32, 64), (1, 1, 1, 16, 32, 128), (0, 1, 1, 4, 128, 128),
                 (2, 0, 1, 16, 32, 128), (3, 1, 1, 32, 128, 128)]:
        assert bias(*args) == TAG_EINVAL, args
    assert all(v == 0.0 for v in y) and all(v == 0.0 for v in ws)
