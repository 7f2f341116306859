"""tests/wino_ref.py without a GPU: the restated launcher formulas against the library's own host queries (they launch nothing),
every claim of every case of the tables against the formulas, the tables against the set of selectable kernel instantiations, the
weight pack against a scalar restatement and against G g G^T, the statements against F.conv2d / autograd, the no-double-rounding
condition of every prologue and mask, and the fp32 floor of every case against a quarter of its GPU bound."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import tag_oracle as O
from tests import conv_ref as R
from tests import conv_x3_ref as X
from tests import wino_ref as WR

F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def handle():
    from texttoaudiogrounding_amd import lib
    return lib.load()


# ------------------------------------------------------------------------------------------------ formulas against the library
GRID_IMAGES = [(B, H, W) for B in (1, 3) for H in (1, 2, 5, 16, 29, 64) for W in (1, 2, 7, 8, 22, 34)] + [(16, 64, 8), (64, 250, 8), (11, 20, 20)]
GRID_CHANNELS = [(32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 64), (192, 192), (192, 64), (128, 128), (256, 512), (1024, 32),
                 (32, 1024), (1024, 1024), (48, 64), (64, 96), (32, 192), (64, 2048), (96, 32), (16, 64), (1088, 64)]


def _shapes():
    seen = set()
    for c in WR.FWD_CASES + WR.POOL_CASES + WR.WGRAD_CASES + WR.KEEP_CASES:
        seen.add(tuple(c[:5]))
    for c in WR.GRAD_CASES:
        seen.add((c[0], c[1], c[2], c[3], c[4]))
    return sorted(seen) + [(*im, ci, co) for im in GRID_IMAGES for ci, co in GRID_CHANNELS]


def test_formulas_against_the_host_queries(handle):
    shapes = _shapes()
    assert len(shapes) > 800
    served = 0
    for B, H, W, Cin, Cout in shapes:
        ok = WR.tag_conv3x3_wino_ok(B, H, W, Cin, Cout)
        assert handle.tag_conv3x3_wino_ok(B, H, W, Cin, Cout) == ok, (B, H, W, Cin, Cout)
        if not ok:
            continue
        served += 1
        assert handle.tag_conv3x3_wino_stats_rows(B, H, W, Cout) == WR.stats_rows(B, H, W, Cout)
        assert handle.tag_conv3x3_wino_ws_bytes(B, H, W, Cin, Cout) == WR.ws_bytes(B, H, W, Cin, Cout)
        nbytes = handle.tag_conv3x3_wino_wgrad_ws_bytes(B, H, W, Cin, Cout)
        assert nbytes == WR.wgrad_ws_bytes(B, H, W, Cin, Cout)
        assert handle.tag_conv3x3_wino_wgrad_can_reuse_v(B, H, W, Cin, Cout) == WR.can_reuse_v(B, H, W, Cin, Cout)
        if WR.wino_fused_wgrad_ok(Cin, Cout):          # S read back from the workspace size
            assert nbytes // (2 * Cin * Cout * 9 * 4) == WR.wg_geom(B, H, W, Cin, Cout)[0]
    assert served > 400
    for B, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert handle.tag_conv3x3_wino_ok(B, H, W, 64, 64) == WR.tag_conv3x3_wino_ok(B, H, W, 64, 64) == 0
    # the 2^31-byte descriptor limit of the fused kernels, by the query alone
    for B in (255, 256, 257):
        assert handle.tag_conv3x3_wino_ok(B, 64, 32, 1024, 64) == WR.tag_conv3x3_wino_ok(B, 64, 32, 1024, 64) == int(B < 256)


def test_the_channel_rules():
    """what include/tag_hip.h states: the fused forward takes Cin % 8 == 0 with Cout % 64 == 0 (of the served shapes: Cin = 32 too),
    the plane form is exactly Cout = 32, the weight gradient is fused only when both sides are multiples of 64"""
    for Cin in range(8, 1100, 8):
        for Cout in range(8, 1100, 8):
            if not WR.tag_conv3x3_wino_ok(1, 4, 4, Cin, Cout):
                continue
            assert WR.wino_fused_ok(Cin, Cout) == (Cout != 32) == (Cout % 64 == 0)
            assert WR.wino_fused_wgrad_ok(Cin, Cout) == (Cin % 64 == 0 and Cout % 64 == 0)
            if Cin % 64:
                assert Cin == 32
            assert WR.stats_rows(1, 4, 4, Cout) == (WR.wino_fused_rows(1, 4, 4) if Cout != 32 else 32)
    assert WR.tag_conv3x3_wino_ok(1, 4, 4, 32, 64) and WR.tag_conv3x3_wino_ok(1, 4, 4, 1024, 32) and not WR.tag_conv3x3_wino_ok(1, 4, 4, 32, 192)
    assert not WR.tag_conv3x3_wino_ok(1, 4, 4, 192, 32) and not WR.tag_conv3x3_wino_ok(1, 4, 4, 48, 64) and not WR.tag_conv3x3_wino_ok(1, 4, 4, 64, 96)
    assert [WR.finish_q(64, 64, S) for S in (7, 8, 31, 32)] == [1, 4, 4, 16] and WR.finish_q(192, 192, 64) == 4 and WR.finish_q(256, 256, 64) == 1


# ------------------------------------------------------------------------------------------------ claims
def test_image_claims():
    for (B, H, W), (T, blocks, why) in WR.IMAGES.items():
        assert WR.tiles(B, H, W)[2] == T and WR.wino_fused_rows(B, H, W) == blocks == -(-T // 64) and why
        px = WR.tile_pixels(B, H, W)
        assert px.numel() == T and int(px.sum()) == B * H * W
        assert sum(WR.block_counts(B, H, W, 64)) == B * H * W and len(WR.block_counts(B, H, W, 64)) == blocks
    for im, P in WR.PLANE_P.items():
        counts = WR.block_counts(*im, 32)
        assert WR.wino_geom(*im, 32)[1:] == (32, P) and len(counts) == P and sum(counts) == im[0] * im[1] * im[2]
    # the edges the images are there for
    assert WR.block_counts(1, 1, 1) == [1] and WR.block_counts(1, 1, 8) == [8] and WR.block_counts(1, 16, 16) == [256]
    assert WR.block_counts(5, 5, 10) == [216, 34]                   # four images of 50 pixels and four whole tiles of the fifth
    assert len(WR.block_counts(3, 26, 32)) == 10 and 10 % WR.FGM == 2
    c = WR.block_counts(1, 6, 22, 32)
    assert c[0] == 8 and c[1:] == [4] * 31 and [len(r) for r in WR.row_tiles(1, 6, 22, 32)] == [2] + [1] * 31
    c = WR.block_counts(257, 1, 2, 32)
    assert c[:32] == [16] * 32 and c[32] == 2 and c[33:] == [0] * 31
    assert WR.pivot_pixels(257, 1, 2, 32)[32] == (256, 0, 0) and WR.pivot_pixels(257, 1, 2, 32)[33] is None
    assert WR.pivot_pixels(5, 5, 10) == [(0, 0, 0), (4, 0, 8)]      # tile 64 = image 4, tile row 0, tile column 4
    assert WR.block_counts(3, 9, 7, 32) == [WR.tile_pixels(3, 9, 7)[[s, s + 32] if s + 32 < 60 else [s]].sum().item() for s in range(32)]


def test_fwd_pool_grad_claims():
    for B, H, W, Cin, Cout, pro, (kind, P, nblk) in WR.FWD_CASES:
        assert WR.tag_conv3x3_wino_ok(B, H, W, Cin, Cout) and (B, H, W) in WR.IMAGES
        assert WR.stats_rows(B, H, W, Cout) == P
        f = WR.form("conv", Cin, Cout, pro, 0)
        assert f == (f"fused<{pro},0>" if kind == "fused" else f"plane in<{pro}> + gemm + out<0>")
        if kind == "fused":
            assert nblk == Cout // 64 and P == WR.IMAGES[(B, H, W)][1] and WR.ws_bytes(B, H, W, Cin, Cout) == 64
        else:
            assert Cout == 32 and P == WR.PLANE_P[(B, H, W)]
    fused = [c for c in WR.FWD_CASES if c[6][0] == "fused"]
    # the shortest and the longest K loop; a ragged last group crossed with more than one cout block; a grid that is no multiple of 8
    assert {c[3] // 8 for c in fused} >= {4, 8, 24, 128}
    assert any(c[6][1] % WR.FGM and c[6][1] > WR.FGM and c[6][2] == 3 for c in fused) and any(c[6][1] * c[6][2] % 8 for c in fused)
    for im in WR.FUSED_IMAGES:
        for Cin in (64, 32):
            assert {c[5] for c in fused if c[:5] == (*im, Cin, 64)} == {0, 1, 2, 3}
    for c in WR.BATCH_CASES:
        assert c[0] == 3 and WR.tag_conv3x3_wino_ok(*c[:5])
    for B, H, W, Cin, Cout, pro, ph, pool, kind in WR.POOL_CASES:
        assert WR.tag_conv3x3_wino_ok(B, H, W, Cin, Cout) and H // ph > 0 and W >= 2 and (ph, pool) in WR.POOL_KINDS
        assert WR.form("conv", Cin, Cout, pro, 3).startswith(kind)
    assert {(c[5], c[6], c[7]) for c in WR.POOL_CASES if c[:5] == (2, 3, 5, 64, 64)} == {(p, *k) for p in range(4) for k in WR.POOL_KINDS}
    assert any(c[1] % c[6] for c in WR.POOL_CASES) and any(c[2] % 2 for c in WR.POOL_CASES)          # the floor drops a row / a column
    for B, H, W, K, C, ph, pool, p, hx, wx, kind in WR.GRAD_CASES:
        assert WR.tag_conv3x3_wino_ok(B, H, W, K, C) and WR.form("conv", K, C, 0, 2 if ph else 1).startswith(kind)
        assert pool in (0, 2, 3) and 0 <= p < 1
        if ph:
            assert (ph * H + hx) // ph == H and (2 * W + wx) // 2 == W
        if kind == "plane":
            assert C == 32 and WR.stats_rows(B, H, W, C) == WR.PLANE_P[(B, H, W)]
    e2 = [c for c in WR.GRAD_CASES if c[5]]
    assert {(c[10], c[6]) for c in e2} == {(k, pool) for k in ("fused", "plane") for pool in (0, 2, 3)}
    assert {(c[5], c[6]) for c in e2 if c[10] == "fused"} >= {(ph, pool) for ph in (1, 2) for pool in (2, 3)}
    assert {c[7] for c in e2} == {0.0, 0.2}


def test_wgrad_keep_pack_claims():
    for B, H, W, Cin, Cout, pro, claim in WR.WGRAD_CASES:
        assert WR.tag_conv3x3_wino_ok(B, H, W, Cin, Cout)
        if claim[0] == "plane":
            assert not WR.wino_fused_wgrad_ok(Cin, Cout) and WR.wino_wg_geom(B, H, W, Cin, Cout) == claim[1:]
            assert WR.form("wgrad", Cin, Cout, pro) == f"plane in<{pro}> + dy + gemm + plane_finish"
        else:
            S, cps = WR.wg_geom(B, H, W, Cin, Cout)
            assert (S, cps, WR.finish_q(Cin, Cout, S)) == claim[1:]
            assert WR.wg_rows_ok(Cin, Cout) == (claim[0] == "rows")
            f = WR.form("wgrad", Cin, Cout, pro, S=S)
            assert f == (f"rows<{pro}> + rows_finish<{claim[3]}>" if claim[0] == "rows" else f"wgrad 64x64x16<{pro}> + finish<{claim[3]}>")
    full = [c for c in WR.WGRAD_CASES if c[6][0] == "64x64x16"]
    assert {c[6][3] for c in full} == {1, 4, 16} and {c[6][2] for c in full} == {1, 2, 3}
    # an odd cps; a last slice shorter than cps whose last chunk holds one valid tile; tw < 8; a 1 x 1 image
    T = WR.tiles(1, 29, 29)[2]
    chunks = (T + 7) // 8
    assert chunks - 14 * 2 == 1 and T - 8 * (chunks - 1) == 1
    assert (WR.tiles(2, 32, 32)[2] + 7) // 8 - 21 * 3 == 1
    # the 16-run finish with a share count that is and is not a multiple of 16
    assert {2 * c[6][1] % 16 for c in full if c[6][3] == 16} == {0, 2}
    assert {WR.tiles(*c[:3])[1] for c in full} >= {1, 3, 4, 8, 15, 16, 17}
    pl = [c for c in WR.WGRAD_CASES if c[6][0] == "plane"]
    assert any(c[6][3] > WR.tiles(*c[:3])[2] and c[6][1] == 2 for c in pl) and any(c[6][3] == WR.tiles(*c[:3])[2] for c in pl)
    for B, H, W, Cin, Cout, pro, f, reuse in WR.KEEP_CASES:
        assert WR.form("conv", Cin, Cout, pro, 0, v_keep=True) == (f if "fused" in f else f"plane in<{pro}> + gemm + out<0>")
        assert WR.can_reuse_v(B, H, W, Cin, Cout) == reuse
    for Cin, Cout, tf, td in WR.PACK_CASES:
        assert (int(WR.wino_fused_ok(Cin, Cout)), int(WR.wino_fused_ok(Cout, Cin))) == (tf, td)
    assert {(c[2], c[3]) for c in WR.PACK_CASES} == {(0, 0), (1, 1), (1, 0), (0, 1)}


def test_tables_reach_every_selectable_instantiation():
    sel, tab = WR.selectable_instantiations(), WR.table_instantiations()
    assert tab == sel, (sorted(sel - tab), sorted(tab - sel))
    assert len(sel) == 34
    n = len(WR.FWD_CASES) + len(WR.POOL_CASES) + len(WR.GRAD_CASES) + len(WR.WGRAD_CASES) + len(WR.KEEP_CASES) + len(WR.PACK_CASES) + len(WR.BATCH_CASES)
    assert 270 <= n <= 330, n


# ------------------------------------------------------------------------------------------------ the pack
def _pack_scalar(w, dgrad, tiled):
    """wino_pack_kernel line by line on Python floats rounded to fp32 after every operation"""
    import struct

    def f32(v):
        return struct.unpack("f", struct.pack("f", v))[0]
    Cout, Cin = w.shape[:2]
    out = [0.0] * (16 * Cin * Cout)
    n = Cin * Cout
    wl = w.tolist()
    for co in range(Cout):
        for ci in range(Cin):
            g = wl[co][ci]
            p = [[0.0] * 3 for _ in range(4)]
            for c in range(3):
                g0, g1, g2 = (g[0][c], g[1][c], g[2][c]) if not dgrad else (g[2][2 - c], g[1][2 - c], g[0][2 - c])
                p[0][c], p[3][c] = g0, g2
                p[1][c] = f32(0.5 * f32(f32(g0 + g1) + g2))
                p[2][c] = f32(0.5 * f32(f32(g0 - g1) + g2))
            for r in range(4):
                u = [p[r][0], f32(0.5 * f32(f32(p[r][0] + p[r][1]) + p[r][2])), f32(0.5 * f32(f32(p[r][0] - p[r][1]) + p[r][2])), p[r][2]]
                base, plane = (ci * Cout + co if not dgrad else co * Cin + ci), n
                if tiled and not dgrad:
                    base, plane = (((co >> 6) * (Cin >> 3) + (ci >> 3)) * 16 * 64 + (co & 63)) * 8 + (ci & 7), 64 * 8
                elif tiled:
                    base, plane = (((ci >> 6) * (Cout >> 3) + (co >> 3)) * 16 * 64 + (ci & 63)) * 8 + (co & 7), 64 * 8
                for s in range(4):
                    out[(4 * r + s) * plane + base] = u[s]
    return torch.tensor(out, dtype=F32)


def test_pack_wino_against_the_scalar_restatement_and_GgGt():
    w = torch.randn(64, 32, 3, 3, generator=torch.Generator().manual_seed(5))            # Cout 64, Cin 32: tiled forward, plane dgrad
    assert torch.equal(WR.pack_wino(w, False, True), _pack_scalar(w, False, True))
    assert torch.equal(WR.pack_wino(w, False, False), _pack_scalar(w, False, False))
    assert torch.equal(WR.pack_wino(w, True, False), _pack_scalar(w, True, False))
    wt = w.transpose(0, 1).contiguous()                                                  # Cout 32, Cin 64: tiled dgrad
    assert torch.equal(WR.pack_wino(wt, True, True), _pack_scalar(wt, True, True))
    # both layouts hold the same 16 K N values
    assert torch.equal(WR.pack_wino(w, False, True).sort().values, WR.pack_wino(w, False, False).sort().values)
    # fp64: U = G g G^T
    G = torch.tensor(O.WINO_G, dtype=F64)
    U = torch.einsum("ri,ocij,sj->rsco", G, w.double(), G).reshape(-1)
    assert (WR.pack_wino(w.double(), False, False).double() - U).abs().max().item() < 1e-6         # (the image is fp32)
    p64 = torch.einsum("ri,ocij,sj->rsoc", G, w.double().flip(2, 3), G).reshape(16, 64, 32)      # Ud[xi][co][ci]
    assert (WR.pack_wino(w, True, False).double().reshape(16, 64, 32) - p64).abs().max().item() < 1e-6
    # the same expression order carried in fp64 is G g G^T to 1e-12
    g = w.double()
    p = WR._gg(g[:, :, 0, :], g[:, :, 1, :], g[:, :, 2, :])
    u = WR._gg(p[..., 0], p[..., 1], p[..., 2]).permute(1, 0, 3, 2).reshape(-1)
    assert (u - U).abs().max().item() < 1e-12


# ------------------------------------------------------------------------------------------------ the statements
def test_statements_against_conv2d_and_autograd():
    for B, H, W, Cin, Cout, pro in ((2, 3, 5, 8, 12, 0), (3, 9, 7, 8, 8, 1), (1, 1, 1, 4, 8, 2), (1, 1, 8, 8, 4, 3)):
        x, w, dy, s, t = WR.inputs(B, H, W, Cin, Cout, 3)
        a = X.operand(x, pro, s, t).double()
        w64 = w.double().clone().requires_grad_(True)
        a64 = WR.nchw(a).requires_grad_(True)
        y = F.conv2d(a64, w64, padding=1)
        y.backward(WR.nchw(dy.double()))
        assert (WR.fwd(x, w, pro, s, t) - WR.nhwc(y.detach())).abs().max().item() < 1e-12
        assert (WR.wgrad(x, dy, pro, s, t) - w64.grad).abs().max().item() < 1e-12
        assert (WR.dgrad(dy, w) - WR.nhwc(a64.grad)).abs().max().item() < 1e-12
        # the oracle's Winograd restatement is the same function (fp64), and its fp32 run is the floor
        assert (WR.nhwc(O.winograd_conv3x3(WR.nchw(a), w.double())) - WR.fwd(x, w, pro, s, t)).abs().max().item() < 1e-12
        assert (O.winograd_conv3x3_wgrad(WR.nchw(a), WR.nchw(dy.double())) - w64.grad).abs().max().item() < 1e-12
        assert WR.fwd(x, w, pro, s, t, F32).dtype == F32 and R.relerr(WR.fwd(x, w, pro, s, t, F32), WR.fwd(x, w, pro, s, t)) < 1e-6
        # the operand: the fp64 prologue of tests/conv_ref.py rounded once
        assert (a - R.prologue(x.double(), pro, s, t)).abs().max().item() < 1e-6
        # V = B^T d B of the padded operand, against the oracle's matrices in fp64 (values are sums of four fp32 numbers)
        Bt = torch.tensor(O.WINO_BT, dtype=F64)
        V64 = torch.einsum("ri,bcthij,sj->rsbthc", Bt, O._wino_tiles(WR.nchw(a)), Bt).reshape(16, -1, Cin)
        assert (WR.input_planes(x, pro, s, t).double() - V64).abs().max().item() < 1e-5
    # the centre-tap matmul of the 1 x 1 image
    x, w, dy, s, t = WR.inputs(1, 1, 1, 8, 4, 9)
    assert (WR.fwd(x, w)[0, 0, 0] - w[:, :, 1, 1].double() @ x[0, 0, 0].double()).abs().max().item() < 1e-12


def test_no_double_rounding_in_any_case():
    """a condition on the inputs, not a tolerance: X.operand is the kernels' fmaf bit for bit on every case of the tables"""
    seen = set()
    for c in WR.FWD_CASES + WR.POOL_CASES + WR.WGRAD_CASES + WR.KEEP_CASES + [(*b, None) for b in WR.BATCH_CASES]:
        key = tuple(c[:6])
        if key in seen or c[5] == 0:
            continue
        seen.add(key)
        x, w, dy, s, t = WR.inputs(*c[:5], WR.seed_of(*c[:5]))
        assert WR.hazards(x, c[5], s, t) == 0, key
    for B, H, W, K, C, ph, pool, p, hx, wx, kind in WR.GRAD_CASES:
        yref, sc, sh, mu, isd = WR.epi_inputs(B, H, W, C, ph, hx, wx)
        assert X.double_rounding_hazards(yref, sc, sh) == 0


# ------------------------------------------------------------------------------------------------ the floors
def test_fp32_floor_is_a_quarter_of_the_bound_at_most():
    worst = {"fwd": (0.0, None), "wgrad": (0.0, None), "dgrad": (0.0, None)}
    for c in WR.FWD_CASES:
        e = R.relerr(WR.fwd_case(*c[:6])[5], WR.fwd_case(*c[:6])[4])
        worst["fwd"] = max(worst["fwd"], (e, c[:6]))
        assert e <= WR.FWD_FLOOR_MAX, (c[:6], e)
    for c in WR.GRAD_CASES:
        d = WR.dgrad_case(*c[:5])
        e = R.relerr(d[3], d[2])
        worst["dgrad"] = max(worst["dgrad"], (e, c[:5]))
        assert e <= WR.FWD_FLOOR_MAX, (c[:5], e)
    for c in WR.WGRAD_CASES:
        e = R.relerr(WR.wgrad_case(*c[:6])[5], WR.wgrad_case(*c[:6])[4])
        worst["wgrad"] = max(worst["wgrad"], (e, c[:6]))
        assert e <= WR.DW_FLOOR_MAX, (c[:6], e)
    print("\n  worst fp32 floors:", worst)
    for f in (WR.fwd_case, WR.dgrad_case, WR.wgrad_case):
        f.cache_clear()
