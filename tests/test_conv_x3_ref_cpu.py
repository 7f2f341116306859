"""No GPU: the statements of tests/conv_x3_ref.py -- the exact operand (against exact rational arithmetic), the one-product
references against F.conv2d / autograd (1e-12), the weight-pack image against a scalar restatement of pack_weight_x3_kernel --, the
no-double-rounding condition on every case of every table, the launcher formulas against the library's own host queries, every
claim of the case tables, the table-reaches-every-selectable-instantiation equality, and the calls the x3 / bf16 entry points refuse
before any HIP call."""
import ctypes
import struct
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R
from tests import conv_x3_ref as X

F64, F32 = torch.float64, torch.float32


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the operand statement
def _round_f32(q):
    """a rational rounded ONCE to the nearest fp32 (ties to even; normal range), as a Python float"""
    if q == 0:
        return 0.0
    e = 0
    a = abs(q)
    while a >= 1 << 24:
        a /= 2
        e += 1
    while a < 1 << 23:
        a *= 2
        e -= 1
    n = round(a)                                        # Fraction.__round__: half to even
    return float((n if q > 0 else -n) * Fraction(2) ** e)


def test_fmaf_statement_is_the_single_rounding_wherever_no_hazard_is_counted():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(3000, generator=g).bfloat16().float()
    v[1500:] = torch.randn(1500, generator=g)
    s, t = torch.rand(3000, generator=g) + 0.5, 0.3 * torch.randn(3000, generator=g)
    got = X.fmaf(v, s, t)
    assert X.double_rounding_hazards(v, s, t) == 0
    for i in range(3000):
        exact = Fraction(v[i].item()) * Fraction(s[i].item()) + Fraction(t[i].item())
        assert got[i].item() == _round_f32(exact), i


def test_double_rounding_is_detected_where_it_happens():
    """v s = 2^36 - 2^-10, t = 2^60 + 2^37: the exact sum lies just BELOW the midpoint of the fp32 values 2^60 + 2^37 and 2^60 + 2^38;
    fp64 rounds it onto the midpoint, the second rounding takes the even neighbour above -- fmaf gives the one below"""
    v = torch.tensor([(1 + 2.0 ** -23) * 2.0 ** 18], dtype=F32)
    s = torch.tensor([(1 - 2.0 ** -23) * 2.0 ** 18], dtype=F32)
    t = torch.tensor([2.0 ** 60 + 2.0 ** 37], dtype=F32)
    exact = Fraction(v.item()) * Fraction(s.item()) + Fraction(t.item())
    assert _round_f32(exact) == 2.0 ** 60 + 2.0 ** 37 and X.fmaf(v, s, t).item() == 2.0 ** 60 + 2.0 ** 38
    assert X.double_rounding_hazards(v, s, t) == 1
    # the same sum made exact in fp64 (a midpoint that IS the value: both roundings tie to even alike) is no hazard
    assert X.double_rounding_hazards(torch.tensor([2.0 ** 36]), torch.tensor([1.0]), t) == 0


def test_operand_modes_and_leaky_product():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(4, 5, 6, 8, generator=g)
    s, t = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    for xx in (x, x.bfloat16()):
        assert torch.equal(X.operand(xx, 0, s, t), xx.float())
        for p in (1, 2, 3):
            assert R.relerr(X.operand(xx, p, s, t), R.prologue(xx.double(), p, s, t)) < 2e-7
        assert torch.equal(X.operand(xx, 1, s, t), torch.relu(X.operand(xx, 3, s, t)))
    lk = X.leaky_f32(x)
    i = int((x.reshape(-1) < 0).nonzero()[0])
    want = struct.unpack("f", struct.pack("f", float(Fraction(x.reshape(-1)[i].item()) * Fraction(torch.tensor(0.1, dtype=F32).item()))))[0]
    assert lk.reshape(-1)[i].item() == want          # one fp32 rounding of the exact product with 0.1f (fp64 holds the product exactly)


@pytest.mark.parametrize("pro", [0, 1, 2, 3])
def test_one_product_statements_against_torch(pro):
    """products = 1: the fp64 convolution / gradients of the bf16-rounded operands, as test_conv3x3_bf16_mode states it"""
    B, H, W, Cin, Cout = 2, 5, 4, 8, 12
    x, w, dy, s, t = X.inputs(B, H, W, Cin, Cout, 5 + pro)
    a = nchw(X.operand(x, pro, s, t).bfloat16().double()).requires_grad_(True)
    wd = w.bfloat16().double().requires_grad_(True)
    y = F.conv2d(a, wd, None, 1, 1)
    y.backward(nchw(dy.bfloat16().double()))
    assert R.relerr(X.fwd_ref(x, w, pro, s, t, 1), nhwc(y)) < 1e-12
    assert R.relerr(X.dgrad_ref(dy, w, 1), nhwc(a.grad)) < 1e-12
    assert R.relerr(X.wgrad_ref(x, dy, pro, s, t, 1), wd.grad) < 1e-12
    # products 6 / 9: the plain statements of tests/conv_ref.py
    assert torch.equal(X.fwd_ref(x, w, pro, s, t, 6), R.conv_fwd(x, w, pro, s, t))
    assert torch.equal(X.wgrad_ref(x, dy, pro, s, t, 9), R.conv_wgrad(x, dy, pro, s, t))
    # bf16 storage: the tensors are bf16 already, rounding them again changes nothing
    xb, _, dyb, _, _ = X.inputs(B, H, W, Cin, Cout, 5 + pro, bf16=True)
    assert torch.equal(X.fwd_ref(xb, w, pro, s, t, 1), X.fwd_ref(xb.float(), w, pro, s, t, 1)) and xb.dtype == torch.bfloat16


def test_epilogue_statements_against_torch():
    """the exact-mask sums equal the fp64 statements of tests/conv_ref.py wherever no pre-activation is within rounding of zero or of
    a tie, and those equal autograd (tests/test_conv_ref_cpu.py)"""
    B, Hf, Wf, C = 3, 7, 6, 8
    yref, sc, sh, mu, isd = X.epi_inputs(B, Hf, Wf, C, 3)
    g = torch.Generator().manual_seed(4)
    da = torch.randn(B, Hf, Wf, C, generator=g)
    a64 = yref.double() * sc.double() + sh.double()
    assert bool((a64.abs() > 1e-5).all())
    for got, ref in zip(X.bn_bwd_sums_x(da, yref, sc, sh, mu, isd), R.bn_bwd_sums(da, yref, sc, sh, mu, isd)):
        assert R.relerr(got, ref) < 1e-12
    for ph in (1, 2):
        for pool in (0, 2, 3):
            dx = torch.randn(B, Hf // ph, Wf // 2, C, generator=g)
            keep = (torch.rand(dx.shape, generator=g) > 0.3).double()
            for k, p in ((None, 0.0), (keep, 0.3)):
                got = X.pool_bwd_sums_x(dx, yref, sc, sh, mu, isd, ph, pool, k, p)
                ref = R.pool_bwd_sums(dx, yref, sc, sh, mu, isd, ph, pool, k, p)
                # keep_scale is the kernel's fp32 1 / (1 - p): 6e-8 from the fp64 quotient
                assert R.relerr(got[0], ref[0]) < 1e-7 and R.relerr(got[1], ref[1]) < 1e-7
                if p == 0.0:
                    assert R.relerr(got[0], ref[0]) < 1e-12 and R.relerr(got[1], ref[1]) < 1e-12


# ------------------------------------------------------------------------------------------------ the pack statement
def _scalar_pack_word(w, dgrad, rne, tap, kk, nb, s, lane, e):
    """pack_weight_x3_kernel for ONE word, in Python scalars"""
    Cout, Cin = w.shape[:2]
    nn, k0 = nb * 32 + (lane & 31), kk * 16 + 8 * (lane >> 5)
    halves = []
    for j in range(2):
        k = k0 + 2 * e + j
        v = w[k, nn, (8 - tap) // 3, (8 - tap) % 3].item() if dgrad else w[nn, k, tap // 3, tap % 3].item()
        bits = lambda f: struct.unpack("I", struct.pack("f", f))[0]
        fl = lambda u: struct.unpack("f", struct.pack("I", u))[0]
        if rne:
            u = bits(v)
            halves.append((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF) if s == 0 else 0)
            continue
        for _ in range(s):
            v = v - fl(bits(v) & 0xFFFF0000)            # exact in fp32 (and in the fp64 Python computes it in)
        halves.append(bits(v) >> 16)
    word = halves[0] | (halves[1] << 16)
    return word - (1 << 32) if word >= 1 << 31 else word


@pytest.mark.parametrize("Cin,Cout", X.PACK_CASES)
def test_pack_statement(Cin, Cout):
    w = torch.randn(Cout, Cin, 3, 3, generator=torch.Generator().manual_seed(Cin + Cout))
    g = torch.Generator().manual_seed(9)
    for dgrad in (False, True):
        K, N = (Cout, Cin) if dgrad else (Cin, Cout)
        weff = R.unpack(R.pack_dgrad(w)) if dgrad else w          # the (N, K, 3, 3) weight of the convolution the pack computes
        for rne in (False, True):
            img = X.pack_x3(w, dgrad, rne)
            assert img.shape == (9, K // 16, N // 32, 3, 64, 4) and img.numel() * 4 == X.pack_bytes(Cin, Cout)
            # the fragment index of the kernel's comment: (((tap K/16 + kk) N/32 + nb) 3 + s) 64 + lane, four words each
            flat = img.reshape(-1, 4)
            for _ in range(40):
                tap, kk, nb, s, lane, e = [int(torch.randint(0, m, (1,), generator=g)) for m in (9, K // 16, N // 32, 3, 64, 4)]
                idx = (((tap * (K // 16) + kk) * (N // 32) + nb) * 3 + s) * 64 + lane
                assert flat[idx, e].item() == _scalar_pack_word(w, dgrad, rne, tap, kk, nb, s, lane, e)
            # the values: [9, kk, nb, lane, e, j] -> (n, k, tap)
            vals = [X.unpack_x3_plane(img, s) for s in range(3)]
            # lane = 32 kl + ml: [nb, kk, (kl, ml), e, j, tap] -> n = nb 32 + ml, k = kk 16 + 8 kl + 2 e + j
            def to_w(v):
                v = v.permute(2, 1, 3, 4, 5, 0).reshape(N // 32, K // 16, 2, 32, 4, 2, 9)        # nb, kk, kl, ml, e, j, tap
                return v.permute(0, 3, 1, 2, 4, 5, 6).reshape(N, K, 3, 3)
            if rne:
                assert torch.equal(to_w(vals[0]), weff.bfloat16().float())
                assert bool((img[:, :, :, 1:] == 0).all())
            else:
                assert torch.equal(to_w(vals[0]) + to_w(vals[1]) + to_w(vals[2]), weff), "hi + mid + lo is the weight, exactly"
                assert torch.equal(to_w(vals[0]), X._trunc_f32(weff)), "hi is the truncation, not the rounding"
                assert not torch.equal(to_w(vals[0]), weff.bfloat16().float())
    # the mirrored tap: the dgrad pack is the forward pack of the flipped, transposed weight
    assert torch.equal(X.pack_x3(w, True), X.pack_x3(R.unpack(R.pack_dgrad(w)), False))
    assert not torch.equal(X.pack_x3(w, True), X.pack_x3(w.permute(1, 0, 2, 3).contiguous(), False))


# ------------------------------------------------------------------------------------------------ formulas against the library
@pytest.fixture(scope="module")
def handle():
    from texttoaudiogrounding_amd import lib
    return lib.load()


def test_formulas_against_the_host_queries(handle):
    """the queries that make no HIP call (the row kernel's strip count asks the device for its CU count: GPU module)"""
    for B in (1, 3):
        for H in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 49, 73):
            for W in (4, 8, 12, 16, 32, 64):
                for Cin, Cout in ((64, 64), (64, 128), (96, 192), (192, 192), (512, 384), (160, 320)):
                    assert handle.tag_conv3x3_x3_stats_rows(B, H, W, Cout) == X.x3_stats_rows(B, H, W, Cout)
                    if W in X.WIDTHS:
                        assert handle.tag_conv3x3_wgrad_x3_ws_bytes(B, H, W, Cin, Cout) == X.wgrad_x3_ws_bytes(B, H, W, Cin, Cout)
                        assert X.alltaps_splits(B, H, W, Cin, Cout, 32)[:2] == R.alltaps_splits(B, H, W, Cin, Cout)[:2]
                    if not X.rows_cfg(H, W, Cin, Cout):
                        assert handle.tag_conv3x3_x3_bf16_stats_rows(B, H, W, Cin, Cout, 1) == X.bf16_stats_rows(B, H, W, Cin, Cout, 1, 256)
                    assert handle.tag_conv3x3_x3_bf16_stats_rows(B, H, W, Cin, Cout, 2) == X.bf16_stats_rows(B, H, W, Cin, Cout, 2, 256)
                    assert handle.tag_conv3x3_dgrad_poolsums_bf16_rows(B, H, W, Cin, Cout) == X.poolsums_bf16_rows(B, H, W, Cin, Cout)
    for Cin, Cout in X.PACK_CASES:
        assert handle.tag_conv3x3_x3_pack_bytes(Cin, Cout) == X.pack_bytes(Cin, Cout)
    # the switch of the row kernel moves its shapes to the tile formula
    was = handle.tag_conv_rows_enable(0)
    try:
        assert handle.tag_conv3x3_dgrad_poolsums_bf16_rows(3, 5, 64, 64, 64) == X.poolsums_bf16_rows(3, 5, 64, 64, 64, rows_on=False) == 9
        assert handle.tag_conv3x3_x3_bf16_stats_rows(3, 5, 64, 64, 64, 0) == X.bf16_stats_rows(3, 5, 64, 64, 64, 0, 256, rows_on=False) == 18
    finally:
        handle.tag_conv_rows_enable(was)
    assert handle.tag_conv3x3_dgrad_poolsums_bf16_rows(3, 5, 64, 64, 64) == 0


def test_tile_geometry_and_rows_rules():
    assert X.tile_sel(64) == (2, 2, 64) and X.tile_sel(192) == (2, 2, 64) and X.tile_sel(384) == (4, 1, 128) and X.tile_sel(320) == (2, 2, 64)
    assert [X.tile_geom(1, W, 64)["TH"] for W in X.WIDTHS] == [16, 8, 4, 2] == [X.tile_geom(1, W, 128)["TH"] for W in X.WIDTHS]
    assert [X.chunk_geom(1, W, 32)[:2] for W in X.WIDTHS] == [(8, 4), (16, 2), (32, 1), (32, 1)]
    assert [X.chunk_geom(1, W, 64)[:2] for W in X.WIDTHS] == [(8, 8), (16, 4), (32, 2), (32, 2)]
    assert X.chunk_geom(5, 64, 64)[2:] == (3, 2)
    assert X.rows_cfg(2, 64, 64, 64) == 2 and X.rows_cfg(2, 32, 64, 384) == 4 and X.rows_cfg(1, 64, 64, 64) is None
    assert X.rows_cfg(9, 64, 64, 128) is None and X.rows_cfg(9, 32, 64, 64) is None and X.rows_cfg(9, 32, 128, 128) is None
    assert not X.rows_takes(9, 64, 64, 64, 2) and X.rows_takes(9, 64, 64, 64, 1) and not X.rows_takes(9, 64, 64, 64, 0, enabled=False)
    # H / 16 rule and the CU cap
    assert [X.rows_strips(1, H, 1, 256) for H in (2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49)] == [1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 3]
    assert X.rows_strips(128, 48, 1, 256) == 2 and X.rows_strips(128, 48, 1, 304) == 3 and X.rows_strips(300, 48, 1, 256) == 1
    assert X.rows_strip_lengths(1, 49, 64, 64, 64, 256) == [16, 16, 17] and X.rows_strip_lengths(1, 33, 32, 64, 128, 256) == [16, 17]


# ------------------------------------------------------------------------------------------------ claims of the tables
def test_tile_case_claims():
    hs = {W: set() for W in X.WIDTHS}
    for B, H, W, Cin, Cout, pro, claim in X.TILE_CASES + X.TILE256_CASES:
        g = X.tile_geom(H, W, Cout)
        assert (g["MB"], g["row_tiles"], g["n_tiles"]) == claim, ((B, H, W, Cin, Cout), g)
        assert Cin % 32 == 0 and Cout % 64 == 0 and Cin <= 512 and B * H * W * max(Cin, Cout) < 5_000_000
        hs[W].add(H)
    for W in X.WIDTHS:
        TH = 128 // W
        assert hs[W] >= {1, TH - 1, TH, TH + 1, 2 * TH + 1} - {0}, W
        assert hs[W] >= {256 // W - 1, 256 // W, 256 // W + 1} or W in (8, 32)
    cases = X.TILE_CASES
    assert {c[3] for c in cases} >= {32, 96, 160, 512} and {c[4] for c in cases} >= {64, 192, 320, 384}
    assert {c[5] for c in cases} == {0, 1, 2, 3}
    assert any(c[0] == 3 and (c[0] * c[6][1]) % 2 == 1 and c[6][1] > 1 for c in cases), "B = 3 with an odd number of row tiles"
    assert {(c[6][0], c[2]) for c in cases} == {(MB, W) for MB in (2, 4) for W in X.WIDTHS}
    for B, H, W, Cin, Cout in X.H1_CASES:
        assert H == 1 and X.rows_cfg(2, W, Cin, Cout) and not X.rows_cfg(1, W, Cin, Cout)
    assert {(c[2], c[3], c[4]) for c in X.H1_CASES} == {(64, 64, 64), (32, 64, 128)}
    for B, H, W, Cin, Cout in X.INST_TILE_CASES:
        assert B == 1 and H == 3 and Cin == 64


def test_rows_case_claims():
    for cus in (64, 256, 304):
        for B, H, W, Cin, Cout, (wn, ns, odd) in X.ROWS_CASES:
            assert X.rows_cfg(H, W, Cin, Cout) == wn and X.rows_takes(H, W, Cin, Cout, 1)
            lens = X.rows_strip_lengths(B, H, W, Cin, Cout, cus)
            assert len(lens) == ns and sum(lens) == H and any(n % 2 for n in lens) == odd
            assert X.rows_partial_rows(B, H, W, Cin, Cout, cus) == B * ns * 2 * (4 // wn)
    for W, Cin in ((64, 64), (32, 64)):
        sub = [c for c in X.ROWS_CASES if c[2] == W]
        assert {c[1] for c in sub} == {2, 3, 15, 16, 17, 31, 32, 33, 47, 49} and {c[0] for c in sub} == {1, 3}
    assert {c[4] for c in X.ROWS_CASES if c[2] == 32} == {128, 256, 384}
    B, H, W, Cin, Cout = X.ROWS_CAP_CASE
    for cus in (64, 128, 256):                      # binds on every part up to 256 CUs (the GPU module derives the count from the device's)
        assert -(-cus // B) < H // 16 and X.rows_strips(B, H, 1, cus) == -(-cus // B)


def test_wgrad_case_claims():
    seen = {k: {W: set() for W in X.WIDTHS} for k in ("x3", "bf16", "dma")}
    for kind, B, H, W, Cin, Cout, pro in X.WGRAD_H_CASES:
        seen[kind][W].add(H)
        assert Cin % 64 == 0 and Cout % 64 == 0 and (kind != "dma" or pro <= 1)
    for kind in seen:
        for W in X.WIDTHS:
            CH = X.chunk_geom(1, W, X.WG_PX[kind])[1]
            assert seen[kind][W] == {h for h in (1, CH - 1, CH, CH + 1, 2 * CH + 1) if h >= 1}, (kind, W)
    tags = {k: set() for k in ("x3", "bf16", "dma")}
    for kind, B, H, W, Cin, Cout, pro, (splits, cps, last, tag) in X.WGRAD_SPLIT_CASES:
        c = X.wgrad_claim(kind, B, H, W, Cin, Cout)
        assert (c["splits"], c["cps"], c["last"]) == (splits, cps, last) and X.split_tag_holds(tag, c), (kind, B, H, W, c)
        assert splits >= 2 and B * H * W * 64 < 5_000_000 and (kind != "dma" or pro <= 1)
        tags[kind].add(tag)
        if tag == "short":
            assert B == 3 and c["chunks"] >= 16
    for kind in tags:
        assert tags[kind] == {"short", "last1", "last2", "start_last", "start_first"}, kind
        assert any(c[0] == kind and c[3] == 64 for c in X.WGRAD_SPLIT_CASES), "W = 64: two column strips"
    # where tag_conv3x3_wgrad_x3_ws_bytes determines the split count of the 32-pixel kernels: s32 >= s64 on every row of the tables
    for c in X.WGRAD_H_CASES + [r[:7] for r in X.WGRAD_SPLIT_CASES] + X.WGRAD_PRO_CASES + X.WGRAD_INST_CASES:
        kind, B, H, W, Cin, Cout, pro = c
        assert X.alltaps_splits(B, H, W, Cin, Cout, 32)[0] >= X.alltaps_splits(B, H, W, Cin, Cout, 64)[0]
    for kind in ("x3", "bf16"):
        sub = [c for c in X.WGRAD_PRO_CASES if c[0] == kind]
        assert {(c[3], c[6]) for c in sub} == {(W, p) for W in X.WIDTHS for p in range(4)}
        assert {(c[4], c[5]) for c in sub} >= {(64, 192), (192, 64), (64, 64), (192, 192)}


def test_epilogue_case_claims():
    paths = set()
    for B, H, W, Cin, Cout, path in X.BNSUMS_CASES:
        assert ("rows" if X.rows_takes(H, W, Cin, Cout, 0) else "tile") == path
        paths.add((path, W, X.tile_sel(Cout)[0] if path == "tile" else X.rows_cfg(H, W, Cin, Cout)))
    assert {p[0] for p in paths} == {"tile", "rows"} and {p[1:] for p in paths if p[0] == "rows"} == {(64, 2), (32, 4)}
    seen = set()
    for B, Hf, Wf, Cin, Cout, ph, pool in X.POOLSUMS_CASES:
        H, W = Hf // ph, Wf // 2
        assert X.poolsums_bf16_rows(B, H, W, Cin, Cout) == B * X.tile_geom(H, W, Cout)["row_tiles"] > 0
        seen.add((ph, pool))
    assert {s[0] for s in seen} == {1, 2} and {s[1] for s in seen} == {0, 2, 3}
    assert any(c[5] == 2 and c[1] % 2 == 1 for c in X.POOLSUMS_CASES), "odd Hf with ph = 2: a row left over"
    assert {c[2] // 2 for c in X.POOLSUMS_CASES} == set(X.WIDTHS)
    B, Hf, Wf, Cin, Cout, ph = X.POOLSUMS_ROWS_REFUSED
    assert X.poolsums_bf16_rows(B, Hf // ph, Wf // 2, Cin, Cout) == 0 and X.rows_takes(Hf // ph, Wf // 2, Cin, Cout, 0)


def test_every_selectable_instantiation_is_in_a_table():
    sel, tab = X.selectable_instantiations(), X.table_instantiations()
    for k in sel:
        assert tab[k] == sel[k], (k, sorted(sel[k] - tab[k]), sorted(tab[k] - sel[k]))
    assert len(sel["tile"]) == 96 + 32 + 16 and len(sel["wgrad"]) == 48 + 16 and len(sel["dma"]) == 8 and len(sel["rows"]) == 10


# ------------------------------------------------------------------------------------------------ the input condition: no double rounding
def _prologue_cases():
    out = [(B, H, W, Cin, Cout) for B, H, W, Cin, Cout in X.INST_TILE_CASES + X.H1_CASES]
    out += [c[:5] for c in X.TILE_CASES + X.TILE256_CASES + X.ROWS_CASES]
    out += [c[1:6] for c in X.WGRAD_H_CASES + X.WGRAD_SPLIT_CASES + X.WGRAD_PRO_CASES + X.WGRAD_INST_CASES]
    out.append((2,) + X.ROWS_CAP_CASE[1:])
    return sorted(set(out))


@pytest.mark.parametrize("case", _prologue_cases(), ids=lambda c: "-".join(map(str, c)))
def test_no_case_has_a_double_rounding_in_its_operand(case):
    """every prologue mode on the fp32 AND the bf16 tensor of the case (a table runs a subset of them)"""
    B, H, W, Cin, Cout = case
    for bf16 in (False, True):
        x, w, dy, s, t = X.inputs(B, H, W, Cin, Cout, X.seed_of(B, H, W, Cin, Cout), bf16)
        for p in (1, 2, 3):
            assert X.operand_hazards(x, p, s, t) == 0, (case, bf16, p)


def test_no_case_has_a_double_rounding_in_its_relu_mask():
    shapes = [(B, H, W, Cout) for B, H, W, Cin, Cout in X.INST_TILE_CASES] + [(c[0], c[1], c[2], c[4]) for c in X.BNSUMS_CASES]
    shapes += [(c[0], c[1], c[2], c[4]) for c in X.ROWS_CASES] + [(c[0], c[1], c[2], c[4]) for c in X.POOLSUMS_CASES]
    shapes += [(B, 2 * H, 2 * W, Cout) for B, H, W, Cin, Cout in X.INST_TILE_CASES]
    for B, H, W, C in sorted(set(shapes)):
        yref, sc, sh, mu, isd = X.epi_case(B, H, W, C)
        assert X.double_rounding_hazards(yref.float(), sc, sh) == 0, (B, H, W, C)


# ------------------------------------------------------------------------------------------------ the operand probe
@pytest.mark.parametrize("case", X.PROBE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_probe_inputs_tell_fmaf_from_multiply_add(case):
    """the identity-weight probe: its expected output IS the operand (checked through the fp64 convolution), its inputs have no
    double rounding, and on every prologue some planted element changes its bf16 operand if the kernel multiplies and then adds"""
    B, H, W, Cin, Cout = case
    w = X.identity_weight(Cout, Cin)
    for p in (1, 2, 3):
        for bf16 in (True, False):
            x, s, t, planted = X.probe_inputs(B, H, W, Cin, p, bf16=bf16)
            assert planted >= 4 and X.operand_hazards(x, p, s, t) == 0, (case, p, planted)
            pre = X.leaky_f32(x) if p == 2 else x.float()
            wrong = X.muladd_f32(pre, s, t)
            wrong = torch.relu(wrong) if p == 1 else wrong
            right = X.operand(x, p, s, t)
            assert int((wrong.bfloat16().float() != right.bfloat16().float()).sum()) >= 4
            if not bf16:
                assert (wrong != right).float().mean().item() > 0.05      # on fp32 operands every tenth element and more tells them apart
            # the fp64 convolution of the exact operand with the identity weight is the operand (products 1: rounded to bf16)
            assert torch.equal(X.probe_expected(x, p, s, t, 6, Cout).double(), R.conv_fwd(X.operand(x, p, s, t), w))
            assert torch.equal(X.probe_expected(x, p, s, t, 1, Cout).double(), X.fwd_ref(x, w, p, s, t, 1))
    # the weight-gradient probe: dy one at PROBE_PIXEL for every cout -> dw[co, ci, ky, kx] = operand[b, h + ky - 1, w + kx - 1, ci]
    if B == 2:
        b0, h0, w0 = X.PROBE_PIXEL
        x, s, t, planted = X.probe_inputs(B, H, W, Cin, 1, pixels=[(b0 * H + h0 + dy) * W + w0 + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
        dy = torch.zeros(B, H, W, Cout)
        dy[b0, h0, w0] = 1.0
        a = X.operand(x, 1, s, t).bfloat16().float()
        want = a[b0, h0 - 1:h0 + 2, w0 - 1:w0 + 2].permute(2, 0, 1).expand(Cout, Cin, 3, 3)
        assert torch.equal(X.wgrad_ref(x, dy, 1, s, t, 1), want.double()) and planted >= 4


@pytest.mark.parametrize("W", X.WIDTHS)
def test_wgrad_probe_inputs(W):
    """the weight-gradient probe at every width, fp32 and bf16, prologues 1..3: discriminators planted in the 3 x 3 neighbourhood
    of PROBE_PIXEL (inside the image), no double rounding"""
    B, H = 2, 5
    b0, h0, w0 = X.PROBE_PIXEL
    assert 1 <= h0 < H - 1 and 1 <= w0 < W - 1 and b0 < B
    pixels = [(b0 * H + h0 + dy) * W + w0 + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    for bf16 in (True, False):
        for p in (1, 2, 3):
            x, s, t, planted = X.probe_inputs(B, H, W, 64, p, pixels=pixels, bf16=bf16)
            assert planted >= 4 and X.operand_hazards(x, p, s, t) == 0
            a, b = X._prologue_pair(x.float(), s, t, p)
            near = a.reshape(-1, 64)[pixels].bfloat16().float() != b.reshape(-1, 64)[pixels].bfloat16().float()
            assert int(near.sum()) >= 4


# ------------------------------------------------------------------------------------------------ refused calls (no HIP call)
TAG_EINVAL = -1


def _buf(n=64):
    return (ctypes.c_float * n)()


def test_x3_entries_refuse_unserved_arguments(handle):
    x, w, y, ws, tb = _buf(), _buf(), _buf(), _buf(), _buf()
    p = lambda b: ctypes.addressof(b)
    f32 = lambda pro, s, t, B, H, W, Cin, Cout: handle.tag_conv3x3_forward_x3(p(x), p(w), pro, s, t, p(y), None, B, H, W, Cin, Cout, 6, None)
    b16 = lambda pro, s, t, B, H, W, Cin, Cout: handle.tag_conv3x3_forward_x3_bf16(p(x), p(w), pro, s, t, p(y), None, B, H, W, Cin, Cout, None)
    for fwd in (f32, b16):
        for args in [(0, None, None, 1, 2, 4, 64, 64), (0, None, None, 1, 2, 12, 64, 64), (0, None, None, 1, 2, 8, 48, 64),
                     (0, None, None, 1, 2, 8, 64, 96), (0, None, None, 1, 2, 8, 576, 64), (4, p(tb), p(tb), 1, 2, 8, 64, 64),
                     (1, None, p(tb), 1, 2, 8, 64, 64), (1, p(tb), None, 1, 2, 8, 64, 64), (0, None, None, 0, 2, 8, 64, 64),
                     (0, None, None, 1, 0, 8, 64, 64)]:
            assert fwd(*args) == TAG_EINVAL, args
            assert b"check failed" in handle.tag_last_error()
    wg32 = lambda pro, s, t, B, H, W, Cin, Cout: handle.tag_conv3x3_wgrad_x3(p(x), pro, s, t, p(y), p(w), B, H, W, Cin, Cout, 6, p(ws), None)
    wg16 = lambda pro, s, t, B, H, W, Cin, Cout: handle.tag_conv3x3_wgrad_x3_bf16(p(x), pro, s, t, p(y), p(w), B, H, W, Cin, Cout, p(ws), None)
    for wg in (wg32, wg16):
        for args in [(0, None, None, 1, 2, 8, 32, 64), (0, None, None, 1, 2, 8, 64, 96), (0, None, None, 1, 2, 4, 64, 64),
                     (0, None, None, 1, 2, 12, 64, 64), (4, p(tb), p(tb), 1, 2, 8, 64, 64), (1, None, None, 1, 2, 8, 64, 64),
                     (0, None, None, 0, 2, 8, 64, 64)]:
            assert wg(*args) == TAG_EINVAL, args
    bn = lambda B, H, W, Cin, Cout: handle.tag_conv3x3_dgrad_bnsums_bf16(p(x), p(w), p(y), p(x), p(tb), p(tb), p(tb), p(tb), p(ws), B, H, W, Cin, Cout, None)
    for args in [(1, 2, 4, 64, 64), (1, 2, 8, 48, 64), (1, 2, 8, 64, 96), (1, 2, 8, 576, 64)]:
        assert bn(*args) == TAG_EINVAL, args
    pool = lambda B, H, W, Cin, Cout, Hf, Wf, ph, pw, kind, dp: handle.tag_conv3x3_dgrad_poolsums_bf16(
        p(x), p(w), p(y), p(x), p(tb), p(tb), p(tb), p(tb), p(ws), B, H, W, Cin, Cout, Hf, Wf, ph, pw, kind, dp, 0, None)
    B, Hf, Wf, Cin, Cout, ph = X.POOLSUMS_ROWS_REFUSED
    for args in [(B, Hf // ph, Wf // 2, Cin, Cout, Hf, Wf, ph, 2, 0, 0.0),                  # a shape the row kernel takes
                 (1, 2, 8, 64, 128, 6, 16, 3, 2, 0, 0.0), (1, 2, 8, 64, 128, 4, 16, 2, 2, 1, 0.0), (1, 2, 8, 64, 128, 4, 16, 2, 2, 0, 1.0),
                 (1, 2, 4, 64, 128, 4, 8, 2, 2, 0, 0.0), (1, 2, 8, 64, 96, 4, 16, 2, 2, 0, 0.0), (1, 2, 8, 64, 128, 4, 16, 2, 4, 0, 0.0)]:
        assert pool(*args) == TAG_EINVAL, args
    assert handle.tag_pack_conv_weight_x3(p(x), p(w), p(y), 48, 64, 6, None) == TAG_EINVAL
    assert handle.tag_pack_conv_weight_x3(p(x), p(w), None, 32, 64, 6, None) == TAG_EINVAL
    assert all(v == 0.0 for b in (x, w, y, ws) for v in b)
