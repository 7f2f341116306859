"""Statements, launcher formulas and case tables of tests/test_gpu_conv_x3_sweep.py: the split-bf16 (x3 / x9), one-product and
bf16-storage convolutions of csrc/conv_x3.hip, csrc/conv_rows.hip and csrc/conv_wgrad_dma.hip.  The convolution statements
themselves are those of tests/conv_ref.py; this module adds

* the OPERAND the kernels multiply, bit for bit: ``operand`` restates prologue1 (fmaxf(fmaf(x, s, t), 0) and its modes 2 and 3) in
  fp64 -- the product of two fp32 values is exact there, so the only way ``(x s + t).float()`` can differ from fmaf is a double
  rounding, which ``double_rounding_hazards`` counts (TwoSum error term non-zero AND the fp64 sum exactly on an fp32 rounding
  midpoint).  tests/test_conv_x3_ref_cpu.py asserts that no case of any table has one: a condition on the inputs, not a tolerance;
* ``pack_x3``: the uint32 image of pack_weight_x3_kernel (truncating three-way split, RNE one-product pack, mirrored dgrad taps);
* the host formulas of the launchers (statistics rows, rows_cfg / rows_strips, split counts, tile selection, chunk geometry);
* the case tables, each row with the CLAIM of which kernel and geometry it reaches, and the instantiation sets.

Layouts as in tests/conv_ref.py: activations (B, H, W, C), weights (Cout, Cin, 3, 3)."""
import torch

from tests import conv_ref as R

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
WIDTHS = (8, 16, 32, 64)
#: build constants of the product library (csrc/conv_x3.hip): TAG_X3_BF16_MB64, TAG_WX3_KS16
X3_BF16_MB64, WX3_KS16 = 2, 4

# ------------------------------------------------------------------------------------------------ bounds (all from tests/test_gpu_kernels.py)
X3 = 5e-6            # forward, dgrad, wgrad of x3 / x9 / one-product on fp32 tensors (test_conv3x3_x3_forward_dgrad, test_conv3x3_bf16_mode)
HALF_ULPS = 1.01     # bf16-stored outputs in half-ulps of bf16 (_bf16_storage_case, no prologue)
WGRAD16 = 1e-5       # bf16-storage weight gradient (_bf16_storage_case, no prologue)
STATS16 = 2e-5       # folded mean / variance against the fp64 statistics of the fp64 y (_bf16_storage_case, no prologue)
SUMS = 1e-5          # EPI 1 / EPI 2 sums (test_conv_dgrad_fused_*)


# ------------------------------------------------------------------------------------------------ the operand, bit for bit
def fmaf(v, s, t):
    """fmaf(v, s, t) of fp32 (or bf16) values as an fp32 tensor: the fp64 product is exact, the sum rounds once to fp64 and once to
    fp32 -- equal to the single rounding of fmaf wherever ``double_rounding_hazards`` counts nothing"""
    return (v.double() * s.double() + t.double()).float()


def double_rounding_hazards(v, s, t):
    """elements where (v s + t).float() can differ from fmaf(v, s, t): the fp64 sum was inexact (TwoSum error term != 0) AND sits
    exactly on the midpoint of two fp32 values (low 29 bits of its significand == 2^28), or is a non-zero fp32 subnormal"""
    a, b = v.double() * s.double(), t.double().expand_as(v.double() * s.double())
    sm = a + b
    bb = sm - a
    err = (a - (sm - bb)) + (b - bb)
    low = sm.contiguous().view(torch.int64) & ((1 << 29) - 1)
    mid = (err != 0) & (low == (1 << 28))
    sub = (sm != 0) & (sm.abs() < 2.0 ** -126)
    return int((mid | sub).sum().item())


def leaky_f32(v):
    """v > 0 ? v : 0.1f * v with the product rounded to fp32, as prologue1 forms it before its fmaf"""
    v = v.float()
    return torch.where(v > 0, v, v * torch.tensor(0.1, dtype=F32))


def operand(x, p, s, t):
    """prologue1(x, p, s, t) as an fp32 tensor, bit for bit (x fp32 or bf16); the bf16-storage and one-product kernels then round it
    to bf16 (RNE): ``operand(...).bfloat16()``"""
    v = x.float()
    if p == 0:
        return v
    if p == 1:
        return torch.relu(fmaf(v, s, t))
    if p == 2:
        return fmaf(leaky_f32(v), s, t)
    return fmaf(v, s, t)


def operand_hazards(x, p, s, t):
    if p == 0:
        return 0
    return double_rounding_hazards(leaky_f32(x) if p == 2 else x.float(), s, t)


def relu_mask(yref, scale, shift):
    """fmaf(yref, scale, shift) > 0 of the EPI 1 / EPI 2 sums, restated the same way"""
    return fmaf(yref, scale, shift) > 0


def fwd_ref(x, w, p, s, t, products, dtype=F64):
    """products 6 | 9: the plain convolution; 1: the convolution of the RNE-bf16-rounded operands (x after its exact prologue)"""
    if products == 1:
        return R.conv_fwd(operand(x, p, s, t).bfloat16(), w.bfloat16(), dtype=dtype)
    return R.conv_fwd(x, w, p, s, t, dtype)


def dgrad_ref(dy, w, products, dtype=F64):
    if products == 1:
        return R.conv_dgrad(dy.bfloat16(), w.bfloat16(), dtype)
    return R.conv_dgrad(dy, w, dtype)


def wgrad_ref(x, dy, p, s, t, products, dtype=F64):
    if products == 1:
        return R.conv_wgrad(operand(x, p, s, t).bfloat16(), dy.bfloat16(), dtype=dtype)
    return R.conv_wgrad(x, dy, p, s, t, dtype)


def half_ulps(got, ref64):
    """max |got - ref| in half-ulps of bf16 at |ref|, with the floor term of _bf16_storage_case"""
    return ((got.double() - ref64).abs() / (ref64.abs() * 2.0 ** -8 + 1e-30 + 1e-3 * 2.0 ** -8)).max().item()


def bn_bwd_sums_x(da, yref, scale, shift, mean, invstd, dtype=F64):
    """R.bn_bwd_sums with the ReLU mask restated exactly (fmaf in fp32)"""
    da, y = da.to(dtype), yref.to(dtype)
    dz = da * relu_mask(yref, scale, shift)
    xhat = (y - mean.to(dtype)) * invstd.to(dtype)
    C = y.shape[-1]
    return dz.reshape(-1, C).sum(0), (dz * xhat).reshape(-1, C).sum(0)


def pool_bwd_sums_x(dx, yref, scale, shift, mean, invstd, ph, pool, keep=None, drop_p=0.0, dtype=F64):
    """R.pool_bwd_sums with a = fmaf(yref, scale, shift) in fp32 (mask and first arg-max as the kernel sees them) and the kernel's
    fp32 scalars keep_scale = 1 / (1 - p), wavg, wavg + wmax"""
    y = yref.to(dtype)
    g = dx.to(dtype)
    if keep is not None:
        g = g * keep.to(dtype) * float(torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(drop_p, dtype=F32)))
    a = R._windows(fmaf(yref, scale, shift), ph)
    xhat = R._windows((y - mean.to(dtype)) * invstd.to(dtype), ph)
    wavg, wmax = R.pool_weights(pool, ph)
    first = torch.nn.functional.one_hot(a.argmax(3), a.shape[3]).movedim(-1, 3).to(dtype)
    dz = (a > 0) * g.unsqueeze(3) * (wavg + first * wmax)
    C = y.shape[-1]
    return dz.reshape(-1, C).sum(0), (dz * xhat).reshape(-1, C).sum(0)


# ------------------------------------------------------------------------------------------------ the weight pack
def _u16_trunc(v):
    return (v.contiguous().view(torch.int32).to(torch.int64) >> 16) & 0xFFFF


def _u16_rne(v):
    u = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def _trunc_f32(v):
    return (v.contiguous().view(torch.int32) & -65536).view(F32)


def pack_x3(w, dgrad=False, rne=False):
    """The image of pack_weight_x3_kernel as int32 [9, K/16, N/32, 3, 64, 4]: fragment (tap, kk, nb, plane s) holds for lane the
    four words e = 0..3, each the bf16 pair (low half first) of k = kk 16 + 8 (lane >> 5) + 2 e + j, n = nb 32 + (lane & 31).
    Forward: K = Cin, N = Cout, value w[n, k, tap]; dgrad: K = Cout, N = Cin, value w[k, n, 8 - tap].  Planes: hi = top 16 bits,
    mid / lo = top 16 bits of the residual, twice (truncation; hi + mid + lo == w exactly); rne: hi rounded to nearest even,
    mid = lo = 0."""
    Cout, Cin = w.shape[:2]
    weff = (w.flip(2, 3).permute(1, 0, 2, 3) if dgrad else w).reshape(*((Cin, Cout) if dgrad else (Cout, Cin)), 9).float()
    N, K = weff.shape[:2]
    lane = torch.arange(64)
    k = (torch.arange(K // 16).view(-1, 1, 1, 1) * 16 + 8 * (lane >> 5).view(1, -1, 1, 1) + 2 * torch.arange(4).view(1, 1, -1, 1)
         + torch.arange(2).view(1, 1, 1, -1))                                   # [kk, lane, e, j]
    n = torch.arange(N // 32).view(-1, 1) * 32 + (lane & 31).view(1, -1)          # [nb, lane]
    # vals[tap, kk, nb, lane, e, j]
    vals = weff.permute(2, 1, 0)[:, k[:, None], n[None, :, :, None, None]]        # [9, kk, nb, lane, e, j]
    if rne:
        planes = [_u16_rne(vals), torch.zeros_like(vals, dtype=torch.int64), torch.zeros_like(vals, dtype=torch.int64)]
    else:
        r1 = vals - _trunc_f32(vals)
        r2 = r1 - _trunc_f32(r1)
        planes = [_u16_trunc(vals), _u16_trunc(r1), _u16_trunc(r2)]
    words = torch.stack([p[..., 0] | (p[..., 1] << 16) for p in planes], 3)        # [9, kk, nb, 3, lane, e]
    return ((words ^ 0x80000000) - 0x80000000).to(torch.int32).contiguous()


def pack_bytes(Cin, Cout):
    return 9 * Cin * Cout * 3 * 2


def unpack_x3_plane(img, s):
    """plane s of a pack image as fp32 values [9, K/16, N/32, 64, 4, 2] (for the CPU checks)"""
    wds = img[:, :, :, s].to(torch.int64) & 0xFFFFFFFF
    lo, hi = (wds & 0xFFFF) << 16, wds & 0xFFFF0000
    both = torch.stack([lo, hi], -1)
    return ((both ^ 0x80000000) - 0x80000000).to(torch.int32).view(F32)


# ------------------------------------------------------------------------------------------------ launcher formulas
def tile_sel(Cout):
    """(MB, WM, BN) of launch_x3: MB = 4 (128 px x 128 co) where Cout % 128 == 0, else MB = 2, WM = 2 (128 px x 64 co); the bf16
    launches take TAG_X3_BF16_MB64 = 2 on the 64-cout tile in the product build: the same 128-pixel tile"""
    return (4, 1, 128) if Cout % 128 == 0 else (2, 2, 64)


def tile_geom(H, W, Cout):
    """dict(MB, WM, TH, row_tiles, n_tiles) of one image"""
    MB, WM, BN = tile_sel(Cout)
    TH = WM * MB * 32 // W
    return dict(MB=MB, WM=WM, TH=TH, row_tiles=-(-H // TH), n_tiles=Cout // BN)


def x3_stats_rows(B, H, W, Cout):
    """tag_conv3x3_x3_stats_rows"""
    if W not in WIDTHS:
        return 0
    th = 128 // W
    return B * -(-H // th) * (1 if Cout % 128 == 0 else 2)


def rows_cfg(H, W, Cin, Cout):
    """WN of the row-streaming kernel (2: W = 64, 64 -> 64; 4: W = 32, 64 -> multiple of 128), None where it refuses (H < 2 too)"""
    wn = 2 if (W == 64 and Cin == 64 and Cout == 64) else (4 if (W == 32 and Cin == 64 and Cout % 128 == 0) else 0)
    return wn if wn and H >= 2 else None


def rows_takes(H, W, Cin, Cout, pro, enabled=True):
    return bool(enabled and pro <= 1 and rows_cfg(H, W, Cin, Cout))


def rows_strips(B, H, NT, cus):
    ns = min(-(-cus // (B * NT)), H // 16)
    return max(ns, 1)


def rows_partial_rows(B, H, W, Cin, Cout, cus):
    wn = rows_cfg(H, W, Cin, Cout)
    return B * rows_strips(B, H, Cout // (wn * 32), cus) * 2 * (4 // wn) if wn else 0


def rows_strip_lengths(B, H, W, Cin, Cout, cus):
    wn = rows_cfg(H, W, Cin, Cout)
    ns = rows_strips(B, H, Cout // (wn * 32), cus)
    return [H * (i + 1) // ns - H * i // ns for i in range(ns)]


def bf16_stats_rows(B, H, W, Cin, Cout, pro, cus, rows_on=True):
    """tag_conv3x3_x3_bf16_stats_rows"""
    if W not in WIDTHS:
        return 0
    if rows_takes(H, W, Cin, Cout, pro, rows_on):
        return rows_partial_rows(B, H, W, Cin, Cout, cus)
    th = (128 if Cout % 128 == 0 else 64 * X3_BF16_MB64) // W
    return B * -(-H // th) * (1 if Cout % 128 == 0 else 2)


def poolsums_bf16_rows(B, H, W, Cin, Cout, rows_on=True):
    """tag_conv3x3_dgrad_poolsums_bf16_rows: one per workgroup m-tile, 0 = not served"""
    if W not in WIDTHS or Cin % 32 or Cout % 64 or Cin > 512 or rows_takes(H, W, Cin, Cout, 0, rows_on):
        return 0
    th = (128 if Cout % 128 == 0 else 64 * X3_BF16_MB64) // W
    return B * -(-H // th)


def chunk_geom(H, W, chunk_px):
    """(CW, CH, rb_per_img, cb_per_row) of the weight-gradient kernels: chunks of CH rows x CW columns, row blocks fastest"""
    cw = 32 if W >= 32 else W
    ch = chunk_px // cw
    return cw, ch, -(-H // ch), W // cw


def alltaps_splits(B, H, W, Cin, Cout, chunk_px=32, target=512):
    """(splits, chunks_per_split, chunks) of tag_wgrad_alltaps_splits"""
    cw, ch, rb, cb = chunk_geom(H, W, chunk_px)
    chunks = B * rb * cb
    tiles = -(-Cin // 64) * -(-Cout // 64)
    s = max(1, min(target // tiles, chunks // 8))
    cps = -(-chunks // s)
    return -(-chunks // cps), cps, chunks


def wgrad_x3_ws_bytes(B, H, W, Cin, Cout):
    return max(alltaps_splits(B, H, W, Cin, Cout, 32)[0], alltaps_splits(B, H, W, Cin, Cout, 64)[0]) * 9 * Cin * Cout * 4


WG_PX = {"x3": 32, "x9": 32, "np1": 32, "bf16": 16 * WX3_KS16, "dma": 16 * WX3_KS16}


def wgrad_claim(kind, B, H, W, Cin, Cout):
    """what a weight-gradient row reaches: dict(splits, cps, chunks, rb, last (chunks of the last split), starts (row block of each
    split's first chunk), ends (row block of each split's last chunk))"""
    px = WG_PX[kind]
    cw, ch, rb, cb = chunk_geom(H, W, px)
    sp, cps, chunks = alltaps_splits(B, H, W, Cin, Cout, px)
    return dict(splits=sp, cps=cps, chunks=chunks, rb=rb, CH=ch, last=chunks - (sp - 1) * cps,
                starts=[(i * cps) % rb for i in range(sp)], ends=[(min(chunks, (i + 1) * cps) - 1) % rb for i in range(sp)])


# ------------------------------------------------------------------------------------------------ inputs
def epi_case(B, Hf, Wf, C):
    return epi_inputs(B, Hf, Wf, C, seed_of(B, Hf, Wf, C, C))


def case(B, H, W, Cin, Cout, bf16=False):
    return inputs(B, H, W, Cin, Cout, seed_of(B, H, W, Cin, Cout), bf16)


def inputs(B, H, W, Cin, Cout, seed, bf16=False):
    """R.conv_inputs; bf16 storage rounds x and dy (the tensors ARE bf16), w stays fp32 (the pack rounds it)"""
    x, w, dy, s, t = R.conv_inputs(B, H, W, Cin, Cout, seed)
    if bf16:
        x, dy = x.bfloat16(), dy.bfloat16()
    return x, w, dy, s, t


def bn_tables(C, seed):
    g = torch.Generator().manual_seed(seed)
    gamma, beta = torch.rand(C, generator=g) + 0.5, 0.2 * torch.randn(C, generator=g)
    mean, var = 0.3 + 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    return gamma * invstd, beta - mean * gamma * invstd, mean, invstd


def epi_inputs(B, Hf, Wf, C, seed):
    """(yref as bf16 (B, Hf, Wf, C), scale, shift, mean, invstd) of the EPI 1 / EPI 2 launches"""
    g = torch.Generator().manual_seed(seed)
    yref = (torch.randn(B, Hf, Wf, C, generator=g) * 2 + 0.3).bfloat16()
    return (yref,) + tuple(bn_tables(C, seed + 1))


def seed_of(B, H, W, Cin, Cout):
    return 300 + 7 * W + H + Cin // 32 + Cout // 64


# ------------------------------------------------------------------------------------------------ the operand probe
def muladd_f32(v, s, t):
    """what a kernel computes that multiplies and then adds (two fp32 roundings) where the statement says fmaf (one)"""
    return v.float() * s.float() + t.float()


def _probe_values():
    bits = torch.arange(1 << 16, dtype=torch.int32)
    v = (bits << 16).view(F32)
    return v[torch.isfinite(v) & (v.abs() >= 2.0 ** -6) & (v.abs() <= 2.0 ** 3)]


def _prologue_pair(v, s, t, p):
    """(with fmaf, with multiply-then-add) of prologue mode p"""
    pre = leaky_f32(v) if p == 2 else v.float()
    a, b = fmaf(pre, s, t), muladd_f32(pre, s, t)
    return (torch.relu(a), torch.relu(b)) if p == 1 else (a, b)


def probe_tables(C, p, seed, tries=48):
    """(s, t, [(value, channel)]): per channel the one of ``tries`` seeded (scale, shift) pairs (drawn like those of conv_inputs) with the
    most DISCRIMINATORS -- bf16 values of moderate size at which bf16_rne of prologue mode p differs between fmaf and
    multiply-then-add (about one value in 10^5 is one) -- and the discriminators of the chosen pairs"""
    g = torch.Generator().manual_seed(seed)
    sc = torch.rand(C, tries, generator=g) + 0.5
    tc = (0.3 + 0.3 * torch.rand(C, tries, generator=g)) * (1 - 2 * (torch.arange(C) % 2))[:, None]
    v = _probe_values()[:, None, None]
    a, b = _prologue_pair(v, sc, tc, p)
    hit = a.bfloat16().float() != b.bfloat16().float()                     # [values, C, tries]
    best = hit.sum(0).argmax(1)
    s, t = sc[torch.arange(C), best], tc[torch.arange(C), best]
    chosen = hit[:, torch.arange(C), best].nonzero()
    return s, t, [(v[i, 0, 0].item(), int(c)) for i, c in chosen.tolist()]


def probe_inputs(B, H, W, C, p, pixels=None, bf16=True):
    """(x, s, t, planted) for the identity-weight probe: x of the case (B, H, W, C, C), the tables of probe_tables, and their
    discriminators (up to 96) planted at ``pixels`` (flat pixel indices, default all): a multiply-then-add prologue changes the
    bf16 operand of every planted element"""
    x, w, dy, s, t = case(B, H, W, C, C, bf16)
    flat = x.reshape(-1, C)
    pixels = list(range(flat.shape[0])) if pixels is None else pixels
    hits = []
    if p:
        s, t, hits = probe_tables(C, p, seed_of(B, H, W, C, C) + p)
        hits = hits[:96]
    for k, (val, c) in enumerate(hits):
        flat[pixels[(k * 7) % len(pixels)], c] = val
    return x, s, t, len(hits)


def identity_weight(Cout, Cin):
    """w[co, co % Cin, 1, 1] = 1: y[..., co] is the operand of channel co % Cin, exactly, in every arithmetic of the kernels (one
    non-zero product of an exactly split or bf16 value with 1.0 per output)"""
    w = torch.zeros(Cout, Cin, 3, 3)
    w[torch.arange(Cout), torch.arange(Cout) % Cin, 1, 1] = 1.0
    return w


def probe_expected(x, p, s, t, products, Cout):
    """the output of the identity convolution: the operand bit for bit (rounded to bf16 by the one-product arithmetic)"""
    a = operand(x, p, s, t)
    if products == 1:
        a = a.bfloat16().float()
    return a[..., torch.arange(Cout) % x.shape[-1]]


#: the probe's shapes: (B, H, W, Cin, Cout); every width, both tile widths, the row kernel's two configurations among them
PROBE_CASES = [(2, 5, 8, 64, 64), (2, 5, 16, 64, 128), (2, 5, 32, 64, 128), (2, 5, 64, 64, 64), (1, 3, 32, 64, 64), (1, 3, 64, 64, 128)]
#: the pixel whose 3 x 3 neighbourhood the weight-gradient probe reads (b, h, w), per shape (B, H, W) = (2, 5, W)
PROBE_PIXEL = (1, 2, 3)


# ------------------------------------------------------------------------------------------------ case tables
#: tag_pack_conv_weight_x3 (Cin, Cout), truncating and RNE
PACK_CASES = [(32, 64), (96, 192), (64, 320), (160, 64)]

PRODUCTS = {"x3": 6, "x9": 9, "np1": 1}

#: one launch per instantiation of the tile kernel: (B, H, W, Cin, Cout) -> every prologue x {x3, x9, np1 on fp32; np1 on bf16}; on
#: bf16 also EPI 1 and EPI 2.  H = 3: a border row above and below the middle row.
INST_TILE_CASES = [(1, 3, W, 64, Cout) for W in WIDTHS for Cout in (64, 128)]

#: tile-kernel edges, x3 on fp32 and one-product on bf16 (row kernel disabled): (B, H, W, Cin, Cout, pro, claim = (MB, row tiles per
#: image, n tiles)).  H over {1, TH - 1, TH, TH + 1, 2 TH + 1} of every width (TH = 16, 8, 4, 2), Cin over {32, 96, 160, 512} (+ 64),
#: Cout over {64, 192, 320, 384} (+ 128), B = 3 with 3 row tiles (9 m-tiles, odd).
TILE_CASES = [
    (1, 1, 8, 32, 64, 0, (2, 1, 1)), (3, 15, 8, 96, 192, 1, (2, 1, 3)), (1, 16, 8, 160, 320, 2, (2, 1, 5)),
    (3, 17, 8, 64, 384, 3, (4, 2, 3)), (3, 33, 8, 512, 64, 1, (2, 3, 1)),
    (3, 1, 16, 96, 384, 1, (4, 1, 3)), (1, 7, 16, 512, 192, 0, (2, 1, 3)), (3, 8, 16, 32, 320, 3, (2, 1, 5)),
    (1, 9, 16, 160, 64, 2, (2, 2, 1)), (3, 17, 16, 64, 192, 1, (2, 3, 3)),
    (1, 1, 32, 160, 192, 2, (2, 1, 3)), (3, 3, 32, 32, 384, 1, (4, 1, 3)), (3, 4, 32, 512, 64, 3, (2, 1, 1)),
    (1, 5, 32, 96, 320, 0, (2, 2, 5)), (3, 9, 32, 64, 128, 1, (4, 3, 1)),
    (3, 1, 64, 32, 192, 1, (2, 1, 3)), (1, 2, 64, 96, 64, 3, (2, 1, 1)), (3, 3, 64, 160, 384, 0, (4, 2, 3)),
    (3, 5, 64, 64, 320, 2, (2, 3, 5)), (1, 5, 64, 512, 128, 1, (4, 3, 1)),
]
#: bf16 only, 64-cout tile, H below / at / above 256 / W: with TAG_X3_BF16_MB64 = 4 these would straddle ONE 256-pixel tile; the
#: product build (MB64 = 2) runs them as two and three 128-pixel tiles.  (B, H, W, Cin, Cout, pro, claim)
TILE256_CASES = [(1, 15, 16, 64, 64, 1, (2, 2, 1)), (3, 16, 16, 64, 64, 0, (2, 2, 1)), (1, 17, 16, 64, 64, 1, (2, 3, 1)),
                 (3, 3, 64, 64, 64, 1, (2, 2, 1)), (1, 4, 64, 64, 64, 0, (2, 2, 1)), (3, 5, 64, 64, 64, 1, (2, 3, 1))]
#: H = 1 at the row kernel's own (W, Cin, Cout): it refuses, the tile kernel serves (default switches)
H1_CASES = [(3, 1, 64, 64, 64), (3, 1, 32, 64, 128)]

#: row-streaming kernel: (B, H, W, Cin, Cout, claim = (WN, strips per image with >= 64 CUs, an odd strip)).  Per case: forward
#: with and without statistics at prologue 0 and 1, and the dgrad with BatchNorm-backward sums (epi_kind 2): its five launches.
ROWS_CASES = [
    (1, 2, 64, 64, 64, (2, 1, False)), (3, 3, 64, 64, 64, (2, 1, True)), (1, 15, 64, 64, 64, (2, 1, True)),
    (3, 16, 64, 64, 64, (2, 1, False)), (1, 17, 64, 64, 64, (2, 1, True)), (3, 31, 64, 64, 64, (2, 1, True)),
    (1, 32, 64, 64, 64, (2, 2, False)), (3, 33, 64, 64, 64, (2, 2, True)), (1, 47, 64, 64, 64, (2, 2, True)),
    (3, 49, 64, 64, 64, (2, 3, True)),
    (3, 2, 32, 64, 128, (4, 1, False)), (1, 3, 32, 64, 256, (4, 1, True)), (3, 15, 32, 64, 384, (4, 1, True)),
    (1, 16, 32, 64, 128, (4, 1, False)), (3, 17, 32, 64, 256, (4, 1, True)), (1, 31, 32, 64, 384, (4, 1, True)),
    (3, 32, 32, 64, 128, (4, 2, False)), (1, 33, 32, 64, 256, (4, 2, True)), (3, 47, 32, 64, 384, (4, 2, True)),
    (1, 49, 32, 64, 128, (4, 3, True)),
]
#: the CU cap of rows_strips binds (ceil(cus / (B NT)) < H / 16 for any cus <= 256): two distinct images repeated alternately
ROWS_CAP_CASE = (128, 48, 64, 64, 64)

#: weight gradients: (kind, B, H, W, Cin, Cout, pro); kind 'x3' = conv3x3_wgrad_x3_kernel<TW, PRO, 6, float> (32-pixel chunks),
#: 'bf16' = <TW, PRO, 1, bf16> (64-pixel chunks, register-staged: tag_wgrad_dma_enable(0)), 'dma' = conv3x3_wgrad_dma_kernel
#: (64-pixel chunks; prologue 1 with tag_wgrad_dma_enable(2)).  CH = 4, 2, 1, 1 (x3) and 8, 4, 2, 2 (bf16, dma) at W = 8, 16, 32, 64.
def _wg_h_sweep():
    out = []
    for kind in ("x3", "bf16", "dma"):
        for W in WIDTHS:
            ch = chunk_geom(1, W, WG_PX[kind])[1]
            hs = sorted({h for h in (1, ch - 1, ch, ch + 1, 2 * ch + 1) if h >= 1})
            for i, H in enumerate(hs):
                pro = (i % 2) if kind == "dma" else (i + W // 8) % 4
                out.append((kind, 1 + 2 * (i % 2), H, W, 64, 64, pro))
    return out


WGRAD_H_CASES = _wg_h_sweep()

#: splits: (kind, B, H, W, Cin, Cout, pro, claim = (splits, chunks per split, chunks of the LAST split, why the row is here)).
#: splits = min(512 / tiles, chunks / 8) makes every split but the last at least 8 chunks long, so the ranges shorter than the DMA
#: prefetch depth are a last split of 1 ('last1') or 2 ('last2') chunks -- and the images of fewer than 3 chunks of the H sweep above.
#: 'short': a last split shorter than the others; 'start_last': some split starts on the LAST row block of a strip (one chunk, then
#: the strip change); 'start_first': some split after the first starts on the first row block of a strip (the one before it ended
#: on a strip's last).  W = 64 has two column strips per image.
WGRAD_SPLIT_CASES = [
    ("x3", 3, 25, 8, 64, 64, 1, (2, 11, 10, "short")), ("x3", 3, 29, 8, 64, 64, 2, (3, 8, 8, "start_first")),
    ("x3", 3, 53, 8, 64, 64, 3, (5, 9, 6, "start_last")), ("x3", 2, 73, 16, 64, 64, 0, (9, 9, 2, "last2")),
    ("x3", 3, 27, 16, 64, 64, 1, (5, 9, 6, "start_last")), ("x3", 1, 73, 32, 64, 64, 1, (9, 9, 1, "last1")),
    ("x3", 1, 65, 32, 64, 64, 2, (8, 9, 2, "last2")), ("x3", 3, 14, 32, 64, 64, 3, (5, 9, 6, "start_last")),
    ("x3", 3, 7, 64, 64, 64, 1, (5, 9, 6, "start_last")), ("x3", 1, 41, 64, 64, 64, 0, (10, 9, 1, "last1")),
    ("x3", 1, 37, 64, 64, 64, 2, (9, 9, 2, "last2")), ("x3", 3, 3, 64, 64, 64, 3, (2, 9, 9, "start_first")),
] + [(kind, B, H, W, 64, 64, (i % 2 if kind == "dma" else (i + 1) % 4), claim)
     for kind in ("bf16", "dma")
     for i, (B, H, W, claim) in enumerate([
         (3, 49, 8, (2, 11, 10, "short")), (3, 57, 8, (3, 8, 8, "start_first")), (3, 53, 16, (5, 9, 6, "start_last")),
         (3, 25, 16, (2, 11, 10, "short")), (2, 73, 32, (9, 9, 2, "last2")), (3, 27, 32, (5, 9, 6, "start_last")),
         (2, 49, 64, (12, 9, 1, "last1")), (1, 73, 64, (9, 9, 2, "last2")), (3, 13, 64, (5, 9, 6, "start_last")),
         (3, 5, 64, (2, 9, 9, "start_first"))])]


def split_tag_holds(tag, c):
    """the reason a WGRAD_SPLIT_CASES row gives, checked on its wgrad_claim()"""
    if tag == "short":
        return c["splits"] >= 2 and c["last"] < c["cps"]
    if tag in ("last1", "last2"):
        return c["splits"] >= 2 and c["last"] == int(tag[-1])
    if tag == "start_last":
        return c["rb"] > 2 and any(s == c["rb"] - 1 for s in c["starts"][1:])
    if tag == "start_first":
        return c["rb"] > 2 and any(s == 0 for s in c["starts"][1:]) and any(e == c["rb"] - 1 for e in c["ends"][:-1])
    return False


#: per W one shape on every prologue (x3, bf16) and nine 64 x 64 tiles: (kind, B, H, W, Cin, Cout, pro)
WGRAD_PRO_CASES = [(kind, 3, H, W, Cin, Cout, pro)
                   for kind in ("x3", "bf16") for (H, W, Cin, Cout) in ((9, 8, 64, 192), (5, 16, 192, 64), (3, 32, 64, 64), (3, 64, 192, 192))
                   for pro in range(4)] + \
                  [("dma", 3, H, W, Cin, Cout, pro) for (H, W, Cin, Cout) in ((9, 8, 64, 192), (5, 16, 192, 64), (3, 32, 64, 64), (3, 64, 192, 192))
                   for pro in (0, 1)]
#: one launch per instantiation of the x9 / one-product-on-fp32 weight gradients: (kind, B, H, W, Cin, Cout, pro)
WGRAD_INST_CASES = [(kind, 1, 3, W, 64, 64, pro) for kind in ("x9", "np1") for W in WIDTHS for pro in range(4)]

#: fused epilogues on bf16: tag_conv3x3_dgrad_bnsums_bf16 (B, H, W, Cin, Cout, path)
BNSUMS_CASES = [(3, 17, 8, 64, 192, "tile"), (1, 9, 16, 128, 128, "tile"), (3, 5, 32, 96, 64, "tile"), (3, 3, 64, 64, 384, "tile"),
                (1, 1, 64, 64, 64, "tile"), (3, 33, 64, 64, 64, "rows"), (1, 17, 32, 64, 128, "rows")]
#: tag_conv3x3_dgrad_poolsums_bf16: (B, Hf, Wf, Cin, Cout, ph, pool); drop_p 0 and 0.3 on each; odd Hf with ph = 2 leaves a row over
POOLSUMS_CASES = [(3, 7, 16, 64, 192, 2, 0), (1, 9, 32, 128, 128, 1, 2), (3, 11, 64, 96, 64, 2, 3), (1, 5, 128, 64, 384, 1, 0),
                  (3, 35, 16, 32, 64, 2, 2), (1, 3, 128, 160, 320, 2, 3)]
#: ... and what it refuses: a shape the row kernel takes (B, Hf, Wf, Cin, Cout, ph)
POOLSUMS_ROWS_REFUSED = (1, 8, 128, 64, 64, 2)


# ------------------------------------------------------------------------------------------------ instantiations
def selectable_instantiations():
    """every template instance the x3 / bf16 entry points can launch: with the default switches, with tag_conv_rows_enable(0) (the
    tile kernel on the row kernel's shapes) and with tag_wgrad_dma_enable(0 | 2).
    tile: (MB, PRO, TW, NP, storage, EPI); wgrad: (TW, PRO, NP, storage); dma: (TW, PRO); rows: (TW, WN, PRO, EPI)"""
    tile = {(MB, pro, TW, NP, "f32", 0) for MB in (2, 4) for pro in range(4) for TW in WIDTHS for NP in (6, 9, 1)}
    tile |= {(MB, pro, TW, 1, "bf16", 0) for MB in (2, 4) for pro in range(4) for TW in WIDTHS}
    tile |= {(MB, 0, TW, 1, "bf16", e) for MB in (2, 4) for TW in WIDTHS for e in (1, 2)}
    wgrad = {(TW, pro, NP, "f32") for TW in WIDTHS for pro in range(4) for NP in (6, 9, 1)}
    wgrad |= {(TW, pro, 1, "bf16") for TW in WIDTHS for pro in range(4)}
    dma = {(TW, pro) for TW in WIDTHS for pro in (0, 1)}
    rows = {(TW, WN, pro, e) for (TW, WN) in ((64, 2), (32, 4)) for (pro, e) in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2))}
    return dict(tile=tile, wgrad=wgrad, dma=dma, rows=rows)


def table_instantiations():
    """what the tables reach, derived with the formulas above the way the GPU module runs them"""
    tile, wgrad, dma, rows = set(), set(), set(), set()
    for B, H, W, Cin, Cout in INST_TILE_CASES:                       # row kernel disabled
        MB = tile_sel(Cout)[0]
        for pro in range(4):
            for NP in (6, 9, 1):
                tile.add((MB, pro, W, NP, "f32", 0))
            tile.add((MB, pro, W, 1, "bf16", 0))
        tile.add((MB, 0, W, 1, "bf16", 1))
        tile.add((MB, 0, W, 1, "bf16", 2))
    for B, H, W, Cin, Cout, pro, claim in TILE_CASES:
        tile.add((tile_sel(Cout)[0], pro, W, 6, "f32", 0))
        tile.add((tile_sel(Cout)[0], pro, W, 1, "bf16", 0))
    for B, H, W, Cin, Cout, claim in ROWS_CASES:
        wn = rows_cfg(H, W, Cin, Cout)
        rows |= {(W, wn, pro, e) for (pro, e) in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2))}
    for kind, B, H, W, Cin, Cout, pro in WGRAD_H_CASES + [c[:7] for c in WGRAD_SPLIT_CASES] + WGRAD_PRO_CASES + WGRAD_INST_CASES:
        if kind == "dma":
            dma.add((W, pro))
        elif kind == "bf16":
            wgrad.add((W, pro, 1, "bf16"))
        else:
            wgrad.add((W, pro, PRODUCTS[kind], "f32"))
    return dict(tile=tile, wgrad=wgrad, dma=dma, rows=rows)
