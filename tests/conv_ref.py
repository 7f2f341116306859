"""Plain-torch statements of every operation of csrc/conv.hip and csrc/conv_c1.hip (channels-last, as the kernels see them), the launchers' host
formulas restated in Python, and the case tables of tests/test_gpu_conv_sweep.py with the CLAIM each row makes about the kernel it
reaches.  tests/test_conv_ref_cpu.py checks the statements against F.conv2d / autograd / F.batch_norm / the torch pools to 1e-12
and every claim against the restated formulas; the GPU module compares the kernels with the statements.

Every statement takes ``dtype``: torch.float64 is the reference, torch.float32 the floor printed beside each error.

Layouts: activations (B, H, W, C); weights (Cout, Cin, 3, 3) as the reference model keeps them; the forward pack (9, Cin, Cout) and
the dgrad pack (9, Cout, Cin) with flipped taps (tag_pack_conv_weight); weight gradients (Cout, Cin, 3, 3)."""
import math

import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ statements
def prologue(x, p, s, t):
    """The producer's BatchNorm folded into the operand load: 0 none, 1 relu(x s + t), 2 leaky_relu(x, 0.1) s + t, 3 x s + t"""
    if p == 0:
        return x
    s, t = s.to(x.dtype), t.to(x.dtype)
    if p == 1:
        return torch.relu(x * s + t)
    if p == 2:
        return torch.where(x > 0, x, 0.1 * x) * s + t
    return x * s + t


def shifted(a, dy, dx):
    """out[b, h, w] = a[b, h + dy, w + dx], zero outside the image (the padding is applied to the prologue's OUTPUT)"""
    B, H, W, C = a.shape
    out = torch.zeros_like(a)
    h0, h1, w0, w1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if h0 < h1 and w0 < w1:
        out[:, h0:h1, w0:w1] = a[:, h0 + dy:h1 + dy, w0 + dx:w1 + dx]
    return out


def conv_fwd(x, w, p=0, s=None, t=None, dtype=F64, bias=None):
    """y[b,h,w,co] = sum_tap sum_ci prologue(x)[b, h+ky-1, w+kx-1, ci] w[co,ci,ky,kx] (+ bias[b, co])"""
    a = prologue(x.to(dtype), p, s, t)
    w = w.to(dtype)
    y = torch.zeros(*x.shape[:3], w.shape[0], dtype=dtype)
    for ky in range(3):
        for kx in range(3):
            y += shifted(a, ky - 1, kx - 1) @ w[:, :, ky, kx].t()
    if bias is not None:
        y = y + bias.to(dtype)[:, None, None, :]
    return y


def pack_fwd(w):
    """(Cout, Cin, 3, 3) -> (9, Cin, Cout)"""
    return w.permute(2, 3, 1, 0).reshape(9, w.shape[1], w.shape[0]).contiguous()


def pack_dgrad(w):
    """(Cout, Cin, 3, 3) -> (9, Cout, Cin), taps flipped: the forward entry on this pack is the data gradient"""
    return w.flip(2, 3).permute(2, 3, 0, 1).reshape(9, w.shape[0], w.shape[1]).contiguous()


def unpack(wp):
    """a (9, K, N) pack read as the (N, K, 3, 3) weight of the convolution K -> N it makes the forward entry compute"""
    return wp.reshape(3, 3, wp.shape[1], wp.shape[2]).permute(3, 2, 0, 1).contiguous()


def conv_dgrad(dy, w, dtype=F64):
    """da[b,h,w,ci] = sum_tap sum_co dy[b, h-(ky-1), w-(kx-1), co] w[co,ci,ky,kx]: the gradient w.r.t. the prologue's output"""
    return conv_fwd(dy, unpack(pack_dgrad(w)), dtype=dtype)


def conv_wgrad(x, dy, p=0, s=None, t=None, dtype=F64):
    """dw[co,ci,ky,kx] = sum_{b,h,w} prologue(x)[b, h+ky-1, w+kx-1, ci] dy[b,h,w,co]"""
    a = prologue(x.to(dtype), p, s, t)
    g = dy.to(dtype).reshape(-1, dy.shape[-1])
    dw = torch.zeros(dy.shape[-1], x.shape[-1], 3, 3, dtype=dtype)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = g.t() @ shifted(a, ky - 1, kx - 1).reshape(-1, x.shape[-1])
    return dw


def bn_fold(y, eps=1e-5):
    """(mean, invstd) per channel over (B, H, W), biased variance: what the folded partial statistics must give"""
    v = y.reshape(-1, y.shape[-1])
    mean = v.mean(0)
    return mean, 1.0 / torch.sqrt(((v - mean) ** 2).mean(0) + eps)


def fold_stats_partials(buf, P, C, eps=1e-5):
    """The forward kernels' partial statistics, [P][3][C] rows of (pivot mu, sum(y - mu), sum((y - mu)^2)) followed by [P] pixel
    counts, merged in fp64: (mean, invstd, total count)"""
    buf = buf.double()
    rows, cnt = buf[:P * 3 * C].view(P, 3, C), buf[P * 3 * C:P * 3 * C + P]
    mu, r, q = rows[:, 0], rows[:, 1], rows[:, 2]
    n = cnt.sum()
    mean = (cnt[:, None] * mu + r).sum(0) / n
    d = mu - mean
    m2 = (q + 2 * d * r + cnt[:, None] * d * d).sum(0)
    return mean, 1.0 / torch.sqrt(m2 / n + eps), int(n.item())


def bn_bwd_sums(da, yref, scale, shift, mean, invstd, dtype=F64):
    """(sum dz, sum dz xhat) per channel with dz = da [bn(yref) > 0], xhat = (yref - mean) invstd"""
    da, y = da.to(dtype), yref.to(dtype)
    dz = da * ((y * scale.to(dtype) + shift.to(dtype)) > 0)
    xhat = (y - mean.to(dtype)) * invstd.to(dtype)
    C = y.shape[-1]
    return dz.reshape(-1, C).sum(0), (dz * xhat).reshape(-1, C).sum(0)


def _windows(a, ph, pw=2):
    """(B, Hf, Wf, C) -> (B, Hf // ph, Wf // pw, ph * pw, C), floor windows in scan order"""
    B, Hf, Wf, C = a.shape
    H, W = Hf // ph, Wf // pw
    return a[:, :H * ph, :W * pw].reshape(B, H, ph, W, pw, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, ph * pw, C)


def pool_weights(pool, ph, pw=2):
    """(wavg, wmax) of pool type 0 'avg+max' | 2 'avg' | 3 'max'"""
    return (0.0 if pool == 3 else 1.0 / (ph * pw)), (0.0 if pool == 2 else 1.0)


def bnrelu_pool(y, scale, shift, ph, pool, dtype=F64):
    """pool(relu(y scale + shift)) with ph x 2 floor windows"""
    win = _windows(torch.relu(y.to(dtype) * scale.to(dtype) + shift.to(dtype)), ph)
    wavg, wmax = pool_weights(pool, ph)
    return win.sum(3) * wavg + win.max(3).values * wmax


def pool_bwd_sums(dx, yref, scale, shift, mean, invstd, ph, pool, keep=None, drop_p=0.0, dtype=F64):
    """(sum dz, sum dz xhat) of relu(bn(yref)) -> pool(ph x 2, floor) -> dropout, given the gradient dx (B, H, W, C) of the dropped
    pooled tensor: dz = [a > 0] g (wavg + [first arg-max of the window] wmax), g = dx keep / (1 - p); rows the floor drops get none"""
    y = yref.to(dtype)
    g = dx.to(dtype)
    if keep is not None:
        g = g * keep.to(dtype) / (1.0 - drop_p)
    a = _windows(y * scale.to(dtype) + shift.to(dtype), ph)
    xhat = _windows((y - mean.to(dtype)) * invstd.to(dtype), ph)
    wavg, wmax = pool_weights(pool, ph)
    first = F.one_hot(a.argmax(3), a.shape[3]).movedim(-1, 3).to(dtype)       # torch.argmax: the first maximum
    dz = (a > 0) * g.unsqueeze(3) * (wavg + first * wmax)
    C = y.shape[-1]
    return dz.reshape(-1, C).sum(0), (dz * xhat).reshape(-1, C).sum(0)


def c1_in(x, cs, ct, dtype=F64):
    """(B, H, W) -> (B, H, W, 1) with the per-COLUMN affine x cs[w] + ct[w] (bn0 over the mel axis), before the zero padding"""
    a = x.to(dtype)
    if cs is not None:
        a = a * cs.to(dtype) + ct.to(dtype)
    return a.unsqueeze(-1)


def c1_fwd(x, w, cs=None, ct=None, dtype=F64, bias=None):
    return conv_fwd(c1_in(x, cs, ct, dtype), w, dtype=dtype, bias=bias)


def c1_wgrad(x, dy, cs=None, ct=None, dtype=F64):
    return conv_wgrad(c1_in(x, cs, ct, dtype), dy, dtype=dtype)


def c1_dgrad(dy, w, dtype=F64):
    """gradient w.r.t. the affine's output, (B, H, W)"""
    return conv_dgrad(dy, w, dtype)[..., 0]


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


# ------------------------------------------------------------------------------------------------ inputs
def conv_inputs(B, H, W, Cin, Cout, seed):
    """x + 0.5, w / sqrt(9 Cin) + 1 / (9 Cin) (so that the statistics of y have means of the order of their deviations), dy and a
    prologue table whose shift has BOTH signs and is nowhere zero: a kernel that pads before the
    prologue turns every border zero into t (pro 2, 3) or relu(t) (pro 1, the positive half)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g) + 0.5
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin) + 1.0 / (9 * Cin)      # channel means of y of order 0.5
    dy = torch.randn(B, H, W, Cout, generator=g)
    s = torch.rand(Cin, generator=g) + 0.5
    t = (0.3 + 0.3 * torch.rand(Cin, generator=g)) * (1 - 2 * (torch.arange(Cin) % 2))
    return x, w, dy, s, t


def c1_inputs(B, H, W, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, generator=g) * 10 - 30
    cs, ct = torch.rand(W, generator=g) * 0.1 + 0.05, torch.randn(W, generator=g) + 3.0
    w = torch.randn(Cout, 1, 3, 3, generator=g) / 3
    dy = torch.randn(B, H, W, Cout, generator=g)
    return x, cs, ct, w, dy


# ------------------------------------------------------------------------------------------------ launcher formulas
HALO_W = (4, 8, 16, 32, 64)


def halo_geom(H, W, Cout, stats_or_epi=False, bn256=1):
    """tag_conv3x3_forward's halo launch: dict(BN, TW, TH, col_tiles, row_tiles, n_tiles, grid)"""
    assert W in HALO_W
    TW = 32 if W == 64 else W
    TH = 128 // TW
    BN = 256 if ((bn256 == 2 or (bn256 == 1 and stats_or_epi)) and W <= 16 and Cout % 256 == 0) else (128 if Cout >= 128 else 64)
    col_tiles = W // TW
    row_tiles = -(-H // TH) * col_tiles
    return dict(BN=BN, TW=TW, TH=TH, col_tiles=col_tiles, row_tiles=row_tiles, n_tiles=-(-Cout // BN))


def stats_rows(B, H, W):
    g = halo_geom(H, W, 64)
    return B * g["row_tiles"] * 2


def magic(d):
    """launch_halo's multiply-shift pair of the divisor d"""
    l = 0
    while (1 << l) < d:
        l += 1
    return ((1 << 32) * ((1 << l) - d)) // d + 1, l


def magic_div(n, d):
    """halo_fdiv: (mulhi(n, mul) + n) >> shr in 32-bit arithmetic"""
    mul, shr = magic(d)
    assert mul < (1 << 32)
    return ((((n * mul) >> 32) + n) & 0xFFFFFFFF) >> shr


def fwd_kernel(W, Cout, conv_impl=0):
    """('halo', BN, TW) or ('tap', BN) of tag_conv3x3_forward without statistics"""
    if conv_impl == 0 and W in HALO_W:
        g = halo_geom(1, W, Cout)
        return ("halo", g["BN"], g["TW"])
    return ("tap", 128 if Cout >= 128 else 64)


def alltaps_splits(B, H, W, Cin, Cout, target=512):
    """(splits, chunks_per_split, chunks per image) of the all-taps / row-ring weight gradient"""
    cw = 32 if W >= 32 else W
    ch = 32 // cw
    per_image = -(-H // ch) * (W // cw)
    chunks = B * per_image
    tiles = -(-Cin // 64) * -(-Cout // 64)
    s = max(1, min(target // tiles, chunks // 8))
    cps = -(-chunks // s)
    return -(-chunks // cps), cps, per_image


def wgrad_tile(Cin, Cout):
    return 128 if Cin >= 128 and Cout >= 128 else 64


def wgrad_splits(M, Cin, Cout):
    """(splits, chunk in pixels) of the per-tap weight gradient"""
    TC = wgrad_tile(Cin, Cout)
    tiles = 9 * -(-Cin // TC) * -(-Cout // TC)
    s = max(1, min(1536 // tiles, -(-M // 512)))
    chunk = -(-(-(-M // s)) // 32) * 32
    return s, chunk


def wgrad_kernel(W, Cin, Cout, conv_impl=0):
    """('alltaps', W) for W 4 / 8, ('ring', W) for W 16 / 32 / 64, else ('tap', TC)"""
    if conv_impl == 0 and W in HALO_W:
        return ("ring" if W >= 16 else "alltaps", W)
    return ("tap", wgrad_tile(Cin, Cout))


def wgrad_ws_bytes(B, H, W, Cin, Cout, conv_impl=0):
    if wgrad_kernel(W, Cin, Cout, conv_impl)[0] != "tap":
        return alltaps_splits(B, H, W, Cin, Cout)[0] * 9 * Cin * Cout * 4
    return wgrad_splits(B * H * W, Cin, Cout)[0] * 9 * Cin * Cout * 4


def tap_chunk_rows(B, H, W, kb, wrap="mod"):
    """conv3x3_wgrad_kernel::load_chunk's index arithmetic for the 32 pixels from kb on: [(m, row, column)] as the kernel locates
    them.  wrap 'mod': the row by a true modulo (this tree); 'once': one conditional subtraction (the parent commit)."""
    rW = (65536 + W - 1) // W
    hw0 = kb % (H * W)
    h0, w0 = divmod(hw0, W)
    out = []
    for pix in range(32):
        t = w0 + pix
        dh = (1 if t >= W else 0) if W >= 32 else (t * rW) >> 16
        hh = h0 + dh
        hh = hh % H if wrap == "mod" else (hh - H if hh >= H else hh)
        out.append((kb + pix, hh, t - dh * W))
    return out


def tap_mislocated(B, H, W, wrap):
    """pixels m < B H W that load_chunk places on another (row, column) than m % (H W) has"""
    M, bad = B * H * W, 0
    for kb in range(0, M, 32):
        for m, hh, ww in tap_chunk_rows(B, H, W, kb, wrap):
            if m < M and (hh, ww) != divmod(m % (H * W), W):
                bad += 1
    return bad


def spans_two_boundaries(B, H, W):
    """some 32-pixel chunk of the per-tap weight gradient holds pixels (below M = B H W) of three images"""
    M = B * H * W
    return W < 32 and any((kb % (H * W)) + min(31, M - 1 - kb) >= 2 * H * W for kb in range(0, M, 32))


def c1_fwd_kernel(W, Cout):
    if W == 64 and Cout == 64:
        return "rows"
    if W % 4 == 0 and 256 % (Cout // 4) == 0:
        return "fwd4"
    return "generic"


def c1_bwd_geom(B, H):
    """(strips, rows) of the fused Cin = 1 kernels"""
    r = max(8, -(-H // max(1, 2048 // B)))
    return -(-H // r), r


def c1_wgrad_blocks(M, Cout):
    rpi = 256 // (Cout // 4)
    return min(1024, max(1, -(-M // (rpi * 64)))), rpi


# ------------------------------------------------------------------------------------------------ case tables
FWD, STAT_MEAN, STAT_INVSTD, SUMS, C1 = 5e-6, 1e-6, 2e-6, 1e-5, 2e-6

#: tag_pack_conv_weight (Cin, Cout); the last has 9 * 256 * 260 = 599040 > 2048 * 256 elements: a second grid-stride trip
PACK_CASES = [(32, 4), (96, 68), (32, 68), (96, 4), (256, 260)]
PACK_GRID_ELEMS = 2048 * 256

#: halo path of tag_conv3x3_forward: (B, H, W, Cin, Cout, pro, claim) with claim = (BN without stats, TW, row_tiles, n_tiles).
#: H runs over {1, TH - 1, TH, TH + 1, 2 TH + 1} of every width (TH = 32, 16, 8, 4, 4), the couts over partial tiles of both widths
#: (4, 36 | 132, 320), B = 3 with row_tiles 3, 5 and 7 and n_tiles 3 for the multiply-shift division by a non-power of two.
HALO_CASES = [
    (1, 1, 4, 32, 4, 0, (64, 4, 1, 1)), (3, 31, 4, 32, 36, 1, (64, 4, 1, 1)), (1, 32, 4, 96, 64, 2, (64, 4, 1, 1)),
    (3, 33, 4, 32, 68, 3, (64, 4, 2, 2)), (3, 65, 4, 32, 132, 1, (128, 4, 3, 2)),
    (1, 1, 8, 32, 36, 1, (64, 8, 1, 1)), (3, 15, 8, 96, 68, 2, (64, 8, 1, 2)), (1, 16, 8, 32, 128, 3, (128, 8, 1, 1)),
    (3, 17, 8, 32, 132, 0, (128, 8, 2, 2)), (3, 33, 8, 32, 320, 1, (128, 8, 3, 3)),
    (3, 1, 16, 32, 68, 2, (64, 16, 1, 2)), (1, 7, 16, 96, 4, 3, (64, 16, 1, 1)), (3, 8, 16, 32, 132, 1, (128, 16, 1, 2)),
    (1, 9, 16, 512, 64, 1, (64, 16, 2, 1)), (3, 17, 16, 32, 320, 0, (128, 16, 3, 3)), (3, 39, 16, 32, 36, 2, (64, 16, 5, 1)),
    (1, 1, 32, 96, 132, 3, (128, 32, 1, 2)), (3, 3, 32, 32, 4, 1, (64, 32, 1, 1)), (1, 4, 32, 32, 68, 0, (64, 32, 1, 2)),
    (3, 5, 32, 32, 128, 2, (128, 32, 2, 1)), (3, 9, 32, 32, 320, 1, (128, 32, 3, 3)), (3, 25, 32, 32, 64, 3, (64, 32, 7, 1)),
    (1, 1, 64, 32, 68, 1, (64, 32, 2, 2)), (3, 3, 64, 32, 36, 2, (64, 32, 2, 1)), (1, 4, 64, 96, 128, 0, (128, 32, 2, 1)),
    (3, 5, 64, 32, 132, 3, (128, 32, 4, 2)), (3, 9, 64, 32, 4, 1, (64, 32, 6, 1)), (3, 10, 64, 32, 320, 0, (128, 32, 6, 3)),
]
#: with statistics the 256-cout tile serves W <= 16 and Cout % 256 == 0: (B, H, W, Cin, Cout, pro)
HALO256_CASES = [(3, 17, 8, 32, 256, 1), (1, 9, 16, 32, 512, 0), (3, 33, 4, 32, 256, 3)]

#: one tiny launch WITH statistics per <BN, PRO, TW, 0> instantiation a default launch can select (44: the 256-cout tile serves
#: W <= 16 when statistics are asked for; a 64-wide image runs on TW = 32 as the tables above show): (B, H, W, Cin, Cout, pro)
HALO_INST_CASES = [(1, 2, W, 32, Cout, pro) for W in (4, 8, 16, 32) for Cout in (64, 128, 256) for pro in (0, 1, 2, 3)
                   if not (Cout == 256 and W == 32)]

#: tap-by-tap forward, (B, H, W, Cin, Cout, pro, M): every width no halo tile serves, M below / equal to / just above 128, H = 1
TAP_FWD_CASES = [
    (3, 5, 1, 32, 64, 0, 15), (1, 64, 2, 32, 128, 1, 128), (3, 14, 3, 32, 36, 2, 126), (1, 26, 5, 96, 132, 3, 130),
    (1, 1, 12, 32, 64, 1, 12), (3, 1, 20, 32, 128, 2, 60), (3, 1, 40, 32, 36, 3, 120), (2, 1, 65, 32, 132, 0, 130),
    (1, 1, 128, 32, 64, 1, 128), (1, 2, 65, 64, 4, 1, 130), (3, 7, 12, 32, 320, 2, 252),
]

#: tag_conv3x3_forward_bias: the served (W, Cin) pairs at Cout 128 with prologues 2 | 3, B = 3: (B, H, W, Cin, pro)
BIAS_CASES = [(3, 9, 16, 32, 2), (3, 8, 16, 128, 3), (3, 33, 4, 32, 3), (3, 31, 4, 128, 2)]

#: all-taps (W 4 / 8) and row-ring (W 16 / 32 / 64) weight gradient: (B, H, W, Cin, Cout, pro, (splits, cps, a split holds pixels of two images))
ALLTAPS_CASES = [
    (1, 1, 4, 4, 4, 0, (1, 1, False)), (3, 2, 8, 36, 64, 1, (1, 3, True)), (3, 3, 4, 64, 36, 2, (1, 3, True)),
    (3, 37, 8, 96, 132, 3, (3, 10, False)), (3, 41, 8, 36, 4, 1, (4, 9, True)), (3, 41, 4, 132, 96, 2, (2, 9, True)),
    (1, 5, 16, 4, 132, 3, (1, 3, False)), (3, 37, 16, 64, 64, 1, (7, 9, True)), (3, 41, 16, 36, 96, 0, (7, 9, True)),
    (3, 1, 32, 36, 36, 2, (1, 3, True)), (3, 2, 32, 64, 4, 1, (1, 6, True)), (3, 37, 32, 96, 64, 3, (13, 9, True)),
    (3, 3, 64, 4, 36, 1, (2, 9, True)), (1, 5, 64, 132, 132, 0, (1, 10, False)), (3, 41, 64, 64, 64, 2, (28, 9, True)),
    # the <TW, PRO> instantiations the rows above leave out
    (1, 2, 4, 4, 4, 1, (1, 1, False)), (1, 2, 4, 4, 4, 3, (1, 1, False)), (1, 2, 8, 4, 4, 0, (1, 1, False)),
    (1, 2, 8, 4, 4, 2, (1, 1, False)), (1, 2, 16, 4, 4, 2, (1, 1, False)), (1, 2, 32, 4, 4, 0, (1, 2, False)),
    (1, 2, 64, 4, 4, 3, (1, 4, False)),
]

#: per-tap weight gradient: (B, H, W, Cin, Cout, pro, (TC, splits, chunk))
TAP_WGRAD_CASES = [
    (3, 9, 1, 32, 64, 0, (64, 1, 32)), (3, 11, 3, 64, 36, 1, (64, 1, 128)), (2, 13, 5, 128, 128, 2, (128, 1, 160)),
    (3, 9, 7, 132, 260, 3, (128, 1, 192)), (3, 5, 12, 4, 132, 1, (64, 1, 192)), (3, 3, 20, 96, 64, 2, (64, 1, 192)),
    (3, 41, 5, 64, 64, 1, (64, 2, 320)), (3, 2, 40, 36, 4, 3, (64, 1, 256)), (2, 7, 40, 128, 132, 0, (128, 2, 288)),
    (2, 9, 3, 128, 128, 1, (128, 1, 64)),
]
#: the tiny images whose 32-pixel chunks span two image boundaries (one row wrap mis-locates pixels), and their controls
TINY_WGRAD = [(3, 1, 5), (3, 2, 5), (3, 3, 5), (3, 2, 7), (3, 1, 12), (3, 7, 1), (3, 5, 3)]
TINY_CONTROLS = [(3, 7, 5), (3, 5, 7)]

#: Cin = 1 forward: (B, H, W, Cout, kernel)
C1_FWD_CASES = [(2, 9, 64, 64, "rows"), (3, 5, 8, 4, "fwd4"), (2, 7, 12, 32, "fwd4"), (1, 3, 64, 128, "fwd4"),
                (2, 5, 62, 64, "generic"), (3, 4, 8, 12, "generic"), (1, 1, 1, 4, "generic")]
#: tag_conv3x3_c1_forward_bias, two clips in one workgroup (H W / 4 pixel groups per clip, fewer than the 256 / (Cout / 4) of a workgroup)
C1_BIAS_CASES = [(3, 3, 8, 64), (2, 5, 4, 4), (3, 1, 12, 128)]
#: Cin = 1 weight gradient and dgrad: (B, H, W, Cout, (kernel, blocks)); the last two rows have M > 1024 rpi 64 (a second
#: grid-stride trip; M Cout is then above 2^26 whatever Cout is, the one place the sweep leaves its 5 M element budget)
C1_WGRAD_CASES = [(1, 1, 3, 4, ("generic", 1)), (2, 5, 7, 64, ("generic", 1)), (3, 9, 8, 256, ("wgrad4", 1)),
                  (2, 33, 12, 32, ("wgrad4", 1)), (3, 70, 64, 256, ("wgrad4", 53)), (5, 43, 63, 256, ("generic", 53)),
                  (1, 4100, 64, 256, ("wgrad4", 1024)), (1, 4166, 63, 256, ("generic", 1024))]
#: fused Cin = 1 backward (W = Cout = 64) around the 8-row strip minimum: (B, H)
C1_BWD_CASES = [(2, 1), (3, 7), (2, 8), (3, 9), (300, 9)]

#: epilogue entries, only what tests/test_gpu_kernels.py lacks: (B, H, W, Cin, Cout) of the dgrad conv Cin -> Cout
BNSUMS_CASES = [(3, 3, 8, 32, 68), (1, 1, 16, 32, 132), (3, 5, 64, 32, 68), (2, 3, 32, 96, 132),
                # the <BN, 0, TW, 1> instantiations the rows above leave out (the 256-cout tile serves W <= 16 here)
                (1, 2, 16, 32, 64), (1, 2, 8, 32, 128), (1, 2, 8, 32, 256), (1, 2, 16, 32, 256)]
#: (B, Hf, Wf, Cin, Cout, ph, pool): H = Hf // ph below one tile, odd Hf with ph = 2, W = Wf / 2 = 64 as two tile columns
POOLSUMS_CASES = [(3, 7, 16, 32, 68, 2, 0), (1, 3, 32, 32, 132, 1, 2), (2, 5, 128, 32, 68, 2, 3), (3, 9, 64, 96, 132, 2, 0),
                  # the <BN, 0, TW, 2> instantiations the rows above leave out
                  (1, 4, 32, 32, 64, 2, 0), (1, 2, 16, 32, 128, 1, 2), (1, 4, 16, 32, 256, 2, 3), (1, 2, 32, 32, 256, 1, 0)]
#: tag_conv3x3_forward_bnrelu_pool_eval: (B, H, W, Cin, Cout, ph, pro, pool)
POOLEVAL_CASES = [(3, 3, 8, 32, 68, 2, 1, 0), (1, 1, 16, 32, 132, 1, 0, 2), (2, 5, 64, 32, 68, 2, 1, 3), (3, 7, 32, 96, 132, 2, 0, 0),
                  (3, 3, 8, 32, 64, 2, 1, 3), (2, 5, 64, 32, 128, 2, 0, 2),      # these two: channel counts tag_bnact_pool_forward serves
                  # the <BN, PRO, TW, 3> instantiations the rows above leave out
                  (1, 2, 8, 32, 64, 1, 0, 0), (1, 2, 16, 32, 64, 1, 0, 2), (1, 2, 16, 32, 64, 2, 1, 3), (1, 2, 32, 32, 64, 1, 0, 0),
                  (1, 2, 8, 32, 128, 2, 0, 2), (1, 2, 8, 32, 128, 1, 1, 3), (1, 2, 16, 32, 128, 2, 1, 0), (1, 2, 32, 32, 128, 1, 1, 2)]


# ------------------------------------------------------------------------------------------------ instantiations
def selectable_instantiations():
    """every template instantiation a launcher of conv.hip can select with the default options (halo_bn256 = 1, conv_impl 0 | 1)"""
    halo = {(BN, pro, TW, 0) for BN in (64, 128, 256) for pro in range(4) for TW in (4, 8, 16, 32) if not (BN == 256 and TW == 32)}
    halo |= {(BN, 0, TW, e) for e in (1, 2) for BN in (64, 128, 256) for TW in (8, 16, 32) if not (BN == 256 and TW == 32)}
    halo |= {(BN, pro, TW, 3) for BN in (64, 128) for pro in (0, 1) for TW in (8, 16, 32)}
    halo |= {(128, pro, TW, 4) for pro in (2, 3) for TW in (4, 16)}
    return dict(halo=halo, tap_fwd={(BN, pro) for BN in (64, 128) for pro in range(4)},
                tap_wgrad={(TC, pro) for TC in (64, 128) for pro in range(4)},
                alltaps={(TW, pro) for TW in (4, 8) for pro in range(4)}, ring={(TW, pro) for TW in (16, 32, 64) for pro in range(4)})


def table_instantiations():
    """the instantiations the DEFAULT process of the sweep launches, derived from the tables with the formulas above"""
    halo, tap_fwd, tap_wgrad, alltaps, ring = set(), set(), set(), set(), set()
    for B, H, W, Cin, Cout, pro in [c[:6] for c in HALO_CASES] + HALO256_CASES + HALO_INST_CASES:
        for st in (False, True):
            g = halo_geom(H, W, Cout, stats_or_epi=st)
            halo.add((g["BN"], pro, g["TW"], 0))
    for B, H, W, Cin, Cout in BNSUMS_CASES:
        g = halo_geom(H, W, Cout, stats_or_epi=True)
        halo.add((g["BN"], 0, g["TW"], 1))
    for B, Hf, Wf, Cin, Cout, ph, pool in POOLSUMS_CASES:
        g = halo_geom(Hf // ph, Wf // 2, Cout, stats_or_epi=True)
        halo.add((g["BN"], 0, g["TW"], 2))
    for B, H, W, Cin, Cout, ph, pro, pool in POOLEVAL_CASES:
        g = halo_geom(H, W, Cout)
        halo.add((g["BN"], pro, g["TW"], 3))
    for B, H, W, Cin, pro in BIAS_CASES:
        halo.add((128, pro, W, 4))
    for c in TAP_FWD_CASES:
        tap_fwd.add((fwd_kernel(c[2], c[4])[1], c[5]))
    for c in TAP_WGRAD_CASES:
        tap_wgrad.add((wgrad_tile(c[3], c[4]), c[5]))
    for c in ALLTAPS_CASES:
        (ring if c[2] >= 16 else alltaps).add((c[2], c[5]))
    return dict(halo=halo, tap_fwd=tap_fwd, tap_wgrad=tap_wgrad, alltaps=alltaps, ring=ring)
