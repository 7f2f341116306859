"""Statements, launcher formulas and case tables of tests/test_gpu_wino_sweep.py: the Winograd F(2x2, 3x3) convolutions of
csrc/conv_wino_fused.hip (one kernel per launch) and csrc/conv_wino.hip (plane form: input transform, 16 batched products, output
transform).  The convolution, BatchNorm and pool statements are those of tests/conv_ref.py and tests/conv_x3_ref.py; this module adds

* the OPERAND: ``conv_x3_ref.operand`` restates the fp32 prologue bit for bit, so every prologue case is the statement of a
  no-prologue case on that operand (tests/test_wino_ref_cpu.py asserts that no case has a double-rounding hazard);
* the fp32 FLOOR: oracle.tag_oracle.winograd_conv3x3 / winograd_conv3x3_wgrad in fp32 -- the same algorithm, stage by stage, on the CPU;
* ``pack_wino``: the float32 image of tag_pack_conv_weight_wino in both layouts, ``input_planes``: V = B^T d B with the kernels'
  expression order (what v_keep receives), ``block_counts`` / ``pivot_tiles``: what every partial statistics row must hold;
* the host formulas of the launchers (which form a launch takes, partial rows, slices, workspace bytes, the finish split);
* the case tables, each row with the CLAIMS it is there for (written out, not computed: the CPU test derives them again).

Layouts as in tests/conv_ref.py: activations (B, H, W, C), weights (Cout, Cin, 3, 3)."""
import functools
import math

import torch

from oracle import tag_oracle as O
from tests import conv_ref as R
from tests import conv_x3_ref as X

F64, F32 = torch.float64, torch.float32

# ------------------------------------------------------------------------------------------------ bounds (tests/test_gpu_wino.py)
FWD = 5e-6           # y, da, dx, pooled outputs (test_wino_forward_and_statistics, _dgrad_*, _forward_bnrelu_pool_eval)
SUMS = 5e-6          # the folded EPI 1 / EPI 2 sums, of the larger of the two (test_wino_dgrad_and_bn_backward_sums, _pool_backward_sums)
DW = 1e-5            # weight gradient (test_wino_wgrad)
STAT_MEAN = 2e-6     # folded mean, of max|mean| + max std (test_wino_forward_and_statistics)
STAT_INVSTD = 5e-6   # folded invstd, relative per channel
#: what the fp32 floor of a case may be at most (a quarter of the bound): tests/test_wino_ref_cpu.py
FWD_FLOOR_MAX, DW_FLOOR_MAX = FWD / 4, DW / 4

WINO_ITERS = 8       # tiles a slot of wino_output_kernel walks
FGM = 8              # tile blocks per workgroup-order group of wino_fused_kernel


def nchw(a):
    return a.permute(0, 3, 1, 2).contiguous()


def nhwc(a):
    return a.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ launcher formulas
def tiles(B, H, W):
    th, tw = (H + 1) // 2, (W + 1) // 2
    return th, tw, B * th * tw


def channels_ok(C):
    """wino_channels_ok: C / 4 threads per tile divide a 256-thread workgroup"""
    return 32 <= C <= 1024 and C % 4 == 0 and 256 % (C // 4) == 0


def wino_fused_ok(Cin, Cout):
    return Cin >= 8 and Cin % 8 == 0 and Cin <= 1024 and Cout >= 64 and Cout % 64 == 0


def wino_fused_wgrad_ok(Cin, Cout):
    return Cin >= 64 and Cin % 64 == 0 and Cout >= 64 and Cout % 64 == 0


def wg_rows_ok(Cin, Cout):
    return Cin % 128 == 0 and Cout % 128 == 0


def tag_conv3x3_wino_ok(B, H, W, Cin, Cout):
    fused = Cin % 64 == 0 and Cout % 64 == 0 and 64 <= Cin <= 1024 and 64 <= Cout <= 1024
    if not (B > 0 and H > 0 and W > 0 and (fused or (channels_ok(Cin) and channels_ok(Cout) and Cin % 32 == 0))):
        return 0
    T = tiles(B, H, W)[2]
    return int(T < (1 << 31) // 16 and B * H * W < (1 << 31) and B * H * W * max(Cin, Cout) < (1 << 29))


def wino_geom(B, H, W, Cout):
    """plane form: (T, G tile slots per workgroup, P partial rows)"""
    T = tiles(B, H, W)[2]
    G = 256 // (Cout // 4)
    per_wg = G * WINO_ITERS
    return T, G, (T + per_wg - 1) // per_wg * G


def wino_fused_rows(B, H, W):
    return (tiles(B, H, W)[2] + 63) // 64


def stats_rows(B, H, W, Cout):
    if wino_fused_ok(32, Cout):
        return wino_fused_rows(B, H, W)
    return wino_geom(B, H, W, Cout)[2] if channels_ok(Cout) else 0


def ws_bytes(B, H, W, Cin, Cout):
    if wino_fused_ok(Cin if Cin > 0 else 32, Cout):
        return 64
    return 16 * tiles(B, H, W)[2] * (Cin + Cout) * 4


def wg_geom(B, H, W, Cin, Cout):
    """fused weight gradient: (S slices of the tile axis, cps 8-tile chunks per slice)"""
    chunks = (tiles(B, H, W)[2] + 7) // 8
    S = max(1, 256 // ((Cin // 64) * (Cout // 64)))
    S = min(S, chunks)
    cps = (chunks + S - 1) // S
    return (chunks + cps - 1) // cps, cps


def wino_wg_geom(B, H, W, Cin, Cout):
    """plane-form weight gradient: (S K slices, kc rows per slice, Tpad = S kc)"""
    T = tiles(B, H, W)[2]
    t16 = ((Cin + 127) // 128) * ((Cout + 127) // 128) * 16
    S = (1024 + t16 - 1) // t16
    S = max(1, min(S, T // 512))
    kc = ((T + S - 1) // S + 15) // 16 * 16
    S = (T + kc - 1) // kc
    return S, kc, S * kc


def finish_q(Cin, Cout, S):
    """the run split of both finish kernels of the fused weight gradient"""
    n4 = Cin * Cout * 9 // 4
    return 1 if (n4 >= 131072 or S < 8) else (4 if (n4 >= 32768 or S < 32) else 16)


def wgrad_ws_bytes(B, H, W, Cin, Cout):
    if wino_fused_wgrad_ok(Cin, Cout):
        return 2 * wg_geom(B, H, W, Cin, Cout)[0] * Cin * Cout * 9 * 4
    S, kc, Tpad = wino_wg_geom(B, H, W, Cin, Cout)
    return (16 * Tpad * (Cin + Cout) + 16 * S * Cin * Cout) * 4


def can_reuse_v(B, H, W, Cin, Cout):
    if wino_fused_wgrad_ok(Cin, Cout):
        return 0
    return int(wino_wg_geom(B, H, W, Cin, Cout)[2] == tiles(B, H, W)[2])


def form(kind, Cin, Cout, pro=0, epi=0, S=None, v_keep=False, v_saved=False):
    """the kernels a launch takes.  kind "conv": forward / dgrad / the epilogue entries (epi 0..3); "wgrad": S = the slice count"""
    if kind == "conv":
        if wino_fused_ok(Cin, Cout):
            return (f"in<{pro}> + " if v_keep else "") + f"fused<{pro},{epi}>"
        return f"plane in<{pro}> + gemm + out<{epi}>"
    if wino_fused_wgrad_ok(Cin, Cout):
        q = finish_q(Cin, Cout, S)
        return f"rows<{pro}> + rows_finish<{q}>" if wg_rows_ok(Cin, Cout) else f"wgrad 64x64x16<{pro}> + finish<{q}>"
    return "plane dy + gemm + plane_finish" if v_saved else f"plane in<{pro}> + dy + gemm + plane_finish"


_KERNELS = {"in": "wino_input_kernel", "out": "wino_output_kernel", "fused": "wino_fused_kernel", "dy": "wino_dy_kernel",
            "plane_finish": "wino_wgrad_finish_kernel", "wgrad 64x64x16": "wino_fused_wgrad_kernel",
            "finish": "wino_fused_wgrad_finish_kernel", "rows": "wino_fused_wgrad_rows_kernel",
            "rows_finish": "wino_fused_wgrad_rows_finish_kernel", "pack": "wino_pack_kernel"}


def form_kernels(f):
    """the kernel instantiations of csrc/conv_wino.hip / conv_wino_fused.hip a form string names (the batched gemm is gemm.hip's)"""
    out = set()
    for part in f.replace("plane ", "").split(" + "):
        name, _, args = part.partition("<")
        if name == "gemm":
            continue
        out.add(_KERNELS[name] + ("<" + args.replace(",", ", ") if args else ""))
    return out


def selectable_instantiations():
    """every kernel instantiation of the two files that an entry point can launch"""
    s = {"wino_pack_kernel", "wino_dy_kernel", "wino_wgrad_finish_kernel"}
    for p in range(4):
        s |= {f"wino_input_kernel<{p}>", f"wino_output_kernel<{p}>", f"wino_fused_kernel<{p}, 0>", f"wino_fused_kernel<{p}, 3>",
              f"wino_fused_wgrad_kernel<{p}>", f"wino_fused_wgrad_rows_kernel<{p}>"}
    s |= {"wino_fused_kernel<0, 1>", "wino_fused_kernel<0, 2>"}                   # the gradient launches have no producer prologue
    s |= {f"wino_fused_wgrad_finish_kernel<{q}>" for q in (1, 4, 16)}
    s |= {f"wino_fused_wgrad_rows_finish_kernel<{q}>" for q in (1, 4)}            # Q = 16 needs n4 < 32768: not with 128 x 128 channels
    return s


# ------------------------------------------------------------------------------------------------ statements
def inputs(B, H, W, Cin, Cout, seed):
    """tests/conv_ref.py's inputs with a prologue shift of ORDER 1 (0.8 .. 1.2, both signs, nowhere zero): a kernel that applies the
    prologue to its padding turns every border zero into t (modes 2, 3) or relu(t) (mode 1) -- far above any bound"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g) + 0.5
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin) + 1.0 / (9 * Cin)
    dy = torch.randn(B, H, W, Cout, generator=g)
    s = torch.rand(Cin, generator=g) + 0.5
    t = (0.8 + 0.4 * torch.rand(Cin, generator=g)) * (1 - 2 * (torch.arange(Cin) % 2))
    return x, w, dy, s, t


def seed_of(B, H, W, Cin, Cout):
    return 1000 * B + 100 * H + 10 * W + Cin + 7 * Cout


def fwd(x, w, pro=0, s=None, t=None, dtype=F64):
    """y = conv(operand(x)): fp64 the direct sum of tests/conv_ref.py, fp32 the oracle's Winograd restatement (the floor)"""
    a = X.operand(x, pro, s, t)
    if dtype == F64:
        return R.conv_fwd(a, w, dtype=F64)
    return nhwc(O.winograd_conv3x3(nchw(a), w.float()))


def dgrad(dy, w, dtype=F64):
    """the gradient with respect to the convolution's input: the forward statement on the tap-flipped, channel-swapped filter"""
    return fwd(dy, w.flip(2, 3).transpose(0, 1).contiguous(), dtype=dtype)


def wgrad(x, dy, pro=0, s=None, t=None, dtype=F64):
    a = X.operand(x, pro, s, t)
    if dtype == F64:
        return R.conv_wgrad(a, dy, dtype=F64)
    return O.winograd_conv3x3_wgrad(nchw(a), nchw(dy.float()))


def hazards(x, pro, s, t):
    return X.operand_hazards(x, pro, s, t)


def _gg(g0, g1, g2):
    """one direction of G g G^T in fp32, the kernel's expression order: 0.5 is exact, the sums round as written"""
    return torch.stack([g0, 0.5 * ((g0 + g1) + g2), 0.5 * ((g0 - g1) + g2), g2])


def pack_wino(w, dgrad=False, tiled=False):
    """The float32 image of tag_pack_conv_weight_wino, flat (16 K N floats): U = G g G^T of the filter (K = Cin, N = Cout) or of the
    tap-flipped, channel-swapped filter (dgrad: K = Cout, N = Cin).  Plane layout [xi][K][N]; tiled (the fused kernel's LDS image per
    64-wide N block and 8-channel K chunk) index ((((n >> 6) (K / 8) + (k >> 3)) 16 + xi) 64 + (n & 63)) 8 + (k & 7)."""
    g = w.float()
    if dgrad:
        g = g.flip(2, 3).transpose(0, 1)
    g = g.contiguous()                                           # (N, K, 3, 3)
    p = _gg(g[:, :, 0, :], g[:, :, 1, :], g[:, :, 2, :])         # (4 r, N, K, 3 c)
    u = _gg(p[..., 0], p[..., 1], p[..., 2])                     # (4 s, 4 r, N, K)
    u = u.permute(1, 0, 2, 3)                                    # (r, s, N, K)
    N, K = g.shape[:2]
    if not tiled:
        return u.permute(0, 1, 3, 2).reshape(-1).contiguous()    # [xi = 4 r + s][K][N]
    return u.reshape(16, N // 64, 64, K // 8, 8).permute(1, 3, 0, 2, 4).reshape(-1).contiguous()


def input_planes(x, pro=0, s=None, t=None):
    """V [16][T][C] = B^T d B of the 4 x 4 window of every tile, fp32, wino_input_kernel's expression order
    (tt0 = d0 - d2, tt1 = d1 + d2, tt2 = d2 - d1, tt3 = d1 - d3 along rows, then the same along columns)"""
    a = X.operand(x, pro, s, t)
    B, H, W, C = a.shape
    th, tw, T = tiles(B, H, W)
    ap = torch.zeros(B, 2 * th + 2, 2 * tw + 2, C)
    ap[:, 1:H + 1, 1:W + 1] = a
    d = [[ap[:, r:r + 2 * th:2, c:c + 2 * tw:2] for c in range(4)] for r in range(4)]
    tt = [[d[0][c] - d[2][c] for c in range(4)], [d[1][c] + d[2][c] for c in range(4)],
          [d[2][c] - d[1][c] for c in range(4)], [d[1][c] - d[3][c] for c in range(4)]]
    V = [[tt[r][0] - tt[r][2], tt[r][1] + tt[r][2], tt[r][2] - tt[r][1], tt[r][1] - tt[r][3]] for r in range(4)]
    return torch.stack([V[r][c].reshape(T, C) for r in range(4) for c in range(4)])


def tile_pixels(B, H, W):
    """valid output pixels of every tile, in tile order t = (b, i, j)"""
    th, tw, T = tiles(B, H, W)
    hv = torch.tensor([min(2, H - 2 * i) for i in range(th)])
    wv = torch.tensor([min(2, W - 2 * j) for j in range(tw)])
    return (hv[:, None] * wv[None, :]).reshape(1, -1).repeat(B, 1).reshape(-1)


def row_tiles(B, H, W, Cout):
    """the tiles of every partial row: fused form 64 consecutive tiles per row; plane form row = workgroup G + slot walks
    tiles (workgroup 8 + it) G + slot"""
    T = tiles(B, H, W)[2]
    if wino_fused_ok(32, Cout):
        return [list(range(64 * m, min(T, 64 * m + 64))) for m in range(wino_fused_rows(B, H, W))]
    _, G, P = wino_geom(B, H, W, Cout)
    return [[t for t in ((row // G * WINO_ITERS + it) * G + row % G for it in range(WINO_ITERS)) if t < T] for row in range(P)]


def block_counts(B, H, W, Cout=64):
    """valid pixels of every partial row (per 64-tile block of the fused form, per slot row of the plane form)"""
    px = tile_pixels(B, H, W)
    return [int(px[r].sum()) if r else 0 for r in row_tiles(B, H, W, Cout)]


def pivot_pixels(B, H, W, Cout=64):
    """(b, h, w) of the output that is the pivot of every partial row: pixel (0, 0) of the row's first tile; None for an empty row"""
    th, tw, _ = tiles(B, H, W)
    return [((r[0] // tw // th, 2 * (r[0] // tw % th), 2 * (r[0] % tw)) if r else None) for r in row_tiles(B, H, W, Cout)]


def bn_tables(C, seed):
    g = torch.Generator().manual_seed(seed)
    gamma, beta = torch.rand(C, generator=g) + 0.5, 0.2 * torch.randn(C, generator=g)
    mean, var = 0.3 + 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    return gamma * invstd, beta - mean * gamma * invstd, mean, invstd


def epi_inputs(B, H, W, C, ph, hx=0, wx=0):
    """what the EPI 1 / EPI 2 sums read: yref (B, Hf, Wf, C) -- the image itself (ph = 0) or the unpooled tensor of the block below --
    and the BatchNorm tables (scale, shift, mean, invstd)"""
    Hf, Wf = (H, W) if ph == 0 else (ph * H + hx, 2 * W + wx)
    yref = torch.randn(B, Hf, Wf, C, generator=torch.Generator().manual_seed(Hf * 31 + Wf)) * 2 + 0.3
    return (yref, *bn_tables(C, H + W))


@functools.lru_cache(maxsize=None)
def fwd_case(B, H, W, Cin, Cout, pro):
    """(x, w, s, t, fp64 y, fp32 floor y): computed once, shared, left unchanged"""
    x, w, dy, s, t = inputs(B, H, W, Cin, Cout, seed_of(B, H, W, Cin, Cout))
    return x, w, s, t, fwd(x, w, pro, s, t), fwd(x, w, pro, s, t, F32)


@functools.lru_cache(maxsize=None)
def dgrad_case(B, H, W, K, C):
    """the data gradient of a convolution C -> K: (dy (B,H,W,K), w (K,C,3,3), fp64 da (B,H,W,C), fp32 floor)"""
    g = torch.Generator().manual_seed(seed_of(B, H, W, K, C) + 1)
    dy = torch.randn(B, H, W, K, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) / math.sqrt(9 * K)
    return dy, w, dgrad(dy, w), dgrad(dy, w, F32)


@functools.lru_cache(maxsize=None)
def wgrad_case(B, H, W, Cin, Cout, pro):
    x, w, dy, s, t = inputs(B, H, W, Cin, Cout, seed_of(B, H, W, Cin, Cout))
    return x, dy, s, t, wgrad(x, dy, pro, s, t), wgrad(x, dy, pro, s, t, F32)


# ------------------------------------------------------------------------------------------------ images
#: (B, H, W) -> (tiles T, 64-tile blocks, why it is there)
IMAGES = {
    (1, 1, 1): (1, 1, "63 empty slots; the convolution is the centre-tap matmul"),
    (1, 1, 8): (4, 1, "every tile hangs over the bottom edge"),
    (2, 3, 5): (12, 1, "odd both ways, tw = 3; images change inside a chunk"),
    (3, 9, 7): (60, 1, "kept from tests/test_gpu_wino.py"),
    (1, 16, 16): (64, 1, "exactly one block"),
    (5, 5, 10): (75, 2, "a full block and a ragged one; image boundaries at non-multiples of 8"),
    (3, 26, 32): (624, 10, "10 blocks: an FGM group of 8 and one of 2"),
    (257, 1, 2): (257, 5, "plane form only: one tile past a 256-tile workgroup"),
    (1, 6, 22): (33, 1, "plane form only: slot 0 walks two tiles, slots 1..31 one"),
    (11, 20, 20): (1100, 18, "plane-form wgrad only: S = 2, Tpad = 1120"),
    (8, 64, 8): (1024, 16, "plane wgrad, Tpad = T"),
    (1, 29, 29): (225, 4, "29 chunks, the last with one tile"),
    (2, 32, 32): (512, 8, "64 chunks"),
    (8, 32, 34): (2176, 34, "272 chunks"),
}
FUSED_IMAGES = [(1, 1, 1), (1, 1, 8), (2, 3, 5), (3, 9, 7), (1, 16, 16), (5, 5, 10), (3, 26, 32)]
#: plane-form partial rows at Cout = 32 (G = 32 slots, 256 tiles per workgroup): image -> P
PLANE_P = {(1, 1, 1): 32, (1, 1, 8): 32, (2, 3, 5): 32, (3, 9, 7): 32, (1, 6, 22): 32, (257, 1, 2): 64, (5, 5, 10): 32, (3, 26, 32): 96}

# ------------------------------------------------------------------------------------------------ FWD (EPI 0)
#: (B, H, W, Cin, Cout, pro, claim): claim = ("fused" | "plane", P partial rows, cout blocks)
FWD_CASES = ([(*im, Cin, 64, pro, ("fused", IMAGES[im][1], 1)) for im in FUSED_IMAGES for Cin in (64, 32) for pro in range(4)]
             + [(*im, Cin, Cout, pro, ("fused", IMAGES[im][1], Cout // 64))          # 3 cout blocks x a ragged group / grid not a multiple of 8
                for im in ((5, 5, 10), (3, 26, 32)) for Cin, Cout in ((64, 192), (192, 64)) for pro in (0, 1)]
             + [(*im, Cin, Cout, pro, ("fused", 1, Cout // 64))                       # the deepest K loop / the widest cout count
                for im in ((1, 1, 8), (2, 3, 5)) for Cin, Cout in ((1024, 64), (64, 1024)) for pro in (1, 3)]
             # plane form (Cout = 32): rows of empty slots, a second workgroup
             + [(1, 6, 22, 64, 32, 0, ("plane", 32, 0)), (1, 6, 22, 64, 32, 2, ("plane", 32, 0)), (257, 1, 2, 64, 32, 1, ("plane", 64, 0)),
                (257, 1, 2, 64, 32, 3, ("plane", 64, 0)), (3, 9, 7, 32, 32, 1, ("plane", 32, 0))])
#: the B = 3 images: rows 0..1 must be bit-equal to a B = 2 launch
BATCH_CASES = [(3, 9, 7, 64, 64, 2), (3, 26, 32, 32, 64, 3)]

# ------------------------------------------------------------------------------------------------ POOL (EPI 3)
POOL_KINDS = [(2, 0), (1, 0), (2, 2), (1, 3), (2, 3), (1, 2)]
POOL_IMAGES = [(2, 3, 5), (3, 9, 7), (5, 5, 10)]
#: (B, H, W, Cin, Cout, pro, ph, pool, form)
POOL_CASES = ([(*im, 64, 64, pro, ph, pool, "fused") for im in POOL_IMAGES for pro in range(4) for ph, pool in POOL_KINDS]
              + [(*im, Cin, Cout, 1, ph, pool, "fused") for im in POOL_IMAGES for Cin, Cout in ((32, 64), (64, 192)) for ph, pool in POOL_KINDS]
              + [(1, 6, 22, 64, 32, k % 4, ph, pool, "plane") for k, (ph, pool) in enumerate(POOL_KINDS)]
              + [(257, 1, 2, 64, 32, k + 1, 1, pool, "plane") for k, pool in enumerate((0, 3, 2))])      # H = 1: ph = 1 only

# ------------------------------------------------------------------------------------------------ GRAD (EPI 1 / EPI 2)
#: (B, H, W, K, C, ph, pool, p, hx, wx, form): the conventions of tests/wino_epilogue_cases.py -- dgrad image (B, H, W), K reduction
#: channels, C output channels; ph = 0 is EPI 1, ph = 1 / 2 EPI 2 with yref (B, ph H + hx, 2 W + wx, C).  hx = 1 needs ph = 2
#: (H == Hf / ph: with ph = 1 the floor leaves no row over).
GRAD_CASES = ([(*im, K, C, ph, 0, p, 1 if ph == 2 else 0, 1 if ph else 0, "fused")
               for im in ((5, 5, 10), (3, 26, 32)) for K, C in ((64, 192), (192, 64)) for ph, p in ((0, 0.0), (2, 0.2))]
              + [(*im, K, 64, ph, pool, (0.0, 0.2)[(ph + pool + K // 64) % 2], 1 if ph == 2 else 0, 1, "fused")
                 for im in ((3, 9, 7), (5, 5, 10)) for K in (64, 128) for ph in (1, 2) for pool in (2, 3)]
              + [(*im, 64, 32, 0, 0, 0.0, 0, 0, "plane") for im in ((1, 6, 22), (257, 1, 2), (3, 9, 7))]
              + [(*im, 64, 32, (1, 2, 2)[k], pool, (0.2, 0.0, 0.2)[k], (0, 1, 1)[k], 1, "plane")
                 for im in ((1, 6, 22), (257, 1, 2), (3, 9, 7)) for k, pool in enumerate((0, 2, 3))])
DROP_SEED = 4242

# ------------------------------------------------------------------------------------------------ WGRAD
#: (B, H, W, Cin, Cout, pro, claim).  claim: ("64x64x16", S, cps, Q) | ("rows", S, cps, Q) | ("plane", S, kc, Tpad)
_WG_CLAIMS = {
    # one chunk or two: S = chunks, cps = 1, Q = 1 (S < 8)
    **{(1, 1, 1, ci, co): ("64x64x16", 1, 1, 1) for ci, co in ((64, 64), (64, 128), (128, 64), (192, 192))},
    **{(2, 3, 5, ci, co): ("64x64x16", 2, 1, 1) for ci, co in ((64, 64), (64, 128), (128, 64), (192, 192), (192, 64))},
    (1, 1, 8, 64, 1024): ("64x64x16", 1, 1, 1), (1, 1, 8, 1024, 64): ("64x64x16", 1, 1, 1),
    # exactly 8 chunks, one per slice: the smallest S whose finish is split (Q = 4)
    **{(1, 16, 16, ci, co): ("64x64x16", 8, 1, 4) for ci, co in ((64, 64), (64, 128), (128, 64), (192, 192))},
    (1, 29, 29, 192, 192): ("64x64x16", 15, 2, 4),     # 29 chunks over 28 slices -> cps 2: the last slice ONE chunk, 7 of its 8 tiles beyond T
    (2, 32, 32, 192, 192): ("64x64x16", 22, 3, 4),     # cps 3: the odd tail of the two-stage loop; the last slice one chunk
    (8, 32, 34, 64, 64): ("64x64x16", 136, 2, 16),     # 272 chunks over 256 slices -> 136 x 2; the 16-run finish, 17 shares per run
    # tw = th = 1: the carry of advance() loops 8 times per chunk; 66 shares over 16 runs of ceil = 5:
    # thirteen full runs, one of a single share, two empty -- a run length taken as the floor (4) would drop two shares
    (257, 1, 2, 64, 64): ("64x64x16", 33, 1, 16),
    (2, 3, 5, 128, 128): ("rows", 2, 1, 1), (2, 3, 5, 256, 256): ("rows", 2, 1, 1),
    (1, 16, 16, 128, 128): ("rows", 8, 1, 4),          # (the only way to rows_finish<4> and rows<2>, <3>)
    **{(2, 3, 5, ci, co): ("plane", 1, 16, 16) for ci, co in ((32, 32), (32, 64), (64, 32), (1024, 32))},
    (11, 20, 20, 32, 32): ("plane", 2, 560, 1120), (11, 20, 20, 32, 64): ("plane", 2, 560, 1120),   # zero pad rows behind T = 1100
    (8, 64, 8, 32, 64): ("plane", 2, 512, 1024),       # Tpad = T: the forward's planes are the operand as they are
}


def _wg(im, ci, co, pros):
    return [(*im, ci, co, p, _WG_CLAIMS[(*im, ci, co)]) for p in pros]


WGRAD_CASES = (_wg((2, 3, 5), 64, 64, range(4)) + _wg((2, 3, 5), 192, 64, range(4))
               + [c for im in ((1, 1, 1), (2, 3, 5), (1, 16, 16)) for ci, co in ((64, 64), (64, 128), (128, 64), (192, 192))
                  if (im, ci, co) != ((2, 3, 5), 64, 64) for c in _wg(im, ci, co, (0, 1))]
               + _wg((1, 1, 8), 64, 1024, (0, 1)) + _wg((1, 1, 8), 1024, 64, (0, 1))
               + _wg((1, 29, 29), 192, 192, (0, 1)) + _wg((2, 32, 32), 192, 192, (0, 1)) + _wg((8, 32, 34), 64, 64, (0, 1))
               + _wg((257, 1, 2), 64, 64, (0, 1))
               + _wg((2, 3, 5), 128, 128, (0,)) + _wg((2, 3, 5), 256, 256, (1,)) + _wg((1, 16, 16), 128, 128, (2, 3))
               + [c for ci, co in ((32, 32), (32, 64), (64, 32), (1024, 32)) for c in _wg((2, 3, 5), ci, co, (0, 1))]
               + _wg((11, 20, 20), 32, 32, (0, 1)) + _wg((11, 20, 20), 32, 64, (0, 1)) + _wg((8, 64, 8), 32, 64, (0, 1)))

# ------------------------------------------------------------------------------------------------ KEEP / PACK
#: (B, H, W, Cin, Cout, pro, forward form, can_reuse_v)
KEEP_CASES = [(8, 64, 8, 32, 64, 1, "in<1> + fused<1,0>", 1), (2, 3, 5, 64, 64, 2, "in<2> + fused<2,0>", 0),
              (11, 20, 20, 32, 32, 3, "plane in<3> + gemm + out<0>", 0)]
#: (Cin, Cout, tiled_f, tiled_d)
PACK_CASES = [(32, 32, 0, 0), (64, 64, 1, 1), (32, 64, 1, 0), (64, 32, 0, 1), (192, 128, 1, 1)]


def table_instantiations():
    s = {"wino_pack_kernel"}
    for c in FWD_CASES:
        s |= form_kernels(form("conv", c[3], c[4], c[5], 0))
    for c in POOL_CASES:
        s |= form_kernels(form("conv", c[3], c[4], c[5], 3))
    for c in GRAD_CASES:
        s |= form_kernels(form("conv", c[3], c[4], 0, 1 if c[5] == 0 else 2))
    for c in WGRAD_CASES:
        S = wg_geom(*c[:5])[0] if wino_fused_wgrad_ok(c[3], c[4]) else None
        s |= form_kernels(form("wgrad", c[3], c[4], c[5], S=S))
    for c in KEEP_CASES:
        s |= form_kernels(form("conv", c[3], c[4], c[5], 0, v_keep=True))
    return s
