"""The bidirectional GRU recurrence of csrc/gru.hip stated plainly at the kernels' own interface, in any dtype: the input projections
gi (B,T,2,3H) are given (the kernels never see x or W_ih), PyTorch gate order (r, z, n), h0 = 0, direction 0 runs t = 0 .. T-1 and
direction 1 runs t = T-1 .. 0.  ``gru_ref`` returns every tensor tag_gru_forward / tag_gru_backward write; the gradients come from
autograd.  In fp64 it is the reference of tests/test_gpu_gru_sweep.py, the same code in fp32 on the CPU is the floor every
comparison prints.  The case tables of the sweep live here, each row with the form, placement and tail it is meant to reach, because
tests/test_gru_ref_cpu.py checks on the CPU that every case is conditioned well enough for the bounds used on the GPU."""
import math

import torch

FWD, GRAD = 5e-6, 2e-5        # the bounds of test_gru_forward_backward (tests/test_gpu_kernels.py), max-normalised relerr
GATE_ABS = 3e-7               # |error| of the 4-row forward kernel's hardware gate functions, the kernel comment's own claim
# relative error of the same functions for |x| <= 20, from the formats and not from a measurement: the argument x log2(e) of
# v_exp_f32 is rounded to fp32 = |x| 2^-24 of e^x = 1.19e-6 at |x| = 20, plus one ulp each (1.19e-7) for v_exp_f32, the addition,
# v_rcp_f32 and the final subtraction of tanh = 1.67e-6; tanh above its series switch: GATE_ABS / tanh(0.2) = 1.52e-6; the series
# below it: 0.0219 x^8 = 5.6e-8 truncation plus four roundings
GATE_REL = 2e-6
STEP, P16, P4 = 1, 2, 3       # tag_gru_last_form
NAMES = ("y", "gates", "dgi", "dgh", "hprev")


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


def gru_ref(gi, w_hh, b_hh, dy=None, dtype=torch.float64):
    """gi (B,T,2,3H), w_hh (2,3H,H), b_hh (2,3H), dy (B,T,2H) or None -> dict of y (B,T,2H), gates (B,T,2,4H) = (r, z, n, gh_n),
    hprev (B,T,2,H) and, with dy, dgi and dgh (B,T,2,3H).  dgh is the gradient of a zero leaf added to gh = h W_hh^T + b_hh."""
    B, T, _, H3 = gi.shape
    H = H3 // 3
    gi = gi.detach().to(dtype, copy=True).requires_grad_(dy is not None)
    w, b = w_hh.detach().to(dtype), b_hh.detach().to(dtype)
    zero = torch.zeros(B, T, 2, H3, dtype=dtype, requires_grad=dy is not None)
    ys = [[None] * T, [None] * T]
    gs = [[None] * T, [None] * T]
    hp = [[None] * T, [None] * T]
    for d in range(2):
        h = torch.zeros(B, H, dtype=dtype)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            gh = h @ w[d].t() + b[d] + zero[:, t, d]
            x = gi[:, t, d]
            r = torch.sigmoid(x[:, :H] + gh[:, :H])
            z = torch.sigmoid(x[:, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(x[:, 2 * H:] + r * gh[:, 2 * H:])
            hp[d][t] = h
            h = (1 - z) * n + z * h
            ys[d][t] = h
            gs[d][t] = torch.cat([r, z, n, gh[:, 2 * H:]], -1)
    y = torch.stack([torch.stack(ys[0], 1), torch.stack(ys[1], 1)], 2)            # (B,T,2,H)
    out = {"y": y.reshape(B, T, 2 * H).detach(),
           "gates": torch.stack([torch.stack(gs[0], 1), torch.stack(gs[1], 1)], 2).detach(),
           "hprev": torch.stack([torch.stack(hp[0], 1), torch.stack(hp[1], 1)], 2).detach()}
    if dy is not None:
        y.reshape(B, T, 2 * H).backward(dy.to(dtype))
        out["dgi"], out["dgh"] = gi.grad, zero.grad
    return out


def gru_inputs(B, T, H, seed, sat=False):
    """gi, w_hh, b_hh, dy in fp32 on the CPU.  Recurrent weights as in test_gru_forward_backward (uniform in +-2/sqrt(H)); gi has
    the spread of x W_ih^T for x ~ N(0,1) at the encoders' widths.  sat: the z third of gi is spread over +-8 sigma so that a good
    share of the update gates lies within 1e-3 of 0 or 1."""
    g = torch.Generator().manual_seed(seed)
    k = 2.0 / math.sqrt(H)
    w_hh = (torch.rand(2, 3 * H, H, generator=g) * 2 - 1) * k
    b_hh = (torch.rand(2, 3 * H, generator=g) * 2 - 1) * k
    gi = torch.randn(B, T, 2, 3 * H, generator=g) * 1.5
    if sat:
        gi[..., H:2 * H] *= 8.0 / 1.5
    dy = torch.randn(B, T, 2 * H, generator=g)
    return gi, w_hh, b_hh, dy


def saturated_share(z):
    return ((z < 1e-3) | (z > 1 - 1e-3)).double().mean().item()


def p4_placement(B):
    """layout p4_decode takes for ceil(B/4) batch tiles x 2 directions, and the rows of the last tile"""
    nbt = (B + 3) // 4
    return ("remapped" if (2 * nbt) % 8 == 0 else "linear"), B - 4 * (nbt - 1)


# ------------------------------------------------------------------------------------------------------------ case tables
# (B, T, H, form a default process must report, what the row is meant to reach)
def _p4_rows():
    rows = []
    for H in (128, 256):
        for B in (1, 3, 4, 5, 13, 16, 17, 61, 64):
            lay, last = p4_placement(B)
            for T in (2, 3, 4):
                steps = {2: "one exchange", 3: "odd T: the unrolled loop ends on its first half", 4: "even T: on its second half"}[T]
                rows.append((B, T, H, P4, f"4-row <{H}>, {lay}, {(B + 3) // 4} tiles, last tile {last} rows, {steps}"))
    return rows


P4_CASES = _p4_rows()
LONG_CASE = (4, 251, 256, P4, "4-row <256>, linear, one full tile, the encoders' real step count: parity alternation, error growth")
STEP0_CASES = [(B, T, H, STEP, f"per-step <0>, H {H}: {H // 16} unit tiles, K slice {H // 4} per wave, "
                f"{(B + 15) // 16} batch tiles, last tile {B - 16 * ((B - 1) // 16)} rows, "
                + ("step 0 only" if T == 1 else f"{T - 1} steps with h_prev"))
               for H in (32, 64, 96, 288) for B in (1, 16, 17) for T in (1, 2, 5)]
# <128> / <256>: T = 1 never goes persistent; at T = 3 neither persistent grid can fit under ANY occupancy: at most 8 workgroups of
# 256 threads per CU, minus the launcher's margin of one, times 256 CUs = 1792 < 16-row grid (H/16) ceil(B/16) 2 = 1824 / 1808
STEPT_CASES = [(1, 1, 128, STEP, "per-step <128>, T = 1: step 0 only, one row"),
               (5, 1, 128, STEP, "per-step <128>, T = 1: step 0 only, 5 rows"),
               (1, 1, 256, STEP, "per-step <256>, T = 1: step 0 only, one row"),
               (5, 1, 256, STEP, "per-step <256>, T = 1: step 0 only, 5 rows"),
               (1800, 3, 128, STEP, "per-step <128>, step > 0: 16-row grid 8 x 113 x 2 = 1808 > 1792, last tile 8 rows"),
               (900, 3, 256, STEP, "per-step <256>, step > 0: 16-row grid 16 x 57 x 2 = 1824 > 1792, last tile 4 rows")]
# the cases of the child process started with TAG_GRU_TILE=16 (form 2 there; a default process runs them on the 4-row form)
P16_CASES = [(B, T, H, P16, f"16-row <{H}>, {(B + 15) // 16} batch tiles, last tile {B - 16 * ((B - 1) // 16)} rows")
             for H in (128, 256) for B in (1, 15, 16, 17, 33) for T in (2, 3, 4)]
# the cases of the child process started with TAG_GRU_XCD=0: remapped placement, write-through publishing
XCD_CASES = [(B, 5, H, P4, f"4-row <{H}>, remapped, last tile {p4_placement(B)[1]} rows") for H in (128, 256) for B in (13, 16, 64)]
# one saturated case per form (z within 1e-3 of 0 or 1 on a good share of the elements)
SAT_CASES = {"p4": (13, 4, 256, P4, "4-row <256>, remapped, last tile 1 row"),
             "p16": (17, 4, 128, P16, "16-row <128>, two tiles, last tile 1 row"),
             "step": (17, 5, 96, STEP, "per-step <0>, two tiles, last tile 1 row")}
# forward accepts H % 16 == 0, backward also needs (3H) % 32 == 0: these run forward only
FWD_ONLY_CASES = [(17, 3, 16, STEP, "per-step <0>, H 16: K slice 4 = one MFMA per wave"),
                  (5, 3, 48, STEP, "per-step <0>, H 48: K slice 12")]
# where the launcher's choice depends on the occupancy the runtime reports: H = 256, 4-row grid 16 ceil(B/4), 16-row grid 32 ceil(B/16)
LADDER_B = (65, 128, 129, 192, 193, 256, 257, 384, 385, 448, 449, 896)

SEEDS = {}                    # (B, T, H, sat) -> seed, for a case whose default draw is not conditioned well enough


def case_inputs(B, T, H, sat=False):
    return gru_inputs(B, T, H, SEEDS.get((B, T, H, sat), 7000 + 131 * B + 17 * T + H + (5 if sat else 0)), sat)


def all_cases():
    """every (B, T, H, sat) the sweep compares with fp64"""
    seen = []
    for tab in (P4_CASES, [LONG_CASE], STEP0_CASES, STEPT_CASES, P16_CASES, XCD_CASES, FWD_ONLY_CASES):
        seen += [(B, T, H, False) for B, T, H, _, _ in tab]
    seen += [(B, T, H, True) for B, T, H, _, _ in SAT_CASES.values()]
    seen += [(B, 2, 256, False) for B in LADDER_B]
    return sorted(set(seen))


# ------------------------------------------------------------------------------------------------------------ gate sample points
def gate_points():
    """0, +-denormals, +-1e-6 .. +-20 log-spaced, the 64 floats on either side of +-0.2 (the tanh series switch), the overflow range
    of e^x and e^2x, +-inf; fp32"""
    f = torch.float32
    pos = [torch.tensor([1e-45, 1e-40, 1.1754942e-38], dtype=f),
           torch.logspace(-6, math.log10(20.0), 193, dtype=torch.float64).to(f)]
    x = torch.tensor([0.2], dtype=f)
    lo, hi = [x.clone()], []
    a, b = x.clone(), x.clone()
    for _ in range(64):
        a = torch.nextafter(a, torch.tensor([0.0], dtype=f))
        b = torch.nextafter(b, torch.tensor([1.0], dtype=f))
        lo.append(a.clone())
        hi.append(b.clone())
    pos += lo + hi
    pos.append(torch.tensor([44.0, 87.0, 88.8, 100.0, 1e4, float("inf")], dtype=f))
    p = torch.cat(pos)
    return torch.cat([torch.zeros(1, dtype=f), p, -p])


def gate_case(B, T, H):
    """gi (B,T,2,3H) whose three gate thirds hold the sample points (repeated to fill), and zero recurrent weights: the saved gates
    are then sigmoid(gi_r), sigmoid(gi_z), tanh(gi_n) of the inputs exactly (gh = 0, r * 0 = 0 for every r in [0, 1])."""
    pts = gate_points()
    n = B * T * 2 * H
    assert pts.numel() <= n
    col = pts.repeat((n + pts.numel() - 1) // pts.numel())[:n].view(B, T, 2, H)
    gi = torch.cat([col, col, col], -1).contiguous()
    return gi, torch.zeros(2, 3 * H, H), torch.zeros(2, 3 * H), col
