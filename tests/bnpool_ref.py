"""CPU helpers of the csrc/bn_pool.hip sweep (tests/test_gpu_bnpool_sweep.py) that are themselves under test
(tests/test_bnpool_ref_cpu.py): the written-out references where torch defines none (BatchNorm over one row, the LPPool gradient
of an all-zero window, the frame head's gated gradient), the synthesiser of the partial statistics rows a conv epilogue writes
with the fp64 Chan merge that must undo it, the repair that moves random inputs away from ReLU and arg-max decisions, and the
bf16 comparison rule.  Everything is plain torch on the CPU; layouts are the kernels' (channels-last) unless a name says nchw."""
import torch
import torch.nn.functional as F

EPS = 1e-5
MARGIN = 1e-4          # decisions closer than MARGIN * max|a| are repaired away (fp32 resolves 6e-8 of the operands)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def bf16r(t):
    """round to bf16-representable values, kept in the tensor's own dtype"""
    return t.bfloat16().to(t.dtype)


# ------------------------------------------------------------------------------------------------ BatchNorm, written out
def bn_moments(v):
    """(mean, biased var, the variance running_var takes) of v (rows, C) over its rows, in v's dtype.  One row: var 0 and the
    biased value for running_var (the kernels' rows > 1 guard); torch refuses that case."""
    n = v.shape[0]
    m = v.mean(0)
    var = ((v - m) ** 2).mean(0)
    return m, var, (var * n / (n - 1) if n > 1 else var)


def bn_train(v, gamma, beta, eps=EPS):
    """training-mode BatchNorm of v (rows, C), written out with differentiable torch ops (defined at rows == 1 too)"""
    m, var, _ = bn_moments(v)
    out = (v - m) / torch.sqrt(var + eps)
    if gamma is not None:
        out = out * gamma
    return out + beta if beta is not None else out


def bn_eval(v, mean, invstd, gamma, beta):
    """eval-mode BatchNorm with the statistics given as (mean, invstd): (v - mean) * invstd * gamma + beta"""
    return (v - mean) * invstd * gamma + beta


def stats_outputs(v, gamma, beta, rm, rv, eps=EPS, momentum=0.1, moments=None):
    """what tag_bn_stats writes, in v's dtype: mean, invstd, scale, shift, running_mean, running_var (None without buffers).
    moments: (mean, biased var) to use instead of v's own two-pass moments"""
    m, var, unb = bn_moments(v)
    if moments is not None:
        m, var = moments
        unb = var * v.shape[0] / (v.shape[0] - 1) if v.shape[0] > 1 else var
    invstd = 1.0 / torch.sqrt(var + eps)
    g = gamma if gamma is not None else torch.ones_like(m)
    b = beta if beta is not None else torch.zeros_like(m)
    out = dict(mean=m, invstd=invstd, scale=g * invstd, shift=b - m * g * invstd)
    out["rm"] = None if rm is None else (1 - momentum) * rm + momentum * m
    out["rv"] = None if rv is None else (1 - momentum) * rv + momentum * unb
    return out


def stats_one_pass_fp32_squares(v32, eps=EPS):
    """The kernels' documented one-pass form on the CPU: fp32 values and fp32 SQUARES, summed in fp64, var = E[v^2] - E[v]^2
    (one row: var 0).  Its distance from the two-pass fp64 moments is the floor of the offset-mean statistics cases."""
    n = v32.shape[0]
    s1 = v32.double().sum(0)
    s2 = (v32 * v32).double().sum(0)
    m = s1 / n
    var = (s2 / n - m * m).clamp_min(0) if n > 1 else torch.zeros_like(m)
    return m, var, 1.0 / torch.sqrt(var + eps)


# ------------------------------------------------------------------------------------------------ partial statistics rows
def tile_counts(P, seed, big_every=0):
    """P tile counts in 0 .. 64: row 0 is never empty; about one row in seven past it is EMPTY (count 0).  big_every > 0: counts
    of 1 .. 4 with a 64 every big_every rows, so that P = 16385 needs no tensor of half a million rows."""
    g = torch.Generator().manual_seed(seed)
    if big_every:
        cnt = torch.randint(1, 5, (P,), generator=g)
        cnt[::big_every] = 64
    else:
        cnt = torch.randint(1, 65, (P,), generator=g)
    empty = torch.rand(P, generator=g) < 1.0 / 7
    empty[0] = False
    cnt[empty] = 0
    if P > 1:
        cnt[1] = 1          # a one-pixel tile: r = q = 0
    return cnt


def synth_partials(x, cnt, seed=0):
    """The rows a conv epilogue writes for x (N, C) fp32 cut into consecutive tiles of cnt[p] rows (sum cnt == N): float32
    (P * 3 * C + P,) = P rows [pivot | sum(y - pivot) | sum((y - pivot)^2)] then the P counts.  The pivot is the tile mean ROUNDED
    TO fp32, the two sums are taken about that rounded pivot (fp64 here, stored as fp32).  Empty rows hold finite garbage."""
    N, C = x.shape
    P = cnt.numel()
    assert int(cnt.sum()) == N and int(cnt[0]) > 0
    tid = torch.repeat_interleave(torch.arange(P), cnt)
    xd = x.double()
    n = cnt.double().clamp_min(1).unsqueeze(1)
    mu = (torch.zeros(P, C, dtype=torch.float64).index_add_(0, tid, xd) / n).float()
    d = xd - mu.double()[tid]
    r = torch.zeros(P, C, dtype=torch.float64).index_add_(0, tid, d)
    q = torch.zeros(P, C, dtype=torch.float64).index_add_(0, tid, d * d)
    rows = torch.stack([mu, r.float(), q.float()], 1)                      # (P, 3, C)
    empty = cnt == 0
    if empty.any():
        g = torch.Generator().manual_seed(seed + 1)
        rows[empty] = 1e3 * torch.randn(int(empty.sum()), 3, C, generator=g)
    return torch.cat([rows.reshape(-1), cnt.float()])


def chan_merge(flat, P, C):
    """fp64 merge (Chan et al.) of synth_partials' rows about the pivot of row 0 -> (mean, biased var, N); empty rows skipped"""
    rows = flat[:P * 3 * C].double().view(P, 3, C)
    n = flat[P * 3 * C:].double()
    live = n > 0
    mu, r, q, n = rows[live, 0], rows[live, 1], rows[live, 2], n[live].unsqueeze(1)
    K = rows[0, 0]
    s = n * (mu - K) + r                              # tile sums about K
    m2 = q - r * r / n                                # tile M2
    Ntot = n.sum()
    S = s.sum(0)
    var = (m2.sum(0) + (s * s / n).sum(0) - S * S / Ntot) / Ntot
    return K + S / Ntot, var, int(Ntot)


# ------------------------------------------------------------------------------------------------ pooling, written out
def windows(a, ph, pw):
    """a (B, C, H, W) -> (B, C, Ho, Wo, ph * pw): the full windows in scan order (h then w); floor-dropped rows / columns left out"""
    B, C, H, W = a.shape
    Ho, Wo = H // ph, W // pw
    return a[:, :, :Ho * ph, :Wo * pw].reshape(B, C, Ho, ph, Wo, pw).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, ph * pw)


def pool_ref(a, ph, pw, pool):
    """pool 0 avg+max | 1 LPPool(4) | 2 avg | 3 max of a (B, C, H, W) with torch's own functions"""
    if pool == 0:
        return F.avg_pool2d(a, (ph, pw)) + F.max_pool2d(a, (ph, pw))
    if pool == 1:
        return F.lp_pool2d(a, 4.0, (ph, pw))
    return F.avg_pool2d(a, (ph, pw)) if pool == 2 else F.max_pool2d(a, (ph, pw))


def lppool_leaky_backward_ref(y, dout, ph, pw):
    """Gradient of LPPool4(leaky_relu(y, 0.1)) written out: dy = dout * a^3 / out^3 * leaky'(y) in every full window, DEFINED AS
    ZERO where out == 0 (torch's autograd gives NaN or zero there, by version) and in floor-dropped rows / columns.  y (B, C, H, W),
    dout (B, C, H // ph, W // pw)."""
    Ho, Wo = dout.shape[2:]
    a = torch.where(y > 0, y, 0.1 * y)
    out = windows(a, ph, pw).pow(4).sum(-1).pow(0.25)
    k = torch.where(out > 0, dout / out.clamp_min(1e-300) ** 3, torch.zeros_like(out))
    k = k.repeat_interleave(ph, 2).repeat_interleave(pw, 3)
    dy = torch.zeros_like(y)
    dy[:, :, :Ho * ph, :Wo * pw] = (k * a[:, :, :Ho * ph, :Wo * pw] ** 3
                                    * torch.where(y[:, :, :Ho * ph, :Wo * pw] > 0, 1.0, 0.1))
    return dy


def frame_head_backward_ref(y, rb, w, sig, dprob):
    """Gradient of prob = clamp(sigmoid((y + rb[b]) . w + b0), 1e-7, 1) given sig (B, T) as stored: dlogit = dprob sig (1 - sig)
    where float32(1e-7) <= sig <= 1 (torch's clamp gradient), else 0.  y (B, T, N), rb (B, N), w (N).  Returns dy, dw, db0,
    drb and the per-clip sums clip (B, 2, N) = [sum_t dlogit (y + rb) | sum_t dlogit]."""
    lo = float(torch.tensor(1e-7, dtype=torch.float32))
    dl = torch.where((sig >= lo) & (sig <= 1.0), dprob * sig * (1.0 - sig), torch.zeros_like(sig))      # (B, T)
    dy = dl.unsqueeze(-1) * w
    s0 = (dl.unsqueeze(-1) * (y + rb.unsqueeze(1))).sum(1)                                              # (B, N)
    s1 = dl.sum(1, keepdim=True).expand(-1, y.shape[2])
    return dy, s0.sum(0), dl.sum(), s1 * w, torch.stack([s0, s1], 1)


# ------------------------------------------------------------------------------------------------ input repair
def decision_violations(a, ph=0, pw=0):
    """a (B, C, H, W) pre-activations -> (near_zero, runner_up): boolean masks of the elements within MARGIN * max|a| of zero, and
    (ph > 0) of the elements of a full window that are not its first maximum yet lie within that margin of a POSITIVE maximum"""
    thr = MARGIN * a.abs().max()
    near = a.abs() < thr
    run = torch.zeros_like(near)
    if ph:
        B, C, H, W = a.shape
        Ho, Wo = H // ph, W // pw
        w = windows(a, ph, pw)
        mx, arg = w.max(-1, keepdim=True)
        first = torch.zeros_like(w, dtype=torch.bool).scatter_(-1, arg, True)
        # torch.max returns SOME maximal index; an exact tie leaves its twin flagged, which is what a violation is
        bad = (~first) & (w >= mx - thr) & (mx > 0)
        run[:, :, :Ho * ph, :Wo * pw] = bad.reshape(B, C, Ho, Wo, ph, pw).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho * ph, Wo * pw)
    return near, run


def repair(y, affine, ph=0, pw=0, bf16=False):
    """Move the elements of y (B, C, H, W) whose pre-activation a = affine(y) sits at a decision: |a| within MARGIN * max|a| of
    zero (pushed out to +-3 margins and beyond), runner-up maxima within the margin of their window's maximum (pushed down).
    affine(y) -> (a, da/dy per channel broadcastable) is re-evaluated after every pass (batch statistics move with y);
    bf16: y stays bf16-representable.  Returns the repaired y; decision_violations(affine(y)[0]) is empty afterwards."""
    y = y.clone()
    for it in range(40):
        a, slope = affine(y)
        near, run = decision_violations(a, ph, pw)
        if not near.any() and not run.any():
            return y
        thr = MARGIN * a.abs().max()
        step = thr * 3.0 * 1.6 ** it
        sgn = torch.where(a >= 0, 1.0, -1.0).to(a.dtype)
        target = torch.where(near, sgn * step, a)
        target = torch.where(run & ~near, a - step, target)
        # a runner-up pushed down may land beside zero: the next pass sees it
        y = torch.where(near | run, y + (target - a) / slope, y)
        if bf16:
            y = bf16r(y)
    raise AssertionError("repair did not converge")


# ------------------------------------------------------------------------------------------------ bf16 comparison
def bf16_ulp(v):
    """the spacing of bf16 values in the binade of |v| (8 significant bits); the smallest normal binade below 2^-126"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def bf16_bounds(ref, delta_rel=4e-6):
    """Per-element bounds for a bf16 result against its fp64 reference ``ref``: (one, half, safe).  one = 1 ulp; half = 1.01
    half-ulps, asserted where ``safe``: the reference lies farther than delta = delta_rel * max|ref| from the nearest bf16 rounding
    boundary (the midpoint between two neighbours), so an fp32 value within delta of it rounds the same way.  Both are computed
    from the reference alone.  The fp32 value that is rounded is itself only known to delta (sums that cancel), so both bounds are
    floored at half an ulp + delta.  That floor is the wider of the two for ``half`` wherever ulp < 200 delta (|v| below about 0.1
    max|ref| at delta_rel 4e-6) and for ``one`` wherever ulp < 2 delta (|v| below 2^8 delta); on the safe set it still refuses the
    wrong neighbour, which lies more than half an ulp + delta away.  A large delta_rel (the floor-rule cases hand in up to 6.5e-3)
    leaves little of either bound."""
    ref = ref.double()
    delta = delta_rel * ref.abs().max()
    ulp = bf16_ulp(ref)
    lo = torch.floor(ref / ulp) * ulp
    safe = (ref - (lo + ulp / 2)).abs() > delta
    floor = ulp / 2 + delta
    return torch.maximum(ulp, floor), torch.maximum(1.01 * ulp / 2, floor), safe

