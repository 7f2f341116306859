"""Plain torch statements of the clip-level BCE objectives of weak phrase training, in the dtype of their input (fp64 on the
CPU = the reference of the tests; fp32 = the yardstick of their tolerance and of tools/clip_bce_bench.py), the analytic
per-element derivative that csrc/clip_bce.hip evaluates, and input builders.  tests/test_clip_bce_cpu.py pins every statement
to the imported reference (tests/golden/clip_bce.npz).

p is clip_sim (B,N), y the label (hard, or soft in [0,1]), aux the (B,N) weight (freq) or prior (prior).  The statements hold
the reference's expressions with the guards of binary_cross_entropy: logarithms clamped at -100, and the derivative
bce'(x,t) = (x - t) / max(x (1 - x), 1e-12).  The focal statement, which the reference writes with a raw log and is NaN / inf
at p = 0 and p = 1, takes its logarithms FROM binary_cross_entropy (ln p = -bce(p,1), ln(1-p) = -bce(p,0)), so that their
derivatives carry that guard, and its powers from ``guarded_pow`` (x^0 = 1 with a zero derivative; d x^g = g x^g / max(x, 1e-12))."""
import math

import numpy as np
import torch
import torch.nn.functional as F

GUARD = float(np.float32(1e-12))        # binary_cross_entropy guards its derivative with the fp32 constant; so do the kernels
KINDS = ("focal", "freq", "sym", "origin", "prior")
# kind -> the loss class of losses.py and the order of its constructor arguments in a config tuple
CLASSES = {"focal": ("FocalClipBceLoss", ("gamma", "alpha")), "freq": ("ClipBceLossFreqWeight", ("C", "gamma")),
           "sym": ("SymmetricClipBceLoss", ("eps",)), "origin": ("OriginSymmetricClipBceLoss", ("a", "b", "eps")),
           "prior": ("PriorAdjustedClipBceLoss", ("data_size", "tau"))}
# the configurations of the fixture; the GPU sweep runs two per kind
GOLDEN_CONFIGS = {"focal": ((2, 0.25), (1.5, 0.4)), "freq": ((100, 0.5),), "sym": ((1e-3,), (1e-2,)),
                  "origin": ((0.7, 1.3, 1e-3), (0.7, 1.3, 1e-2)), "prior": ((1000, 0.5), (1000, 1))}
SWEEP_CONFIGS = dict(GOLDEN_CONFIGS, freq=((100, 0.5), (30, 2.0)))
GOLDEN_SHAPES = ((1, 1), (5, 7), (3, 64))


def golden_group(B, N, soft):
    return f"{B}x{N}_{'soft' if soft else 'hard'}"


def golden_names():
    return [f"{kind}_{golden_group(B, N, soft)}_c{ci}" for (B, N) in GOLDEN_SHAPES for soft in (False, True) for kind in KINDS
            for ci in range(len(GOLDEN_CONFIGS[kind]))]


def load_golden(path):
    """tests/golden/clip_bce.npz -> {case name: {kind, cfg, p, label, counts, loss_f64, loss_f32, dp_f64, dp_f32}} (numpy);
    the file stacks the cases of one input in the order of its name list."""
    fx = np.load(path)
    cases, seen = {}, {}
    for name in (str(n) for n in fx["names"]):
        kind, rest = name.split("_", 1)
        group = rest.rsplit("_", 1)[0]
        i = seen.get(group, 0)
        seen[group] = i + 1
        case = {"kind": kind, "cfg": tuple(float(c) for c in fx[f"{group}/cfg"][i] if not np.isnan(c))}
        for k in ("p", "label", "counts"):
            case[k] = fx[f"{group}/{k}"]
        for k in ("loss_f64", "loss_f32", "dp_f64", "dp_f32"):
            case[k] = fx[f"{group}/{k}"][i]
        cases[name] = case
    return cases


def module_kwargs(kind, cfg):
    return dict(zip(CLASSES[kind][1], cfg))


class _GuardedPow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g):
        ctx.save_for_backward(x)
        ctx.g = g
        return torch.pow(x, g)                       # pow(0, 0) = 1

    @staticmethod
    def backward(ctx, d):
        (x,) = ctx.saved_tensors
        return d * ctx.g * torch.pow(x, ctx.g) / x.clamp_min(GUARD), None


def guarded_pow(x, g):
    return _GuardedPow.apply(x, g)


def clamped_log(p):
    """max(ln p, -100) with the derivative -bce'(p, 1)."""
    return -F.binary_cross_entropy(p, torch.ones_like(p), reduction="none")


def clamped_log1m(p):
    """max(ln(1 - p), -100) with the derivative -bce'(p, 0)."""
    return -F.binary_cross_entropy(p, torch.zeros_like(p), reduction="none")


def focal(p, y, gamma, alpha):
    loss = -alpha * guarded_pow(1 - p, gamma) * y * clamped_log(p) - (1 - alpha) * guarded_pow(p, gamma) * (1.0 - y) * clamped_log1m(p)
    return loss.mean()


def freq_weight(p, y, weight):
    return F.binary_cross_entropy(p, y, weight=torch.where(y == 0.0, torch.ones_like(weight), weight))


def symmetric(p, y, eps):
    return F.binary_cross_entropy(p, y) + F.binary_cross_entropy(y.clamp(eps, 1.0 - eps), p)


def origin_symmetric(p, y, a, b, A):
    reverse = -(y * (1 - p) * A + (1 - y) * A * p).mean()
    return a * F.binary_cross_entropy(p, y) + b * reverse


def prior_adjusted(p, y, prior, tau):
    one = p * prior ** tau
    zero = (1 - p) * (1 - prior) ** tau
    return F.binary_cross_entropy(one / (one + zero), y)


def aux_from_counts(kind, cfg, counts):
    """The host table the loss modules form from counts (B,N) with the reference's expression, fp64 numpy; None for the kinds
    that read none."""
    counts = np.asarray(counts, dtype=np.float64)
    if kind == "freq":
        C, gamma = cfg
        return (C / (C + counts)) ** gamma
    if kind == "prior":
        return counts / cfg[0]
    return None


def statement(kind, cfg, label, aux=None):
    """The objective as a function of clip_sim alone; label / aux are converted to clip_sim's dtype."""
    def to(t, p):
        return torch.as_tensor(t).to(p)
    if kind == "focal":
        return lambda p: focal(p, to(label, p), cfg[0], cfg[1])
    if kind == "freq":
        return lambda p: freq_weight(p, to(label, p), to(aux, p))
    if kind == "sym":
        return lambda p: symmetric(p, to(label, p), cfg[0])
    if kind == "origin":
        return lambda p: origin_symmetric(p, to(label, p), cfg[0], cfg[1], math.log(cfg[2]))
    if kind == "prior":
        return lambda p: prior_adjusted(p, to(label, p), to(aux, p), cfg[1])
    raise KeyError(kind)


def _log100(x):
    return torch.log(x).clamp_min(-100.0)


def _dbce(x, t):
    return (x - t) / (x * (1 - x)).clamp_min(GUARD)


def dterm(kind, cfg, p, y, aux=None):
    """d e_i / d p_i of include/tag_hip.h, written out (no autograd): d loss / d p = dterm / M."""
    if kind == "focal":
        g, al = cfg
        pw1, pw0 = torch.pow(1 - p, g), torch.pow(p, g)
        d_pw1, d_pw0 = -g * pw1 / (1 - p).clamp_min(GUARD), g * pw0 / p.clamp_min(GUARD)
        d_lp, d_lq = -_dbce(p, torch.ones_like(p)), -_dbce(p, torch.zeros_like(p))
        return -al * y * (d_pw1 * _log100(p) + pw1 * d_lp) - (1 - al) * (1 - y) * (d_pw0 * _log100(1 - p) + pw0 * d_lq)
    if kind == "freq":
        return torch.where(y == 0.0, torch.ones_like(aux), aux) * _dbce(p, y)
    if kind == "sym":
        yc = y.clamp(cfg[0], 1.0 - cfg[0])
        return _dbce(p, y) + _log100(1 - yc) - _log100(yc)
    if kind == "origin":
        a, b, eps = cfg
        return a * _dbce(p, y) - b * math.log(eps) * (1 - 2 * y)
    if kind == "prior":
        u, v = aux ** cfg[1], (1 - aux) ** cfg[1]
        s = p * u + (1 - p) * v
        return _dbce(p * u / s, y) * u * v / (s * s)
    raise KeyError(kind)


def loss_and_grad(fn, p, upstream=1.0):
    """-> (loss, d (upstream * loss) / d p) as detached tensors."""
    pr = p.detach().clone().requires_grad_(True)
    loss = fn(pr)
    (g,) = torch.autograd.grad(loss * upstream, pr)
    return loss.detach(), g


def make_inputs(B, N, seed, soft=False):
    """-> fp64 (p uniform in [0.01, 0.99], label, counts in [1, 499]).  Hard labels are 0/1 with 40% positives; soft labels keep
    the exact 0 of a third of the entries (the weight switch of ``freq`` reads label == 0), an exact 1 of some, and are uniform
    elsewhere, as max(label, teacher clip_sim) of the self-supervision runner leaves them."""
    g = torch.Generator().manual_seed(seed)
    p = 0.01 + 0.98 * torch.rand(B, N, generator=g, dtype=torch.float64)
    hard = (torch.rand(B, N, generator=g) < 0.4).double()
    if soft:
        u = torch.rand(B, N, generator=g, dtype=torch.float64)
        pick = torch.rand(B, N, generator=g)
        label = torch.where(pick < 0.33, torch.zeros_like(u), torch.where(pick > 0.85, torch.ones_like(u), torch.maximum(hard, u)))
    else:
        label = hard
    counts = torch.randint(1, 500, (B, N), generator=g).double()
    return p, label, counts


def end_point_inputs():
    """clip_sim with exact 0.0 and 1.0 under the labels 0, 1 and 0.3, beside interior values: (2,6) fp64 p, label, counts."""
    p = torch.tensor([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0], [0.25, 0.5, 0.75, 0.001, 0.999, 0.5]], dtype=torch.float64)
    label = torch.tensor([[0.0, 1.0, 0.3, 0.0, 1.0, 0.3], [0.0, 1.0, 0.3, 1.0, 0.0, 0.0]], dtype=torch.float64)
    counts = torch.tensor([[3.0, 40.0, 499.0, 1.0, 250.0, 17.0], [5.0, 60.0, 7.0, 300.0, 2.0, 90.0]], dtype=torch.float64)
    return p, label, counts
