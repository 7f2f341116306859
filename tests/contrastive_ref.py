"""Plain torch statements of the sentence-level contrastive objectives, in the dtype and on the device of their input (fp64 on
the CPU = the reference of the tests; fp32 = the yardstick of their tolerance and of tools/contrastive_bench.py).  Gradients
come from autograd.  tests/test_contrastive_cpu.py pins every function to the imported reference (tests/golden/contrastive.npz).

x is the (n,n) clip-versus-caption matrix: x[i][j] = clip i against caption j, the diagonal holds the true pairs."""
import torch


def _diag(x):
    return torch.diagonal(x)


def _offdiag(x, fill):
    """x with its diagonal replaced by ``fill``."""
    n = x.shape[0]
    return x.masked_fill(torch.eye(n, dtype=torch.bool, device=x.device), fill)


def infonce(x, tau):
    """Each clip must pick its caption among the row, each caption its clip among the column: the mean of the two softmax
    cross-entropies of x / tau against the diagonal."""
    z = x / tau
    d = _diag(z)
    return 0.5 * ((torch.logsumexp(z, 1) - d).mean() + (torch.logsumexp(z, 0) - d).mean())


def max_triplet(x, margin):
    """Hinge of the hardest negative: per row the largest off-diagonal entry against the row's diagonal, per column the
    largest off-diagonal entry against the column's diagonal; the sum of both over n."""
    n = x.shape[0]
    if n == 1:
        return x.sum() * 0
    neg = _offdiag(x, float("-inf"))
    d = _diag(x)
    rows = torch.relu(margin + neg.max(1).values - d)
    cols = torch.relu(margin + neg.max(0).values - d)
    return (rows.sum() + cols.sum()) / n


def random_triplet(x, margin, s_index, a_index):
    """Hinge of one drawn negative per row i: x[i][s_i] against x[i][i], and x[i][a_i] against the diagonal of column a_i; a
    draw of the diagonal itself counts nothing."""
    n = x.shape[0]
    i = torch.arange(n, device=x.device)
    s, a = torch.as_tensor(s_index, device=x.device).long(), torch.as_tensor(a_index, device=x.device).long()
    d = _diag(x)
    ts = torch.relu(margin + x[i, s] - d) * (s != i)
    ta = torch.relu(margin + x[i, a] - d[a]) * (a != i)
    return (ts.sum() + ta.sum()) / n


def weighted_triplet(x, margin):
    """For every row of x and of its transpose: p the diagonal entry, q the largest of the others; when q + margin > p the row
    pays max(0.2 p^2 - 0.7 p + 0.5, 0) + max(0.9 q^2 - 0.4 q + 0.03, 0).  The sum over n; nothing at all when no row pays."""
    n = x.shape[0]
    if n == 1:
        return x.sum() * 0
    neg = _offdiag(x, float("-inf"))
    p = _diag(x)
    total = 0
    for q in (neg.max(1).values, neg.max(0).values):
        pays = torch.clamp(0.2 * p * p - 0.7 * p + 0.5, min=0) + torch.clamp(0.9 * q * q - 0.4 * q + 0.03, min=0)
        total = total + torch.where(q + margin > p, pays, torch.zeros_like(pays)).sum()
    return total / n


def milnce(c, label, tau):
    """Per clip, minus the log of the softmax mass (over its N phrases, at temperature tau) of the label-weighted scores:
    LSE_n(c / tau) - LSE_n(c * label / tau), averaged over the clips."""
    return (torch.logsumexp(c / tau, 1) - torch.logsumexp(c * label / tau, 1)).mean()


def loss_and_grad(fn, x, *args, upstream=1.0):
    """-> (loss, d (upstream * loss) / d x) as detached tensors."""
    xr = x.detach().clone().requires_grad_(True)
    loss = fn(xr, *args)
    (g,) = torch.autograd.grad(loss * upstream, xr, allow_unused=True)
    return loss.detach(), (torch.zeros_like(xr) if g is None else g)


def raised_diagonal_input(n, seed, dtype=torch.float64, cols=None):
    """Uniform [0,1) entries with the diagonal of every other row raised by 1.5: at margin 0.2 those rows and columns are
    inactive (plain uniform entries leave every row active, so the inactive branch would never run)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, n if cols is None else cols, generator=g, dtype=torch.float64)
    if cols is None:
        idx = torch.arange(0, n, 2)
        x[idx, idx] += 1.5
    return x.to(dtype)


# the roots of the two clamped polynomials of weighted_triplet: p = 1, 2.5; q = (0.4 -+ sqrt(0.052)) / 1.8
P_ROOTS = (1.0, 2.5)
Q_ROOTS = ((0.4 - 0.052 ** 0.5) / 1.8, (0.4 + 0.052 ** 0.5) / 1.8)


def triplet_precondition(x, margin, weighted=False, tie_gap=0.0, kink=1e-5):
    """True when x (fp64) is away from every point where the triplet objectives are not differentiable or where fp32 and fp64
    may decide differently: the two largest off-diagonal entries of every row and column differ (no exact tie), the activity
    m + x_top - x_diag is at least ``kink`` from 0, and (weighted) p and q are at least ``kink`` from the clamps' roots."""
    n = x.shape[0]
    if n == 1:
        return True
    neg = _offdiag(x.double(), float("-inf"))
    d = _diag(x.double())
    for m in (neg, neg.t()):
        top = torch.topk(m, min(2, n - 1), dim=1).values
        if n > 2 and bool(((top[:, 0] - top[:, 1]) <= tie_gap).any()):
            return False
        if bool(((margin + top[:, 0] - d).abs() < kink).any()):
            return False
        if weighted:
            for r in Q_ROOTS:
                if bool(((top[:, 0] - r).abs() < kink).any()):
                    return False
    if weighted:
        for r in P_ROOTS:
            if bool(((d - r).abs() < kink).any()):
                return False
    return True


def random_precondition(x, margin, s_index, a_index, kink=1e-5):
    n = x.shape[0]
    i = torch.arange(n)
    s, a = torch.as_tensor(s_index).long(), torch.as_tensor(a_index).long()
    d = _diag(x.double())
    hs = (margin + x.double()[i, s] - d)[s != i]
    ha = (margin + x.double()[i, a] - d[a])[a != i]
    return not bool((torch.cat([hs, ha]).abs() < kink).any())


def statement(kind, cfg, label=None, s_index=None, a_index=None):
    """The objective named like the cases of tests/golden/contrastive.npz as a function of its differentiable input alone."""
    if kind == "infonce":
        return lambda x: infonce(x, cfg)
    if kind == "max":
        return lambda x: max_triplet(x, cfg)
    if kind == "weighted":
        return lambda x: weighted_triplet(x, cfg)
    if kind == "random":
        return lambda x: random_triplet(x, cfg, s_index, a_index)
    if kind == "milnce":
        return lambda x: milnce(x, label.to(x), cfg)
    raise KeyError(kind)
