"""fp64 numpy reference of the device k-means (csrc/kmeans.hip, utils/phrase_cluster.py) and an input builder that keeps every
row's assignment outside THE GAP.

The gap.  The kernel scores a row against a centre as ||c||^2 - 2 x . c in fp32.  Such a score errs by at most about
D * 2^-24 * (||x||^2 + ||c||^2) and the difference of two scores by at most twice that, which for D <= 1024 is
1.2e-4 * (||x||^2 + max_k ||c_k||^2).  A row is INSIDE THE GAP when the margin between its best and its second-best fp64 score is
below GAP * (||x_i||^2 + max_k ||c_k||^2) with GAP = 2.5e-4; outside it every fp32 implementation picks the centre fp64 picks,
so the single-step tests demand exact equality of labels.  ``build_inputs`` re-draws rows inside the gap until none is left.
"""
import numpy as np

GAP = 2.5e-4


def scores64(x, c):
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)


def assign_ref(x, c):
    """-> (labels int32: argmin_k of the fp64 score, the lowest k on a tie; dist2 fp64: sum_d (x - c_label)^2; margin fp64: the
    second-best score minus the best, +inf for K = 1)."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    s = scores64(x, c)
    labels = s.argmin(1)
    dist2 = ((x - c[labels]) ** 2).sum(1)
    if c.shape[0] > 1:
        two = np.partition(s, 1, axis=1)[:, :2]
        margin = two[:, 1] - two[:, 0]
    else:
        margin = np.full(x.shape[0], np.inf)
    return labels.astype(np.int32), dist2, margin


def gap_width(x, c):
    """(N,) the margin below which a row counts as inside the gap."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return GAP * ((x * x).sum(1) + (c * c).sum(1).max())


def inside_gap(x, c):
    return assign_ref(x, c)[2] < gap_width(x, c)


def update_ref(x, labels, K):
    """-> (sums fp64 (K, D), count int64 (K,), abs_sums fp64 (K, D) = sum_{i in k} |x_id|, for the error bound)."""
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[1]
    sums, abs_sums = np.zeros((K, D)), np.zeros((K, D))
    np.add.at(sums, labels, x)
    np.add.at(abs_sums, labels, np.abs(x))
    count = np.bincount(labels, minlength=K).astype(np.int64)
    return sums, count, abs_sums


def lloyd_ref(x, init, max_iter=300, tol=1e-4):
    """Lloyd in fp64 with the stopping and relocation rules of utils/phrase_cluster.py (sklearn's): stop when the labels equal
    the previous iteration's, or when sum ||delta c||^2 <= tol * mean(var(x, axis 0)), then one more assignment; an empty
    cluster takes the row with the largest dist2 (largest first), which leaves its donor's sum and count before the division.
    -> dict(labels, centers, inertia, n_iter, strict, relocations, last_shift, tol_abs)."""
    x = np.asarray(x, dtype=np.float64)
    c = np.array(init, dtype=np.float64)
    K = c.shape[0]
    tol_abs = tol * x.var(axis=0).mean()
    prev = np.full(x.shape[0], -1, dtype=np.int32)
    strict, relocations, shift = False, 0, np.inf
    for it in range(max_iter):
        labels, dist2, _ = assign_ref(x, c)
        sums, count, _ = update_ref(x, labels, K)
        empty = np.flatnonzero(count == 0)
        if empty.size:
            far = np.argsort(-dist2, kind="stable")[:empty.size]
            for k, i in zip(empty, far):
                sums[labels[i]] -= x[i]
                count[labels[i]] -= 1
                sums[k] = x[i]
                count[k] = 1
                relocations += 1
        new = c.copy()
        new[count > 0] = sums[count > 0] / count[count > 0, None]
        shift = ((new - c) ** 2).sum()
        c = new
        n_iter = it + 1
        if np.array_equal(labels, prev):
            strict = True
            break
        if shift <= tol_abs:
            break
        prev = labels
    if not strict:
        labels, dist2, _ = assign_ref(x, c)
    dist2 = ((x - c[labels]) ** 2).sum(1)
    return dict(labels=labels, centers=c, inertia=float(dist2.sum()), n_iter=n_iter, strict=strict, relocations=relocations,
                last_shift=float(shift), tol_abs=float(tol_abs))


def kmeanspp_ref(x, K, first, uniforms):
    """Plain D^2 sampling in fp64, fed the uniforms the device path draws: pick 0 = ``first``; pick j = the first row whose prefix
    sum of closest reaches uniforms[j - 1] * total, clipped to N - 1.  -> (picks (K,), rel (K - 1,): how far, relative to the
    total, the drawn value lies from the nearest of the two prefix sums that decide the pick)."""
    x = np.asarray(x, dtype=np.float64)
    picks, rel = [int(first)], []
    closest = None
    for j in range(1, K):
        d = ((x - x[picks[-1]]) ** 2).sum(1)
        closest = d if closest is None else np.minimum(closest, d)
        cs = np.cumsum(closest)
        target = uniforms[j - 1] * cs[-1]
        p = min(int(np.searchsorted(cs, target)), x.shape[0] - 1)
        below = cs[p - 1] if p > 0 else -np.inf
        rel.append(min(cs[p] - target, target - below) / cs[-1])
        picks.append(p)
    return np.array(picks, dtype=np.int64), np.array(rel)


def build_inputs(N, K, D, seed=0, max_rounds=100):
    """fp32 x (N, D) and centres (K, D): centres from a normal distribution, every other row of x near a random centre (the
    centre plus unit noise), the rest normal: both terms of the score matter.  Rows inside the gap are re-drawn until none is
    left.  -> (x, centres, rounds)."""
    g = np.random.RandomState(seed)
    c = g.randn(K, D).astype(np.float32)

    def draw(n):
        rows = g.randn(n, D)
        near = np.arange(n) % 2 == 0
        rows[near] += c[g.randint(K, size=int(near.sum()))]
        return rows.astype(np.float32)

    x = draw(N)
    for rounds in range(max_rounds + 1):
        bad = inside_gap(x, c)
        if not bad.any():
            break
        assert rounds < max_rounds, "the gap builder did not converge"
        x[bad] = draw(int(bad.sum()))
    return x, c, rounds


def blobs(N, K, D, seed=0, noise=0.05):
    """Planted blobs: means randn(K, D), row i belongs to blob i % K and is its mean plus ``noise`` * randn.  -> (x fp32,
    planted labels, init fp32 = one point per blob (rows 0 .. K - 1))."""
    g = np.random.RandomState(seed)
    means = g.randn(K, D)
    planted = (np.arange(N) % K).astype(np.int32)
    x = (means[planted] + noise * g.randn(N, D)).astype(np.float32)
    return x, planted, x[:K].copy()
