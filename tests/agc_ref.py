"""fp64 numpy restatement of the device average-linkage clustering (csrc/agc.hip, utils/phrase_cluster.AgglomerativeClustering), a
dense Lance-Williams average linkage to pin it against, and an input builder that keeps every row's nearest neighbour decided.

The formulation.  u = x / max(||x||, 1e-12).  A cluster A is its sum s_A = sum_{i in A} u_i and its size; m_A = s_A / |A|.  The
average of 1 - u_i . u_j over i in A, j in B is 1 - m_A . m_B, so
  nearest:  nn[a] = argmax_{b != a} m_a . m_b (ties to the lowest b),  dist[a] = 1 - m_a . m_nn[a];
  pairs:    a is the left half of a pair when nn[nn[a]] == a and a < nn[a];
  merge:    the survivors keep their relative order, the merged clusters follow in ascending a (sum and size added), node id
            next_id + rank, and the log gets (dist[a], id_a, id_b, new id);
  rounds until one cluster is left; the log is sorted by height (stably), nodes renumbered N + rank with children (min, max),
  and the tree is cut by sklearn's rule (``cut``).
Average linkage is reducible (d(A u B, C) >= min(d(A, C), d(B, C))), so merging all reciprocal pairs of a round gives the merges
of the serial algorithm (``lance_williams``), which tests/test_agc_cpu.py checks.

The error bound of a device distance, ``bound(D) = (D + 6) * 2^-24``.  The device computes 1 - sum_d a_d b_d in fp32 from fp32
means of norm <= 1.  With eps = 2^-24 (the unit roundoff of fp32): each of the D products and each of
the D additions of the running sum rounds once, and every partial sum is at most sum |a_d b_d| <= ||a|| ||b|| <= 1 in
magnitude, so the accumulated sum errs by at most D eps sum |a_d b_d| <= D eps to first order (the standard dot-product bound
gamma_D * |a| . |b|).  Rounding the two means to fp32 (one rounding each, relative eps, against the fp64 sums) moves the
product by at most 2 eps, the subtraction from 1 rounds once more (result <= 2: at most 2 eps), and the second-order terms fit
in the remaining 2 eps.  Against the fp64 value of the SAME fp32 means the mean roundings do not even enter.
"""
import heapq

import numpy as np

EPS32 = 2.0 ** -24


def bound(D):
    return (D + 6) * EPS32


def unit_rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


def nearest_ref(m):
    """m (M, D) -> (nn int64 (M,), dist fp64 (M,), gap fp64 (M,)): the fp64 nearest other row, its distance 1 - m_i . m_nn, and
    how far the second-best distance lies above the best (inf with fewer than three rows).  M = 1: nn = -1, dist = inf."""
    m = np.asarray(m, dtype=np.float64)
    M = m.shape[0]
    if M == 1:
        return np.full(1, -1, dtype=np.int64), np.full(1, np.inf), np.full(1, np.inf)
    d = 1.0 - m @ m.T
    np.fill_diagonal(d, np.inf)
    nn = d.argmin(1)                                # the first minimum: ties to the lowest index
    best = d[np.arange(M), nn]
    if M > 2:
        d[np.arange(M), nn] = np.inf
        gap = d.min(1) - best
    else:
        gap = np.full(M, np.inf)
    return nn.astype(np.int64), best, gap


def pair_roles(nn):
    """-> (left rows ascending, their partners, survivor rows ascending); an nn outside [0, M) pairs with nothing."""
    nn = np.asarray(nn, dtype=np.int64)
    M = nn.size
    a = np.arange(M)
    ok = (nn >= 0) & (nn < M) & (nn != a)
    back = np.where(ok, nn[np.clip(nn, 0, M - 1)], -1)
    mutual = ok & (back == a)
    left = a[mutual & (a < nn)]
    return left, nn[left], a[~mutual]


def merge_ref(nn, dist, sums, sizes, ids, next_id):
    """One round's bookkeeping -> dict(sums, sizes, ids, means (fp64 quotient rounded to fp32), log_dist, log_ids, pairs)."""
    left, right, keep = pair_roles(nn)
    sums, sizes, ids = np.asarray(sums, dtype=np.float64), np.asarray(sizes, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    new_ids = next_id + np.arange(left.size)
    out_sums = np.concatenate([sums[keep], sums[left] + sums[right]])
    out_sizes = np.concatenate([sizes[keep], sizes[left] + sizes[right]])
    return dict(sums=out_sums, sizes=out_sizes, ids=np.concatenate([ids[keep], new_ids]),
                means=(out_sums / out_sizes[:, None].astype(np.float64)).astype(np.float32),
                log_dist=np.asarray(dist)[left], log_ids=np.stack([ids[left], ids[right], new_ids], axis=1).reshape(-1, 3),
                pairs=int(left.size))


def rounds_ref(x):
    """The rounds in fp64 on the unit rows of x -> (heights (N - 1,), id_a, id_b, rounds): the merge log in the order written
    (row r made node N + r)."""
    u = unit_rows(x)
    N = u.shape[0]
    sums, sizes, ids = u.copy(), np.ones(N, dtype=np.int64), np.arange(N, dtype=np.int64)
    hs, las, lbs, rounds = [], [], [], 0
    while sums.shape[0] > 1:
        nn, dist, _ = nearest_ref(sums / sizes[:, None])
        r = merge_ref(nn, dist, sums, sizes, ids, N + len(hs))
        assert r["pairs"] >= 1, "a round merged nothing"
        sums, sizes, ids = r["sums"], r["sizes"], r["ids"]
        hs.extend(r["log_dist"].tolist())
        las.extend(r["log_ids"][:, 0].tolist())
        lbs.extend(r["log_ids"][:, 1].tolist())
        rounds += 1
    return np.array(hs, dtype=np.float64), np.array(las, dtype=np.int64), np.array(lbs, dtype=np.int64), rounds


def tree(heights, id_a, id_b, N):
    """Sort the log by height (stably) and renumber as scipy does -> (children (N - 1, 2) with (min, max), distances)."""
    order = np.argsort(heights, kind="stable")
    rank = np.empty(N - 1, dtype=np.int64)
    rank[order] = np.arange(N - 1)
    ren = lambda i: N + rank[i - N] if i >= N else i            # noqa: E731
    children = np.array([sorted((ren(int(id_a[r])), ren(int(id_b[r])))) for r in order], dtype=np.int64).reshape(N - 1, 2)
    return children, np.asarray(heights, dtype=np.float64)[order]


def cut(children, N, k):
    """sklearn's _hc_cut rule: a heap of negated node ids, k - 1 times the largest node gives way to its children; labels in the
    order of the heap's list."""
    labels = np.zeros(N, dtype=np.int64)
    if N == 1:
        return labels
    nodes = [-(2 * N - 2)]
    for _ in range(k - 1):
        c = children[-nodes[0] - N]
        heapq.heappush(nodes, -int(c[0]))
        heapq.heappushpop(nodes, -int(c[1]))

    for i, node in enumerate(nodes):
        todo, found = [-node], []
        while todo:                                 # (no recursion: a chain-shaped tree is N deep)
            n = todo.pop()
            if n < N:
                found.append(n)
            else:
                todo.extend(int(c) for c in children[n - N])
        labels[found] = i
    return labels


def agc_ref(x, ks):
    """-> dict(labels {k: (N,) int64}, children, distances, rounds, log=(heights, id_a, id_b))."""
    N = np.asarray(x).shape[0]
    h, a, b, rounds = rounds_ref(x)
    children, distances = tree(h, a, b, N)
    return dict(labels={int(k): cut(children, N, int(k)) for k in ks}, children=children, distances=distances, rounds=rounds,
                log=(h, a, b))


def lance_williams(dist):
    """Dense serial average linkage on a symmetric (N, N) fp64 distance matrix: merge the closest pair (the lowest (i, j) on a
    tie), d(A u B, C) = (|A| d(A, C) + |B| d(B, C)) / (|A| + |B|).  -> the sorted heights (N - 1,) and the list of leaf sets of
    every merge, in merge order.  O(N^3): for small N."""
    d = np.array(dist, dtype=np.float64)
    N = d.shape[0]
    np.fill_diagonal(d, np.inf)
    size = np.ones(N)
    members = {i: frozenset([i]) for i in range(N)}
    alive = np.ones(N, dtype=bool)
    heights, sets = [], []
    for _ in range(N - 1):
        sub = np.where(alive[:, None] & alive[None, :], d, np.inf)
        i, j = np.unravel_index(np.argmin(sub), sub.shape)
        heights.append(sub[i, j])
        new = (size[i] * d[i] + size[j] * d[j]) / (size[i] + size[j])
        d[i], d[:, i] = new, new
        d[i, i] = np.inf
        alive[j] = False
        size[i] += size[j]
        members[i] = members[i] | members[j]
        sets.append(members[i])
    return np.array(heights), sets


def merge_sets(children, N):
    """The leaf set of every merge of a tree, in node order."""
    sets = {i: frozenset([i]) for i in range(N)}
    out = []
    for r, (a, b) in enumerate(np.asarray(children).tolist()):
        sets[N + r] = sets[a] | sets[b]
        out.append(sets[N + r])
    return out


def build_inputs(N, D, seed=0, max_rounds=200):
    """fp32 rows (N, D) of norm in [0.3, 1] (cluster means are shorter than their rows): directions around min(N // 16 + 2, 8)
    planted means plus 20 % unstructured rows.  Rows whose best and second-best distance 1 - m_i . m_j differ by less than
    4 * bound(D) are re-drawn until none is left, so that every fp32 implementation within bound(D) picks the fp64 neighbour.
    -> (m, re-draws)."""
    g = np.random.RandomState(seed)
    K = min(N // 16 + 2, 8)
    means = unit_rows(g.randn(K, D))

    def draw(n):
        rows = unit_rows(g.randn(n, D))
        blob = g.rand(n) < 0.8
        k = g.randint(K, size=n)
        rows[blob] = unit_rows(means[k[blob]] + 0.7 * rows[blob])
        return (rows * g.uniform(0.3, 1.0, size=(n, 1))).astype(np.float32)

    m = draw(N)
    for rounds in range(max_rounds + 1):
        bad = np.flatnonzero(nearest_ref(m)[2] < 4.0 * bound(D))
        if not bad.size:
            return m, rounds
        assert rounds < max_rounds, "the gap builder did not converge"
        m[bad] = draw(bad.size)
