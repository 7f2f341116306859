"""fp64 numpy restatement of the device DBSCAN (csrc/dbscan.hip, utils/phrase_cluster.py) and an input builder that keeps every
pair outside THE GAP.

The formulation (equal LABELS to sklearn's DBSCAN(metric="precomputed") on (1 - cosine_similarity).clip(0), not merely the same
partition; tests/test_dbscan_cpu.py checks that):
  adj[i][j] = [u_i . u_j >= 1 - eps], u = x / max(||x||, 1e-12), the diagonal computed like any pair;  degree = row popcount;
  core = degree >= min_samples;  root[i] of a core row = the smallest index of its component of the core-core graph;  a row that
  is not core takes the smallest root among its core neighbours, or -1;  labels = the rank of the root among the distinct roots.
The components come from FastSV hooking on a parent array f (``fastsv``), pass for pass what tag_dbscan_hook does, so the pass
counts are comparable.

The gap.  The fp32 error of a cosine of unit rows at D <= 1024 is below 1.3e-4 (D * 2^-24 for the products and their sum, plus
the two normalisations).  A pair (i, j), i != j, is INSIDE THE GAP when |u_i . u_j - (1 - eps)| < GAP = 2.5e-4 (the GAP of
kmeans_ref); outside it every fp32 implementation puts the pair on the side fp64 does, so the tests demand equal bits.  The
diagonal is 1 (or 0 for an all-zero row) to within 1e-6 and every eps the tests use keeps 1 - eps away from both.
"""
import numpy as np

GAP = 2.5e-4
BIG = np.iinfo(np.int64).max


def unit_rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


def cosines(x):
    u = unit_rows(x)
    return u @ u.T


def adjacency(x, eps):
    """(N, N) bool."""
    return cosines(x) >= 1.0 - eps


def gap_pairs(x, eps):
    """(N, N) bool: the pairs i != j inside the gap."""
    bad = np.abs(cosines(x) - (1.0 - eps)) < GAP
    np.fill_diagonal(bad, False)
    return bad


def fastsv(n, src, dst, max_passes=10000):
    """FastSV hooking over the directed edge list (src[e], dst[e]) (both directions of every edge present, sorted by src or not)
    on n nodes: per pass, with gf = f[f] and m_i = min of gf[dst] over the edges leaving i,
        f'[f[i]] = min(f'[f[i]], m_i),   f'[i] = min(f'[i], m_i, gf[i])      (reading f, writing f'),
    until f' == f.  A node without an edge only takes gf[i].  -> (f, passes), the last pass (which changes nothing) counted."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.argsort(src, kind="stable")
    src, dst = src[order], dst[order]
    heads, starts = np.unique(src, return_index=True)       # the nodes with at least one edge and where their runs begin
    f = np.arange(n, dtype=np.int64)
    for passes in range(1, max_passes + 1):
        gf = f[f]
        new = np.minimum(f, gf)
        if heads.size:
            m = np.minimum.reduceat(gf[dst], starts)
            np.minimum.at(new, f[heads], m)
            new[heads] = np.minimum(new[heads], m)
        if np.array_equal(new, f):
            return f, passes
        f = new
    raise AssertionError("fastsv did not reach a fixed point")


def dbscan_ref(x=None, eps=0.5, min_samples=5, adj=None):
    """-> dict(labels int64 (N,), core_sample_indices int64, n_passes, adj bool (N, N), degree, root).  ``adj`` may be given
    in place of x."""
    if adj is None:
        adj = adjacency(x, eps)
    adj = np.asarray(adj, dtype=bool)
    n = adj.shape[0]
    degree = adj.sum(1)
    core = degree >= min_samples
    cc = adj & core[:, None] & core[None, :]
    src, dst = np.nonzero(cc)
    f, passes = fastsv(n, src, dst)
    # a row that is not core: the smallest f over its core neighbours
    cand = np.where(adj & core[None, :], f[None, :], BIG).min(1) if n else np.zeros(0, dtype=np.int64)
    root = np.where(core, f, np.where(cand == BIG, -1, cand))
    roots = np.unique(root[root >= 0])
    labels = np.where(root >= 0, np.searchsorted(roots, root), -1).astype(np.int64)
    return dict(labels=labels, core_sample_indices=np.flatnonzero(core).astype(np.int64), n_passes=passes, adj=adj,
                degree=degree.astype(np.int64), root=root)


def pack_bits(adj):
    """(N, N) bool -> (N, W) int32 as tag_dbscan_graph lays it out: W = 4 ceil(N / 128), bit j % 32 of word j // 32."""
    adj = np.asarray(adj, dtype=bool)
    n = adj.shape[0]
    W = 4 * ((n + 127) // 128)
    wide = np.zeros((n, 32 * W), dtype=np.uint8)
    wide[:, :n] = adj
    return np.packbits(wide, axis=1, bitorder="little").view(np.uint32).view(np.int32).reshape(n, W)


def unpack_bits(words):
    """(N, W) int32 -> (N, 32 W) bool."""
    words = np.ascontiguousarray(words, dtype=np.int32)
    return np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little").astype(bool)


def build_inputs(N, D, eps=0.5, seed=0, max_rounds=100):
    """fp32 x (N, D): 85 % blob rows on the sphere (unit(mean_k + 0.9 * unit noise), min(N / 24 + 2, 8) blobs of unequal sizes, so
    that dense clusters, thin ones, border rows and noise all occur at eps = 0.5) and 15 % unstructured rows (random directions),
    every row scaled by a random length in [0.5, 2).  The higher-indexed row of every pair inside the gap is re-drawn until no
    pair is left.  -> (x, rounds)."""
    g = np.random.RandomState(seed)
    K = min(N // 24 + 2, 8)
    means = unit_rows(g.randn(K, D))
    weights = g.rand(K) + 0.1
    weights /= weights.sum()

    def draw(n):
        rows = unit_rows(g.randn(n, D))
        blob = g.rand(n) < 0.85
        k = g.choice(K, size=n, p=weights)
        rows[blob] = unit_rows(means[k[blob]] + 0.9 * rows[blob])
        return (rows * g.uniform(0.5, 2.0, size=(n, 1))).astype(np.float32)

    x = draw(N)
    for rounds in range(max_rounds + 1):
        bad = np.flatnonzero(np.triu(gap_pairs(x, eps), 1).any(0))      # column j > row i: the higher index of the pair
        if not bad.size:
            return x, rounds
        assert rounds < max_rounds, "the gap builder did not converge"
        x[bad] = draw(bad.size)


def path_rows(N, perm=None):
    """The path graph as rows: x_i = e_i + e_{i+1} + e_{i+2} in D = N + 2 dimensions: consecutive rows have cosine 2/3, the next
    1/3, all others 0, so at eps = 0.5 row i is adjacent to i - 1, i and i + 1.  ``perm``: node i of the path is row perm[i]."""
    x = np.zeros((N, N + 2), dtype=np.float32)
    i = np.arange(N)
    for o in range(3):
        x[i, i + o] = 1.0
    if perm is not None:
        out = np.empty_like(x)
        out[np.asarray(perm)] = x
        x = out
    return x


def path_edges(N, perm=None):
    """The same graph as a directed edge list with the self loops, both directions."""
    i = np.arange(N - 1)
    src = np.concatenate([np.arange(N), i, i + 1])
    dst = np.concatenate([np.arange(N), i + 1, i])
    if perm is not None:
        perm = np.asarray(perm)
        src, dst = perm[src], perm[dst]
    return src, dst
