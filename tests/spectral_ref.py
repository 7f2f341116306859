"""The matrix-free spectral embedding of utils/phrase_cluster.SpectralClustering restated in numpy, in fp64 or in emulated fp32
(every N-tall array is stored in ``dtype``; the small Gram matrices and the Rayleigh-Ritz solve are fp64, as on the device), and
the bounds the GPU tests hold the three kernels of csrc/spectral.hip to.

The operator (sklearn's, not an approximation): u = x / max(||x||, 1e-12), W = [u | 1], A = W W^T / 2.  scipy's Laplacian ignores
the diagonal: deg_i = W_i . (W^T 1) / 2 - a_ii with a_ii = (u_i . u_i + 1) / 2; s = deg^-1/2, e = a_ii / deg, Y = diag(s) W / sqrt 2.
sklearn takes the k largest eigenpairs of M = Y Y^T - diag(e) and returns (v_j * s)_j in descending order of the eigenvalue after
its deterministic sign flip.
"""
import numpy as np

U32 = 2.0 ** -24


def generate(N, D, C, noise, seed=1):
    """The recorded cases' generator: C centres, N noisy rows -> (x fp32, planted labels)."""
    r = np.random.RandomState(seed)
    cen = r.randn(C, D)
    lab = r.randint(C, size=N)
    x = (cen[lab] + noise * r.randn(N, D)).astype(np.float32)
    return x, lab


def unit_rows(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    n = np.sqrt((x * x).sum(1, keepdims=True, dtype=dtype))
    return (x / np.maximum(n, dtype(1e-12))).astype(dtype)


def rows_ref(u):
    """(Y, s, e, deg) in fp64 from unit rows u (any float dtype)."""
    u = np.asarray(u, dtype=np.float64)
    N = u.shape[0]
    t = u.sum(0)
    aii = 0.5 * ((u * u).sum(1) + 1.0)
    deg = 0.5 * (u @ t + N) - aii
    with np.errstate(divide="ignore", invalid="ignore"):
        s = 1.0 / np.sqrt(deg)
        e = aii / deg
    Y = (s / np.sqrt(2.0))[:, None] * np.concatenate([u, np.ones((N, 1))], axis=1)
    return Y, s, e, deg


def dense_affinity(x):
    """The reference's matrix: (cosine_similarity + 1) / 2 in fp64."""
    u = unit_rows(x)
    return (u @ u.T + 1.0) / 2.0


def default_block(D, k):
    return max(k, min(D + 1, 2 * k))


def sign_flip(maps):
    """sklearn's _deterministic_vector_sign_flip on the columns of an (N, k) embedding."""
    maps = np.array(maps)
    rows = np.argmax(np.abs(maps), axis=0)
    sign = np.sign(maps[rows, np.arange(maps.shape[1])])
    sign[sign == 0] = 1
    return maps * sign


def ritz(S, H):
    """The b x b generalised problem H c = lambda S c in fp64 -> (lambda descending, C with C^T S C = I)."""
    S = 0.5 * (S + S.T)
    H = 0.5 * (H + H.T)
    Lc = np.linalg.cholesky(S)
    A = np.linalg.solve(Lc, np.linalg.solve(Lc, H).T)
    lam, V = np.linalg.eigh(0.5 * (A + A.T))
    order = np.argsort(-lam, kind="stable")
    return lam[order], np.linalg.solve(Lc.T, V[:, order])


def spectral_ref(x, k, block=None, steps=6, dtype=np.float64):
    """-> dict(maps (N, k) in fp64 = sklearn's embedding, eigenvalues (k,), residuals (one per step: the largest
    ||M x_j - lambda_j x_j|| over the first k Ritz vectors, from the vectors themselves))."""
    x = np.asarray(x, dtype=np.float32)
    N, D = x.shape
    b = default_block(D, k) if block is None else int(block)
    u = unit_rows(x, dtype)
    Y64, s, e, deg = rows_ref(u)
    if not np.all(deg > 0):
        raise ValueError(f"row {int(np.argmin(deg > 0))} has degree <= 0")
    Y, e_t = Y64.astype(dtype), e.astype(dtype)
    f64 = lambda a: a.astype(np.float64)       # noqa: E731
    mu, Q = np.linalg.eigh(f64(Y).T @ f64(Y))
    top = np.argsort(-mu, kind="stable")[:b]
    X = (Y @ (Q[:, top] / np.sqrt(mu[top])).astype(dtype)).astype(dtype)
    # the power step runs on M + sigma I, sigma = max e: M + diag(e) = Y Y^T is positive semi-definite, so every eigenvalue of the
    # shifted operator is >= 0 and the largest in magnitude are the largest of M (at small N, where e is not small, M has
    # eigenvalues near -e that are larger in magnitude than lambda_k)
    sigma = dtype(e_t.max())
    residuals = []
    for _ in range(steps):
        T = (f64(Y).T @ f64(X)).astype(dtype)
        MX = ((Y @ T).astype(dtype) - (e_t[:, None] * X).astype(dtype)).astype(dtype)
        lam, C = ritz(f64(X).T @ f64(X), f64(X).T @ f64(MX))
        Xn = (X @ C.astype(dtype)).astype(dtype)
        MXn = (MX @ C.astype(dtype)).astype(dtype)
        R = f64(MXn) - f64(Xn) * lam
        residuals.append(float(np.sqrt((R * R).sum(0))[:k].max()))
        X = ((MXn + sigma * Xn).astype(dtype) / np.where(lam + sigma > 1e-30, lam + sigma, 1.0).astype(dtype)).astype(dtype)
    maps = sign_flip(f64(Xn[:, :k]) * s[:, None])
    return {"maps": maps, "eigenvalues": lam[:k], "residuals": residuals, "block": b}


def vector_errors(maps, want):
    """Per vector: max |maps_j - want_j| / max |want_j|."""
    maps, want = np.asarray(maps, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(maps - want).max(0) / np.abs(want).max(0)


def same_partition(a, b):
    """ARI = 1: the two labelings are one partition up to the numbering."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.shape != b.shape:
        return False
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


# ---- bounds of the kernels ----
def gram_ref(P, Q, w=None):
    """(fp64 product, sum_i |w_i P_ia Q_ib|)."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    wv = np.ones(P.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    return (P * wv[:, None]).T @ Q, np.abs(P * wv[:, None]).T @ np.abs(Q)


def gram_bound(mag, chain):
    """|err_ab| <= chain 2^-24 sum_i |w_i P_ia Q_ib| + one fp64 ulp of that sum: no term of a slice passes through more than
    ``chain`` fp32 roundings, and the slices are added in fp64."""
    return chain * U32 * mag + np.spacing(mag)


def apply_ref(Y, T, e, X):
    Y, T, e, X = (np.asarray(a, dtype=np.float64) for a in (Y, T, e, X))
    return Y @ T - e[:, None] * X, np.abs(Y) @ np.abs(T) + np.abs(e[:, None] * X)


def apply_bound(mag, Dp):
    return (Dp + 2) * U32 * mag
