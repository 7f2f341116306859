"""k-means, DBSCAN, average-linkage and spectral clustering over phrase embeddings on the device: what python_scripts/clustering/kmeans_emb.py,
dbscan_emb.py, agc_emb.py and spectral_emb.py of the reference do with sklearn on the host.  ``DBSCAN`` / ``dbscan_cluster_map`` (csrc/dbscan.hip) are described at the class; their
cluster map feeds the same ``neg_samp_stratg="clustering"`` and ``SpectralMappingDataset`` / ``SpectralMappingEvalDataset``.
k-means makes the ``cluster_map`` JSON that ``AudioSamplePhrasesDataset(neg_samp_stratg="clustering")`` reads and the cluster model that ``KmeansMappingDataset`` / ``KmeansMappingEvalDataset`` turn phrases into class indices with.

``KMeans`` runs Lloyd's algorithm on three entry points of csrc/kmeans.hip (``ops.kmeans_assign`` / ``kmeans_update`` /
``kmeans_seed_step``): no (N, K) matrix exists on the device and two fits from the same start give the same bits.  The stopping
rules are sklearn's: stop when the labels equal the previous iteration's, or when sum ||delta c||^2 <= tol * mean(var(x, axis 0))
(then one more assignment so that ``labels_`` match the centres); ``n_iter_`` counts completed iterations.  An empty cluster
takes the row with the largest squared distance to its centre (several empty clusters: the largest first), and that row
leaves its donor cluster's sum and count before the division.

``AgglomerativeClustering`` / ``agc_cluster_map`` (csrc/agc.hip) are python_scripts/clustering/agc_emb.py: average linkage over the
cosine distance without the N x N matrix.  A cluster is the fp64 sum of its unit rows (the average distance of two clusters is
1 - mean_A . mean_B), every round merges all reciprocal nearest neighbours at once (``ops.agc_nearest`` + ``ops.agc_merge``, one
host read per round), and the host half (``agc_tree`` / ``agc_cut``, plain numpy, no GPU) orders the merges and cuts the tree as
sklearn does; the class states when the labels are sklearn's own.

``SpectralClustering`` / ``spectral_cluster_map`` (csrc/spectral.hip) are python_scripts/clustering/spectral_emb.py: sklearn's
spectral embedding of the affinity (cos + 1) / 2 without the N x N matrix.  The affinity has rank D + 1, so the normalised
operator is applied through two tall-skinny products (``ops.spectral_gram`` / ``spectral_rows`` / ``spectral_apply``), a block
subspace iteration with a host Rayleigh-Ritz step (``spectral_start`` / ``spectral_ritz`` / ``spectral_sign_flip``, plain numpy, no
GPU) finds the leading eigenvectors, and the device ``KMeans`` labels the rows of the embedding.

Deviations from sklearn: ``"k-means++"`` is plain D^2 sampling with one candidate per step (no greedy multi-trial), x is not
mean-centred before the fit, and the arithmetic is fp32 with fp64 cluster sums.
"""
import os
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch


def cluster_map_from_labels(phrases: Sequence[str], labels) -> Dict[str, List[str]]:
    """{str(label): [phrases ...]} with keys in order of first appearance: the reference's ``result``."""
    result: Dict[str, List[str]] = {}
    for phrase, label in zip(phrases, labels):
        result.setdefault(str(int(label)), []).append(phrase)
    return result


def load_cluster_centers(path) -> np.ndarray:
    """The (K, D) fp32 centres of a cluster model file: an ``.npz`` written by ``KMeans.save`` is read natively; any other suffix is
    tried through joblib and the object's ``cluster_centers_`` taken, so a checkpoint of the reference's script still loads."""
    path = os.fspath(path)
    if path.endswith(".npz"):
        with np.load(path) as f:
            return np.ascontiguousarray(f["cluster_centers"], dtype=np.float32)
    try:
        import joblib
    except ImportError:
        raise RuntimeError(f"{path}: only .npz cluster models (KMeans.save) are read natively; any other file is taken for a "
                           "joblib checkpoint of sklearn's KMeans, and joblib is not importable here") from None
    return np.ascontiguousarray(joblib.load(path).cluster_centers_, dtype=np.float32)


class KMeans:
    """sklearn-shaped k-means on the device.  ``init``: "k-means++" or a (K, D) array; ``n_init`` > 1 (k-means++ only) keeps the
    run with the lowest inertia.  After ``fit``: ``cluster_centers_`` (numpy fp32), ``labels_`` (numpy int32), ``inertia_`` (the
    fp64 sum of the squared distances), ``n_iter_``."""

    def __init__(self, n_clusters, init="k-means++", n_init=1, max_iter=300, tol=1e-4, random_state=None, device="cuda:0"):
        self.n_clusters = int(n_clusters)
        self.init = init
        self.n_init = int(n_init)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.random_state = random_state
        self.device = device
        if self.n_clusters < 1 or self.n_init < 1 or self.max_iter < 1:
            raise ValueError(f"n_clusters, n_init and max_iter must be >= 1 (got {n_clusters}, {n_init}, {max_iter})")
        if isinstance(init, str) and init != "k-means++":
            raise ValueError(f"init: expected 'k-means++' or a (K, D) array, got {init!r}")
        self.cluster_centers_: Optional[np.ndarray] = None
        self.labels_: Optional[np.ndarray] = None
        self.inertia_: Optional[float] = None
        self.n_iter_: Optional[int] = None
        self._centers_dev = None

    # ---- plumbing ----
    def _rows(self, x):
        """(N, D) fp32 on self.device; a device tensor is taken as it is."""
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
        x = x.to(device=self.device, dtype=torch.float32)
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"x: expected a (N >= 1, D >= 1) matrix, got {tuple(x.shape)}")
        return x

    def _centers(self, D=None):
        if self.cluster_centers_ is None:
            raise RuntimeError("this KMeans has no centres yet: call fit or KMeans.load first")
        if self._centers_dev is None or str(self._centers_dev.device) != str(torch.device(self.device)):
            self._centers_dev = torch.from_numpy(self.cluster_centers_).to(self.device)
        if D is not None and self._centers_dev.shape[1] != D:
            raise ValueError(f"x has D = {D}, the centres have D = {self._centers_dev.shape[1]}")
        return self._centers_dev

    # ---- seeding ----
    def seed_picks(self, x, rs) -> torch.Tensor:
        """k-means++ by plain D^2 sampling -> the (K,) int64 row indices, on the device.  The uniforms come from ``rs`` (a
        numpy RandomState) on the host, ``randint(N)`` then ``random_sample(K - 1)``; pick j is the first row whose fp64 prefix
        sum of ``closest`` reaches u_j times the total.  Nothing is read back inside the loop."""
        from .. import ops
        N, K = x.shape[0], self.n_clusters
        first = int(rs.randint(N))
        u = torch.from_numpy(np.asarray(rs.random_sample(K - 1), dtype=np.float64)).to(x.device)
        picks = torch.empty(K, device=x.device, dtype=torch.int64)
        picks[0] = first
        closest = torch.empty(N, device=x.device, dtype=torch.float32)
        for j in range(1, K):
            ops.kmeans_seed_step(x, picks[j - 1:j], closest, first=(j == 1))
            cs = torch.cumsum(closest.double(), 0)
            picks[j] = torch.searchsorted(cs, (u[j - 1] * cs[-1]).reshape(1)).clamp_(max=N - 1)[0]
        return picks

    # ---- Lloyd ----
    def _lloyd(self, x, centers, tol_abs):
        """One run from ``centers`` (K, D) fp32 on the device, updated in place -> (labels int32, dist2 fp32, n_iter)."""
        from .. import ops
        N = x.shape[0]
        prev = torch.full((N,), -1, device=x.device, dtype=torch.int32)
        strict, n_iter = False, 0
        for it in range(self.max_iter):
            label, dist2 = ops.kmeans_assign(x, centers)
            old = centers.clone()
            sums, count = ops.kmeans_update(x, label, centers, check_labels=False)
            empty = count == 0
            shift = ((centers.double() - old.double()) ** 2).sum()
            same, n_empty, small = torch.stack(((label == prev).all().double(), empty.sum().double(),
                                                (shift <= tol_abs).double())).tolist()       # the iteration's one host read
            if n_empty:
                self._relocate(x, label, dist2, sums, count, centers, torch.nonzero(empty).flatten().tolist())
                small = bool(((centers.double() - old.double()) ** 2).sum() <= tol_abs)
            n_iter = it + 1
            if same:
                strict = True
                break
            if small:
                break
            prev = label
        if not strict:
            label, dist2 = ops.kmeans_assign(x, centers)
        return label, dist2, n_iter

    @staticmethod
    def _relocate(x, label, dist2, sums, count, centers, empty):
        """sklearn's rule for empty clusters (rare: plain torch indexing on the fp64 sums): they take the rows with the largest
        dist2, the largest first; each such row leaves its donor cluster before the division."""
        far = torch.argsort(dist2, descending=True, stable=True)[:len(empty)].tolist()
        touched = set()
        for k, i in zip(empty, far):
            donor = int(label[i])
            row = x[i].double()
            sums[donor] -= row
            count[donor] -= 1
            sums[k] = row
            count[k] = 1
            touched.update((donor, k))
        for k in sorted(touched):
            if int(count[k]) > 0:
                centers[k] = (sums[k] / count[k].double()).float()

    def fit(self, x):
        x = self._rows(x)
        N, D = x.shape
        K = self.n_clusters
        if K > N:
            raise ValueError(f"n_samples={N} should be >= n_clusters={K}")
        explicit = not isinstance(self.init, str)
        if explicit:
            init = self._rows(self.init)
            if tuple(init.shape) != (K, D):
                raise ValueError(f"init: expected a ({K}, {D}) array, got {tuple(init.shape)}")
        tol_abs = self.tol * x.double().var(dim=0, unbiased=False).mean()
        rs = np.random.RandomState(self.random_state)
        best = None
        for _ in range(1 if explicit else self.n_init):
            centers = init.clone().contiguous() if explicit else x[self.seed_picks(x, rs)].contiguous()
            label, dist2, n_iter = self._lloyd(x, centers, tol_abs)
            inertia = float(dist2.double().sum())
            if best is None or inertia < best[0]:
                best = (inertia, centers, label, n_iter)
        self.inertia_, self._centers_dev, label, self.n_iter_ = best
        self.cluster_centers_ = self._centers_dev.cpu().numpy()
        self.labels_ = label.cpu().numpy()
        return self

    def fit_predict(self, x):
        return self.fit(x).labels_

    def _assign(self, x):
        from .. import ops
        x = self._rows(x)
        return ops.kmeans_assign(x, self._centers(x.shape[1]))

    def predict(self, x) -> np.ndarray:
        return self._assign(x)[0].cpu().numpy()

    def min_distance(self, x) -> np.ndarray:
        """sqrt(dist2): what ``transform(x).min(1)`` gives, without the (N, K) matrix."""
        return torch.sqrt(self._assign(x)[1]).cpu().numpy()

    def predict_min_distance(self, x):
        """(labels, distances to the assigned centre) from ONE assignment call."""
        label, dist2 = self._assign(x)
        return label.cpu().numpy(), torch.sqrt(dist2).cpu().numpy()

    def transform(self, x) -> np.ndarray:
        """(N, K) Euclidean distances (interface parity; the one place an N x K array exists): ||x||^2 + ||c||^2 - 2 x . c with
        the products from ops.gemm, clamped at 0 before the root."""
        from .. import ops
        x = self._rows(x).contiguous()
        c = self._centers(x.shape[1])
        N, D = x.shape
        xc = ops.gemm(x, c, N, c.shape[0], D, transB=True)
        d2 = (x * x).sum(1, keepdim=True) + (c * c).sum(1)[None, :] - 2.0 * xc
        return torch.sqrt(d2.clamp_(min=0.0)).cpu().numpy()

    # ---- files ----
    def save(self, path):
        """An ``.npz`` holding the centres and the constructor settings (``load_cluster_centers`` / ``KMeans.load`` read it)."""
        if self.cluster_centers_ is None:
            raise RuntimeError("this KMeans has no centres yet: call fit first")
        np.savez(path, cluster_centers=self.cluster_centers_, n_clusters=self.n_clusters, n_init=self.n_init, max_iter=self.max_iter,
                 tol=self.tol, random_state=-1 if self.random_state is None else int(self.random_state),
                 has_random_state=self.random_state is not None, inertia=np.nan if self.inertia_ is None else self.inertia_,
                 n_iter=-1 if self.n_iter_ is None else self.n_iter_)

    @classmethod
    def load(cls, path, device="cuda:0"):
        with np.load(path) as f:
            km = cls(int(f["n_clusters"]), n_init=int(f["n_init"]), max_iter=int(f["max_iter"]), tol=float(f["tol"]),
                     random_state=int(f["random_state"]) if bool(f["has_random_state"]) else None, device=device)
            km.cluster_centers_ = np.ascontiguousarray(f["cluster_centers"], dtype=np.float32)
            km.inertia_ = None if np.isnan(f["inertia"]) else float(f["inertia"])
            km.n_iter_ = None if int(f["n_iter"]) < 0 else int(f["n_iter"])
        return km

    @classmethod
    def from_centers(cls, centers, device="cuda:0"):
        """A model that only predicts: the (K, D) centres of ``load_cluster_centers``."""
        centers = np.ascontiguousarray(centers, dtype=np.float32)
        km = cls(centers.shape[0], device=device)
        km.cluster_centers_ = centers
        return km


def kmeans_cluster_map(phrase_to_emb: Mapping[str, np.ndarray], n_clusters: int, **kw):
    """The reference's ``KmeansClustering().kmeans`` on a {phrase: embedding} table -> {"score": inertia, "model": the fitted
    KMeans, "result": {str(label): [phrases ...]}}; ``kw`` goes to ``KMeans``."""
    phrases = list(phrase_to_emb)
    embs = np.stack([np.asarray(phrase_to_emb[p], dtype=np.float32).reshape(-1) for p in phrases])
    model = KMeans(n_clusters, **kw)
    labels = model.fit_predict(embs)
    return {"score": model.inertia_, "model": model, "result": cluster_map_from_labels(phrases, labels)}


class DBSCAN:
    """sklearn-shaped DBSCAN over the cosine distance on the device: what python_scripts/clustering/dbscan_emb.py of the reference
    does with ``DBSCAN(metric="precomputed")`` on ``(1 - cosine_similarity).clip(0)``, without the N x N float matrix (the graph
    is N^2 / 8 bytes of bits, csrc/dbscan.hip).  The labels are sklearn's own, not merely the same partition:

    * neighbours: ``u_i . u_j >= 1 - eps`` with ``u = x / max(||x||, 1e-12)``, the diagonal computed like any pair (an all-zero
      row has no neighbour, not even itself: noise);
    * a row is core when it has at least ``min_samples`` neighbours; the clusters are the connected components of the core-core
      graph (FastSV hooking on a parent array, ``n_passes_`` passes of ``ops.dbscan_hook`` with one host read each);
    * a row that is not core takes the cluster with the lowest root (= lowest core index) among its core neighbours -- sklearn
      grows its clusters one at a time in that order --, or -1 without one;
    * the clusters are numbered in ascending order of their roots.

    After ``fit``: ``labels_`` (numpy int64, -1 = noise), ``core_sample_indices_`` (numpy int64), ``n_passes_``.  ``sample_weight``
    and other metrics are not offered."""

    def __init__(self, eps=0.5, min_samples=5, device=None):
        self.eps = float(eps)
        self.min_samples = int(min_samples)
        self.device = "cuda:0" if device is None else device
        if not 0.0 < self.eps <= 2.0:
            raise ValueError(f"eps: expected a cosine distance in (0, 2], got {eps}")
        if self.min_samples < 1:
            raise ValueError(f"min_samples must be >= 1 (got {min_samples})")
        self.labels_: Optional[np.ndarray] = None
        self.core_sample_indices_: Optional[np.ndarray] = None
        self.n_passes_: Optional[int] = None

    def fit(self, x):
        from .. import ops
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.array(x, dtype=np.float32, order="C"))       # (a copy: the caller's array may be read-only)
        x = x.to(device=self.device, dtype=torch.float32)
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"x: expected a (N >= 1, D >= 1) matrix, got {tuple(x.shape)}")
        N = x.shape[0]
        adj, degree = ops.dbscan_graph(x, eps=self.eps, normalize=True)
        core_bits = ops.dbscan_core(degree, self.min_samples)
        f = torch.arange(N, device=x.device, dtype=torch.int32)
        g = torch.empty_like(f)
        changed = torch.empty(1, device=x.device, dtype=torch.int32)
        passes = 0
        while True:
            ops.dbscan_hook(adj, core_bits, f, g, changed, check=False)
            f, g = g, f
            passes += 1
            if not int(changed):                    # the pass's one host read
                break
        root = ops.dbscan_roots(adj, core_bits, f).long()
        roots = torch.unique(root[root >= 0])       # ascending
        labels = torch.where(root >= 0, torch.searchsorted(roots, root.clamp(min=0)), torch.full_like(root, -1))
        self.labels_ = labels.cpu().numpy()
        self.core_sample_indices_ = torch.nonzero(degree >= self.min_samples).flatten().cpu().numpy()
        self.n_passes_ = passes
        return self

    def fit_predict(self, x):
        return self.fit(x).labels_


def dbscan_cluster_map(phrase_to_emb: Mapping[str, np.ndarray], eps: float = 0.5, min_samples: int = 5, device=None):
    """The reference's ``Runner().dbscan`` on a {phrase: embedding} table -> {"result": {str(label): [phrases ...]} with the keys
    in order of first appearance and noise under "-1", "model": the fitted DBSCAN}."""
    phrases = list(phrase_to_emb)
    embs = np.stack([np.asarray(phrase_to_emb[p], dtype=np.float32).reshape(-1) for p in phrases])
    model = DBSCAN(eps=eps, min_samples=min_samples, device=device)
    labels = model.fit_predict(embs)
    return {"result": cluster_map_from_labels(phrases, labels), "model": model}


def agc_tree(heights, id_a, id_b, n_leaves):
    """The host half of the agglomerative fit, numpy only: the merge log in the order the rounds wrote it (row r made node
    ``n_leaves + r`` out of nodes ``id_a[r]`` and ``id_b[r]`` at ``heights[r]``) -> (children (N - 1, 2) int64, distances (N - 1,)
    float64) as scipy / sklearn number a dendrogram: merges sorted by height, stably, node ``n_leaves + rank``, children as
    (min, max).  Average linkage has no inversions, but a rounded height may fall an ulp below a child's: the sort key of a node
    is the largest height on its subtree (``distances`` holds that key), so a child always precedes its parent."""
    h = np.asarray(heights, dtype=np.float64).reshape(-1)
    a = np.asarray(id_a, dtype=np.int64).reshape(-1)
    b = np.asarray(id_b, dtype=np.int64).reshape(-1)
    N = int(n_leaves)
    if not (h.size == a.size == b.size == N - 1):
        raise ValueError(f"a tree over {N} leaves has {N - 1} merges, got {h.size}, {a.size}, {b.size} log rows")
    both = np.concatenate([a, b])
    if N > 1 and not np.array_equal(np.sort(both), np.arange(2 * N - 2)):
        raise ValueError("the merge log is not a binary tree: every node but the root must be merged exactly once")
    if np.any(np.maximum(a, b) >= N + np.arange(N - 1)):
        raise ValueError("the merge log is out of order: a row merges a node that a later row makes")
    key = h.copy()
    for r in np.flatnonzero(np.maximum(a, b) >= N):             # (leaf-leaf merges keep their height)
        for c in (a[r], b[r]):
            if c >= N and key[c - N] > key[r]:
                key[r] = key[c - N]
    order = np.argsort(key, kind="stable")
    rank = np.empty(N - 1, dtype=np.int64)
    rank[order] = np.arange(N - 1)

    def renumber(ids):
        return np.where(ids >= N, N + rank[np.clip(ids - N, 0, max(N - 2, 0))], ids) if N > 1 else ids

    ca, cb = renumber(a)[order], renumber(b)[order]
    return np.stack([np.minimum(ca, cb), np.maximum(ca, cb)], axis=1).reshape(N - 1, 2), key[order]


def agc_cut(children, n_leaves, n_clusters):
    """The flat clustering sklearn's ``_hc_cut`` reads off a tree: a heap of negated node ids that starts at the root and
    ``n_clusters - 1`` times replaces its largest node by that node's two children; label i goes to the leaves under the i-th
    entry of the heap's list.  -> (n_leaves,) int64."""
    import heapq
    N, K = int(n_leaves), int(n_clusters)
    if not 1 <= K <= N:
        raise ValueError(f"n_clusters = {K}: expected 1 .. {N} for a tree with {N} leaves")
    children = np.asarray(children, dtype=np.int64).reshape(N - 1, 2)
    labels = np.zeros(N, dtype=np.int64)
    if N == 1:
        return labels
    nodes = [-(2 * N - 2)]
    for _ in range(K - 1):
        left, right = children[-nodes[0] - N]
        heapq.heappush(nodes, -int(left))
        heapq.heappushpop(nodes, -int(right))
    for i, node in enumerate(nodes):
        stack = [-node]
        while stack:
            n = stack.pop()
            if n < N:
                labels[n] = i
            else:
                stack.extend(children[n - N].tolist())
    return labels


class AgglomerativeClustering:
    """sklearn-shaped average-linkage clustering over the cosine distance on the device: what python_scripts/clustering/agc_emb.py of
    the reference does with ``AgglomerativeClustering(n_clusters, linkage="average", affinity="precomputed")`` on
    ``1 - cosine_similarity``, without the N x N float matrix (csrc/agc.hip; device memory about 20 N D bytes).

    * rows: ``u = x / max(||x||, 1e-12)``; a cluster is the fp64 sum of its rows and its fp32 mean, and the distance of two
      clusters is ``1 - mean_A . mean_B`` in fp32 (error about (D + 6) 2^-24);
    * a round merges every pair of clusters that are each other's nearest (``ops.agc_nearest``, ``ops.agc_merge``); average
      linkage is reducible, so the set of merges and their heights are those of the serial algorithm; ``n_rounds_`` rounds with
      one host read each, and the merge log is read once;
    * the merges are sorted by height, numbered and cut as scipy and sklearn do (``agc_tree``, ``agc_cut``).

    The labels are sklearn's own, element for element, where the top ``n_clusters`` merge heights are separated by more than the
    fp32 error of a height.  Under exact ties (duplicate phrases, say) the result is still a valid average-linkage cut, but the
    order of tied merges is scipy's nearest-neighbour-chain order, which is not reproduced, so labels may be permuted or tied
    merges resolved differently.

    Only ``linkage="average"`` is offered (anything else raises ValueError).  After ``fit``: ``labels_`` (numpy int64),
    ``children_`` ((N - 1, 2) int64), ``distances_`` ((N - 1,) float64, ascending), ``n_leaves_``, ``n_rounds_``;
    ``labels_for(k)`` re-cuts the stored tree."""

    def __init__(self, n_clusters=2, linkage="average", device=None):
        if linkage != "average":
            raise ValueError(f"linkage: only 'average' over the cosine distance is offered, got {linkage!r}")
        self.n_clusters = int(n_clusters)
        if self.n_clusters < 1:
            raise ValueError(f"n_clusters must be >= 1 (got {n_clusters})")
        self.linkage = linkage
        self.device = "cuda:0" if device is None else device
        self.labels_: Optional[np.ndarray] = None
        self.children_: Optional[np.ndarray] = None
        self.distances_: Optional[np.ndarray] = None
        self.n_leaves_: Optional[int] = None
        self.n_rounds_: Optional[int] = None

    def _set_tree(self, heights, id_a, id_b, n_leaves, n_rounds):
        """The host half: from a merge log to the fitted attributes (no GPU)."""
        if self.n_clusters > n_leaves:
            raise ValueError(f"n_samples={n_leaves} should be >= n_clusters={self.n_clusters}")
        self.children_, self.distances_ = agc_tree(heights, id_a, id_b, n_leaves)
        self.n_leaves_, self.n_rounds_ = int(n_leaves), int(n_rounds)
        self.labels_ = self.labels_for(self.n_clusters)
        return self

    def labels_for(self, n_clusters) -> np.ndarray:
        """The labels of another ``n_clusters`` from the stored tree, without a fit."""
        if self.children_ is None:
            raise RuntimeError("this AgglomerativeClustering has no tree yet: call fit first")
        return agc_cut(self.children_, self.n_leaves_, n_clusters)

    def fit(self, x):
        from .. import ops
        from ..dispatch import _unit_rows
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.array(x, dtype=np.float32, order="C"))       # (a copy: the caller's array may be read-only)
        x = x.to(device=self.device, dtype=torch.float32)
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"x: expected a (N >= 1, D >= 1) matrix, got {tuple(x.shape)}")
        N, D = x.shape
        if self.n_clusters > N:
            raise ValueError(f"n_samples={N} should be >= n_clusters={self.n_clusters}")
        if not bool(torch.isfinite(x).all()):
            raise ValueError("x holds NaN or infinite values: such a row has no nearest cluster")
        if N == 1:
            return self._set_tree(np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 1, 0)
        dev = x.device
        means = _unit_rows(x.contiguous(), N, D)                    # a cluster of one row: sum = mean = the row
        sums, sizes, ids = means.double(), torch.ones(N, device=dev, dtype=torch.int64), torch.arange(N, device=dev, dtype=torch.int32)
        sums2, sizes2, ids2 = torch.empty_like(sums), torch.empty_like(sizes), torch.empty_like(ids)
        log_dist = torch.empty(N - 1, device=dev, dtype=torch.float32)
        log_ids = torch.empty(N - 1, 3, device=dev, dtype=torch.int32)
        counts = torch.empty(2, device=dev, dtype=torch.int32)
        M, rounds = N, 0
        while M > 1:                                                # every round merges at least one pair: at most N - 1 rounds
            nn, dist = ops.agc_nearest(means[:M])
            ops.agc_merge(nn, dist, sums, sizes, ids, sums2, sizes2, ids2, means, log_dist, log_ids, counts, log_off=N - M,
                          next_id=2 * N - M)
            pairs, new_m = counts.tolist()                          # the round's one host read
            if pairs < 1 or new_m != M - pairs:
                raise RuntimeError(f"round {rounds + 1} at {M} clusters merged {pairs} pairs: no two clusters are each other's "
                                   "nearest, which the bit-symmetric scores of agc_nearest rule out for finite rows")
            sums, sums2, sizes, sizes2, ids, ids2 = sums2, sums, sizes2, sizes, ids2, ids
            M = new_m
            rounds += 1
        log = log_ids.cpu().numpy()
        if not np.array_equal(log[:, 2], N + np.arange(N - 1)):
            raise RuntimeError("the merge log does not number its nodes N, N + 1, ...")
        return self._set_tree(log_dist.cpu().numpy(), log[:, 0], log[:, 1], N, rounds)

    def fit_predict(self, x):
        return self.fit(x).labels_


def agc_cluster_map(phrase_to_emb: Mapping[str, np.ndarray], n_clusters: int, device=None):
    """The reference's ``Runner().agc`` on a {phrase: embedding} table -> {"result": {str(label): [phrases ...]} with the keys in
    order of first appearance, "model": the fitted AgglomerativeClustering}."""
    phrases = list(phrase_to_emb)
    embs = np.stack([np.asarray(phrase_to_emb[p], dtype=np.float32).reshape(-1) for p in phrases])
    model = AgglomerativeClustering(n_clusters, device=device)
    labels = model.fit_predict(embs)
    return {"result": cluster_map_from_labels(phrases, labels), "model": model}


def spectral_block(n_rows, dim, n_clusters, block=None):
    """Columns of the iterated block: ``n_clusters`` plus guard columns, ``min(D + 1, 2 k)`` by default (a block of exactly k columns
    converges at the rate lambda_(k+1) / lambda_k, which is close to 1 when two eigenvalues are close), never more than the rank
    bound ``min(N, D + 1)`` of the affinity."""
    k, cap = int(n_clusters), min(int(n_rows), int(dim) + 1)
    b = min(cap, 2 * k) if block is None else int(block)
    if not k <= b <= cap:
        raise ValueError(f"block = {b}: expected n_clusters = {k} <= block <= min(N, D + 1) = {cap}")
    return b


def spectral_start(gram, block):
    """The host half of the start, numpy fp64: the (D + 1)^2 Gram matrix Y^T Y -> (mu (block,) descending, coef (D + 1, block)) with
    X0 = Y coef = Y Q mu^-1/2, orthonormal eigenvectors of Y Y^T.  M differs from Y Y^T by diag(e) = O(2 / N), so X0 already has
    a residual near 1e-4.  An eigenvalue at the rounding level of the largest has no direction to start from and raises."""
    G = np.asarray(gram, dtype=np.float64)
    G = 0.5 * (G + G.T)
    mu, Q = np.linalg.eigh(G)
    top = np.argsort(-mu, kind="stable")[:int(block)]
    mu, Q = mu[top], Q[:, top]
    if not np.all(np.isfinite(mu)) or mu[-1] <= 1e-10 * mu[0]:
        raise ValueError(f"the affinity has fewer than {int(block)} independent directions (eigenvalues of Y^T Y: {mu[0]:.3g} down "
                         f"to {mu[-1]:.3g}): the embeddings span a lower dimension, choose a smaller n_clusters / block")
    return mu, np.ascontiguousarray(Q / np.sqrt(mu))            # (Q[:, top] is column-major: the device reads row-major)


def spectral_ritz(S, H):
    """The Rayleigh-Ritz step, numpy fp64: S = X^T X and H = X^T M X of a block X -> (lam (b,) descending, C (b, b)) with
    H C = S C diag(lam) and C^T S C = I (Cholesky of S, a symmetric eigenproblem, back-substitution): X C are the Ritz vectors."""
    S = np.asarray(S, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    S, H = 0.5 * (S + S.T), 0.5 * (H + H.T)
    try:
        Lc = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        raise ValueError("the block lost rank (X^T X is not positive definite): choose a smaller block") from None
    A = np.linalg.solve(Lc, np.linalg.solve(Lc, H).T)
    lam, V = np.linalg.eigh(0.5 * (A + A.T))
    order = np.argsort(-lam, kind="stable")
    return lam[order], np.ascontiguousarray(np.linalg.solve(Lc.T, V[:, order]))


def _to_device(a, dev):
    """A host fp64 matrix as a row-major fp32 tensor on the device (the kernels take a pointer and a row stride)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def spectral_sign_flip(maps):
    """sklearn's ``_deterministic_vector_sign_flip`` on the columns of an (N, k) embedding: the entry of largest magnitude of every
    vector (the first one on ties) becomes positive."""
    maps = np.array(maps)
    rows = np.argmax(np.abs(maps), axis=0)
    sign = np.sign(maps[rows, np.arange(maps.shape[1])])
    sign[sign == 0] = 1
    return maps * sign.astype(maps.dtype)


class SpectralClustering:
    """sklearn-shaped spectral clustering over the cosine affinity on the device: what python_scripts/clustering/spectral_emb.py of
    the reference does with ``SpectralClustering(n_clusters, affinity="precomputed", random_state=seed)`` on the dense matrix
    ``(cosine_similarity + 1) / 2``, without the N x N matrix (csrc/spectral.hip).

    * rows: ``u = x / max(||x||, 1e-12)``, ``W = [u | 1]``; the affinity is ``W W^T / 2``, rank D + 1.  scipy's Laplacian ignores
      the diagonal: ``deg_i = W_i . (W^T 1) / 2 - a_ii``; with ``s = deg^-1/2``, ``e = a_ii / deg``, ``Y = diag(s) W / sqrt 2``
      (``ops.spectral_rows``) sklearn's eigenproblem is the k largest pairs of ``M = Y Y^T - diag(e)``, and
      ``M X = Y (Y^T X) - e * X`` is two tall-skinny products (``ops.spectral_gram``, ``ops.spectral_apply``);
    * solver: block subspace iteration with Rayleigh-Ritz on ``block`` columns (``spectral_block``: ``min(D + 1, 2 k)``), started
      from the eigenvectors of ``Y Y^T`` (``spectral_start``).  An iteration applies M, forms ``X^T X`` and ``X^T M X`` in fp64 on
      the device, solves the small problem on the host (``spectral_ritz``, numpy fp64), rotates both blocks with ``ops.gemm`` and
      continues from ``(M + sigma I) X C / (lambda + sigma)`` with ``sigma = max e``: ``M + diag(e) = Y Y^T`` is positive
      semi-definite, so the shifted operator has no negative eigenvalue and its dominant vectors are the largest of M for every N
      (e is O(2 / N); at a handful of rows M has eigenvalues near -e that exceed lambda_k in magnitude).  The residual
      ``max_j<k ||M x_j - lambda_j x_j||`` is taken from the rotated vectors themselves and is read with the NEXT iteration's Gram
      matrices: one host read per iteration and one at the end.  The loop ends one iteration after the residual is at most
      ``tol`` or no longer halves, or at ``max_iter``;
    * ``maps_`` = the Ritz vectors times s after sklearn's sign flip (``spectral_sign_flip``): sklearn's ``spectral_embedding`` in
      descending order of the eigenvalue; ``labels_`` = the device ``KMeans(n_clusters, n_init=n_init, random_state=random_state)``
      on its rows.  sklearn seeds k-means with its greedy k-means++, so the labels are its PARTITION where the clusters of the
      embedding are separated, not its numbering.

    ``tol`` defaults to 2e-7, two to five times the measured fp32 floor of the residual (docs/experiments_spectral.md).  After ``fit``:
    ``labels_`` (numpy int64), ``maps_`` ((N, k) fp32), ``eigenvalues_`` ((k,) fp64, of M: sklearn's Laplacian has 1 - these),
    ``residuals_`` (one per iteration), ``n_iter_``, ``block_``.  ``n_clusters`` above ``min(N, D + 1)`` is refused: the affinity
    has no more eigenvectors than that."""

    def __init__(self, n_clusters=8, n_init=10, random_state=None, block=None, max_iter=10, tol=None, device=None):
        self.n_clusters = int(n_clusters)
        self.n_init = int(n_init)
        self.random_state = random_state
        self.block = None if block is None else int(block)
        self.max_iter = int(max_iter)
        self.tol = 2e-7 if tol is None else float(tol)
        self.device = "cuda:0" if device is None else device
        if self.n_clusters < 1 or self.n_init < 1 or self.max_iter < 1:
            raise ValueError(f"n_clusters, n_init and max_iter must be >= 1 (got {n_clusters}, {n_init}, {max_iter})")
        if not self.tol > 0.0:
            raise ValueError(f"tol must be > 0 (got {tol})")
        self.labels_: Optional[np.ndarray] = None
        self.maps_: Optional[np.ndarray] = None
        self.eigenvalues_: Optional[np.ndarray] = None
        self.residuals_: Optional[List[float]] = None
        self.n_iter_: Optional[int] = None
        self.block_: Optional[int] = None

    def _check_shape(self, N, D):
        """-> the block size; the refusals that need no GPU."""
        if self.n_clusters > min(N, D + 1):
            raise ValueError(f"n_clusters={self.n_clusters} should be <= min(n_samples, D + 1) = min({N}, {D + 1}): the affinity "
                             f"(cos + 1) / 2 of {D}-dimensional rows has rank D + 1, it has no more eigenvectors than that")
        return spectral_block(N, D, self.n_clusters, self.block)

    def _embed(self, x, b):
        """(Ritz vectors (N, k) on the device, s (N,), eigenvalues) of the fitted block of b columns."""
        from .. import ops
        from ..dispatch import _unit_rows
        N, D = x.shape
        k, dev = self.n_clusters, x.device
        u = _unit_rows(x.contiguous(), N, D)
        t = ops.spectral_gram(u, torch.ones(N, 1, device=dev))[:, 0].contiguous()
        Y, s, e = ops.spectral_rows(u, t)
        G = ops.spectral_gram(Y, Y)
        host = torch.cat((G.flatten(), e.max().double().reshape(1), (s <= 0).sum().double().reshape(1))).cpu().numpy()
        sigma = float(host[-2])                                          # (the start's one host read: G, max e, the rows reported)
        if host[-1]:
            row = int(torch.nonzero(s <= 0)[0])
            raise ValueError(f"row {row} has degree <= 0 in the affinity (cos + 1) / 2 without its diagonal (every other row is "
                             "opposite to it): the normalised Laplacian does not exist")
        G = host[:-2].reshape(D + 1, D + 1)
        _, coef = spectral_start(G, b)
        X = ops.gemm(Y, _to_device(coef, dev), N, b, D + 1, lda=Y.stride(0))
        self.residuals_, resid = [], None
        for it in range(1, self.max_iter + 1):
            MX = ops.spectral_apply(Y, ops.spectral_gram(Y, X).float(), e, X)
            S, H = ops.spectral_gram(X, X), ops.spectral_gram(X, MX)
            parts = [S.flatten(), H.flatten()] + ([resid] if resid is not None else [])
            host = torch.cat(parts).cpu().numpy()                       # the iteration's one host read
            done = False
            if resid is not None:
                self.residuals_.append(float(host[2 * b * b:].max()))
                r = self.residuals_
                done = r[-1] <= self.tol or (len(r) > 1 and r[-1] > 0.5 * r[-2])
            lam, C = spectral_ritz(host[:b * b].reshape(b, b), host[b * b:2 * b * b].reshape(b, b))
            Cd = _to_device(C, dev)
            lam_d = torch.from_numpy(lam).to(dev)
            Xn, MXn = ops.gemm(X, Cd, N, b, b), ops.gemm(MX, Cd, N, b, b)
            resid = ((MXn[:, :k].double() - Xn[:, :k].double() * lam_d[:k]) ** 2).sum(0).sqrt()
            self.n_iter_ = it
            if done:
                break
            scale = lam_d + sigma
            X = (MXn + sigma * Xn) / torch.where(scale > 1e-30, scale, torch.ones_like(scale)).float()
        self.residuals_.append(float(resid.max()))
        return Xn[:, :k], s, lam[:k]

    def fit(self, x):
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.array(x, dtype=np.float32, order="C"))       # (a copy: the caller's array may be read-only)
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"x: expected a (N >= 1, D >= 1) matrix, got {tuple(x.shape)}")
        N, D = x.shape
        b = self._check_shape(N, D)
        if not bool(torch.isfinite(x).all()):
            raise ValueError("x holds NaN or infinite values: such a row has no affinity")
        self.block_ = b
        if N == 1:                                                      # (one row: one cluster, nothing to embed)
            self.labels_, self.maps_ = np.zeros(1, dtype=np.int64), np.ones((1, 1), dtype=np.float32)
            self.eigenvalues_, self.residuals_, self.n_iter_ = np.zeros(1), [], 0
            return self
        x = x.to(device=self.device, dtype=torch.float32)
        vec, s, lam = self._embed(x, b)
        self.maps_ = spectral_sign_flip((vec * s[:, None]).cpu().numpy())
        self.eigenvalues_ = np.asarray(lam, dtype=np.float64)
        km = KMeans(self.n_clusters, n_init=self.n_init, random_state=self.random_state, device=self.device)
        self.labels_ = km.fit_predict(self.maps_).astype(np.int64)
        return self

    def fit_predict(self, x):
        return self.fit(x).labels_


def spectral_cluster_map(phrase_to_emb: Mapping[str, np.ndarray], n_clusters: int, seed=0, device=None):
    """The reference's ``Spectral().spectral_sklearn`` on a {phrase: embedding} table -> {"model": the fitted SpectralClustering,
    "result": {str(label): [phrases ...]} with the keys in order of first appearance}."""
    phrases = list(phrase_to_emb)
    embs = np.stack([np.asarray(phrase_to_emb[p], dtype=np.float32).reshape(-1) for p in phrases])
    model = SpectralClustering(n_clusters, random_state=seed, device=device)
    labels = model.fit_predict(embs)
    return {"model": model, "result": cluster_map_from_labels(phrases, labels)}
