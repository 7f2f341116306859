"""k-means, DBSCAN and average-linkage clustering over phrase embeddings on the device: what python_scripts/clustering/kmeans_emb.py,
dbscan_emb.py and agc_emb.py of the reference do with sklearn on the host.  ``DBSCAN`` / ``dbscan_cluster_map`` (csrc/dbscan.hip) are described at the class; their
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
