"""csrc/kmeans.hip and utils/phrase_cluster.py against the fp64 reference of tests/kmeans_ref.py and the recorded output of the
reference's sklearn path (tests/golden/make_golden_kmeans.py).  The single-step inputs keep every row outside the gap (see
kmeans_ref), so labels are compared for exact equality.

Row slices of tag_kmeans_update (kmeans.hip, make_uplan): a workgroup is one (32-column tile of d, group of KT 32-cluster tiles,
row slice) with KT = 1 for K <= 32, 2 for K <= 64, else 4; the launch wants 512 workgroups, so with units = ceil(D / 32) *
ceil(K / (32 KT)) the rows are cut into slices of rows_each = max(128, ceil(N / ceil(512 / units))) rows rounded up to a
multiple of 8, slices = ceil(N / rows_each), and ws = slices * K * (4 D + 4) bytes.  N = 257 at (K, D) = (5, 33) is the smallest
N with three slices (128 + 128 + 1 rows: the last one partial, and three of its four waves without a row)."""
import functools
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 300, 512), (33, 5, 5), (64, 32, 32), (65, 129, 33), (130, 257, 48), (257, 130, 512), (300, 7, 768),
          (128, 128, 64),       # whole tiles, whole chunks, aligned rows: the loaders without tail tests
          (1152, 256, 32),      # the same with 9 row blocks
          (3, 515, 40)]
THREE_SLICES = (257, 5, 33)
IDS = lambda s: "x".join(map(str, s))       # noqa: E731
GOLDEN_CASES = [("sim40_k4", "sim40_emb.pkl", 4), ("sim40_k7", "sim40_emb.pkl", 7), ("phrase_k5", "phrase_emb.pkl", 5)]


@functools.lru_cache(maxsize=None)
def inputs(N, K, D):
    x, c, rounds = R.build_inputs(N, K, D, seed=N + 7 * K + 31 * D)
    labels, dist2, margin = R.assign_ref(x, c)
    for a in (x, c, labels, dist2):
        a.setflags(write=False)
    return x, c, labels, dist2, rounds


def to_dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def update_bound(count, abs_sums):
    return np.maximum(count, 1)[:, None] * 2.0 ** -24 * abs_sums


def check_assign(label, dist2, want_label, want_dist2, D, tag):
    assert label.dtype == torch.int32 and dist2.dtype == torch.float32
    label, dist2 = label.cpu().numpy(), dist2.cpu().numpy().astype(np.float64)
    err = np.abs(dist2 - want_dist2) / np.maximum(want_dist2, 1e-300)
    print(f"{tag}: label mismatches {int((label != want_label).sum())}, dist2 rel err {err.max():.3g} (bound {(D + 4) * 2.0 ** -23:.3g})")
    assert np.array_equal(label, want_label)
    assert (np.abs(dist2 - want_dist2) <= (D + 4) * 2.0 ** -23 * want_dist2).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_assign_equals_fp64_reference(dev, shape):
    from texttoaudiogrounding_amd import ops
    N, K, D = shape
    x, c, want_label, want_dist2, rounds = inputs(N, K, D)
    label, dist2 = ops.kmeans_assign(to_dev(x, dev), to_dev(c, dev))
    check_assign(label, dist2, want_label, want_dist2, D, f"{shape} (re-draw rounds {rounds})")
    assert ops.query("tag_kmeans_assign_ws_bytes", N, K, D) == 4 * K


@pytest.mark.parametrize("K", [5, 129])
def test_padded_columns_never_win(dev, K):
    """Rows at and near the origin against far centres: every real score ||c||^2 - 2 x . c is positive, so a padded column that
    scored the 0 of a zero-filled centre would win."""
    from texttoaudiogrounding_amd import ops
    N, D = 70, 24
    g = np.random.RandomState(K)
    c = (4.0 * np.sign(g.randn(K, D)) + g.randn(K, D)).astype(np.float32)
    x = (1e-3 * g.randn(N, D)).astype(np.float32)
    x[0] = 0.0
    x[N // 2:] = (c[g.randint(K, size=N - N // 2)] * 0.05 + 1e-3 * g.randn(N - N // 2, D)).astype(np.float32)
    assert (R.scores64(x, c) > 0).all()
    want_label, want_dist2, _ = R.assign_ref(x, c)
    keep = ~R.inside_gap(x, c)
    keep[0] = False                               # the all-zero row scores ||c||^2: no gap is asked of it, only label < K
    assert keep.sum() >= N // 2
    label, dist2 = ops.kmeans_assign(to_dev(x, dev), to_dev(c, dev))
    label = label.cpu().numpy()
    assert label.min() >= 0 and label.max() < K
    assert np.array_equal(label[keep], want_label[keep])
    n0 = (c.astype(np.float64) ** 2).sum(1)
    assert n0[label[0]] <= n0.min() * (1 + 1e-5)


def test_ties_go_to_the_lowest_index(dev):
    """Exact copies of 20 centre rows k at k + 1 and k + 128 (another lane of the same wave, and the same lane one tile later):
    the scores are bit-identical, only the lowest index may appear."""
    from texttoaudiogrounding_amd import ops
    N, D, K = 600, 40, 280
    base = 7 * np.arange(20)
    first = np.setdiff1d(np.arange(K), np.concatenate([base + 1, base + 128]))
    x, cu, want_u, _, _ = inputs(N, len(first), D)               # gapped against the centres without their copies
    c = np.empty((K, D), dtype=np.float32)
    c[first] = cu
    c[base + 1] = c[base + 128] = c[base]
    want = first[want_u]
    tied = np.isin(want, base)
    assert tied.sum() >= 20
    label, _ = ops.kmeans_assign(to_dev(x, dev), to_dev(c, dev))
    label = label.cpu().numpy()
    print(f"ties: {int(tied.sum())} rows have a tied best centre, mismatches {int((label != want).sum())}")
    assert np.array_equal(label, want)


@pytest.mark.parametrize("D,pad", [(48, 4), (33, 3), (512, 8)])
def test_row_strides_larger_than_D(dev, D, pad):
    """Views of wider buffers whose padding holds NaN: a read past D turns scores, distances and sums into NaN."""
    from texttoaudiogrounding_amd import ops
    N, K = 65, 129
    x, c, want_label, want_dist2, _ = inputs(N, K, D)
    wx = torch.full((N, D + pad), float("nan"), device=dev)
    wc = torch.full((K, D + 2 * pad), float("nan"), device=dev)
    wx[:, :D] = to_dev(x, dev)
    wc[:, :D] = to_dev(c, dev)
    vx, vc = wx[:, :D], wc[:, :D]
    assert vx.stride(0) == D + pad and vc.stride(0) == D + 2 * pad
    label, dist2 = ops.kmeans_assign(vx, vc)
    check_assign(label, dist2, want_label, want_dist2, D, f"strided D = {D}")
    sums, count = ops.kmeans_update(vx, label, vc)
    want_sums, want_count, abs_sums = R.update_ref(x, want_label, K)
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert (np.abs(sums.cpu().numpy() - want_sums) <= update_bound(want_count, abs_sums)).all()
    assert torch.isnan(wc[:, D:]).all() and torch.isnan(wx[:, D:]).all()       # the padding was neither read into a sum nor written
    got_c = vc.cpu().numpy()
    live = want_count > 0
    assert np.isfinite(got_c[live]).all() and np.array_equal(got_c[~live], c[~live])
    pick = torch.tensor([N - 1], device=dev)
    closest = torch.empty(N, device=dev)
    ops.kmeans_seed_step(vx, pick, closest, first=True)
    want = ((x.astype(np.float64) - x[N - 1].astype(np.float64)) ** 2).sum(1)
    assert (np.abs(closest.cpu().numpy() - want) <= (D + 4) * 2.0 ** -23 * want).all()


@pytest.mark.parametrize("shape", SHAPES + [THREE_SLICES], ids=IDS)
def test_update_equals_fp64_reference(dev, shape):
    from texttoaudiogrounding_amd import ops
    N, K, D = shape
    x, c, labels, _, _ = inputs(N, K, D)
    labels = labels.copy()
    if K > 1:
        labels[labels == K - 1] = 0               # the last cluster is empty by construction
    want_sums, want_count, abs_sums = R.update_ref(x, labels, K)
    assert K == 1 or want_count[K - 1] == 0
    if shape == THREE_SLICES:
        assert ops.query("tag_kmeans_update_ws_bytes", N, K, D) == 3 * K * (4 * D + 4)
    centers = torch.full((K, D), float("nan"), device=dev)
    sums, count = ops.kmeans_update(to_dev(x, dev), to_dev(labels, dev), centers)
    assert sums.dtype == torch.float64 and count.dtype == torch.int64 and tuple(sums.shape) == (K, D)
    sums, count, centers = sums.cpu().numpy(), count.cpu().numpy(), centers.cpu().numpy()
    assert np.array_equal(count, want_count)
    bound = update_bound(want_count, abs_sums)
    err = np.abs(sums - want_sums)
    print(f"{shape}: largest sums error over its bound {np.max(err / np.maximum(bound, 1e-300)):.3g}, empty clusters "
          f"{int((want_count == 0).sum())}")
    assert (err <= bound).all()
    live = want_count > 0
    quot = sums[live] / want_count[live, None]
    assert (np.abs(centers[live] - quot) <= 2.0 ** -23 * np.abs(quot)).all()
    assert np.isnan(centers[~live]).all()         # a cluster without rows keeps the NaN it was given


def test_two_calls_give_the_same_bits(dev):
    from texttoaudiogrounding_amd import ops
    N, K, D = 1152, 256, 32
    x, c, labels, _, _ = inputs(N, K, D)
    tx, tc = to_dev(x, dev), to_dev(c, dev)
    a, b = ops.kmeans_assign(tx, tc), ops.kmeans_assign(tx, tc)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    c1, c2 = tc.clone(), tc.clone()
    u, v = ops.kmeans_update(tx, a[0], c1), ops.kmeans_update(tx, a[0], c2)
    assert torch.equal(u[0].view(torch.int64), v[0].view(torch.int64)) and torch.equal(u[1], v[1])
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32))


def test_seed_step_first_and_min(dev):
    from texttoaudiogrounding_amd import ops
    N, D = 131, 33
    x = R.build_inputs(N, 5, D, seed=2)[0]
    x64 = x.astype(np.float64)
    tx = to_dev(x, dev)
    closest = torch.full((N,), float("nan"), device=dev)
    ops.kmeans_seed_step(tx, torch.tensor([7], device=dev), closest, first=True)
    d7, d90 = ((x64 - x64[7]) ** 2).sum(1), ((x64 - x64[90]) ** 2).sum(1)
    got = closest.cpu().numpy()
    assert got[7] == 0.0 and (np.abs(got - d7) <= (D + 4) * 2.0 ** -23 * d7).all()
    ops.kmeans_seed_step(tx, torch.tensor([90], device=dev), closest)
    got2 = closest.cpu().numpy()
    want = np.minimum(d7, d90)
    assert got2[90] == 0.0 and (np.abs(got2 - want) <= (D + 4) * 2.0 ** -23 * want).all()
    assert (got2 <= got).all()


def test_errors_are_reported_before_any_launch(dev):
    from texttoaudiogrounding_amd import lib, ops
    x = torch.zeros(4, 8, device=dev)
    lab, d2 = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, device=dev)
    sums, cnt = torch.zeros(4, 8, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    ws = torch.zeros(4096, device=dev)
    p = lib.ptr
    with pytest.raises(RuntimeError, match=r"row strides ldx = 4, ldc = 8 must be >= D = 8"):
        lib.call("tag_kmeans_assign", p(x), 4, p(x), 8, p(lab), p(d2), 4, 4, 8, p(ws))
    with pytest.raises(RuntimeError, match=r"must be >= 1 \(got 4, 0, 8\)"):
        lib.call("tag_kmeans_assign", p(x), 8, p(x), 8, p(lab), p(d2), 4, 0, 8, p(ws))
    with pytest.raises(RuntimeError, match=r"N = 2147483647 exceeds 2147483519"):
        lib.call("tag_kmeans_assign", p(x), 8, p(x), 8, p(lab), p(d2), 2**31 - 1, 4, 8, p(ws))
    with pytest.raises(RuntimeError, match=r"row strides ldx = 8, ldc = 7 must be >= D = 8"):
        lib.call("tag_kmeans_update", p(x), 8, p(lab), p(sums), p(cnt), p(x), 7, 4, 4, 8, p(ws))
    with pytest.raises(RuntimeError, match=r"must be >= 1 \(got 0, 4, 8\)"):
        lib.call("tag_kmeans_update", p(x), 8, p(lab), p(sums), p(cnt), p(x), 8, 0, 4, 8, p(ws))
    with pytest.raises(RuntimeError, match=r"row stride ldx = 3 must be >= D = 8"):
        lib.call("tag_kmeans_seed_step", p(x), 3, p(cnt), p(d2), 1, 4, 8)
    with pytest.raises(RuntimeError, match=r"must be >= 1"):
        lib.call("tag_kmeans_seed_step", p(x), 8, p(cnt), p(d2), 1, 4, 0)
    with pytest.raises(RuntimeError, match="argument check failed"):
        lib.call("tag_kmeans_assign", p(x), 8, p(x), 8, None, p(d2), 4, 4, 8, p(ws))
    for name in ("tag_kmeans_assign_ws_bytes", "tag_kmeans_update_ws_bytes"):
        assert ops.query(name, 0, 4, 8) == 0 and ops.query(name, 4, 0, 8) == 0 and ops.query(name, 4, 4, 0) == 0
        assert ops.query(name, 4, 4, 8) > 0
    # the wrappers
    with pytest.raises(RuntimeError, match="expected x's device"):
        ops.kmeans_assign(x, torch.zeros(4, 9, device=dev))
    with pytest.raises(RuntimeError, match="expected a float32 matrix"):
        ops.kmeans_assign(x.double(), x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans_assign(x, x.cpu())
    with pytest.raises(RuntimeError, match=r"label: expected torch.int32 \(4,\)"):
        ops.kmeans_update(x, lab.long(), x.clone())
    with pytest.raises(RuntimeError, match=r"label: values must lie in \[0, 4\), got min 0, max 4"):
        ops.kmeans_update(x, torch.tensor([0, 1, 4, 2], dtype=torch.int32, device=dev), x.clone())
    with pytest.raises(RuntimeError, match=r"label: values must lie in \[0, 4\), got min -1, max 2"):
        ops.kmeans_update(x, torch.tensor([0, 1, -1, 2], dtype=torch.int32, device=dev), x.clone())
    with pytest.raises(RuntimeError, match="centers: expected a float32"):
        ops.kmeans_update(x, lab, torch.zeros(4, 9, device=dev))
    with pytest.raises(RuntimeError, match="pick: expected one int64"):
        ops.kmeans_seed_step(x, torch.zeros(1, dtype=torch.int32, device=dev), d2)
    with pytest.raises(RuntimeError, match="closest: expected contiguous float32"):
        ops.kmeans_seed_step(x, torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(5, device=dev))
    from texttoaudiogrounding_amd.utils.phrase_cluster import KMeans
    with pytest.raises(ValueError, match="n_samples=4 should be >= n_clusters=5"):
        KMeans(5, device=dev).fit(x)


# ---- the reference's sklearn path ----

@functools.lru_cache(maxsize=None)
def golden():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with np.load(os.path.join(d, "kmeans.npz")) as f:
        return {k: f[k] for k in f.files}


def table(golden_dir, name):
    with open(os.path.join(golden_dir, "multi_phrase", name), "rb") as f:
        emb = pickle.load(f)
    return emb, np.stack([emb[p] for p in emb])


@pytest.mark.parametrize("case,pkl,K", GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_reference_golden(dev, golden_dir, tmp_path, case, pkl, K):
    from texttoaudiogrounding_amd.datasets import AudioSamplePhrasesDataset, write_waveform_pack
    from texttoaudiogrounding_amd.utils.phrase_cluster import KMeans, kmeans_cluster_map
    G = golden()
    emb, X = table(golden_dir, pkl)
    centers, labels = G[f"{case}/centers"], G[f"{case}/labels"]
    km = KMeans.from_centers(centers, device=dev)
    assert np.array_equal(km.predict(X), G[f"{case}/predict"])
    assert np.allclose(km.min_distance(X), G[f"{case}/min_dist"], rtol=1e-5, atol=0)
    full = km.transform(X)
    assert full.shape == (X.shape[0], K) and np.allclose(full.min(1), G[f"{case}/min_dist"], rtol=1e-4, atol=1e-5)
    fit = KMeans(K, init=centers, device=dev).fit(X)
    assert np.array_equal(fit.labels_, labels) and fit.labels_.dtype == np.int32
    assert np.abs(fit.cluster_centers_ - centers).max() <= 1e-5 * np.abs(X).max()
    assert abs(fit.inertia_ - float(G[f"{case}/inertia"])) <= 1e-5 * float(G[f"{case}/inertia"])
    print(f"{case}: n_iter {fit.n_iter_}, inertia {fit.inertia_:.6f} (recorded {float(G[f'{case}/inertia']):.6f})")
    with open(os.path.join(golden_dir, "kmeans", f"{case}_result.json")) as f:
        want = json.load(f)
    res = kmeans_cluster_map(emb, K, init=centers, device=dev)
    assert res["result"] == want and list(res["result"]) == list(want)
    assert res["score"] == fit.inertia_ and res["model"].n_clusters == K
    if pkl == "phrase_emb.pkl":
        # the map feeds the clustering strategy of the weak-phrase dataset
        with open(tmp_path / "map.json", "w") as f:
            json.dump(res["result"], f, indent=2)
        with open(os.path.join(golden_dir, "multi_phrase", "label.json")) as f:
            clips = json.load(f)
        g = np.random.RandomState(5)
        tsv = write_waveform_pack(str(tmp_path / "pack.npz"), [(c["audio_id"], 0.1 * g.randn(200)) for c in clips])
        ds = AudioSamplePhrasesDataset(tsv, os.path.join(golden_dir, "multi_phrase", "label.json"), 3, False,
                                       neg_samp_stratg="clustering", cluster_map=str(tmp_path / "map.json"), sample_rate=100)
        np.random.seed(1)
        item = ds[0]
        assert len(item["phrases"]) == 3 and item["waveform"].dtype == np.float32 and sum(item["label"]) >= 1


@pytest.mark.parametrize("shape", [(300, 5, 33), (515, 257, 40)], ids=IDS)
def test_fit_on_planted_blobs(dev, shape):
    from texttoaudiogrounding_amd.utils.phrase_cluster import KMeans
    N, K, D = shape
    x, planted, init = R.blobs(N, K, D, seed=K)
    ref = R.lloyd_ref(x, init)
    assert np.array_equal(ref["labels"], planted) and ref["n_iter"] == 2 and ref["strict"]
    km = KMeans(K, init=init, device=dev).fit(x)
    assert np.array_equal(km.labels_, planted) and km.n_iter_ == 2
    sums, count, abs_sums = R.update_ref(x, planted, K)
    means = sums / count[:, None]
    bound = update_bound(count, abs_sums) / count[:, None] + 2.0 ** -23 * np.abs(means)
    assert (np.abs(km.cluster_centers_ - means) <= bound).all()
    assert abs(km.inertia_ - ref["inertia"]) <= 1e-5 * ref["inertia"]
    # save / load keep the model
    assert np.array_equal(KMeans.from_centers(km.cluster_centers_, device=dev).predict(x), planted)


def test_empty_cluster_takes_the_farthest_row(dev):
    """Four blobs, three blob points and one point far from all data as the init: the fourth cluster is empty after the first
    assignment and takes the row with the largest dist2; the fit ends in the planted partition, as lloyd_ref does."""
    from texttoaudiogrounding_amd.utils.phrase_cluster import KMeans
    N, K, D = 200, 4, 33
    x, planted, init = R.blobs(N, K, D, seed=11)
    init = init.copy()
    init[3] = 50.0
    ref = R.lloyd_ref(x, init)
    assert ref["relocations"] >= 1

    def same_partition(labels):
        pairs = set(zip(labels.tolist(), planted.tolist()))
        return len(pairs) == K and len({a for a, _ in pairs}) == K

    assert same_partition(ref["labels"])
    km = KMeans(K, init=init, device=dev).fit(x)
    assert same_partition(km.labels_)
    assert np.array_equal(km.labels_, ref["labels"]) and km.n_iter_ == ref["n_iter"]
    assert abs(km.inertia_ - ref["inertia"]) <= 1e-5 * ref["inertia"]


def test_kmeanspp_picks_equal_the_fp64_restatement(dev):
    from texttoaudiogrounding_amd.utils.phrase_cluster import KMeans
    N, K, D = 300, 5, 33
    x, planted, _ = R.blobs(N, K, D, seed=K)
    seed = 4
    rs = np.random.RandomState(seed)
    first, u = int(rs.randint(N)), rs.random_sample(K - 1)
    want, rel = R.kmeanspp_ref(x, K, first, u)
    assert sorted(planted[want].tolist()) == list(range(K)), "re-seed: the restatement does not pick one row per blob"
    assert rel.min() > 1e-6, "re-seed: a drawn value lies at a prefix sum"
    km = KMeans(K, random_state=seed, device=dev)
    picks = km.seed_picks(to_dev(x, dev), np.random.RandomState(seed)).cpu().numpy()
    assert np.array_equal(picks, want)
    km.fit(x)
    assert len(set(zip(km.labels_.tolist(), planted.tolist()))) == K       # the planted partition, under some naming
    best = KMeans(K, random_state=seed, n_init=3, device=dev).fit(x)
    assert best.inertia_ <= km.inertia_


def test_fixed_point_on_unclustered_rows(dev):
    from texttoaudiogrounding_amd.utils.phrase_cluster import KMeans
    N, K, D = 4096, 64, 512
    g = np.random.RandomState(0)
    x = g.randn(N, D)
    x = (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float32)
    km = KMeans(K, random_state=0, device=dev).fit(x)
    c = km.cluster_centers_
    want, dist2, _ = R.assign_ref(x, c)
    inside = R.inside_gap(x, c)
    print(f"fixed point: n_iter {km.n_iter_}, inertia {km.inertia_:.4f}, rows inside the gap {int(inside.sum())} of {N}, "
          f"mismatches outside it {int((km.labels_ != want)[~inside].sum())}")
    assert inside.mean() <= 0.01
    assert np.array_equal(km.labels_[~inside], want[~inside])
    assert abs(km.inertia_ - ((x.astype(np.float64) - c[km.labels_]) ** 2).sum()) <= 1e-5 * km.inertia_
    sums, count, abs_sums = R.update_ref(x, km.labels_, K)
    assert (count > 0).all()
    means = sums / count[:, None]
    bound = update_bound(count, abs_sums) / count[:, None] + 2.0 ** -23 * np.abs(means)
    at_means = (np.abs(c - means) <= bound).all()
    shift = ((means - c) ** 2).sum()
    print(f"fixed point: centres at the means of labels_ {bool(at_means)}, sum ||means - c||^2 {shift:.3g}, tol "
          f"{1e-4 * x.astype(np.float64).var(0).mean():.3g}")
    assert at_means or shift <= 1e-4 * x.astype(np.float64).var(0).mean()


# ---- the class-mapping datasets ----

def test_kmeans_mapping_datasets_equal_the_reference(dev, golden_dir, tmp_path):
    import random
    from texttoaudiogrounding_amd.datasets import KmeansMappingDataset, KmeansMappingEvalDataset, write_waveform_pack
    from texttoaudiogrounding_amd.utils.phrase_cluster import KMeans
    G = golden()
    model = str(tmp_path / "model.npz")
    KMeans.from_centers(G["phrase_k5/centers"], device=dev).save(model)
    label = os.path.join(golden_dir, "kmeans", "mapping_label.json")
    with open(label) as f:
        clips = json.load(f)
    waves = {c["audio_id"]: G[f"wave/{c['audio_id']}"] for c in clips}
    tsv = write_waveform_pack(str(tmp_path / "pack.npz"), list(waves.items()))
    common = dict(waveform=tsv, label=label, phrase_embed=os.path.join(golden_dir, "multi_phrase", "phrase_emb.pkl"),
                  cluster_model=model, device=dev)
    for label_type, keys in (("weak", ("label",)), ("strong", ("weak_label", "strong_label"))):
        ds = KmeansMappingDataset(label_type=label_type, max_dist_percent=80, time_resolution=0.1, sample_rate=100, **common)
        assert ds.classes_num == 5 and len(ds) == len(clips)
        assert abs(ds.max_distance - float(G[f"{label_type}/max_distance"])) <= 1e-5 * float(G[f"{label_type}/max_distance"])
        for i, clip in enumerate(clips):
            item = ds[i]
            assert (item["audiocap_id"], item["audio_id"], item["text"]) == (clip["audiocap_id"], clip["audio_id"], clip["tokens"])
            assert item["waveform"].dtype == np.float32 and np.array_equal(item["waveform"], waves[clip["audio_id"]].astype(np.float32))
            for k in keys:
                assert item[k].dtype == np.float64 and np.array_equal(item[k], G[f"{label_type}/{i}/{k}"]), (label_type, i, k)
    ds = KmeansMappingDataset(label_type="strong", max_dist_percent=80, time_resolution=0.1, sample_rate=100, max_audio_length=1.0,
                              **common)
    random.seed(3)
    for i in range(len(clips)):
        item = ds[i]
        assert np.array_equal(item["waveform"], G[f"crop/{i}/waveform"]) and np.array_equal(item["strong_label"], G[f"crop/{i}/strong_label"])
    assert "waveform" not in KmeansMappingDataset(label_type="weak", max_dist_percent=80, sample_rate=100, no_waveform=True, **common)[0]
    ev = KmeansMappingEvalDataset(**common)
    assert ev.classes_num == 5 and len(ev) == len(G["eval/text_idx"])
    items = [ev[i] for i in range(len(ev))]
    assert [int(it["text_idx"]) for it in items] == G["eval/text_idx"].tolist()
    assert [it["start_index"] for it in items] == G["eval/start_index"].tolist()
    assert [it["end_index"] for it in items] == G["eval/end_index"].tolist()
    assert set(items[0]) == {"audiocap_id", "audio_id", "text", "waveform", "text_idx", "start_index", "end_index"}
