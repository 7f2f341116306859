"""csrc/dbscan.hip and utils/phrase_cluster.DBSCAN against the fp64 restatement of tests/dbscan_ref.py and the recorded output of
the reference's sklearn path (tests/golden/make_golden_dbscan.py).  The inputs keep every pair outside the gap (see dbscan_ref),
so adjacency bits, degrees, labels and core rows are compared for exact equality."""
import functools
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import dbscan_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (31, 5), (32, 5), (33, 5), (64, 32), (65, 33),
          (128, 64),            # whole tiles, whole chunks, aligned rows: the loader without tail tests
          (129, 48), (257, 512), (300, 768),
          (1152, 32)]           # the same loader with 9 row blocks
FIT_SHAPES = [s for s in SHAPES if s[0] >= 31]
CONTESTED_SEEDS = [0, 35, 52, 60]
TABLES = [("sim40", "sim40_emb.pkl"), ("phrase", "phrase_emb.pkl")]
PARAMS = [(0.5, 5), (0.3, 3), (0.2, 2)]
IDS = lambda s: "x".join(map(str, s))       # noqa: E731


@functools.lru_cache(maxsize=None)
def inputs(N, D):
    x, rounds = R.build_inputs(N, D, seed=N + 31 * D)
    ref = R.dbscan_ref(x, 0.5, 5)
    for a in (x, ref["adj"], ref["labels"], ref["core_sample_indices"], ref["degree"]):
        a.setflags(write=False)
    return x, ref, rounds


def to_dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def check_graph(adj, degree, want_adj, tag):
    N = want_adj.shape[0]
    W = 4 * ((N + 127) // 128)
    assert adj.dtype == torch.int32 and degree.dtype == torch.int32 and tuple(adj.shape) == (N, W) and tuple(degree.shape) == (N,)
    bits = R.unpack_bits(adj.cpu().numpy())
    print(f"{tag}: bit mismatches {int((bits[:, :N] != want_adj).sum())}, bits past N {int(bits[:, N:].sum())}, density "
          f"{want_adj.mean():.3f}")
    assert np.array_equal(bits[:, :N], want_adj)                   # every bit equals the fp64 adjacency
    assert not bits[:, N:].any()                                   # columns >= N and the words of the row padding are 0
    assert np.array_equal(degree.cpu().numpy(), want_adj.sum(1))
    assert np.array_equal(bits[:, :N], bits[:, :N].T)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_graph_equals_fp64_adjacency(dev, shape):
    from texttoaudiogrounding_amd import ops
    N, D = shape
    x, ref, rounds = inputs(N, D)
    adj, degree = ops.dbscan_graph(to_dev(x, dev), eps=0.5)
    check_graph(adj, degree, ref["adj"], f"{shape} (re-draw rounds {rounds})")
    assert ops.dbscan_words(N) == adj.shape[1]
    # the graph of rows taken as given: already-unit rows through normalize=False
    u = R.unit_rows(x).astype(np.float32)
    if not R.gap_pairs(u, 0.5).any() and np.array_equal(R.adjacency(u, 0.5), ref["adj"]):
        adj2, degree2 = ops.dbscan_graph(to_dev(u, dev), eps=0.5, normalize=False)
        check_graph(adj2, degree2, ref["adj"], f"{shape} unit rows as given")


@pytest.mark.parametrize("D,pad", [(48, 4), (33, 3), (512, 8)])
def test_row_strides_larger_than_D(dev, D, pad):
    """Views of wider buffers whose padding holds NaN: a read past D turns every score of the row into NaN (no neighbours)."""
    from texttoaudiogrounding_amd import ops
    N = {48: 129, 33: 65, 512: 257}[D]
    x, ref, _ = inputs(N, D)
    u = R.unit_rows(x).astype(np.float32)
    assert not R.gap_pairs(u, 0.5).any() and np.array_equal(R.adjacency(u, 0.5), ref["adj"])
    wide = torch.full((N, D + pad), float("nan"), device=dev)
    wide[:, :D] = to_dev(u, dev)
    view = wide[:, :D]
    assert view.stride(0) == D + pad
    adj, degree = ops.dbscan_graph(view, eps=0.5, normalize=False)     # (normalize=True would copy the view first)
    check_graph(adj, degree, ref["adj"], f"strided D = {D}")
    assert torch.isnan(wide[:, D:]).all() and torch.equal(wide[:, :D], to_dev(u, dev))       # the padding was neither read nor written
    adj, degree = ops.dbscan_graph(view, eps=0.5)
    check_graph(adj, degree, ref["adj"], f"strided D = {D}, normalised")


def test_two_calls_give_the_same_bits(dev):
    from texttoaudiogrounding_amd import ops
    x, ref, _ = inputs(1152, 32)
    tx = to_dev(x, dev)
    a, b = ops.dbscan_graph(tx), ops.dbscan_graph(tx)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    core = ops.dbscan_core(a[1], 5)
    f = torch.arange(1152, device=dev, dtype=torch.int32)
    outs = []
    for _ in range(2):
        g, changed = torch.full_like(f, -7), torch.full((1,), 9, device=dev, dtype=torch.int32)
        ops.dbscan_hook(a[0], core, f, g, changed)
        outs.append((g, changed))
    assert torch.equal(outs[0][0], outs[1][0]) and int(outs[0][1]) == int(outs[1][1]) == 1


def test_random_unit_rows_4096x512(dev):
    """Unstructured rows, eps = 0.9 (threshold 0.1, 2.3 sigma of a random cosine at D = 512: density 1.2 %): no gap-free
    construction at this size, so the bits are compared for every pair OUTSIDE the gap and the pairs inside it are counted (the
    fp64 reference alone puts 0.036 % of the pairs there)."""
    from texttoaudiogrounding_amd import ops
    N, D, eps = 4096, 512, 0.9
    x = np.random.RandomState(0).randn(N, D).astype(np.float32)
    c = R.cosines(x)
    want = c >= 1.0 - eps
    inside = np.abs(c - (1.0 - eps)) < R.GAP
    np.fill_diagonal(inside, False)
    adj, degree = ops.dbscan_graph(to_dev(x, dev), eps=eps)
    bits = R.unpack_bits(adj.cpu().numpy())[:, :N]
    wrong = bits != want
    print(f"density {want.mean():.4f}, pairs inside the gap {inside.mean():.5%}, mismatches outside the gap "
          f"{int((wrong & ~inside).sum())}, inside {int((wrong & inside).sum())}")
    assert inside.mean() <= 0.002
    assert not (wrong & ~inside).any()
    assert np.array_equal(degree.cpu().numpy(), bits.sum(1)) and np.array_equal(bits, bits.T)


# ---- core flags, one pass, roots ----

def test_core_hook_and_roots_step_by_step(dev):
    from texttoaudiogrounding_amd import ops
    N, D = 300, 768
    x, ref, _ = inputs(N, D)
    adj, degree = ops.dbscan_graph(to_dev(x, dev))
    core_bits = ops.dbscan_core(degree, 5)
    W = adj.shape[1]
    assert core_bits.dtype == torch.int32 and tuple(core_bits.shape) == (W,)
    core = R.unpack_bits(core_bits.cpu().numpy()[None, :])[0]
    want_core = ref["degree"] >= 5
    assert np.array_equal(core[:N], want_core) and not core[N:].any()
    # pass for pass against the restatement's loop
    cc = ref["adj"] & want_core[:, None] & want_core[None, :]
    src, dst = np.nonzero(cc)
    heads, starts = np.unique(src, return_index=True)
    f64 = np.arange(N, dtype=np.int64)
    f = torch.arange(N, device=dev, dtype=torch.int32)
    g, changed = torch.empty_like(f), torch.empty(1, device=dev, dtype=torch.int32)
    for _ in range(ref["n_passes"]):
        gf = f64[f64]
        new = np.minimum(f64, gf)
        m = np.minimum.reduceat(gf[dst], starts)
        np.minimum.at(new, f64[heads], m)
        new[heads] = np.minimum(new[heads], m)
        ops.dbscan_hook(adj, core_bits, f, g, changed)
        assert np.array_equal(g.cpu().numpy(), new) and int(changed) == int(not np.array_equal(new, f64))
        f64 = new
        f, g = g, f
    assert int(changed) == 0
    root = ops.dbscan_roots(adj, core_bits, f)
    assert root.dtype == torch.int32 and np.array_equal(root.cpu().numpy(), ref["root"])


# ---- fit ----

def check_fit(model, ref, tag):
    print(f"{tag}: clusters {ref['labels'].max() + 1}, noise {int((ref['labels'] < 0).sum())}, core {ref['core_sample_indices'].size}, "
          f"passes {model.n_passes_} (restatement {ref['n_passes']})")
    assert model.labels_.dtype == np.int64 and model.core_sample_indices_.dtype == np.int64
    assert np.array_equal(model.labels_, ref["labels"])
    assert np.array_equal(model.core_sample_indices_, ref["core_sample_indices"])
    assert model.n_passes_ == ref["n_passes"]


@pytest.mark.parametrize("shape", FIT_SHAPES, ids=IDS)
def test_fit_equals_the_restatement(dev, shape):
    from texttoaudiogrounding_amd.utils.phrase_cluster import DBSCAN
    x, ref, _ = inputs(*shape)
    check_fit(DBSCAN(device=dev).fit(x), ref, str(shape))


@pytest.mark.parametrize("seed", CONTESTED_SEEDS)
def test_fit_on_a_contested_border_row(dev, seed):
    from texttoaudiogrounding_amd.utils.phrase_cluster import DBSCAN
    x = np.random.RandomState(seed).randn(160, 3).astype(np.float32)
    assert not R.gap_pairs(x, 0.06).any()
    ref = R.dbscan_ref(x, 0.06, 5)
    core = np.zeros(160, dtype=bool)
    core[ref["core_sample_indices"]] = True
    assert any(not core[i] and len(set(ref["labels"][np.flatnonzero(ref["adj"][i] & core)])) > 1 for i in range(160))
    check_fit(DBSCAN(eps=0.06, min_samples=5, device=dev).fit(x), ref, f"seed {seed}")


def test_fit_all_noise_and_an_all_zero_row(dev):
    from texttoaudiogrounding_amd.utils.phrase_cluster import DBSCAN
    x, _, _ = inputs(65, 33)
    model = DBSCAN(min_samples=66, device=dev)
    labels = model.fit_predict(torch.from_numpy(np.array(x)))
    assert labels is model.labels_ and (labels == -1).all() and model.core_sample_indices_.size == 0 and model.n_passes_ == 1
    z = np.array(x)
    z[7] = 0.0
    assert not R.gap_pairs(z, 0.5).any()
    ref = R.dbscan_ref(z, 0.5, 5)
    assert ref["degree"][7] == 0
    model = DBSCAN(device=dev).fit(z)
    check_fit(model, ref, "zero row")
    assert model.labels_[7] == -1


@pytest.mark.parametrize("shuffled", [False, True], ids=["ordered", "shuffled"])
def test_fit_on_a_path_of_300(dev, shuffled):
    from texttoaudiogrounding_amd.utils.phrase_cluster import DBSCAN
    N = 300
    x = R.path_rows(N, np.random.RandomState(N).permutation(N) if shuffled else None)
    assert x.shape == (N, N + 2)
    ref = R.dbscan_ref(x, 0.5, 2)
    model = DBSCAN(eps=0.5, min_samples=2, device=dev).fit(x)
    print(f"path of {N} ({'shuffled' if shuffled else 'ordered'}): {model.n_passes_} passes (restatement {ref['n_passes']})")
    assert (model.labels_ == 0).all() and model.n_passes_ == ref["n_passes"] and model.n_passes_ <= 22
    assert np.array_equal(model.core_sample_indices_, np.arange(N))


# ---- the reference's sklearn path ----

@functools.lru_cache(maxsize=None)
def golden():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with np.load(os.path.join(d, "dbscan.npz")) as f:
        return {k: f[k] for k in f.files}


def table(golden_dir, name):
    with open(os.path.join(golden_dir, "multi_phrase", name), "rb") as f:
        emb = pickle.load(f)
    return emb, np.stack([emb[p] for p in emb])


@pytest.mark.parametrize("name,pkl", TABLES, ids=[t[0] for t in TABLES])
def test_reference_golden(dev, golden_dir, tmp_path, name, pkl):
    from texttoaudiogrounding_amd.datasets import AudioSamplePhrasesDataset, SpectralMappingDataset, write_waveform_pack
    from texttoaudiogrounding_amd.utils.phrase_cluster import DBSCAN, dbscan_cluster_map
    G = golden()
    emb, X = table(golden_dir, pkl)
    for eps, ms in PARAMS:
        model = DBSCAN(eps=eps, min_samples=ms, device=dev).fit(X)
        assert np.array_equal(model.labels_, G[f"{name}/{eps}_{ms}/labels"]), (eps, ms)
        assert np.array_equal(model.core_sample_indices_, G[f"{name}/{eps}_{ms}/core"]), (eps, ms)
    with open(os.path.join(golden_dir, "dbscan", f"{name}_result.json")) as f:
        want = json.load(f)
    res = dbscan_cluster_map(emb, device=dev)
    assert res["result"] == want and list(res["result"]) == list(want) and "-1" in res["result"]
    assert set(res) == {"result", "model"} and (res["model"].eps, res["model"].min_samples) == (0.5, 5)
    if pkl == "phrase_emb.pkl":
        # the map written to disk feeds the clustering strategy of the weak-phrase dataset and the cluster-map datasets
        with open(tmp_path / "map.json", "w") as f:
            json.dump(res["result"], f, indent=2)
        label = os.path.join(golden_dir, "multi_phrase", "label.json")
        with open(label) as f:
            clips = json.load(f)
        g = np.random.RandomState(5)
        tsv = write_waveform_pack(str(tmp_path / "pack.npz"), [(c["audio_id"], 0.1 * g.randn(200)) for c in clips])
        ds = AudioSamplePhrasesDataset(tsv, label, 3, False, neg_samp_stratg="clustering", cluster_map=str(tmp_path / "map.json"),
                                       sample_rate=100)
        np.random.seed(1)
        item = ds[0]
        assert len(item["phrases"]) == 3 and item["waveform"].dtype == np.float32 and sum(item["label"]) >= 1
        mlabel = os.path.join(golden_dir, "kmeans", "mapping_label.json")
        with open(mlabel) as f:
            mclips = json.load(f)
        with np.load(os.path.join(golden_dir, "kmeans.npz")) as f:
            waves = [(c["audio_id"], f[f"wave/{c['audio_id']}"]) for c in mclips]
        mtsv = write_waveform_pack(str(tmp_path / "mpack.npz"), waves)
        sm = SpectralMappingDataset(mtsv, mlabel, str(tmp_path / "map.json"), time_resolution=0.1, sample_rate=100)
        assert sm.classes_num == len(want) == int(G["weak/classes_num"])
        for i in range(len(mclips)):
            assert np.array_equal(sm[i]["label"], G[f"weak/{i}/label"])


# ---- errors ----

def test_errors_are_reported_before_any_launch(dev):
    from texttoaudiogrounding_amd import lib, ops
    x = torch.zeros(4, 8, device=dev)
    adj = torch.zeros(4, 4, dtype=torch.int32, device=dev)
    ints, other = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    p = lib.ptr
    with pytest.raises(RuntimeError, match=r"row stride ldx = 7 must be >= D = 8"):
        lib.call("tag_dbscan_graph", p(x), 7, 0.5, p(adj), p(ints), 4, 8)
    with pytest.raises(RuntimeError, match=r"N, D must be >= 1 \(got 0, 8\)"):
        lib.call("tag_dbscan_graph", p(x), 8, 0.5, p(adj), p(ints), 0, 8)
    with pytest.raises(RuntimeError, match=r"N, D must be >= 1 \(got 4, 0\)"):
        lib.call("tag_dbscan_graph", p(x), 8, 0.5, p(adj), p(ints), 4, 0)
    with pytest.raises(RuntimeError, match=r"tag_dbscan_graph: N = 2147483647 exceeds 2147483519"):
        lib.call("tag_dbscan_graph", p(x), 8, 0.5, p(adj), p(ints), 2**31 - 1, 8)
    with pytest.raises(RuntimeError, match="argument check failed"):
        lib.call("tag_dbscan_graph", p(x), 8, 0.5, None, p(ints), 4, 8)
    with pytest.raises(RuntimeError, match=r"tag_dbscan_core: N must be >= 1 \(got 0\)"):
        lib.call("tag_dbscan_core", p(ints), 5, p(ints), 0)
    with pytest.raises(RuntimeError, match="argument check failed"):
        lib.call("tag_dbscan_core", None, 5, p(ints), 4)
    with pytest.raises(RuntimeError, match=r"tag_dbscan_hook: N = 2147483520 exceeds 2147483519"):
        lib.call("tag_dbscan_hook", p(adj), p(ints), p(ints), p(other), p(one), 2**31 - 128)
    with pytest.raises(RuntimeError, match="argument check failed"):
        lib.call("tag_dbscan_hook", p(adj), p(ints), p(ints), p(ints), p(one), 4)        # f_out is f_in
    with pytest.raises(RuntimeError, match="argument check failed"):
        lib.call("tag_dbscan_hook", p(adj), p(ints), p(ints), p(other), None, 4)
    with pytest.raises(RuntimeError, match=r"tag_dbscan_roots: N must be >= 1 \(got -3\)"):
        lib.call("tag_dbscan_roots", p(adj), p(ints), p(ints), p(other), -3)
    with pytest.raises(RuntimeError, match="argument check failed"):
        lib.call("tag_dbscan_roots", p(adj), p(ints), None, p(other), 4)
    assert ops.query("tag_dbscan_words", 0) == 0 and ops.query("tag_dbscan_words", 2**31 - 128) == 0
    assert ops.query("tag_dbscan_words", 4) == 4
    # the wrappers
    with pytest.raises(RuntimeError, match="expected a float32 matrix"):
        ops.dbscan_graph(x.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dbscan_graph(x.cpu())
    with pytest.raises(ValueError, match=r"eps: expected a cosine distance in \(0, 2\], got 0.0"):
        ops.dbscan_graph(x, eps=0.0)
    with pytest.raises(RuntimeError, match=r"degree: expected contiguous int32 \(4,\)"):
        ops.dbscan_core(ints.long(), 5)
    with pytest.raises(RuntimeError, match=r"adj: expected contiguous int32 \(4, 4\)"):
        ops.dbscan_hook(torch.zeros(4, 5, dtype=torch.int32, device=dev), ints, ints, other, one)
    with pytest.raises(RuntimeError, match=r"core_bits: expected contiguous int32 \(4,\)"):
        ops.dbscan_hook(adj, torch.zeros(3, dtype=torch.int32, device=dev), ints, other, one)
    with pytest.raises(RuntimeError, match="f_out: expected a buffer other than f_in"):
        ops.dbscan_hook(adj, ints, ints, ints, one)
    with pytest.raises(RuntimeError, match=r"f_in: values must lie in \[0, 4\), got min 0, max 4"):
        ops.dbscan_hook(adj, ints, torch.tensor([0, 1, 4, 2], dtype=torch.int32, device=dev), other, one)
    with pytest.raises(RuntimeError, match=r"changed: expected contiguous int32 \(1,\)"):
        ops.dbscan_hook(adj, ints, ints, other, one.long())
    with pytest.raises(RuntimeError, match=r"f: expected contiguous int32 \(4,\)"):
        ops.dbscan_roots(adj, ints, ints.long())
    from texttoaudiogrounding_amd.utils.phrase_cluster import DBSCAN
    with pytest.raises(ValueError, match=r"x: expected a \(N >= 1, D >= 1\) matrix"):
        DBSCAN(device=dev).fit(np.zeros((0, 4), dtype=np.float32))
