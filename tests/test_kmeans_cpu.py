"""CPU side of the device k-means: the helpers of utils/phrase_cluster.py that need no GPU, the model files, the fp64 reference
of tests/kmeans_ref.py against sklearn, and the build plumbing of csrc/kmeans.hip."""
import json
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from tests import kmeans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("sim40_k4", "sim40_emb.pkl", 4), ("sim40_k7", "sim40_emb.pkl", 7), ("phrase_k5", "phrase_emb.pkl", 5)]
SYMBOLS = ["tag_kmeans_assign_ws_bytes", "tag_kmeans_assign", "tag_kmeans_update_ws_bytes", "tag_kmeans_update",
           "tag_kmeans_seed_step"]


def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "kmeans.npz")) as f:
        return {k: f[k] for k in f.files}


def table(golden_dir, name):
    with open(os.path.join(golden_dir, "multi_phrase", name), "rb") as f:
        emb = pickle.load(f)
    return emb, np.stack([emb[p] for p in emb])


@pytest.mark.parametrize("case,pkl,K", CASES, ids=[c[0] for c in CASES])
def test_cluster_map_from_labels_equals_the_reference_result(golden_dir, case, pkl, K):
    from texttoaudiogrounding_amd.utils.phrase_cluster import cluster_map_from_labels
    emb, _ = table(golden_dir, pkl)
    with open(os.path.join(golden_dir, "kmeans", f"{case}_result.json")) as f:
        want = json.load(f)
    got = cluster_map_from_labels(list(emb), golden(golden_dir)[f"{case}/labels"])
    assert got == want and list(got) == list(want) and len(got) == K
    assert sorted(p for ps in got.values() for p in ps) == sorted(emb)


def test_save_load_round_trip(golden_dir, tmp_path):
    from texttoaudiogrounding_amd.utils.phrase_cluster import KMeans, load_cluster_centers
    centers = golden(golden_dir)["sim40_k7/centers"]
    km = KMeans(7, n_init=3, max_iter=50, tol=1e-3, random_state=9, device="cuda:0")
    with pytest.raises(RuntimeError, match="no centres yet"):
        km.save(str(tmp_path / "none.npz"))
    km.cluster_centers_, km.inertia_, km.n_iter_ = centers.copy(), 146.25, 3
    path = str(tmp_path / "model.npz")
    km.save(path)
    back = KMeans.load(path, device="cuda:0")
    assert np.array_equal(back.cluster_centers_, centers) and back.cluster_centers_.dtype == np.float32
    assert (back.n_clusters, back.n_init, back.max_iter, back.tol, back.random_state) == (7, 3, 50, 1e-3, 9)
    assert (back.inertia_, back.n_iter_) == (146.25, 3)
    assert np.array_equal(load_cluster_centers(path), centers)
    plain = KMeans.from_centers(centers)
    plain.save(str(tmp_path / "plain.npz"))
    back = KMeans.load(str(tmp_path / "plain.npz"))
    assert back.random_state is None and back.inertia_ is None and back.n_iter_ is None and back.n_clusters == 7


def test_load_cluster_centers_reads_a_joblib_checkpoint_of_sklearn(golden_dir, tmp_path):
    joblib = pytest.importorskip("joblib")
    cluster = pytest.importorskip("sklearn.cluster")
    from texttoaudiogrounding_amd.utils.phrase_cluster import load_cluster_centers
    _, X = table(golden_dir, "phrase_emb.pkl")
    clf = cluster.KMeans(n_clusters=5, n_init=1, random_state=0).fit(X)
    path = str(tmp_path / "5_score=173.jbl")
    joblib.dump(clf, path)
    got = load_cluster_centers(path)
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, clf.cluster_centers_.astype(np.float32))


def test_load_cluster_centers_without_joblib_names_it(tmp_path, monkeypatch):
    from texttoaudiogrounding_amd.utils.phrase_cluster import load_cluster_centers
    path = tmp_path / "model.jbl"
    path.write_bytes(b"not a checkpoint")
    monkeypatch.setitem(sys.modules, "joblib", None)             # ``import joblib`` raises ImportError
    with pytest.raises(RuntimeError, match="joblib is not importable"):
        load_cluster_centers(str(path))


def test_wrappers_refuse_cpu_tensors():
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils.phrase_cluster import KMeans
    x = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans_assign(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans_update(x, torch.zeros(4, dtype=torch.int32), x.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans_seed_step(x, torch.zeros(1, dtype=torch.int64), torch.zeros(4))
    with pytest.raises(ValueError, match="expected 'k-means\\+\\+'"):
        KMeans(3, init="random")
    with pytest.raises(RuntimeError, match="no centres yet"):
        KMeans(3)._centers()


@pytest.mark.parametrize("case,pkl,K", CASES, ids=[c[0] for c in CASES])
def test_lloyd_ref_agrees_with_sklearn(golden_dir, case, pkl, K):
    cluster = pytest.importorskip("sklearn.cluster")
    _, X = table(golden_dir, pkl)
    init = X[np.random.RandomState(K).choice(X.shape[0], size=K, replace=False)]
    clf = cluster.KMeans(n_clusters=K, init=init, n_init=1).fit(X.astype(np.float64))
    ref = R.lloyd_ref(X, init)
    assert np.array_equal(ref["labels"], clf.labels_) and ref["n_iter"] == clf.n_iter_
    assert np.allclose(ref["centers"], clf.cluster_centers_, rtol=0, atol=1e-9)
    assert abs(ref["inertia"] - clf.inertia_) <= 1e-9 * clf.inertia_
    # and from the recorded centres it stays where the reference's own run stopped
    G = golden(golden_dir)
    again = R.lloyd_ref(X, G[f"{case}/centers"])
    assert np.array_equal(again["labels"], G[f"{case}/labels"]) and abs(again["inertia"] - float(G[f"{case}/inertia"])) <= 1e-5 * again["inertia"]


def test_reference_helpers():
    x, c, rounds = R.build_inputs(65, 129, 33, seed=1)
    labels, dist2, margin = R.assign_ref(x, c)
    assert not R.inside_gap(x, c).any() and labels.dtype == np.int32 and (margin > 0).all()
    s = R.scores64(x, c)
    assert np.array_equal(labels, s.argmin(1)) and np.allclose(dist2, s.min(1) + (x.astype(np.float64) ** 2).sum(1))
    dup = np.concatenate([c[:3], c[:3]])
    assert np.array_equal(R.assign_ref(x, dup)[0], R.assign_ref(x, c[:3])[0])            # a tie goes to the lowest index
    sums, count, abs_sums = R.update_ref(x, labels, 129)
    assert count.sum() == 65 and np.allclose(sums.sum(0), x.astype(np.float64).sum(0)) and (abs_sums >= np.abs(sums) - 1e-12).all()


def test_kmeans_hip_is_built_and_declared():
    with open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "Makefile")) as f:
        srcs = re.search(r"^SRCS\s*=(.*)$", f.read(), flags=re.M).group(1).split()
    assert "kmeans.hip" in srcs
    with open(os.path.join(ROOT, "include", "tag_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    from texttoaudiogrounding_amd import lib
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in lib.declared_symbols()


def test_cli_accepts_the_reference_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kmeans_emb_tool", os.path.join(ROOT, "tools", "kmeans_emb.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.build_parser().parse_args(["--embedding", "e.pkl", "--n_cluster", "32", "--output", "exp/32.json"])
    assert (a.embedding, a.n_cluster, a.output, a.seed, a.n_init, a.device) == ("e.pkl", 32, "exp/32.json", None, 1, "cuda:0")
    a = tool.build_parser().parse_args(["-e", "e.pkl", "-nc", "256", "-o", "256.json", "--seed", "3", "--n_init", "4", "--device", "cuda:1"])
    assert (a.n_cluster, a.seed, a.n_init, a.device) == (256, 3, 4, "cuda:1")
    with pytest.raises(SystemExit):
        tool.build_parser().parse_args(["-e", "e.pkl"])
    m, n = tool.output_paths("exp/kmeans/32.json", 21137.4)
    assert (str(m), str(n)) == ("exp/kmeans/32_score=21137.json", "exp/kmeans/32_score=21137.npz")
