"""CPU side of the device average-linkage clustering: the fp64 restatement of tests/agc_ref.py against the recorded output of the
reference's sklearn recipe (tests/golden/make_golden_agc.py) and against a dense Lance-Williams average linkage, the product's
host half (utils/phrase_cluster.agc_tree / agc_cut / labels_for) on the restatement's merge log, the recorded cluster maps, the
argument errors, and the build plumbing of csrc/agc.hip."""
import functools
import json
import os
import pickle
import re

import numpy as np
import pytest

from tests import agc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [("sim40", (2, 4, 7, 13)), ("phrase", (2, 3, 5)), ("blobs2000", (2, 8, 30))]
CASE_KS = [(name, k) for name, ks in CASES for k in ks]
JSON_CASES = [("sim40", "sim40_emb.pkl", 4), ("phrase", "phrase_emb.pkl", 3)]
SYMBOLS = ["tag_agc_nearest_ws_bytes", "tag_agc_nearest", "tag_agc_merge_ws_bytes", "tag_agc_merge"]


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLDEN, "agc.npz")) as f:
        out = {k: f[k] for k in f.files}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement of one recorded case, computed once and shared."""
    g = golden()
    return R.agc_ref(g[f"{name}/x"], dict(CASES)[name])


def table(name):
    with open(os.path.join(GOLDEN, "multi_phrase", name), "rb") as f:
        emb = pickle.load(f)
    return emb, np.stack([emb[p] for p in emb])


@pytest.mark.parametrize("name,k", CASE_KS)
def test_restatement_reproduces_the_recorded_labels(name, k):
    g = golden()
    assert np.array_equal(restated(name)["labels"][k], g[f"{name}/labels_k{k}"])
    D = g[f"{name}/x"].shape[1]
    assert g[f"{name}/gap_k{k}"] >= 100 * R.bound(D)              # the recorded cut is decided far above the fp32 error of a height


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_restatement_reproduces_the_recorded_heights(name):
    g = golden()
    ref = restated(name)
    err = np.abs(ref["distances"] - g[f"{name}/heights"]).max()
    print(f"{name}: {ref['rounds']} rounds, heights within {err:.3g} of scipy's")
    assert err <= 1e-12
    assert ref["rounds"] == {"sim40": 12, "phrase": 12, "blobs2000": 40}[name]


@pytest.mark.parametrize("name", ["sim40", "phrase"])
def test_rounds_build_the_tree_of_the_serial_lance_williams_linkage(name):
    """All reciprocal pairs of a round at once give the merges of the serial algorithm: the same leaf set per merge and the same
    heights (the tables have no tied heights)."""
    x = golden()[f"{name}/x"]
    u = R.unit_rows(x)
    heights, sets = R.lance_williams(1.0 - u @ u.T)
    ref = restated(name)
    assert np.all(np.diff(heights) > 0)
    assert np.abs(ref["distances"] - heights).max() <= 1e-12
    assert R.merge_sets(ref["children"], len(x)) == sets


def test_recorded_clustered_rows_are_the_stated_construction():
    rng = np.random.RandomState(0)
    c = rng.randn(30, 64)
    x = c[rng.randint(30, size=2000)] + 0.6 * rng.randn(2000, 64)
    assert np.array_equal(golden()["blobs2000/x"], x.astype(np.float32))


@pytest.mark.parametrize("name,k", CASE_KS)
def test_host_half_on_the_restatements_log_gives_the_recorded_labels(name, k):
    from texttoaudiogrounding_amd.utils.phrase_cluster import AgglomerativeClustering, agc_cut, agc_tree
    g = golden()
    ref = restated(name)
    h, a, b = ref["log"]
    N = g[f"{name}/x"].shape[0]
    children, distances = agc_tree(h, a, b, N)
    assert np.array_equal(children, ref["children"]) and np.array_equal(distances, ref["distances"])
    assert children.dtype == np.int64 and distances.dtype == np.float64 and np.all(children[:, 0] < children[:, 1])
    assert np.array_equal(agc_cut(children, N, k), g[f"{name}/labels_k{k}"])
    model = AgglomerativeClustering(k)._set_tree(h.astype(np.float32), a, b, N, ref["rounds"])      # (heights as the device logs them)
    assert np.array_equal(model.labels_, g[f"{name}/labels_k{k}"]) and model.labels_.dtype == np.int64
    assert (model.n_leaves_, model.n_rounds_) == (N, ref["rounds"])
    for other in dict(CASES)[name]:
        assert np.array_equal(model.labels_for(other), g[f"{name}/labels_k{other}"])
    assert np.array_equal(model.labels_for(1), np.zeros(N, dtype=np.int64))
    assert sorted(model.labels_for(N).tolist()) == list(range(N))


def test_host_half_keeps_children_before_parents_when_a_height_dips():
    """A parent whose rounded height falls below its child's still follows it."""
    from texttoaudiogrounding_amd.utils.phrase_cluster import agc_cut, agc_tree
    # leaves 0..3: (0, 1) at 0.5 -> node 4, (2, 3) at 0.2 -> node 5, (4, 5) at 0.4999999 -> node 6
    children, distances = agc_tree([0.5, 0.2, 0.4999999], [0, 2, 4], [1, 3, 5], 4)
    assert children.tolist() == [[2, 3], [0, 1], [4, 5]] and distances.tolist() == [0.2, 0.5, 0.5]
    assert agc_cut(children, 4, 2).tolist() in ([0, 0, 1, 1], [1, 1, 0, 0])
    assert agc_tree(np.zeros(0), [], [], 1)[0].shape == (0, 2) and agc_cut(np.zeros((0, 2)), 1, 1).tolist() == [0]


@pytest.mark.parametrize("case,pkl,k", JSON_CASES)
def test_cluster_map_of_the_recorded_labels_equals_the_recorded_json(case, pkl, k):
    from texttoaudiogrounding_amd.utils.phrase_cluster import cluster_map_from_labels
    emb, x = table(pkl)
    assert np.array_equal(np.asarray(x, dtype=np.float32), golden()[f"{case}/x"])
    with open(os.path.join(GOLDEN, "agc", f"{case}_k{k}_result.json")) as f:
        want = json.load(f)
    mine = cluster_map_from_labels(list(emb), golden()[f"{case}/labels_k{k}"])
    assert mine == want and list(mine) == list(want)


def test_constructor_and_argument_errors():
    from texttoaudiogrounding_amd.utils.phrase_cluster import AgglomerativeClustering, agc_cut, agc_tree
    for linkage in ("ward", "complete", "single", None):
        with pytest.raises(ValueError, match="only 'average'"):
            AgglomerativeClustering(3, linkage=linkage)
    with pytest.raises(ValueError, match="n_clusters must be >= 1"):
        AgglomerativeClustering(0)
    model = AgglomerativeClustering(3)
    assert (model.n_clusters, model.linkage, model.device, model.labels_) == (3, "average", "cuda:0", None)
    with pytest.raises(RuntimeError, match="no tree yet"):
        model.labels_for(2)
    with pytest.raises(ValueError, match="should be >= n_clusters"):
        AgglomerativeClustering(5)._set_tree([0.1, 0.2], [0, 3], [1, 2], 3, 2)
    with pytest.raises(ValueError, match="has 2 merges"):
        agc_tree([0.1], [0], [1], 3)
    with pytest.raises(ValueError, match="not a binary tree"):
        agc_tree([0.1, 0.2], [0, 0], [1, 2], 3)
    with pytest.raises(ValueError, match="out of order"):
        agc_tree([0.1, 0.2], [3, 0], [2, 1], 3)
    with pytest.raises(ValueError, match="expected 1 .. 3"):
        agc_cut([[0, 1], [2, 3]], 3, 4)
    with pytest.raises(ValueError, match="expected 1 .. 3"):
        agc_cut([[0, 1], [2, 3]], 3, 0)


def test_builder_keeps_every_nearest_neighbour_decided():
    for N, D in [(3, 3), (33, 5), (129, 48), (1152, 32)]:
        m, redraws = R.build_inputs(N, D, seed=N + 31 * D)
        nn, dist, gap = R.nearest_ref(m)
        assert m.dtype == np.float32 and gap.min() >= 4 * R.bound(D) and np.sqrt((m.astype(np.float64) ** 2).sum(1)).max() <= 1.0 + 1e-6
        assert np.array_equal(R.build_inputs(N, D, seed=N + 31 * D)[0], m)
        print(f"{N} x {D}: {redraws} re-draws, smallest gap {gap.min():.3g} against 4 x bound {4 * R.bound(D):.3g}")


def test_merge_restatement_on_a_hand_made_round():
    nn = np.array([1, 0, 3, 4, 3, 9, -1])                          # 0 <-> 1, 3 <-> 4, 2 -> 3 unanswered, 5 and 6 point nowhere
    sums = np.arange(14, dtype=np.float64).reshape(7, 2)
    r = R.merge_ref(nn, np.arange(7) / 10.0, sums, np.arange(1, 8), np.arange(10, 17), next_id=40)
    assert r["pairs"] == 2 and r["ids"].tolist() == [12, 15, 16, 40, 41] and r["sizes"].tolist() == [3, 6, 7, 3, 9]
    assert r["sums"].tolist() == [[4, 5], [10, 11], [12, 13], [2, 4], [14, 16]]
    assert r["log_dist"].tolist() == [0.0, 0.3] and r["log_ids"].tolist() == [[10, 11, 40], [13, 14, 41]]


def test_build_plumbing():
    from texttoaudiogrounding_amd import lib
    header = open(os.path.join(ROOT, "include", "tag_hip.h")).read()
    makefile = open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bagc\.hip\b", makefile, flags=re.M)
    for s in SYMBOLS:
        assert s in lib.declared_symbols() and re.search(rf"\b{s}\s*\(", header), s
    csrc = os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc")
    # agc.hip's products are the shared exact-fp32 MFMA march of march_f32.h: both files are held to the same rules
    code, march = (re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read()) for f in ("agc.hip", "march_f32.h"))
    assert "atomic" not in code + march and "cooperative" not in (code + march).lower()
    assert '#include "march_f32.h"' in code and re.search(r"\bmarch_tiles<", code)
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in march
    assert re.search(r"^HDRS = .*\bmarch_f32\.h\b", makefile, flags=re.M)
