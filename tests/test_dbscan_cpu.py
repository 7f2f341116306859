"""CPU side of the device DBSCAN: the fp64 restatement of tests/dbscan_ref.py against sklearn (through the reference's recipe)
and against the recorded goldens, its pass counts on path graphs, the SpectralMapping datasets against the recorded output of the
reference's classes, and the build plumbing of csrc/dbscan.hip."""
import json
import math
import os
import pickle
import random
import re

import numpy as np
import pytest
import torch

from tests import dbscan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (2, 3), (31, 5), (33, 5), (65, 33), (129, 48), (257, 512), (300, 768), (1152, 32), (2048, 64)]
CONTESTED_SEEDS = [0, 35, 52, 60]
TABLES = [("sim40", "sim40_emb.pkl"), ("phrase", "phrase_emb.pkl")]
PARAMS = [(0.5, 5), (0.3, 3), (0.2, 2)]
SYMBOLS = ["tag_dbscan_words", "tag_dbscan_graph", "tag_dbscan_core", "tag_dbscan_hook", "tag_dbscan_roots"]
IDS = lambda s: "x".join(map(str, s))       # noqa: E731


def sklearn_recipe(x, eps, min_samples):
    """dbscan_emb.py of the reference: DBSCAN(metric="precomputed") on (1 - cosine_similarity).clip(0)."""
    cluster = pytest.importorskip("sklearn.cluster")
    pairwise = pytest.importorskip("sklearn.metrics.pairwise")
    distances = (1 - pairwise.cosine_similarity(x, x)).clip(0.0)
    return cluster.DBSCAN(metric="precomputed", eps=eps, min_samples=min_samples).fit(distances)


def contested_input(seed):
    return np.random.RandomState(seed).randn(160, 3).astype(np.float32)


def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "dbscan.npz")) as f:
        return {k: f[k] for k in f.files}


def table(golden_dir, name):
    with open(os.path.join(golden_dir, "multi_phrase", name), "rb") as f:
        emb = pickle.load(f)
    return emb, np.stack([emb[p] for p in emb])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_restatement_equals_sklearn_on_the_builder_shapes(shape):
    N, D = shape
    x, rounds = R.build_inputs(N, D, seed=N + 31 * D)
    assert not R.gap_pairs(x, 0.5).any()
    ref = R.dbscan_ref(x, 0.5, 5)
    clf = sklearn_recipe(x, 0.5, 5)
    print(f"{shape}: re-draw rounds {rounds}, density {ref['adj'].mean():.3f}, clusters {ref['labels'].max() + 1}, noise "
          f"{int((ref['labels'] < 0).sum())}, passes {ref['n_passes']}")
    assert np.array_equal(ref["labels"], clf.labels_) and ref["labels"].dtype == np.int64
    assert np.array_equal(ref["core_sample_indices"], clf.core_sample_indices_)
    assert np.array_equal(R.unpack_bits(R.pack_bits(ref["adj"]))[:, :N], ref["adj"])


@pytest.mark.parametrize("seed", CONTESTED_SEEDS)
def test_a_contested_border_row_takes_the_lower_cluster(seed):
    x = contested_input(seed)
    eps, ms = 0.06, 5
    assert not R.gap_pairs(x, eps).any()
    ref = R.dbscan_ref(x, eps, ms)
    labels, adj = ref["labels"], ref["adj"]
    core = np.zeros(len(x), dtype=bool)
    core[ref["core_sample_indices"]] = True
    contested = [i for i in range(len(x)) if not core[i] and len(set(labels[np.flatnonzero(adj[i] & core)])) > 1]
    print(f"seed {seed}: contested border rows {contested}")
    assert contested
    for i in contested:
        assert labels[i] == labels[np.flatnonzero(adj[i] & core)].min()
    clf = sklearn_recipe(x, eps, ms)
    assert np.array_equal(labels, clf.labels_) and np.array_equal(ref["core_sample_indices"], clf.core_sample_indices_)


@pytest.mark.parametrize("shuffled", [False, True], ids=["ordered", "shuffled"])
def test_path_graph_is_one_cluster_in_few_passes(shuffled):
    N = 300
    perm = np.random.RandomState(N).permutation(N) if shuffled else None
    x = R.path_rows(N, perm)
    c = R.cosines(x)
    assert sorted(np.unique(np.round(c, 12))) == [0.0, round(1 / 3, 12), round(2 / 3, 12), 1.0]
    ref = R.dbscan_ref(x, 0.5, 2)
    assert (ref["degree"] >= 2).all() and ref["degree"].max() == 3
    bound = 2 * math.ceil(math.log2(N)) + 4
    print(f"path of {N} ({'shuffled' if shuffled else 'ordered'}): {ref['n_passes']} passes (bound {bound})")
    assert (ref["labels"] == 0).all() and ref["n_passes"] <= bound == 22
    src, dst = R.path_edges(N, perm)
    f, passes = R.fastsv(N, src, dst)
    assert passes == ref["n_passes"] and (f == 0).all()


@pytest.mark.parametrize("shuffled", [False, True], ids=["ordered", "shuffled"])
def test_path_of_2000_on_an_edge_list(shuffled):
    N = 2000
    perm = np.random.RandomState(N).permutation(N) if shuffled else None
    f, passes = R.fastsv(N, *R.path_edges(N, perm))
    bound = 2 * math.ceil(math.log2(N)) + 4
    print(f"path of {N} ({'shuffled' if shuffled else 'ordered'}): {passes} passes (bound {bound})")
    assert (f == 0).all() and passes <= bound == 26


def test_all_noise_and_an_all_zero_row():
    x, _ = R.build_inputs(65, 33, seed=3)
    ref = R.dbscan_ref(x, 0.5, 66)                  # min_samples > N
    assert (ref["labels"] == -1).all() and ref["core_sample_indices"].size == 0 and ref["n_passes"] == 1
    clf = sklearn_recipe(x, 0.5, 66)
    assert np.array_equal(ref["labels"], clf.labels_)
    x = x.copy()
    x[7] = 0.0
    ref = R.dbscan_ref(x, 0.5, 5)
    assert ref["degree"][7] == 0 and not ref["adj"][7].any() and not ref["adj"][:, 7].any() and ref["labels"][7] == -1
    clf = sklearn_recipe(x, 0.5, 5)
    assert np.array_equal(ref["labels"], clf.labels_) and np.array_equal(ref["core_sample_indices"], clf.core_sample_indices_)


@pytest.mark.parametrize("name,pkl", TABLES, ids=[t[0] for t in TABLES])
def test_recorded_goldens_equal_the_restatement(golden_dir, name, pkl):
    from texttoaudiogrounding_amd.utils.phrase_cluster import cluster_map_from_labels
    G = golden(golden_dir)
    emb, X = table(golden_dir, pkl)
    for eps, ms in PARAMS:
        assert not R.gap_pairs(X, eps).any()
        ref = R.dbscan_ref(X, eps, ms)
        assert np.array_equal(ref["labels"], G[f"{name}/{eps}_{ms}/labels"]), (eps, ms)
        assert np.array_equal(ref["core_sample_indices"], G[f"{name}/{eps}_{ms}/core"]), (eps, ms)
    with open(os.path.join(golden_dir, "dbscan", f"{name}_result.json")) as f:
        want = json.load(f)
    got = cluster_map_from_labels(list(emb), G[f"{name}/0.5_5/labels"])
    assert got == want and list(got) == list(want) and "-1" in got


def test_spectral_mapping_datasets_equal_the_reference(golden_dir, tmp_path):
    from texttoaudiogrounding_amd.datasets import SpectralMappingDataset, SpectralMappingEvalDataset, write_waveform_pack
    G = golden(golden_dir)
    with np.load(os.path.join(golden_dir, "kmeans.npz")) as f:
        K = {k: f[k] for k in f.files if k.startswith("wave/")}
    label = os.path.join(golden_dir, "kmeans", "mapping_label.json")
    cluster_map = os.path.join(golden_dir, "dbscan", "phrase_result.json")
    with open(label) as f:
        clips = json.load(f)
    with open(cluster_map) as f:
        cmap = json.load(f)
    assert "-1" in cmap                             # the noise key counts as a class and indexes the last column
    waves = {c["audio_id"]: K[f"wave/{c['audio_id']}"] for c in clips}
    tsv = write_waveform_pack(str(tmp_path / "pack.npz"), list(waves.items()))
    common = dict(waveform=tsv, label=label, cluster_map=cluster_map)
    for label_type, keys in (("weak", ("label",)), ("strong", ("weak_label", "strong_label"))):
        ds = SpectralMappingDataset(label_type=label_type, time_resolution=0.1, sample_rate=100, **common)
        assert ds.classes_num == len(cmap) == int(G[f"{label_type}/classes_num"]) and len(ds) == len(clips)
        for i, clip in enumerate(clips):
            item = ds[i]
            assert set(item) == {"audiocap_id", "audio_id", "text", "waveform", *keys}
            assert (item["audiocap_id"], item["audio_id"], item["text"]) == (clip["audiocap_id"], clip["audio_id"], clip["tokens"])
            assert item["waveform"].dtype == np.float32 and np.array_equal(item["waveform"], waves[clip["audio_id"]].astype(np.float32))
            for k in keys:
                assert item[k].dtype == np.float64 and np.array_equal(item[k], G[f"{label_type}/{i}/{k}"]), (label_type, i, k)
    ds = SpectralMappingDataset(label_type="strong", time_resolution=0.1, sample_rate=100, max_audio_length=1.0, **common)
    random.seed(3)
    for i in range(len(clips)):
        item = ds[i]
        assert np.array_equal(item["waveform"], G[f"crop/{i}/waveform"]) and np.array_equal(item["strong_label"], G[f"crop/{i}/strong_label"])
    item = SpectralMappingDataset(label_type="weak", sample_rate=100, no_waveform=True, **common)[0]
    assert set(item) == {"audiocap_id", "audio_id", "text", "label"} and np.array_equal(item["label"], G["no_waveform/0/label"])
    ev = SpectralMappingEvalDataset(**common)
    assert len(ev) == len(G["eval/text_idx"])
    items = [ev[i] for i in range(len(ev))]
    assert [it["text_idx"] for it in items] == G["eval/text_idx"].tolist() and all(type(it["text_idx"]) is int for it in items)
    assert -1 in G["eval/text_idx"]                 # a phrase of the noise key indexes class -1, as in the reference
    assert [it["start_index"] for it in items] == G["eval/start_index"].tolist()
    assert [it["end_index"] for it in items] == G["eval/end_index"].tolist()
    assert set(items[0]) == {"audiocap_id", "audio_id", "text", "waveform", "text_idx", "start_index", "end_index"}
    assert items[0]["waveform"].dtype == np.float32


def test_wrappers_refuse_cpu_tensors_and_bad_settings():
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils.phrase_cluster import DBSCAN
    x = torch.zeros(4, 8)
    ints = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dbscan_graph(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dbscan_core(ints, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dbscan_hook(torch.zeros(4, 4, dtype=torch.int32), ints, ints, ints.clone(), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dbscan_roots(torch.zeros(4, 4, dtype=torch.int32), ints, ints)
    for eps in (0.0, -0.1, 2.5):
        with pytest.raises(ValueError, match=r"eps: expected a cosine distance in \(0, 2\]"):
            ops.dbscan_graph(x, eps=eps)
        with pytest.raises(ValueError, match=r"eps: expected a cosine distance in \(0, 2\]"):
            DBSCAN(eps=eps)
    with pytest.raises(ValueError, match="min_samples must be >= 1"):
        DBSCAN(min_samples=0)
    assert ops.dbscan_words(1) == 4 and ops.dbscan_words(128) == 4 and ops.dbscan_words(129) == 8
    assert ops.query("tag_dbscan_words", 0) == 0 and ops.query("tag_dbscan_words", 2**31 - 128) == 0
    assert ops.query("tag_dbscan_words", 2**31 - 129) == 4 * (2**24 - 1)


def test_dbscan_hip_is_built_and_declared():
    with open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "Makefile")) as f:
        srcs = re.search(r"^SRCS\s*=(.*)$", f.read(), flags=re.M).group(1).split()
    assert "dbscan.hip" in srcs
    with open(os.path.join(ROOT, "include", "tag_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    from texttoaudiogrounding_amd import lib
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in lib.declared_symbols()


def test_cli_accepts_the_reference_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dbscan_emb_tool", os.path.join(ROOT, "tools", "dbscan_emb.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.build_parser().parse_args(["--embedding", "e.pkl", "--output", "exp/dbscan.json"])
    assert (a.embedding, a.output, a.eps, a.min_samples, a.device) == ("e.pkl", "exp/dbscan.json", 0.5, 5, "cuda:0")
    a = tool.build_parser().parse_args(["-e", "e.pkl", "-o", "d.json", "--eps", "0.3", "--min_samples", "3", "--device", "cuda:1"])
    assert (a.eps, a.min_samples, a.device) == (0.3, 3, "cuda:1")
    with pytest.raises(SystemExit):
        tool.build_parser().parse_args(["-e", "e.pkl"])
