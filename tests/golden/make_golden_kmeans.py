#!/usr/bin/env python3
"""tests/golden/kmeans.npz + tests/golden/kmeans/*.json: what the REFERENCE's own code (imported through ref_import) makes of
the multi_phrase fixtures --

* clustering: ``KmeansClustering().kmeans`` of python_scripts/clustering/kmeans_emb.py (sklearn KMeans, ``np.random.seed(0)`` set
  before each call) on sim40_emb.pkl with 4 and with 7 clusters and on phrase_emb.pkl with 5: the centres, ``labels_``,
  ``inertia_``, ``predict(embs)``, ``transform(embs).min(1)`` in kmeans.npz and the ``result`` dict in kmeans/<case>_result.json.
  The generator asserts that sklearn converged strictly (the centres are the means of ``labels_``) and that no row lies inside
  the gap of tests/kmeans_ref.py under the recorded centres (the smallest margin is at least ten times the gap width).
* datasets: ``KmeansMappingDataset`` (weak and strong, ``max_dist_percent=80``, one pass with a crop under ``random.seed``) and
  ``KmeansMappingEvalDataset`` of datasets/class_mapping_dataset.py on kmeans/mapping_label.json (4 clips, 13 distinct phrases
  out of phrase_emb.pkl's 33) with the 5-cluster model, stored through joblib in a temporary directory.  h5py is not installed:
  the module's ``read_from_h5`` is replaced by a function over the fixture's arrays (``wave/<audio_id>`` in kmeans.npz).  It
  asserts that no phrase's distance lies within 1e-4 relative of the percentile.

Only recorded data is committed.  The generator needs the reference checkout (ref_import.REF), sklearn, joblib and pandas."""
import json
import os
import pickle
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
FIX = os.path.join(HERE, "multi_phrase")
OUT = os.path.join(HERE, "kmeans")

CASES = [("sim40_k4", "sim40_emb.pkl", 4), ("sim40_k7", "sim40_emb.pkl", 7), ("phrase_k5", "phrase_emb.pkl", 5)]
DATASET_CASE = "phrase_k5"
SR, RES = 100, 0.1
MAX_DIST_PERCENT = 80
CROP_S, CROP_SEED = 1.0, 3


def table(name):
    with open(os.path.join(FIX, name), "rb") as f:
        emb = pickle.load(f)
    return list(emb), np.stack([emb[p] for p in emb])


def mapping_label():
    phrases, _ = table("phrase_emb.pkl")
    g = np.random.RandomState(21)
    picked = [phrases[i] for i in g.choice(len(phrases), size=13, replace=False)]
    clips, at = [], 0
    for c, n in enumerate((4, 3, 5, 4)):                        # 16 entries over 13 distinct phrases: three repeat
        items = []
        for j in range(n):
            start = round(float(g.uniform(0.0, 0.6)), 2)
            segs = [[start, round(start + float(g.uniform(0.15, 0.5)), 2)]]
            if j == 0:
                segs.append([0.9, 1.2])
            items.append({"phrase": picked[at % 13], "start_index": 2 * j, "end_index": 2 * j + 2, "segments": segs})
            at += 1
        clips.append({"audio_id": f"K{c}.wav", "audiocap_id": 500 + c, "tokens": " ".join(i["phrase"] for i in items), "phrases": items})
    return clips


def mapping_clips():
    g = np.random.RandomState(22)
    return [(f"K{c}.wav", (0.3 * g.randn(n)).astype(np.float16)) for c, n in enumerate((150, 173, 240, 90))]


def load_ref(name):
    import importlib.util
    import ref_import
    spec = importlib.util.spec_from_file_location("ref_" + name.replace("/", "_"), os.path.join(ref_import.REF, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plain(item):
    return {k: (np.asarray(v) if isinstance(v, (np.ndarray, np.generic)) else v) for k, v in item.items()}


if __name__ == "__main__":
    import joblib
    import ref_import
    from tests import kmeans_ref as R
    ref_import.install()
    os.makedirs(OUT, exist_ok=True)
    out = {}
    models = {}
    km = load_ref("python_scripts/clustering/kmeans_emb")
    for case, pkl, K in CASES:
        phrases, embs = table(pkl)
        np.random.seed(0)
        res = km.KmeansClustering().kmeans(os.path.join(FIX, pkl), n_clusters=K)
        clf = res["model"]
        labels = np.asarray(clf.labels_)
        means = np.stack([embs[labels == k].astype(np.float64).mean(0) for k in range(K)])
        assert np.abs(clf.cluster_centers_ - means).max() <= 1e-6, "sklearn did not stop on the means of labels_"
        ref_labels, _, margin = R.assign_ref(embs, clf.cluster_centers_)
        rel = (margin / (R.gap_width(embs, clf.cluster_centers_) / R.GAP)).min()
        assert np.array_equal(ref_labels, labels) and rel >= 10 * R.GAP, (case, rel)
        assert np.array_equal(clf.predict(embs), labels)
        out[f"{case}/centers"] = np.asarray(clf.cluster_centers_, dtype=np.float32)
        out[f"{case}/labels"] = labels.astype(np.int32)
        out[f"{case}/inertia"] = np.float64(clf.inertia_)
        out[f"{case}/predict"] = np.asarray(clf.predict(embs), dtype=np.int32)
        out[f"{case}/min_dist"] = np.asarray(clf.transform(embs).min(1), dtype=np.float64)
        with open(os.path.join(OUT, f"{case}_result.json"), "w") as f:
            json.dump(res["result"], f, indent=1)
        models[case] = clf
        print(f"{case}: inertia {clf.inertia_:.4f}, iterations {clf.n_iter_}, smallest relative margin {rel:.3g}")

    label = mapping_label()
    with open(os.path.join(OUT, "mapping_label.json"), "w") as f:
        json.dump(label, f, indent=1)
    clips = dict(mapping_clips())
    for aid, w in clips.items():
        out[f"wave/{aid}"] = w
    ds_mod = load_ref("datasets/class_mapping_dataset")
    ds_mod.read_from_h5 = lambda key, key_to_h5, cache: clips[key]
    with tempfile.TemporaryDirectory() as tmp:
        jbl = os.path.join(tmp, "model.jbl")
        joblib.dump(models[DATASET_CASE], jbl)
        tsv = os.path.join(tmp, "wave.csv")
        with open(tsv, "w") as f:
            f.write("audio_id\thdf5_path\n" + "".join(f"{aid}\tnone.h5\n" for aid in clips))
        common = dict(waveform=tsv, label=os.path.join(OUT, "mapping_label.json"), phrase_embed=os.path.join(FIX, "phrase_emb.pkl"),
                      cluster_model=jbl)
        for label_type in ("weak", "strong"):
            ds = ds_mod.KmeansMappingDataset(label_type=label_type, max_dist_percent=MAX_DIST_PERCENT, time_resolution=RES,
                                             sample_rate=SR, **common)
            dist = np.array(list(ds.phrase_to_distance.values()), dtype=np.float64)
            assert len(dist) == 13 and (np.abs(dist - ds.max_distance) > 1e-4 * ds.max_distance).all(), "a distance is at the percentile"
            assert 0 < (dist <= ds.max_distance).sum() < len(dist)
            out[f"{label_type}/max_distance"] = np.float64(ds.max_distance)
            assert ds.classes_num == 5 and len(ds) == 4
            for i in range(len(ds)):
                item = plain(ds[i])
                assert item["audiocap_id"] == label[i]["audiocap_id"] and item["text"] == label[i]["tokens"]
                assert np.array_equal(item["waveform"], clips[item["audio_id"]].astype(np.float32))
                for k in ("label", "weak_label", "strong_label"):
                    if k in item:
                        out[f"{label_type}/{i}/{k}"] = item[k]
        ds = ds_mod.KmeansMappingDataset(label_type="strong", max_dist_percent=MAX_DIST_PERCENT, time_resolution=RES, sample_rate=SR,
                                         max_audio_length=CROP_S, **common)
        random.seed(CROP_SEED)
        for i in range(len(ds)):
            item = plain(ds[i])
            out[f"crop/{i}/waveform"] = item["waveform"]
            out[f"crop/{i}/strong_label"] = item["strong_label"]
        ds = ds_mod.KmeansMappingDataset(label_type="weak", max_dist_percent=MAX_DIST_PERCENT, sample_rate=SR, no_waveform=True,
                                         **common)
        assert "waveform" not in ds[0]
        ev = ds_mod.KmeansMappingEvalDataset(**common)
        assert len(ev) == 16
        out["eval/text_idx"] = np.array([int(ev[i]["text_idx"]) for i in range(len(ev))], dtype=np.int32)
        out["eval/start_index"] = np.array([int(ev[i]["start_index"]) for i in range(len(ev))], dtype=np.int32)
        out["eval/end_index"] = np.array([int(ev[i]["end_index"]) for i in range(len(ev))], dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "kmeans.npz"), **out)
    print("wrote", os.path.join(HERE, "kmeans.npz"), os.path.getsize(os.path.join(HERE, "kmeans.npz")), sorted(os.listdir(OUT)))
