#!/usr/bin/env python3
"""tests/golden/dbscan.npz + tests/golden/dbscan/*.json: what the REFERENCE's own code (imported through ref_import) and sklearn
make of the multi_phrase fixtures --

* clustering: ``Runner().dbscan`` of python_scripts/clustering/dbscan_emb.py (sklearn ``DBSCAN(metric="precomputed")`` at its
  defaults eps = 0.5, min_samples = 5 on ``(1 - cosine_similarity).clip(0)``) on sim40_emb.pkl and phrase_emb.pkl: the ``result``
  dicts in dbscan/<table>_result.json; and ``labels_`` / ``core_sample_indices_`` of the same sklearn call on the same clipped
  matrix at (eps, min_samples) = (0.5, 5), (0.3, 3) and (0.2, 2) in dbscan.npz (<table>/<eps>_<min_samples>/labels, .../core).
  The generator asserts that the (0.5, 5) labels give the reference's result dict, that the fp64 restatement of
  tests/dbscan_ref.py gives the same labels and core rows, and that no pair of either table lies inside the gap of dbscan_ref
  at any of the three eps (the smallest margins are printed).
* datasets: ``SpectralMappingDataset`` (weak, strong, one cropped pass under ``random.seed``, ``no_waveform``) and
  ``SpectralMappingEvalDataset`` of datasets/class_mapping_dataset.py on kmeans/mapping_label.json with the (0.5, 5) map of
  phrase_emb.pkl and the clips of make_golden_kmeans.py (``wave/<audio_id>`` in kmeans.npz).  h5py is not installed: the module's
  ``read_from_h5`` is replaced by a function over those arrays.

Only recorded data is committed.  The generator needs the reference checkout (ref_import.REF), sklearn and pandas."""
import json
import os
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
OUT = os.path.join(HERE, "dbscan")

TABLES = [("sim40", "sim40_emb.pkl"), ("phrase", "phrase_emb.pkl")]
PARAMS = [(0.5, 5), (0.3, 3), (0.2, 2)]
SR, RES = 100, 0.1
CROP_S, CROP_SEED = 1.0, 3


def case_key(table, eps, min_samples):
    return f"{table}/{eps}_{min_samples}"


if __name__ == "__main__":
    import ref_import
    from make_golden_kmeans import load_ref, mapping_clips, plain, table
    from sklearn.cluster import DBSCAN
    from sklearn.metrics.pairwise import cosine_similarity
    from tests import dbscan_ref as R
    ref_import.install()
    os.makedirs(OUT, exist_ok=True)
    out = {}
    db = load_ref("python_scripts/clustering/dbscan_emb")
    for name, pkl in TABLES:
        phrases, embs = table(pkl)
        res = db.Runner().dbscan(os.path.join(FIX, pkl))["result"]
        with open(os.path.join(OUT, f"{name}_result.json"), "w") as f:
            json.dump(res, f, indent=1)
        distances = (1 - cosine_similarity(embs, embs)).clip(0.0)
        for eps, ms in PARAMS:
            clf = DBSCAN(metric="precomputed", eps=eps, min_samples=ms).fit(distances)
            labels, core = np.asarray(clf.labels_, dtype=np.int64), np.asarray(clf.core_sample_indices_, dtype=np.int64)
            margin = np.abs(R.cosines(embs) - (1.0 - eps))
            np.fill_diagonal(margin, np.inf)
            assert not R.gap_pairs(embs, eps).any() and margin.min() >= R.GAP, (name, eps, margin.min())
            ref = R.dbscan_ref(embs, eps, ms)
            assert np.array_equal(ref["labels"], labels) and np.array_equal(ref["core_sample_indices"], core), (name, eps, ms)
            if (eps, ms) == PARAMS[0]:
                mine = {}
                for phrase, label in zip(phrases, labels):
                    mine.setdefault(str(int(label)), []).append(phrase)
                assert mine == res and list(mine) == list(res)
            out[case_key(name, eps, ms) + "/labels"] = labels
            out[case_key(name, eps, ms) + "/core"] = core
            print(f"{name} eps {eps} min_samples {ms}: {labels.max() + 1} clusters, {int((labels < 0).sum())} noise rows, "
                  f"{core.size} core rows, smallest margin {margin.min():.3g}")

    label_path = os.path.join(HERE, "kmeans", "mapping_label.json")
    with open(label_path) as f:
        label = json.load(f)
    clips = dict(mapping_clips())
    ds_mod = load_ref("datasets/class_mapping_dataset")
    ds_mod.read_from_h5 = lambda key, key_to_h5, cache: clips[key]
    with tempfile.TemporaryDirectory() as tmp:
        tsv = os.path.join(tmp, "wave.csv")
        with open(tsv, "w") as f:
            f.write("audio_id\thdf5_path\n" + "".join(f"{aid}\tnone.h5\n" for aid in clips))
        common = dict(waveform=tsv, label=label_path, cluster_map=os.path.join(OUT, "phrase_result.json"))
        with open(common["cluster_map"]) as f:
            n_keys = len(json.load(f))
        for label_type in ("weak", "strong"):
            ds = ds_mod.SpectralMappingDataset(label_type=label_type, time_resolution=RES, sample_rate=SR, **common)
            assert ds.classes_num == n_keys and len(ds) == len(label)
            out[f"{label_type}/classes_num"] = np.int64(ds.classes_num)
            for i in range(len(ds)):
                item = plain(ds[i])
                assert item["audiocap_id"] == label[i]["audiocap_id"] and item["text"] == label[i]["tokens"]
                assert np.array_equal(item["waveform"], clips[item["audio_id"]].astype(np.float32))
                for k in ("label", "weak_label", "strong_label"):
                    if k in item:
                        out[f"{label_type}/{i}/{k}"] = item[k]
        ds = ds_mod.SpectralMappingDataset(label_type="strong", time_resolution=RES, sample_rate=SR, max_audio_length=CROP_S, **common)
        random.seed(CROP_SEED)
        for i in range(len(ds)):
            item = plain(ds[i])
            out[f"crop/{i}/waveform"] = item["waveform"]
            out[f"crop/{i}/strong_label"] = item["strong_label"]
        ds = ds_mod.SpectralMappingDataset(label_type="weak", sample_rate=SR, no_waveform=True, **common)
        item = plain(ds[0])
        assert "waveform" not in item
        out["no_waveform/0/label"] = item["label"]
        ev = ds_mod.SpectralMappingEvalDataset(**common)
        assert len(ev) == 16
        out["eval/text_idx"] = np.array([int(ev[i]["text_idx"]) for i in range(len(ev))], dtype=np.int32)
        out["eval/start_index"] = np.array([int(ev[i]["start_index"]) for i in range(len(ev))], dtype=np.int32)
        out["eval/end_index"] = np.array([int(ev[i]["end_index"]) for i in range(len(ev))], dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "dbscan.npz"), **out)
    print("wrote", os.path.join(HERE, "dbscan.npz"), os.path.getsize(os.path.join(HERE, "dbscan.npz")), sorted(os.listdir(OUT)))
