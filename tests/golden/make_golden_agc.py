#!/usr/bin/env python3
"""tests/golden/agc.npz + tests/golden/agc/*.json: what the REFERENCE's own code and sklearn / scipy make of three inputs --

* ``Runner().agc`` of python_scripts/clustering/agc_emb.py (sklearn ``AgglomerativeClustering(n_clusters, linkage="average",
  affinity="precomputed")`` on ``1 - cosine_similarity(embs, embs)``) on multi_phrase/sim40_emb.pkl at k in {2, 4, 7, 13}, on
  multi_phrase/phrase_emb.pkl at k in {2, 3, 5}, and on a clustered 2000 x 64 set (``clustered_rows``) at k in {2, 8, 30}, written
  as a pickle of {name: row} into a temporary directory.  sklearn 1.7 no longer accepts ``affinity``: the generator puts a small
  wrapper of its own under the name ``AgglomerativeClustering`` in the imported module's namespace, which hands ``affinity`` on
  as ``metric``; the reference's text runs unchanged.
* per case in agc.npz: ``<case>/x`` (the fp32 input), ``<case>/labels_k<k>`` (sklearn's labels, recovered from the Runner's result
  dict), ``<case>/heights`` (scipy's fp64 ``linkage(squareform(1 - cos), "average")[:, 2]`` with cos from fp64 unit rows),
  ``<case>/gap_k<k>`` (the smallest difference among the top k heights).  agc/sim40_k4_result.json and agc/phrase_k3_result.json are
  the Runner's ``result`` dicts.

The generator asserts that the fp64 restatement of tests/agc_ref.py gives the same labels and the same heights to 1e-12, and that
every recorded gap is at least 100 times the fp32 error bound of a height.  Only recorded data is committed.  The generator needs
the reference checkout (ref_import.REF), sklearn and scipy."""
import json
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
FIX = os.path.join(HERE, "multi_phrase")
OUT = os.path.join(HERE, "agc")

CASES = [("sim40", "sim40_emb.pkl", (2, 4, 7, 13)), ("phrase", "phrase_emb.pkl", (2, 3, 5)), ("blobs2000", None, (2, 8, 30))]
JSON_CASES = [("sim40", 4), ("phrase", 3)]


def clustered_rows():
    rng = np.random.RandomState(0)
    c = rng.randn(30, 64)
    x = c[rng.randint(30, size=2000)] + 0.6 * rng.randn(2000, 64)
    return x.astype(np.float32)


if __name__ == "__main__":
    import sklearn.cluster
    from make_golden_kmeans import load_ref, table
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    from tests import agc_ref as R

    class AgglomerativeClustering(sklearn.cluster.AgglomerativeClustering):
        def __init__(self, n_clusters=2, linkage="ward", affinity="euclidean"):
            super().__init__(n_clusters=n_clusters, linkage=linkage, metric=affinity)
            self.affinity = affinity

    mod = load_ref("python_scripts/clustering/agc_emb")
    mod.AgglomerativeClustering = AgglomerativeClustering
    os.makedirs(OUT, exist_ok=True)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, pkl, ks in CASES:
            if pkl is None:
                x = clustered_rows()
                phrases = [f"row {i}" for i in range(len(x))]
                path = os.path.join(tmp, name + ".pkl")
                with open(path, "wb") as f:
                    pickle.dump({p: row for p, row in zip(phrases, x)}, f)
            else:
                phrases, x = table(pkl)
                x = np.asarray(x, dtype=np.float32)
                path = os.path.join(FIX, pkl)
            N, D = x.shape
            u = R.unit_rows(x)
            dist = 1.0 - u @ u.T
            heights = linkage(squareform(dist, checks=False), "average")[:, 2]
            ref = R.agc_ref(x, ks)
            err = np.abs(ref["distances"] - heights).max()
            assert err <= 1e-12, (name, err)
            out[f"{name}/x"] = x
            out[f"{name}/heights"] = heights.astype(np.float64)
            index = {p: i for i, p in enumerate(phrases)}
            for k in ks:
                res = mod.Runner().agc(path, k)["result"]
                labels = np.full(N, -1, dtype=np.int64)
                for key, members in res.items():
                    labels[[index[p] for p in members]] = int(key)
                assert labels.min() == 0 and labels.max() == k - 1
                gap = float(np.diff(heights[-k:]).min()) if k > 1 and N > 2 else np.inf
                assert gap >= 100 * R.bound(D), (name, k, gap)
                assert np.array_equal(ref["labels"][k], labels), (name, k)
                out[f"{name}/labels_k{k}"] = labels
                out[f"{name}/gap_k{k}"] = np.float64(gap)
                if (name, k) in JSON_CASES:
                    with open(os.path.join(OUT, f"{name}_k{k}_result.json"), "w") as f:
                        json.dump(res, f, indent=1)
                print(f"{name} ({N} x {D}) k {k}: smallest top-k gap {gap:.3g}, restatement heights within {err:.3g}, rounds "
                      f"{ref['rounds']}")
    np.savez_compressed(os.path.join(HERE, "agc.npz"), **out)
    print("wrote", os.path.join(HERE, "agc.npz"), os.path.getsize(os.path.join(HERE, "agc.npz")), sorted(os.listdir(OUT)))
