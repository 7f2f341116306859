#!/usr/bin/env python3
"""tests/golden/spectral.npz + tests/golden/spectral/*.json: what the REFERENCE's own code and sklearn make of four inputs --

* ``Spectral().spectral_sklearn`` of python_scripts/clustering/spectral_emb.py (sklearn ``SpectralClustering(n_clusters,
  affinity="precomputed", random_state=seed)`` on ``(cosine_similarity + 1) / 2``) at seed 1 on the rows of
  ``spectral_ref.generate(N, D, C, noise)`` with k = C, written as a pickle of {name: row} into a temporary directory:
  ``blobs600`` (600, 16, 6, 0.3), ``edge600`` (the same with row 5 zero and row 77 a copy of row 78), ``blobs257`` (257, 8, 4, 0.2)
  and ``blobs1000`` (1000, 32, 10, 0.5).
* per case in spectral.npz: ``<case>/x`` (the fp32 input; ``edge600`` is derived from ``blobs600/x``), ``<case>/planted`` (the
  generator's labels), ``<case>/labels`` (sklearn's, recovered from the result dict), ``<case>/maps``
  (``sklearn.manifold.spectral_embedding(A, k, eigen_solver="arpack", drop_first=False)`` of the same dense fp64 matrix, stored
  as fp32: what SpectralClustering runs k-means on), ``<case>/eigenvalues`` (of M, from the fp64 restatement), ``<case>/gap`` (the
  smallest difference of neighbouring eigenvalues among the first k + 1) and ``<case>/err32`` (the largest per-vector error of the
  emulated-fp32 restatement of tests/spectral_ref.py against ``maps``, relative to the vector's largest entry).
  spectral/blobs257_result.json is the reference's ``result`` dict of that case.

The generator asserts that the fp64 restatement agrees with sklearn's embedding to 1e-6 per vector, that sklearn's labels are the
planted partition (but for the zero row of ``edge600``) and that every gap is at least 1e-3.  Only recorded data is committed.  The
generator needs the reference checkout (ref_import.REF) and sklearn."""
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
OUT = os.path.join(HERE, "spectral")

CASES = [("blobs600", (600, 16, 6, 0.3), False), ("edge600", (600, 16, 6, 0.3), True), ("blobs257", (257, 8, 4, 0.2), False),
         ("blobs1000", (1000, 32, 10, 0.5), False)]
JSON_CASE = "blobs257"
SEED = 1


def case_rows(shape, edge):
    from tests import spectral_ref as R
    x, planted = R.generate(*shape)
    if edge:
        x[5] = 0
        x[77] = x[78]
        planted[77] = planted[78]
    return x, planted


if __name__ == "__main__":
    from make_golden_kmeans import load_ref
    from sklearn.manifold import spectral_embedding
    from tests import spectral_ref as R

    mod = load_ref("python_scripts/clustering/spectral_emb")
    os.makedirs(OUT, exist_ok=True)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, shape, edge in CASES:
            x, planted = case_rows(shape, edge)
            N, k = x.shape[0], shape[2]
            phrases = [f"row {i}" for i in range(N)]
            path = os.path.join(tmp, name + ".pkl")
            with open(path, "wb") as f:
                pickle.dump({p: row for p, row in zip(phrases, x)}, f)
            res = mod.Spectral().spectral_sklearn(path, n_clusters=k, seed=SEED)["result"]
            index = {p: i for i, p in enumerate(phrases)}
            labels = np.full(N, -1, dtype=np.int64)
            for key, members in res.items():
                labels[[index[p] for p in members]] = int(key)
            assert labels.min() == 0 and labels.max() == k - 1
            keep = np.arange(N) != 5 if edge else np.ones(N, dtype=bool)
            assert R.same_partition(labels[keep], planted[keep]), name
            maps = spectral_embedding(R.dense_affinity(x), n_components=k, eigen_solver="arpack", drop_first=False, random_state=SEED)
            r64 = R.spectral_ref(x, k, steps=6)
            r32 = R.spectral_ref(x, k, steps=6, dtype=np.float32)
            err64, err32 = R.vector_errors(r64["maps"], maps).max(), R.vector_errors(r32["maps"], maps).max()
            assert err64 <= 1e-6, (name, err64)
            lam = R.spectral_ref(x, min(k + 1, x.shape[1] + 1), steps=8)["eigenvalues"]
            gap = float(np.abs(np.diff(lam)).min())
            assert gap >= 1e-3, (name, gap)
            if not edge:                                        # (edge600's rows are blobs600's with the two edits above)
                out[f"{name}/x"] = x
            out[f"{name}/planted"] = planted.astype(np.int64)
            out[f"{name}/labels"] = labels
            out[f"{name}/maps"] = maps.astype(np.float32)
            out[f"{name}/eigenvalues"] = r64["eigenvalues"]
            out[f"{name}/gap"] = np.float64(gap)
            out[f"{name}/err32"] = np.float64(err32)
            if name == JSON_CASE:
                with open(os.path.join(OUT, f"{name}_result.json"), "w") as f:
                    json.dump(res, f, indent=1)
            print(f"{name} {shape}: fp64 restatement within {err64:.3g} of sklearn's embedding, emulated fp32 within {err32:.3g}; "
                  f"smallest eigenvalue gap {gap:.3g}; fp32 residuals {['%.2g' % v for v in r32['residuals']]}")
    np.savez_compressed(os.path.join(HERE, "spectral.npz"), **out)
    print("wrote", os.path.join(HERE, "spectral.npz"), os.path.getsize(os.path.join(HERE, "spectral.npz")), sorted(os.listdir(OUT)))
