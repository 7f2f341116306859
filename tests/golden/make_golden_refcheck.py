#!/usr/bin/env python3
"""tests/golden/refcheck.npz: outputs of the REFERENCE's match heads (models/match.py ExpNegL2, DotProduct) and of its
post-processing chain (utils/eval_util.py median_filter -> connect_clusters -> find_contiguous_regions) on the seeded inputs of
tests/test_oracle_golden.py::test_oracle_vs_imported_reference_when_present, so that the test checks the oracle against them
without the reference present.  Build container only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
from oracle import tag_oracle as O  # noqa: E402

mods = ref_import.install()
g = torch.Generator().manual_seed(0)
audio, text = torch.randn(2, 7, 16, generator=g), torch.randn(2, 16, generator=g)
fd = {"audio_emb": audio, "text_emb": {"seq_emb": text}}
out = {"audio": audio.numpy(), "text": text.numpy(),
       "exp_neg_l2": mods["models.match"].ExpNegL2()(fd).numpy(),
       "dot_product": mods["models.match"].DotProduct()(fd).numpy()}
x = np.random.RandomState(1).rand(60).astype(np.float32)
out["x"] = x
EU = mods["utils.eval_util"]
ths = O.eval_thresholds(50)[::7]
out["thresholds"] = np.asarray(ths, dtype=np.float64)
for i, th in enumerate(ths):
    filt = EU.median_filter(torch.from_numpy(x).unsqueeze(0), window_size=3, threshold=th)[0]
    out[f"segments/{i}"] = np.asarray(EU.find_contiguous_regions(EU.connect_clusters(filt, 7))).reshape(-1, 2).astype(np.int64)
np.savez_compressed(os.path.join(HERE, "refcheck.npz"), **out)
print("wrote", os.path.join(HERE, "refcheck.npz"), len(out), "arrays")
