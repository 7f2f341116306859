#!/usr/bin/env python3
"""tests/golden/clip_bce.npz: the REFERENCE's clip-level BCE objectives (losses.py: FocalClipBceLoss :59,
ClipBceLossFreqWeight :75, SymmetricClipBceLoss :90, OriginSymmetricClipBceLoss :107, PriorAdjustedClipBceLoss :125) at
(B,N) = (1,1), (5,7), (3,64) with hard and soft labels: the fp64 inputs (clip_sim uniform in [0.01, 0.99], label, counts in
[1, 499]; data_size 1000), the configuration, and loss and gradient from the fp64 run and from the fp32 run.  counts is handed
over as a tensor of the run's dtype.  Every recorded result is finite (asserted).  The cases of one input are stacked
(tests/clip_bce_ref.py load_golden unpacks them).  Build container only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.install()
import losses as ref_losses  # noqa: E402  (the reference)
from tests import clip_bce_ref as R  # noqa: E402

out = {}
names = []
for (B, N) in R.GOLDEN_SHAPES:
    for soft in (False, True):
        p, label, counts = R.make_inputs(B, N, seed=1000 * B + 10 * N + int(soft), soft=soft)
        group = R.golden_group(B, N, soft)
        res = {k: [] for k in ("cfg", "loss_f64", "loss_f32", "dp_f64", "dp_f32")}
        for kind in R.KINDS:
            for ci, cfg in enumerate(R.GOLDEN_CONFIGS[kind]):
                name = f"{kind}_{group}_c{ci}"
                names.append(name)
                loss_fn = getattr(ref_losses, R.CLASSES[kind][0])(**R.module_kwargs(kind, cfg))
                res["cfg"].append(np.asarray(list(cfg) + [np.nan] * (3 - len(cfg)), dtype=np.float64))
                for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                    d = {"clip_sim": p.to(dt).clone().requires_grad_(True), "label": label.to(dt), "counts": counts.to(dt)}
                    loss = loss_fn(d)
                    (g,) = torch.autograd.grad(loss, d["clip_sim"])
                    assert torch.isfinite(loss) and torch.isfinite(g).all(), name
                    res[f"loss_{tag}"].append(loss.detach().numpy())
                    res[f"dp_{tag}"].append(g.numpy())
                print(name, float(res["loss_f64"][-1]), float(res["loss_f32"][-1]))
        out[f"{group}/p"], out[f"{group}/label"], out[f"{group}/counts"] = p.numpy(), label.numpy(), counts.numpy()
        for k, v in res.items():
            out[f"{group}/{k}"] = np.stack(v)

assert sorted(names) == sorted(R.golden_names())
out["names"] = np.array(names)
path = os.path.join(HERE, "clip_bce.npz")
np.savez_compressed(path, **out)
print("wrote clip_bce.npz", os.path.getsize(path))
