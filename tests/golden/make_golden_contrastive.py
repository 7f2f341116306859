#!/usr/bin/env python3
"""tests/golden/contrastive.npz: the REFERENCE's sentence-level objectives (losses.py: InfoNceLoss :267,
MaxTripletLoss :285, RandomTripletLoss :319, WeightedTripletLoss :355, MilNceLoss :46) on small inputs: the fp64 input, the config,
loss and gradient from the fp64 twin and from the fp32 run, and for RandomTripletLoss the numpy seed with the two index vectors
it produced.  Inputs are uniform in [0,1) with the diagonal of every other row raised by 1.5 (inactive rows and columns at margin
0.2), plus one wide-range InfoNce case (randn * 40 at tau 0.07).  Build container only."""
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
from losses import InfoNceLoss, MaxTripletLoss, MilNceLoss, RandomTripletLoss, WeightedTripletLoss  # noqa: E402  (the reference)

out = {}
names = []


def run(loss_fn, inputs, key, seed=None):
    """inputs: dict of fp64 tensors; the gradient is taken with respect to inputs[key]."""
    res = {}
    for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        d = {k: v.to(dt).clone() for k, v in inputs.items()}
        d[key].requires_grad_(True)
        if seed is not None:
            np.random.seed(seed)
        loss = loss_fn(d)
        (g,) = torch.autograd.grad(loss, d[key], allow_unused=True)
        res[f"loss_{tag}"] = loss.detach().numpy()
        res[f"dx_{tag}"] = (torch.zeros_like(d[key]) if g is None else g).numpy()
    return res


def square(n, gen):
    x = torch.rand(n, n, generator=gen, dtype=torch.float64)
    idx = torch.arange(0, n, 2)
    x[idx, idx] += 1.5
    return x


gen = torch.Generator().manual_seed(2024)
for n in (1, 2, 5, 9):
    for ci, (tau, margin) in enumerate(((0.07, 0.2), (1.0, 1.0))):
        x = square(n, gen)
        seed = 100 * n + ci
        np.random.seed(seed)
        s_index = np.random.randint(n, size=n)
        a_index = np.random.randint(n, size=n)
        for kind, fn, cfg, sd in (("infonce", InfoNceLoss(tau), tau, None), ("max", MaxTripletLoss(margin), margin, None),
                                  ("weighted", WeightedTripletLoss(margin), margin, None),
                                  ("random", RandomTripletLoss(margin), margin, seed)):
            name = f"{kind}_n{n}_c{ci}"
            names.append(name)
            out[f"{name}/x"], out[f"{name}/cfg"] = x.numpy(), np.float64(cfg)
            for k, v in run(fn, {"sim": x}, "sim", sd).items():
                out[f"{name}/{k}"] = v
            if kind == "random":
                out[f"{name}/seed"], out[f"{name}/s_index"], out[f"{name}/a_index"] = np.int64(seed), s_index, a_index
            print(name, float(out[f"{name}/loss_f64"]), float(out[f"{name}/loss_f32"]))

x = torch.randn(9, 9, generator=gen, dtype=torch.float64) * 40
name = "infonce_wide"
names.append(name)
out[f"{name}/x"], out[f"{name}/cfg"] = x.numpy(), np.float64(0.07)
for k, v in run(InfoNceLoss(0.07), {"sim": x}, "sim").items():
    out[f"{name}/{k}"] = v
print(name, float(out[f"{name}/loss_f64"]), "finite gradient:", bool(np.isfinite(out[f"{name}/dx_f64"]).all()))

for (B, N), tau in (((5, 7), 1.0), ((5, 7), 0.07), ((1, 1), 1.0)):
    c = torch.rand(B, N, generator=gen, dtype=torch.float64)
    lab = (torch.rand(B, N, generator=gen) < 0.4).double()
    name = f"milnce_{B}x{N}_t{tau}"
    names.append(name)
    out[f"{name}/x"], out[f"{name}/label"], out[f"{name}/cfg"] = c.numpy(), lab.numpy(), np.float64(tau)
    for k, v in run(MilNceLoss(tau), {"clip_sim": c, "label": lab}, "clip_sim").items():
        out[f"{name}/{k}"] = v
    print(name, float(out[f"{name}/loss_f64"]))

out["names"] = np.array(names)
path = os.path.join(HERE, "contrastive.npz")
np.savez_compressed(path, **out)
print("wrote contrastive.npz", os.path.getsize(path))
