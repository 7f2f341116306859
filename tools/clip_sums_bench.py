#!/usr/bin/env python3
"""CrossCDur's bias gradients dt[b, c] = sum_{h,w} dz[b, h, w, c] at the benched shapes (B = 64 x 10 s), per site: the backward
pass that also emits the per-clip sums (tag_lppool_leaky_backward_clip / tag_bn_act_backward_clip, what the model runs) against
the plain pass followed by tag_rowgroup_colsum over dz, and the plain pass alone.  The three forms are alternated and timed with
device events (launches included); prints the medians per site and their totals as JSON.

    python tools/clip_sums_bench.py [--out FILE.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from texttoaudiogrounding_amd import dispatch, functions  # noqa: E402

dev = torch.device("cuda:0")
REPS = 60
g = torch.Generator().manual_seed(0)
sites = [("block1 lppool(2,4)", (64, 501, 64, 32), "pool", 2, 4, 0.0), ("block2 bn_act", (64, 250, 16, 128), "bn", 0, 0, 0.0),
         ("block3 lppool(2,4)", (64, 250, 16, 128), "pool", 2, 4, 0.0), ("block4 bn_act", (64, 125, 4, 128), "bn", 0, 0, 0.0),
         ("block5 lppool(1,4)+dropout", (64, 125, 4, 128), "pool", 1, 4, 0.3)]
out = {}
tot = {"fused": 0.0, "separate": 0.0, "plain_without_sums": 0.0}
for name, shp, kind, ph, pw, drop in sites:
    B, H, W, C = shp
    z = torch.randn(*shp, generator=g).to(dev)
    if kind == "pool":
        dout = torch.randn(B, H // ph, W // pw, C, generator=g).to(dev)
        fused = lambda: dispatch.lppool_leaky_backward_clip(z, dout, ph, pw, drop, 99)
        plain = lambda: dispatch.lppool_leaky_backward(z, dout, ph, pw, drop, 99)
    else:
        du = torch.randn(*shp, generator=g).to(dev)
        gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(dev)
        st = dispatch.bn_stats(z.view(-1, C), gamma, gamma * 0, torch.zeros(C, device=dev), torch.ones(C, device=dev), True, pre_op=1)
        fused = lambda: dispatch.bn_act_backward_clip(z, 1, st, gamma, du)
        plain = lambda: dispatch.bn_act_backward(z, 1, st, gamma, du)
    def separate():
        r = plain()
        dz = r if kind == "pool" else r[0]
        return functions._clip_sums(dz)
    forms = {"fused": fused, "separate": separate, "plain_without_sums": plain}
    for f in forms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(REPS):
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3)
    out[name] = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "p90_us": float(np.percentile(v, 90))} for k, v in t.items()}
    for k in tot:
        tot[k] += out[name][k]["median_us"]
    print(name, {k: round(v["median_us"], 1) for k, v in out[name].items()}, flush=True)
out["total_median_us"] = tot
print(json.dumps(tot))
if len(sys.argv) > 2 and sys.argv[1] == "--out":
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
