"""Cases and runner shared by tests/test_gpu_wino_epilogue.py and tests/golden/make_golden_wino_epilogue.py: the two gradient
forms of the fused Winograd kernel (csrc/conv_wino_fused.hip, EPI 1 = dgrad + BatchNorm-backward sums, EPI 2 = dgrad +
pool-backward sums) at the smallest shapes at which their last phase -- the batched yref reads, the validity flags of the eight
(tile, pixel) iterations, the clamped / out-of-range addresses -- can go wrong.

A case is (B, H, W, K, C, ph, p, hx, wx): dgrad image (B, H, W), K reduction channels (the forward conv's outputs), C output
channels (the channels of yref; C = 128 is two cout blocks).  ph = 0 is EPI 1; ph = 1 / 2 is EPI 2 with a ph x 2 pool window,
dropout probability p, and yref (B, ph H + hx, 2 W + wx, C): hx / wx add the row / column that the floor of the pool leaves over.

  1x2x8   4 tiles: 60 of the 64 tile slots of the block are invalid
  1x3x8   the bottom tile row is half outside the image
  3x9x7   odd height AND width (tests/test_gpu_wino.py), 60 tiles
  2x1x8   one-pixel-high images: every tile hangs over the bottom edge
  3x6x16  72 tiles: a full 64-tile block and a ragged one
"""
import math

import torch

EPI1_CASES = [(1, 2, 8, 64, 64, 0, 0.0, 0, 0), (1, 2, 8, 128, 128, 0, 0.0, 0, 0), (1, 3, 8, 64, 128, 0, 0.0, 0, 0),
              (1, 3, 8, 128, 64, 0, 0.0, 0, 0), (3, 9, 7, 128, 64, 0, 0.0, 0, 0), (2, 1, 8, 64, 128, 0, 0.0, 0, 0),
              (3, 6, 16, 64, 128, 0, 0.0, 0, 0), (3, 6, 16, 128, 64, 0, 0.0, 0, 0)]
EPI2_CASES = [(1, 2, 8, 64, 64, 2, 0.2, 0, 0), (1, 2, 8, 128, 128, 1, 0.0, 0, 0), (1, 3, 8, 64, 128, 1, 0.2, 0, 1),
              (1, 3, 8, 128, 64, 2, 0.0, 1, 0), (3, 9, 7, 128, 64, 2, 0.2, 1, 1), (3, 9, 7, 64, 64, 1, 0.0, 0, 1),
              (2, 1, 8, 64, 128, 2, 0.0, 0, 0), (2, 1, 8, 128, 64, 1, 0.2, 0, 0), (3, 6, 16, 64, 128, 2, 0.2, 0, 0),
              (3, 6, 16, 128, 64, 1, 0.2, 0, 0), (3, 6, 16, 64, 64, 2, 0.0, 1, 1)]
CASES = EPI1_CASES + EPI2_CASES
SEED = 4242          # dropout seed of the EPI 2 cases
MARGIN = 4096        # floats of NaN on either side of a guarded tensor (a multiple of 4: the kernels read 16-byte vectors)


def case_id(c):
    B, H, W, K, C, ph, p, hx, wx = c
    return f"epi{1 if ph == 0 else 2}-{B}x{H}x{W}-{K}to{C}" + ("" if ph == 0 else f"-ph{ph}-p{p}-x{hx}{wx}")


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def host_inputs(c):
    """Everything a case reads, as CPU fp32 tensors (NCHW for the images), from a generator seeded by the case alone."""
    B, H, W, K, C, ph, p, hx, wx = c
    g = torch.Generator().manual_seed(1000 * B + 100 * H + 10 * W + K + 7 * C + 3 * ph + hx + 2 * wx)
    Hf, Wf = (H, W) if ph == 0 else (ph * H + hx, 2 * W + wx)
    d = {"dy": torch.randn(B, K, H, W, generator=g),
         "w": torch.randn(K, C, 3, 3, generator=g) / math.sqrt(9 * K),        # the forward conv C -> K whose dgrad is taken
         "yref": torch.randn(B, C, Hf, Wf, generator=g) * (1.0 + torch.arange(C).view(1, C, 1, 1) % 5) + 0.3,
         "scale": torch.rand(C, generator=g) + 0.5, "shift": 0.3 * torch.randn(C, generator=g),
         "mean": 0.1 * torch.randn(C, generator=g), "invstd": torch.rand(C, generator=g) + 0.5}
    return d


def guarded(t, dev, guard):
    """t on the device: a tight allocation, or (guard) the interior of a larger buffer that is NaN everywhere else."""
    if not guard:
        return t.to(dev), None
    buf = torch.full((t.numel() + 2 * MARGIN,), float("nan"), device=dev)
    view = buf[MARGIN:MARGIN + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def run_case(ops, dev, c, guard=False):
    """One launch of the entry the case names.  Returns (y, part, P) -- y (B, H, W, C) and the P x 2 C partial-sum rows, both
    allocated NaN-filled -- and keeps nothing else."""
    B, H, W, K, C, ph, p, hx, wx = c
    d = host_inputs(c)
    ud = torch.empty(16, K, C, device=dev)
    uf = torch.empty(16, C, K, device=dev)
    wd = d["w"].to(dev)
    ops.call("tag_pack_conv_weight_wino", ops.ptr(wd), ops.ptr(uf), ops.ptr(ud), C, K)
    dy, dy_buf = guarded(nhwc(d["dy"]), dev, guard)
    yref, yref_buf = guarded(nhwc(d["yref"]), dev, guard)
    sc, sh, mu, isd = (d[k].to(dev) for k in ("scale", "shift", "mean", "invstd"))
    P = ops.query("tag_conv3x3_wino_stats_rows", B, H, W, C)
    y = torch.full((B, H, W, C), float("nan"), device=dev)
    part = torch.full((P * 2 * C,), float("nan"), device=dev)
    ws = torch.empty(ops.query("tag_conv3x3_wino_ws_bytes", B, H, W, K, C) // 4 + 16, device=dev)
    assert ops.query("tag_conv3x3_wino_ok", B, H, W, K, C) == 1
    if ph == 0:
        ops.call("tag_conv3x3_wino_dgrad_bnsums", ops.ptr(dy), ops.ptr(ud), ops.ptr(y), ops.ptr(yref), ops.ptr(sc), ops.ptr(sh),
                 ops.ptr(mu), ops.ptr(isd), ops.ptr(part), B, H, W, K, C, ops.ptr(ws))
    else:
        ops.call("tag_conv3x3_wino_dgrad_poolsums", ops.ptr(dy), ops.ptr(ud), ops.ptr(y), ops.ptr(yref), ops.ptr(sc), ops.ptr(sh),
                 ops.ptr(mu), ops.ptr(isd), ops.ptr(part), B, H, W, K, C, ph * H + hx, 2 * W + wx, ph, 2, 0, float(p), SEED,
                 ops.ptr(ws))
    torch.cuda.synchronize()
    ops.check_async_errors()
    del dy_buf, yref_buf
    return y, part, P
