"""Cases and the launch of tests/test_gpu_wino_wgrad_rows.py, shared with tests/golden/make_golden_wino_wgrad_rows.py (which
records the same launches with the library of the commit before the row-split weight-gradient kernel).

A case is (B, H, W, Cin, Cout, prologue).  The shapes are the smallest at which the row-split kernel can go wrong:
  * channel pairs with one and two 128-channel blocks on either side; 1024 channels on either side (many blocks); 192 -> 128, which
    is no multiple of 128 and must take the 64 x 64 x 16 kernel;
  * images: 1 x 5 x 8 (odd height, 12 tiles: a ragged second chunk), 2 x 4 x 16, 3 x 7 x 32 (192 tiles = 24 chunks, which the
    slice count does not divide for 256 x 256: 12 slices of 2), 1 x 1 x 8 (one pixel high: every tile hangs over the bottom
    edge, and half of the gradient rows are outside the image), 1 x 2 x 4 (2 tiles: ONE chunk, so that the slice count 64 of
    128 -> 128 is clamped to 1).  Every image here has fewer chunks than 256 / blocks for 128 -> 128 (S clamped), and 3 x 7 x 32
    has more for 256 -> 256 (S = 16 -> 12) and 1024 <-> 128 (S = 8).
"""
import hashlib

import torch

IMAGES = [(1, 5, 8), (2, 4, 16), (3, 7, 32), (1, 1, 8), (1, 2, 4)]
PAIRS = [(128, 128), (128, 256), (256, 128), (256, 256)]

CASES = [(B, H, W, ci, co, pro) for (ci, co) in PAIRS for (B, H, W) in IMAGES for pro in (0, 1)]
CASES += [(3, 7, 32, ci, co, pro) for (ci, co) in [(1024, 128), (128, 1024), (192, 128)] for pro in (0, 1)]
CASES += [(2, 4, 16, 128, 256, 2), (1, 5, 8, 256, 128, 3)]

GUARD = 4096            # NaN floats on either side of every tensor (the x descriptor starts Cin floats before x)
SAMPLE = 251            # every SAMPLE-th float of dw is kept in the fixture beside the digest of all of them


def case_id(c):
    return "b{}_{}x{}_{}to{}_p{}".format(*c)


def inputs(c):
    """Seeded CPU tensors: x (B,Cin,H,W), dy (B,Cout,H,W), scale, shift."""
    B, H, W, Cin, Cout, pro = c
    g = torch.Generator().manual_seed(1000 * B + 100 * H + W + Cin + 3 * Cout + pro)
    x = torch.randn(B, Cin, H, W, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    s, t = torch.rand(Cin, generator=g) + 0.5, 0.3 * torch.randn(Cin, generator=g)
    return x, dy, s, t


class Guarded:
    """A tensor of the given shape in the middle of a NaN-filled buffer."""

    def __init__(self, shape, dev, src=None):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if src is not None:
            self.t.copy_(src)

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all())


def run_case(ops, dev, c):
    """dw (Cout,Cin,3,3) of tag_conv3x3_wino_wgrad with every operand inside NaN guards and a NaN-filled workspace."""
    B, H, W, Cin, Cout, pro = c
    x, dy, s, t = inputs(c)
    xg = Guarded((B, H, W, Cin), dev, x.permute(0, 2, 3, 1))
    dyg = Guarded((B, H, W, Cout), dev, dy.permute(0, 2, 3, 1))
    sg, tg = Guarded((Cin,), dev, s), Guarded((Cin,), dev, t)
    dwg = Guarded((Cout, Cin, 3, 3), dev)
    wsg = Guarded((ops.query("tag_conv3x3_wino_wgrad_ws_bytes", B, H, W, Cin, Cout) // 4,), dev)
    ops.call("tag_conv3x3_wino_wgrad", ops.ptr(xg.t), pro, ops.ptr(sg.t), ops.ptr(tg.t), ops.ptr(dyg.t), ops.ptr(dwg.t),
             B, H, W, Cin, Cout, ops.ptr(wsg.t), None)
    torch.cuda.synchronize()
    ok = all(g.guards_intact() for g in (xg, dyg, sg, tg, dwg, wsg))
    return dwg.t.clone(), ok


def digest(dw):
    """sha256 over the bits of dw (the fixture cannot hold 40 MB of filters; equal digests = equal bits)."""
    return hashlib.sha256(dw.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
