#!/usr/bin/env python3
"""Fixture of tests/test_gpu_wino_epilogue.py: y and the partial-sum rows of the fused Winograd gradient launches
(tag_conv3x3_wino_dgrad_bnsums / tag_conv3x3_wino_dgrad_poolsums) at the cases of tests/wino_epilogue_cases.py.  Data only.

    python tests/golden/make_golden_wino_epilogue.py [out.npz]      (needs the MI355X)

Recorded with the library of the commit BEFORE the last phase's yref reads were batched (TAG_HIP_LIB=<that library>
TAG_ALLOW_STALE_LIB=1 selects it without a second checkout): the test compares bit for bit, so the file is re-recorded only by a
change that means to alter the arithmetic or its order.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import wino_epilogue_cases as WC  # noqa: E402
from texttoaudiogrounding_amd import ops  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wino_epilogue.npz")
    dev = torch.device("cuda:0")
    arrays = {}
    for c in WC.CASES:
        y, part, _ = WC.run_case(ops, dev, c)
        y2, part2, _ = WC.run_case(ops, dev, c)
        assert torch.equal(y, y2) and torch.equal(part, part2), f"{WC.case_id(c)}: two runs differ"
        assert torch.isfinite(y).all() and torch.isfinite(part).all(), WC.case_id(c)
        arrays[WC.case_id(c) + "/y"] = y.cpu().numpy()
        arrays[WC.case_id(c) + "/part"] = part.cpu().numpy()
    np.savez(out, **arrays)
    print(f"{len(WC.CASES)} cases, {os.path.getsize(out)} bytes -> {out}")


if __name__ == "__main__":
    main()
