#!/usr/bin/env python3
"""Fixture of tests/test_gpu_wino_wgrad_rows.py: dw of tag_conv3x3_wino_wgrad at the cases of tests/wino_wgrad_rows_cases.py, as
the sha256 of its bits and every 251st float (the filters themselves are 40 MB).  Data only.

    python tests/golden/make_golden_wino_wgrad_rows.py [out.npz]      (needs the MI355X)

Recorded with the library of the commit BEFORE the row-split weight-gradient kernel (TAG_HIP_LIB=<that library>
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

from tests import wino_wgrad_rows_cases as RC  # noqa: E402
from texttoaudiogrounding_amd import ops  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wino_wgrad_rows.npz")
    dev = torch.device("cuda:0")
    arrays = {}
    for c in RC.CASES:
        dw, ok = RC.run_case(ops, dev, c)
        dw2, _ = RC.run_case(ops, dev, c)
        assert ok, f"{RC.case_id(c)}: a guard was overwritten"
        assert torch.equal(dw, dw2), f"{RC.case_id(c)}: two runs differ"
        assert torch.isfinite(dw).all(), RC.case_id(c)
        arrays[RC.case_id(c) + "/sha256"] = np.array(RC.digest(dw))
        arrays[RC.case_id(c) + "/sample"] = dw.cpu().contiguous().view(-1)[::RC.SAMPLE].numpy()
    np.savez(out, **arrays)
    print(f"{len(RC.CASES)} cases, {os.path.getsize(out)} bytes -> {out}")


if __name__ == "__main__":
    main()
