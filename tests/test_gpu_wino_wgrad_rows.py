"""Row-split fused Winograd weight gradient (csrc/conv_wino_fused.hip, wino_fused_wgrad_rows_kernel + its finish kernel): a
workgroup owns ONE transform row x 128 ci x 128 co and writes raw per-xi sums; the finish kernel folds them with the 64 x 64 x 16
kernel's own expressions in its own share order.  Neither the staged values nor any order of summation changed, so dw has the
bits it had.  tests/wino_wgrad_rows_cases.py has the shapes and says why each is there.

Per case, on ONE launch (every operand inside NaN guards, the workspace NaN-filled: a read outside a tensor or a share that
nobody wrote reaches dw as a NaN):
  * against fp64 autograd at the bound tests/test_gpu_wino.py sets for the fused weight gradient (1e-5 of the largest entry);
  * the parent's bits: tests/golden/wino_wgrad_rows.npz holds, for every case, the sha256 of dw and every 251st float of it as
    recorded with the library BEFORE the row split (tests/golden/make_golden_wino_wgrad_rows.py; the fixture cannot hold the
    40 MB of filters themselves).  192 -> 128 still takes the 64 x 64 x 16 kernel and is held to the same equality.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wino_wgrad_rows_cases as RC

pytestmark = pytest.mark.gpu

IDS = [RC.case_id(c) for c in RC.CASES]


@pytest.fixture(scope="module")
def ops(dev):
    from texttoaudiogrounding_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def launched(ops, dev):
    """case -> (dw on the host, guards intact), computed once and left unchanged."""
    cache = {}

    def get(c):
        if c not in cache:
            dw, ok = RC.run_case(ops, dev, c)
            cache[c] = (dw.cpu(), ok)
        return cache[c]
    return get


@pytest.fixture(scope="module")
def parent_bits(golden_dir):
    return np.load(os.path.join(golden_dir, "wino_wgrad_rows.npz"))


def prologue64(x, mode, s, t):
    if mode == 1:
        return torch.relu(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1))
    if mode == 2:
        return F.leaky_relu(x, 0.1) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
    if mode == 3:
        return x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
    return x


@pytest.mark.parametrize("c", RC.CASES, ids=IDS)
def test_weight_gradient_against_fp64(launched, c):
    B, H, W, Cin, Cout, pro = c
    dw, ok = launched(c)
    assert ok, "a NaN guard around an operand was overwritten"
    assert torch.isfinite(dw).all()
    x, dy, s, t = RC.inputs(c)
    w64 = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(prologue64(x.double(), pro, s.double(), t.double()), w64, padding=1).backward(dy.double())
    e = (dw.double() - w64.grad).abs().max().item() / (w64.grad.abs().max().item() + 1e-30)
    print(f"{RC.case_id(c)}: err {e:.2e} of the largest entry")
    assert e < 1e-5, e


@pytest.mark.parametrize("c", RC.CASES, ids=IDS)
def test_same_bits_as_the_64x64x16_kernel(launched, parent_bits, c):
    dw, _ = launched(c)
    k = RC.case_id(c)
    sample = dw.contiguous().view(-1)[::RC.SAMPLE].numpy().view(np.uint32)
    ref = parent_bits[k + "/sample"].view(np.uint32)
    differ = int((sample != ref).sum())
    print(f"{k}: {differ} of {sample.size} sampled floats differ")
    assert differ == 0
    assert RC.digest(dw) == str(parent_bits[k + "/sha256"])
