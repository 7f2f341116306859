#!/usr/bin/env python3
"""tests/golden/sed_double_threshold.npz: the regions the REFERENCE's ``_double_threshold(x, high, low, n_connect,
return_arr=False)`` (utils/sed_utils.py:170-197, imported as it is) gives for seeded float32 rows -- data only.

Rows of T in {1, 2, 3, 64, 250}; n_connect in {0, 1, 13}; (high, low) in {(0.75, 0.25), (0.5, 0.5), (0.3, 0.3), (0.9, 0.1)}.
Beside random rows (a level, a slow sine and noise) every length holds the rows the device kernel can get wrong: a score equal
to float32(0.3) (numpy compares the float32 row with the Python float ROUNDED to float32, so that frame is not above 0.3); a
low run without a high frame between two kept runs within the gap (the filter comes before the connection: the two are only
connected when the whole span from one to the other is within n_connect); an all-low row; an all-high row; a run touching each
end.  Stored per case: x (R, T) float32, and per (row, n_connect, pair) the regions flattened with their row offsets.
Build container only."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.install()
SU = importlib.import_module("utils.sed_utils")
assert SU.__file__.startswith(ref_import.REF), SU.__file__

LENGTHS = (1, 2, 3, 64, 250)
N_CONNECT = (0, 1, 13)
PAIRS = ((0.75, 0.25), (0.5, 0.5), (0.3, 0.3), (0.9, 0.1))
F03 = np.float32(0.3)


def rows_for(T, rng):
    rows = []
    for _ in range(6):                                          # random rows
        t = np.arange(T, dtype=np.float64)
        rows.append(np.clip(rng.uniform(0.2, 0.7) + 0.35 * np.sin(t / rng.uniform(3.0, 8.0)) + 0.08 * rng.standard_normal(T),
                            1e-7, 1.0))
    rows.append(np.full(T, 0.05))                               # all low
    rows.append(np.full(T, 0.95))                               # all high
    exact = np.full(T, 0.05)                                    # a score equal to float32(0.3): above 0.25 and 0.1, NOT above 0.3
    exact[::2] = F03
    exact[T // 2] = 0.95 if T > 2 else exact[T // 2]
    rows.append(exact)
    ends = np.full(T, 0.05)                                     # a run touching each end
    ends[:max(T // 8, 1)] = 0.95
    ends[T - max(T // 8, 1):] = 0.8
    rows.append(ends)
    if T >= 64:                                                 # kept run, low-only run, kept run: gaps 3 + 3 around 4 low frames
        x = np.full(T, 0.05)
        x[5:12] = 0.95
        x[15:19] = 0.4                                          # above every low but 0.5, never above a high but 0.3
        x[22:30] = 0.95
        x[31:33] = 0.6                                          # gap 1 behind the second run; high only for (0.5, 0.5), (0.3, 0.3)
        x[36:40] = 0.95                                         # kept, gap 1, low-only, gap 1, kept: n_connect 1 must not bridge
        x[41:44] = 0.4
        x[45:49] = 0.95
        x[55:57] = 0.2                                          # above 0.1 only
        rows.append(x)
    return np.stack(rows).astype(np.float32)


rng = np.random.default_rng(2024)
out = {"lengths": np.array(LENGTHS), "n_connect": np.array(N_CONNECT), "pairs": np.array(PAIRS)}
for T in LENGTHS:
    x = rows_for(T, rng)
    assert x.dtype == np.float32 and (x == F03).any()
    flat, offsets = [], [0]
    total = 0
    for r in range(x.shape[0]):
        for n in N_CONNECT:
            for high, low in PAIRS:
                got = SU._double_threshold(x[r], high, low, n_connect=n, return_arr=False)
                flat.extend([int(a), int(b)] for a, b in got)
                offsets.append(len(flat))
                total += len(got)
    if total == 0:
        raise SystemExit(f"T = {T}: no stored case has a region")
    out[f"x{T}"] = x
    out[f"regions{T}"] = np.array(flat, dtype=np.int64).reshape(-1, 2)
    out[f"offsets{T}"] = np.array(offsets, dtype=np.int64)
    print(f"T {T}: {x.shape[0]} rows, {len(offsets) - 1} cases, {total} regions")
# the filter comes before the connection: a low-only run one frame from kept runs on both sides does not bridge them at n_connect 1
x = out["x64"][-1]
assert SU._double_threshold(x, 0.75, 0.25, n_connect=1, return_arr=False) == [(5, 12), (22, 30), (36, 40), (45, 49)]
assert SU._double_threshold(x, 0.75, 0.25, n_connect=13, return_arr=False) == [(5, 49)]
assert SU._double_threshold(x, 0.3, 0.3, n_connect=1, return_arr=False) == [(5, 12), (15, 19), (22, 33), (36, 49)]
path = os.path.join(HERE, "sed_double_threshold.npz")
np.savez_compressed(path, **out)
print("wrote sed_double_threshold.npz", os.path.getsize(path))
