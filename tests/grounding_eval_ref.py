"""Scalar fp64 restatement of the operating-point counts of ONE (detections, ground truths) pair -- what csrc/grounding_eval.hip
computes per (clip, threshold) -- with the order of every addition written out, and the builder of the inputs the grounding
evaluation tests share.

The yardstick is utils/grounding_eval.py (numpy).  Its sums are, for a file with D detections and G ground truths:

* over the ground truths of one detection (``det_prec.sum(1)``, ``(det_prec * gtc_pass[None, :]).sum(1)``): numpy's contiguous
  fp64 reduction, ``np_sum`` below;
* over the detections of one ground truth (``gt_cov.sum(0)``, ``(gt_cov * mask[:, None]).sum(0)``): row after row, i.e. left to
  right in d, when G >= 2 -- and ``np_sum`` over d when G == 1, because a (D, 1) array is contiguous along d and numpy reduces it
  with the same pairwise routine;
* a masked term is the ratio times 0.0 or 1.0 and is still added (inf * 0 = NaN).

Python floats are IEEE doubles; ``_div`` supplies the inf / NaN quotients numpy produces where Python raises.
"""
import math

import numpy as np
import torch


def _div(a: float, b: float) -> float:
    if b != 0.0:
        return a / b
    if a == 0.0 or a != a:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def np_sum(a) -> float:
    """numpy's pairwise_sum over a sequence of doubles: < 8 terms left to right; <= 128 terms eight running lanes
    r[j] += a[i + j], ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the remainder in order; above that the two halves (the first
    rounded down to a multiple of 8) on their own."""
    n = len(a)
    if n < 8:
        s = 0.0
        for x in a:
            s = s + x
        return s
    if n <= 128:
        r = [a[j] for j in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = r[j] + a[i + j]
            i += 8
        s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            s = s + a[i]
            i += 1
        return s
    n2 = n // 2
    n2 -= n2 % 8
    return np_sum(a[:n2]) + np_sum(a[n2:])


def _seq_sum(a) -> float:
    s = 0.0
    for x in a:
        s = s + x
    return s


def pair_counts(det, gt, dtc: float = 0.5, gtc: float = 0.5, row_sum=None, col_sum=None):
    """det (D,2), gt (G,2) in seconds -> (tp_preds, tp_refs, psds_tp, psds_fp) of that file.  row_sum / col_sum replace the
    order of the sums over the ground truths / over the detections (the tests use them to show that the order matters)."""
    det = [(float(a), float(b)) for a, b in det]
    gt = [(float(a), float(b)) for a, b in gt]
    D, G = len(det), len(gt)
    if D == 0:
        return 0, 0, 0, 0
    if G == 0:
        return 0, 0, 0, D
    cross = [[False] * G for _ in range(D)]
    prec = [[0.0] * G for _ in range(D)]
    cov = [[0.0] * G for _ in range(D)]
    for d, (on_d, off_d) in enumerate(det):
        for g, (on_g, off_g) in enumerate(gt):
            if on_d <= off_g and on_g <= off_d:
                inter = (off_d if (off_d <= off_g or off_d != off_d) else off_g) - (on_d if (on_d >= on_g or on_d != on_d) else on_g)
                cross[d][g] = True
                prec[d][g] = _div(inter, off_d - on_d)
                cov[d][g] = _div(inter, off_g - on_g)
    col_sum = col_sum or (np_sum if G == 1 else _seq_sum)
    row_sum = row_sum or np_sum
    row = [row_sum(prec[d]) for d in range(D)]
    relevant = [row[d] >= dtc for d in range(D)]
    dtc_pass = [relevant[d] and any(cross[d]) for d in range(D)]
    psds_fp = sum(not r for r in relevant)
    tp_refs = psds_tp = 0
    gtc_pass = []
    for g in range(G):
        column = [cov[d][g] for d in range(D)]
        by_passing = col_sum([column[d] * (1.0 if dtc_pass[d] else 0.0) for d in range(D)])
        tp_refs += by_passing >= gtc and any(cross[d][g] and dtc_pass[d] for d in range(D))
        psds_tp += col_sum([column[d] * (1.0 if relevant[d] else 0.0) for d in range(D)]) >= gtc
        gtc_pass.append(col_sum(column) >= gtc and any(cross[d][g] for d in range(D)))
    tp_preds = 0
    for d in range(D):
        by_passing = row_sum([prec[d][g] * (1.0 if gtc_pass[g] else 0.0) for g in range(G)])
        tp_preds += by_passing >= dtc and any(cross[d][g] and gtc_pass[g] for g in range(G))
    return tp_preds, tp_refs, psds_tp, psds_fp


def counts_ref(regions, counts, gt, gt_count, time_resolution, dtc=0.5, gtc=0.5) -> torch.Tensor:
    """The (B, NT, 4) int32 tensor ops.grounding_counts must return, from host arrays shaped like its arguments."""
    regions, counts = np.asarray(regions), np.asarray(counts)
    gt, gt_count = np.asarray(gt, dtype=np.float64), np.asarray(gt_count)
    B, NT = counts.shape
    out = torch.zeros(B, NT, 4, dtype=torch.int32)
    for b in range(B):
        rows = gt[b, :gt_count[b]]
        for t in range(NT):
            det = regions[b, t, :counts[b, t]].astype(np.float64) * time_resolution
            out[b, t] = torch.tensor(pair_counts(det, rows, dtc, gtc), dtype=torch.int32)
    return out


# ------------------------------------------------------------------------------------------------ inputs

def build_scores(B: int, T: int, seed: int = 17) -> torch.Tensor:
    """Frame scores (B, T) float32 on the host: a level per clip, a slow sine and noise, as in
    test_gpu_path.test_device_segments_to_th_auc_and_psds."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B, 1, generator=g) * 0.5 + 0.2
    return (base + 0.35 * torch.sin(torch.arange(T)[None, :] / (3.0 + 5.0 * torch.rand(B, 1, generator=g))) +
            0.05 * torch.randn(B, T, generator=g)).clamp(1e-7, 1.0)


def build_ground_truth(B: int, gmax: int, T: int, res: float, seed: int = 5):
    """List over clips of [[onset, offset], ...] with 0 .. gmax rows (clip 0 has none, clip 1 has gmax), of three kinds: on the
    frame grid (onset = k * res, 1 .. 59 frames long: sums of ratios land on 0.5 all the time), off the grid, and one
    zero-duration row (onset == offset != 0) here and there."""
    rng = np.random.default_rng(seed)
    items = []
    for b in range(B):
        n = 0 if b == 0 else gmax if b == 1 else int(rng.integers(0, gmax + 1))
        rows = []
        for i in range(n):
            kind = (b + i) % 3 if i else 0
            if kind == 2 and i % 4 == 1:
                on = float(rng.integers(1, T)) * res
                rows.append([on, on])
            elif kind == 1:
                on = float(rng.uniform(0.0, T * res * 0.9))
                rows.append([on, on + float(rng.uniform(0.05, 2.5))])
            else:
                k = int(rng.integers(0, max(T - 1, 1)))
                rows.append([k * res, (k + int(rng.integers(1, 60))) * res])
        items.append(rows)
    return items


def cpu_segments(scores: torch.Tensor, thresholds, window_size: int, n_connect: int):
    """The host pipeline of utils/eval_util.py per (clip, threshold): list over clips of list over thresholds of (K,2) int64."""
    from texttoaudiogrounding_amd.utils import eval_util as EU
    out = []
    for row in scores.numpy():
        per_th = []
        for th in thresholds:
            filtered = EU.median_filter(row[None, :], window_size=window_size, threshold=th)[0]
            per_th.append(EU.find_contiguous_regions(EU.connect_clusters(filtered, n_connect)).astype(np.int64).reshape(-1, 2))
        out.append(per_th)
    return out


def pack_segments(segments, max_regions: int, fill: int = -7):
    """cpu_segments' lists -> (regions (B,NT,max_regions,2) int64 with ``fill`` beyond the counts, counts (B,NT) int32)."""
    B, NT = len(segments), len(segments[0])
    regions = np.full((B, NT, max_regions, 2), fill, dtype=np.int64)
    counts = np.zeros((B, NT), dtype=np.int32)
    for b in range(B):
        for t in range(NT):
            k = len(segments[b][t])
            regions[b, t, :k] = segments[b][t]
            counts[b, t] = k
    return regions, counts


def hand_regions(B: int, NT: int, D, max_regions: int, seed: int = 3, fill: int = 2 ** 40):
    """Hand-built sorted, disjoint integer regions: D detections (an int, or a (B,NT) array) per pair, 1 .. 4 frames long with
    gaps of 1 .. 3 frames, garbage beyond the counts."""
    rng = np.random.default_rng(seed)
    counts = np.broadcast_to(np.asarray(D, dtype=np.int32), (B, NT)).copy()
    regions = np.full((B, NT, max_regions, 2), fill, dtype=np.int64)
    for b in range(B):
        for t in range(NT):
            k = int(counts[b, t])
            length = rng.integers(1, 5, k)
            gap = rng.integers(1, 4, k)
            off = np.cumsum(length + gap)
            regions[b, t, :k, 0] = off - length
            regions[b, t, :k, 1] = off
    return regions, counts


def grid_ground_truth(B: int, G, gmax: int, span: int, res: float, seed: int = 9, pad: float = -1.0e30):
    """(gt (B,gmax,2) float64, gt_count (B,) int32): G rows per clip (an int or a list over clips), mostly on the frame grid
    inside [0, span) frames, every fifth off the grid, garbage in the padding."""
    rng = np.random.default_rng(seed)
    gt_count = np.broadcast_to(np.asarray(G, dtype=np.int32), (B,)).copy()
    gt = np.full((B, gmax, 2), pad, dtype=np.float64)
    for b in range(B):
        for i in range(int(gt_count[b])):
            k = int(rng.integers(0, max(span, 2)))
            n = int(rng.integers(1, 60))
            if i % 5 == 4:
                on = float(rng.uniform(0, span * res))
                gt[b, i] = [on, on + float(rng.uniform(0.03, 1.5))]
            else:
                gt[b, i] = [k * res, (k + n) * res]
    return gt, gt_count


def tie_case(kind: str, n: int, seed: int, res: float = 0.04):
    """(det (D,2) int64 frames, gt (G,2) float64 seconds) whose ratio sum is 1/2 up to rounding, so that the ORDER of the
    additions decides the comparison with dtc = gtc = 0.5: n pieces on the frame grid that fill exactly half of a span of 2m
    frames.  kind "col1": the pieces are the detections and the span the only ground truth (numpy sums that column pairwise);
    "col2": the same beside a second, distant ground truth (numpy sums the column left to right); "row": the span is the one
    detection and the pieces are the ground truths (row sums: pairwise)."""
    rng = np.random.default_rng(seed)
    m = int(rng.integers(n, 3 * n + 1))
    cuts = np.sort(rng.choice(np.arange(1, m), n - 1, replace=False))
    lens = np.diff(np.concatenate(([0], cuts, [m])))
    gaps = rng.multinomial(m, np.full(n + 1, 1.0 / (n + 1)))
    k0 = int(rng.integers(0, 50))
    onset = k0 + np.cumsum(gaps[:n]) + np.concatenate(([0], np.cumsum(lens[:-1])))
    pieces = np.stack([onset, onset + lens], axis=1).astype(np.int64)
    span = np.array([[k0, k0 + 2 * m]], dtype=np.int64)
    assert pieces[-1, 1] <= span[0, 1] and lens.sum() * 2 == 2 * m
    if kind == "row":
        return span, pieces.astype(np.float64) * res
    gt = span.astype(np.float64) * res
    if kind == "col2":
        gt = np.concatenate([gt, np.array([[k0 + 2 * m + 5, k0 + 2 * m + 9]], dtype=np.float64) * res])
    return pieces, gt


def pack_cases(cases, fill: int = 2 ** 40, pad: float = -1.0e30):
    """[(det, gt), ...] -> (regions (B,1,maxD,2) int64, counts (B,1) int32, gt (B,maxG,2) float64, gt_count (B,) int32), one
    case per clip, garbage beyond the counts."""
    max_d, max_g = max(len(d) for d, _ in cases), max(len(g) for _, g in cases)
    regions = np.full((len(cases), 1, max_d, 2), fill, dtype=np.int64)
    gts = np.full((len(cases), max_g, 2), pad, dtype=np.float64)
    for b, (d, g) in enumerate(cases):
        regions[b, 0, :len(d)] = d
        gts[b, :len(g)] = g
    return (regions, np.array([[len(d)] for d, _ in cases], dtype=np.int32), gts,
            np.array([len(g) for _, g in cases], dtype=np.int32))


def tie_cases():
    """The seeded tie-prone cases the CPU and the GPU test share."""
    return ([tie_case("col1", n, 100 + 7 * n + s) for n in (9, 17, 40, 125, 300) for s in range(6)] +
            [tie_case("col2", n, 200 + 7 * n + s) for n in (9, 40, 125) for s in range(6)] +
            [tie_case("row", n, 300 + 7 * n + s) for n in (9, 17, 65, 128) for s in range(6)])
