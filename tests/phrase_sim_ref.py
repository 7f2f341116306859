"""fp64 numpy reference of ops.phrase_sim_count and an input builder whose cosines keep a GAP from every threshold under test.

An fp32 dot product of two unit rows of length D errs by at most about D * 2^-24 <= 6.1e-5 for D <= 1024, and normalising in
fp32 adds a few ulp.  With no cosine within GAP = 1e-4 of a threshold, every implementation that computes in fp32 agrees with
fp64 on every pair, so the tests demand exact integer equality."""
import numpy as np

GAP = 1e-4
THRESHOLDS = (0.0, 0.5, 0.9)


def unit_rows64(x):
    """x / max(||x||, 1e-12) per row in fp64 (sklearn's normalize / F.normalize: an all-zero row stays zero)."""
    x = np.asarray(x, dtype=np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


def count_ref(q, bank, weight, threshold):
    """out[i] = sum_j weight[j] * [q[i] . bank[j] >= threshold], products and sums in fp64, counts in int64."""
    sims = np.asarray(q, dtype=np.float64) @ np.asarray(bank, dtype=np.float64).T
    w = np.ones(sims.shape[1], dtype=np.int64) if weight is None else np.asarray(weight, dtype=np.int64)
    return ((sims >= threshold) * w[None, :]).sum(1).astype(np.int64)


def near_threshold(q, bank, thresholds):
    """(N,) bool: bank rows with a cosine to some q row within GAP of some threshold."""
    sims = np.asarray(q, dtype=np.float64) @ np.asarray(bank, dtype=np.float64).T
    bad = np.zeros(sims.shape[1], dtype=bool)
    for t in thresholds:
        bad |= (np.abs(sims - t) < GAP).any(0)
    return bad


def assert_gap(q, bank, thresholds):
    assert not near_threshold(q, bank, thresholds).any(), "a cosine lies within GAP of a threshold"


def build_inputs(M, N, D, thresholds=THRESHOLDS, seed=0, same=False, raw=False, max_rounds=100):
    """fp32 q (M, D) and bank (N, D) (``same``: one matrix for both), rows drawn from a normal distribution; every third bank
    row is a near-duplicate of a q row, so counts at threshold 0.9 are not all zero.  Rows are normalised in fp64 and rounded
    to fp32; ``raw`` leaves them unnormalised (random row scales, row 0 of each operand all zero) for normalize=True.  Any
    bank row with a cosine within GAP of a threshold is re-drawn until none is left; the cosines are those of the fp64
    normalisation of the fp32 arrays returned.  -> (q, bank, rounds)."""
    g = np.random.RandomState(seed)

    def finish(rows, scale):
        u = unit_rows64(rows)
        if raw:
            u = u * scale[:, None]
            u[0] = 0.0
        return u.astype(np.float32)

    rq = g.randn(M, D)
    sq = np.exp(g.uniform(-3, 3, M))
    if same:
        N = M
        rb, sb = rq, sq
        for j in range(1, N, 3):
            rb[j] = rb[j - 1] + 0.2 * g.randn(D)
    else:
        rb = g.randn(N, D)
        sb = np.exp(g.uniform(-3, 3, N))
        for j in range(0, N, 3):
            rb[j] = rq[g.randint(M)] + 0.2 * g.randn(D)
    for rounds in range(max_rounds + 1):
        b32 = finish(rb, sb)
        q32 = b32 if same else finish(rq, sq)
        bad = near_threshold(unit_rows64(q32), unit_rows64(b32), thresholds)
        if not bad.any():
            break
        assert rounds < max_rounds, "the gap builder did not converge"
        rb[bad] = g.randn(int(bad.sum()), D)
    # (the zero rows of ``raw`` have cosine exactly 0 with everything: thresholds there must keep the gap from 0 as well)
    assert_gap(unit_rows64(q32), unit_rows64(b32), thresholds)
    return q32, b32, rounds
