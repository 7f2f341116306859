"""Restatement of the BERTScore phrase-to-label map (csrc/bertscore.hip, dispatch.bertscore_map) in plain torch, in the dtype of its
inputs (the tests run it in float64 as the reference and in float32 for its own rounding), and the seeded inputs of the tests.

With unit token vectors and s_ij = a[n,i] . b[c,j] over i < a_len[n], j < b_len[c]:
    P = sum_i a_w[n,i] max_j s_ij / sum_i a_w[n,i]    R = sum_j b_w[c,j] max_i s_ij / sum_j b_w[c,j]    F = 2 P R / (P + R)
a zero weight sum gives P = 0 (R = 0), P + R == 0 gives F = 0; positions at and past a length enter no maximum and no sum.
This is the published algorithm of the ``bert_score`` package with idf=False as restated by this project; the package itself is
not available to the tests (utils/bertscore_map.py lists the known differences)."""
import numpy as np
import torch


def unit(x):
    """x / max(||x||, 1e-12) over the last axis"""
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def default_weights(lens, L, special_tokens=True, dtype=torch.float32):
    """1 below the length; with special_tokens 0 for the first and the last token of an item"""
    pos = torch.arange(L)[None, :]
    n = torch.as_tensor(lens).long()[:, None]
    return ((pos >= 1) & (pos < n - 1) if special_tokens else pos < n).to(dtype)


def scores(a, a_len, a_w, b, b_len, b_w, normalize=True):
    """-> (3, N, C) = P, R, F in a's dtype.  a (N, La, D), a_len (N,), a_w (N, La); b (C, Lb, D), b_len (C,), b_w (C, Lb)."""
    dt = a.dtype
    a_w, b_w, b = a_w.to(dt), b_w.to(dt), b.to(dt)
    if normalize:
        a, b = unit(a), unit(b)
    ma = torch.arange(a.shape[1])[None, :] < torch.as_tensor(a_len).long()[:, None]            # (N, La)
    mb = torch.arange(b.shape[1])[None, :] < torch.as_tensor(b_len).long()[:, None]            # (C, Lb)
    s = torch.einsum("nid,cjd->ncij", a, b)
    ninf = torch.tensor(float("-inf"), dtype=dt)
    zero = torch.zeros((), dtype=dt)
    row_max = torch.where(mb[None, :, None, :], s, ninf).amax(dim=3)                            # (N, C, La)
    col_max = torch.where(ma[:, None, :, None], s, ninf).amax(dim=2)                            # (N, C, Lb)
    p_sum = torch.where(ma[:, None, :], a_w[:, None, :] * row_max, zero).sum(dim=2)
    r_sum = torch.where(mb[None, :, :], b_w[None, :, :] * col_max, zero).sum(dim=2)
    wa = torch.where(ma, a_w, zero).sum(dim=1)[:, None]
    wb = torch.where(mb, b_w, zero).sum(dim=1)[None, :]
    one = torch.ones((), dtype=dt)
    P = torch.where(wa != 0, p_sum / torch.where(wa != 0, wa, one), zero).expand_as(p_sum)
    R = torch.where(wb != 0, r_sum / torch.where(wb != 0, wb, one), zero).expand_as(r_sum)
    den = P + R
    F = torch.where(den != 0, 2 * P * R / torch.where(den != 0, den, one), zero)
    return torch.stack([P, R, F])


def select(prf):
    """(3, N, C) -> (best int64 (N,) = argmax_c F with ties to the lowest c, best_f, best_p, best_r)"""
    f = prf[2].numpy()
    best = np.argmax(f, axis=1)                          # (numpy returns the first of equal maxima)
    rows = np.arange(f.shape[0])
    return best, f[rows, best], prf[0].numpy()[rows, best], prf[1].numpy()[rows, best]


def top_two_gap(prf):
    """per row the difference of the two largest F (inf with a single label)"""
    f = np.sort(prf[2].numpy().astype(np.float64), axis=1)
    return f[:, -1] - f[:, -2] if f.shape[1] > 1 else np.full(f.shape[0], np.inf)


def rel_err(x, ref):
    """max |x - ref| relative to the largest entry of ref"""
    x, ref = torch.as_tensor(x).double(), torch.as_tensor(ref).double()
    return ((x - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def random_lengths(g, rows, L):
    """random in 1 .. L, item 0 at full length and the last item at length 1 (one item: full length)"""
    lens = torch.randint(1, L + 1, (rows,), generator=g)
    lens[-1] = 1
    lens[0] = L
    return lens.to(torch.int32)


def make_case(seed, N, C, La, Lb, D, sign=1.0, noise=0.25):
    """Float32 inputs with positive cosines and a planted answer: every token is scale * unit(g + common) with ||g|| ~ 1 and a
    unit ``common``; the tokens of phrase n are noisy copies of the tokens of label plant[n] (token i of token i % b_len).
    sign = -1 puts the phrases near +common and the labels near -common: every cosine is negative.  The tokens are not unit
    (scale in [0.5, 2]) and the positions past a length hold values that must not be used.  Weights are in [0.5, 1.5]."""
    g = torch.Generator().manual_seed(seed)

    def randn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    common = unit(randn(D))
    a_len, b_len = random_lengths(g, N, La), random_lengths(g, C, Lb)
    b = unit(randn(C, Lb, D) / D ** 0.5 + common)
    plant = torch.randint(0, C, (N,), generator=g)
    j = torch.arange(La)[None, :] % b_len.long()[plant][:, None]                                  # (N, La)
    a = unit(b[plant[:, None], j] + noise * randn(N, La, D) / D ** 0.5)
    if sign < 0:
        a = unit(randn(N, La, D) / D ** 0.5 + common)
        b = unit(randn(C, Lb, D) / D ** 0.5 - common)
    a = a * (0.5 + 1.5 * torch.rand(N, La, 1, generator=g, dtype=torch.float64))
    b = b * (0.5 + 1.5 * torch.rand(C, Lb, 1, generator=g, dtype=torch.float64))
    # what stands past a length points where it would score high (positive in the all-negative case): a maximum or a sum that
    # lets it in is far off
    a = torch.where(torch.arange(La)[None, :, None] < a_len.long()[:, None, None], a, sign * 3.0 * common.expand_as(a))
    b = torch.where(torch.arange(Lb)[None, :, None] < b_len.long()[:, None, None], b, 3.0 * common.expand_as(b))
    a_w = 0.5 + torch.rand(N, La, generator=g)
    b_w = 0.5 + torch.rand(C, Lb, generator=g)
    return dict(a=a.float(), a_len=a_len, a_w=a_w.float(), b=b.float(), b_len=b_len, b_w=b_w.float(), plant=plant)


def host_bertscore_map(a, a_len, a_w, b, b_len, b_w, want_scores=False, normalize=True):
    """dispatch.bertscore_map restated on the host in float64 (for the tests that patch it in): the same named tuple, of CPU
    tensors, and the same defaults."""
    from texttoaudiogrounding_amd.dispatch import BertScoreMapResult
    a_len = torch.full((a.shape[0],), a.shape[1]) if a_len is None else a_len
    b_len = torch.full((b.shape[0],), b.shape[1]) if b_len is None else b_len
    a_w = default_weights(a_len, a.shape[1]) if a_w is None else a_w
    b_w = default_weights(b_len, b.shape[1]) if b_w is None else b_w
    prf = scores(a.double(), a_len, a_w, b.double(), b_len, b_w, normalize=normalize).float()
    best, f, p, r = select(prf)
    return BertScoreMapResult(torch.from_numpy(best).int(), torch.from_numpy(f), torch.from_numpy(p), torch.from_numpy(r),
                              prf if want_scores else None)
