"""Phrases -> AudioSet label indices through BERTScore: what utils/data/create_phrase_event_mapping/prepare_phrase_bertscore.py in
the reference does with ``bert_score.score`` on every (phrase, label) pair, re-encoding both texts of each pair through a
transformer.  The score is a function of the TOKEN embeddings of the phrases and of the labels alone, so here both are encoded
once (by the caller) and one fused kernel does the all-pairs greedy matching (csrc/bertscore.hip, ``dispatch.bertscore_map``).

The rule, with unit token vectors and s_ij = a_i . b_j over the tokens of phrase a and label b:

    P = sum_i wa_i max_j s_ij / sum_i wa_i      R = sum_j wb_j max_i s_ij / sum_j wb_j      F = 2 P R / (P + R)

a zero weight sum giving P = 0 (R = 0) and P + R == 0 giving F = 0; a phrase maps to argmax_c F, ties to the lowest index.  The
weights (``token_weights``) are bert_score's with ``idf=False``: 1 for every token except 0 for the first and the last of an item,
its [CLS] and [SEP]; ``special_tokens=False`` weighs every token 1, for embeddings that carry no special tokens.

Parity with the ``bert_score`` package is UNPINNED: the package is neither installed beside this project nor vendored in the
reference, so no test compares against it; the rule above is its published algorithm as restated here (tests/bertscore_ref.py
is the fp64 restatement the kernel is tested against).  Known differences from the package:

* the package multiplies the scores of padded positions by 0 and lets them into the maxima; here a padded position enters no
  maximum.  The two differ only where every valid cosine of a pair is negative and the batch was padded;
* baseline rescaling and idf tables are out of scope (idf weights can be passed as ``phrase_weights`` / ``label_weights``).

``BertScoreMap(label_tokens, device, chunk_rows)`` keeps the labels on the device; ``map(phrase_tokens)`` takes a list of (L_i, D)
arrays, 1 <= L_i <= 32, runs ``chunk_rows`` phrases per call and returns numpy arrays.  There is no CPU fallback.
"""
import collections

import numpy as np

#: the longest item (tokens, special tokens included) the kernel takes
MAX_TOKENS = 32

BertScoreMapping = collections.namedtuple("BertScoreMapping", "best best_f best_p best_r scores")


def token_weights(lengths, L, special_tokens=True):
    """(rows, L) float32: 1 below the length, and with ``special_tokens`` 0 for the first and the last token of every item (an
    item of one or two tokens then has no weight left: its P, or R, is 0)."""
    n = np.asarray(lengths, dtype=np.int64)[:, None]
    pos = np.arange(int(L), dtype=np.int64)[None, :]
    inside = (pos >= 1) & (pos < n - 1) if special_tokens else pos < n
    return inside.astype(np.float32)


def pack_tokens(items, dim=None, name="tokens"):
    """A list of (L_i, D) arrays -> (tokens (rows, max L_i, D) float32 zero-padded, lengths (rows,) int32)."""
    arrs = [np.asarray(v, dtype=np.float32) for v in items]
    if not arrs:
        raise ValueError(f"{name}: expected at least one item")
    D = arrs[0].shape[-1] if arrs[0].ndim == 2 else -1
    for k, v in enumerate(arrs):
        if v.ndim != 2 or v.shape[1] != D or D < 1 or (dim is not None and D != dim):
            raise ValueError(f"{name}[{k}]: expected a (L, {D if dim is None else dim}) array, got {v.shape}")
        if not 1 <= v.shape[0] <= MAX_TOKENS:
            raise ValueError(f"{name}[{k}]: {v.shape[0]} tokens; an item has 1 .. {MAX_TOKENS} tokens")
    lengths = np.array([v.shape[0] for v in arrs], dtype=np.int32)
    out = np.zeros((len(arrs), int(lengths.max()), D), dtype=np.float32)
    for k, v in enumerate(arrs):
        out[k, : v.shape[0]] = v
    return out, lengths


class BertScoreMap:
    def __init__(self, label_tokens, device="cuda:0", chunk_rows=1 << 15, special_tokens=True, label_weights=None):
        self.labels, self.label_len = pack_tokens(label_tokens, name="label_tokens")
        self.classes_num, _, self.dim = self.labels.shape
        self.special_tokens = bool(special_tokens)
        self.label_w = self._weights(label_weights, self.label_len, self.labels.shape[1], "label_weights")
        self.device = device
        self.chunk_rows = int(chunk_rows)
        if self.chunk_rows < 1:
            raise ValueError(f"chunk_rows = {chunk_rows} must be >= 1")
        self._dev = None

    def _weights(self, given, lengths, L, name):
        if given is None:
            return token_weights(lengths, L, self.special_tokens)
        w = np.zeros((len(lengths), L), dtype=np.float32)
        if len(given) != len(lengths):
            raise ValueError(f"{name}: {len(given)} weight rows for {len(lengths)} items")
        for k, row in enumerate(given):
            row = np.asarray(row, dtype=np.float32).reshape(-1)
            if row.shape[0] != lengths[k]:
                raise ValueError(f"{name}[{k}]: {row.shape[0]} weights for {lengths[k]} tokens")
            w[k, : row.shape[0]] = row
        return w

    def _call(self, tok, lens, w, want_scores):
        """One chunk of phrases on the device -> numpy (best, best_f, best_p, best_r, scores or None)."""
        import torch
        from .. import dispatch
        if self._dev is None:
            self._dev = tuple(torch.from_numpy(x).to(self.device) for x in (self.labels, self.label_len, self.label_w))
        a, a_len, a_w = (torch.from_numpy(np.ascontiguousarray(x)).to(self.device) for x in (tok, lens, w))
        res = dispatch.bertscore_map(a, a_len, a_w, self._dev[0], self._dev[1], self._dev[2], want_scores=want_scores)
        return tuple(None if t is None else t.cpu().numpy() for t in (res.best, res.best_f, res.best_p, res.best_r, res.scores))

    def map(self, phrase_tokens, phrase_weights=None, want_scores=False):
        """-> BertScoreMapping(best int64 (N,), best_f, best_p, best_r float32 (N,), scores float32 (3, N, C) = P, R, F or None)"""
        tok, lens = pack_tokens(phrase_tokens, dim=self.dim, name="phrase_tokens")
        w = self._weights(phrase_weights, lens, tok.shape[1], "phrase_weights")
        parts = []
        for r0 in range(0, tok.shape[0], self.chunk_rows):
            r1 = r0 + self.chunk_rows
            L = int(lens[r0:r1].max())                # (a chunk is as wide as its longest phrase)
            parts.append(self._call(tok[r0:r1, :L], lens[r0:r1], w[r0:r1, :L], want_scores))
        best, best_f, best_p, best_r, scores = zip(*parts)
        return BertScoreMapping(np.concatenate(best).astype(np.int64), np.concatenate(best_f), np.concatenate(best_p),
                                np.concatenate(best_r), np.concatenate(scores, axis=1) if want_scores else None)
