"""Phrases -> AudioSet label indices through the cosine similarity of their embeddings: what ``ASMappingEvalDataset``,
``ASMappingWeakDataset`` (``assign_phrase_label``, ``calc_thresholds``), ``ASMappingStrongDataset`` and
``ASMappingEvalLabelSimDataset`` of datasets/class_mapping_dataset.py and utils/data/map_phrase_to_event.py in the reference do
with sklearn's ``cosine_similarity(phrase_emb, label_embs)`` on the host, one phrase per call.

``LabelMap(label_embs, device)`` keeps the (C, D) label embeddings on the device; ``map(phrase_embs, thresholds, topk)`` is ONE
``ops.label_map`` call over all phrases (csrc/label_map.hip; row chunks of ``chunk_rows`` when N is large) and returns numpy
arrays: ``best`` (the argmax over all labels, the eval datasets' ``text_idx``), ``best_sim`` (that similarity: the tool's ``sim``
column and the input of the ``min_sim_percent`` percentile), ``labels`` (per phrase the int64 indices the phrase labels) and
optionally ``sim`` (N, C) float32.

A phrase labels only members of its WINDOW, the labels with thresholds[0] <= sim <= thresholds[1] and sim != 0 (the comparisons
in float32, as numpy compares the reference's float32 similarities with a Python float or a float32 percentile):
``topk`` == 1 the window's best, ``topk`` >= 2 its best ``topk`` in descending similarity, ``topk`` <= 0 all of them in ascending
index (``np.where``).  Ties go to the lowest index.  An empty window labels nothing.  There is no CPU fallback.
"""
import collections

import numpy as np

LabelMapping = collections.namedtuple("LabelMapping", "best best_sim labels sim")

_EMPTY = np.zeros(0, dtype=np.int64)


def stack_embeddings(table):
    """The values of an embedding pickle's dict, in insertion order, as one float32 (rows, D) array."""
    return np.stack([np.asarray(v, dtype=np.float32).reshape(-1) for v in table.values()])


def window_members(win_bits, C):
    """(N, ceil(C / 32)) words of ``ops.label_map`` -> (N, C) bool."""
    words = np.ascontiguousarray(win_bits).view(np.uint32)
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return bits.reshape(words.shape[0], -1)[:, :C].astype(bool)


class LabelMap:
    def __init__(self, label_embs, device="cuda:0", chunk_rows=1 << 18):
        self.label_embs = np.array(label_embs, dtype=np.float32, order="C")       # (a copy: torch wants writable memory)
        if self.label_embs.ndim != 2 or self.label_embs.shape[0] < 1 or self.label_embs.shape[1] < 1:
            raise ValueError(f"label_embs: expected a (C >= 1, D >= 1) array, got {self.label_embs.shape}")
        self.classes_num, self.dim = self.label_embs.shape
        self.device = device
        self.chunk_rows = int(chunk_rows)
        self._labels_dev = None

    def _call(self, x, th0, th1, topk, want_sim):
        """One chunk of rows on the device -> numpy (best, best_sim, win_best, win_bits, idx or None, sim or None)."""
        import torch
        from .. import ops
        if self._labels_dev is None:
            self._labels_dev = torch.from_numpy(self.label_embs).to(self.device)
        res = ops.label_map(torch.from_numpy(x).to(self.device), self._labels_dev, th0, th1, topk=topk, want_sim=want_sim)
        host = [None if t is None else t.cpu().numpy() for t in (res.best, res.best_sim, res.win_best, res.win_bits, res.idx, res.sim)]
        return tuple(host)

    def map(self, phrase_embs, thresholds=None, topk=1, want_sim=False):
        """-> LabelMapping(best int64 (N,), best_sim float32 (N,), labels: a list of N int64 arrays, sim float32 (N, C) or None).
        thresholds: (low, high), None for the whole line (every label with a non-zero similarity is a window member)."""
        x = np.array(phrase_embs, dtype=np.float32, order="C")
        if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] != self.dim:
            raise ValueError(f"phrase_embs: expected a (N >= 1, {self.dim}) array, got {x.shape}")
        th0, th1 = (-np.inf, np.inf) if thresholds is None else (float(np.float32(thresholds[0])), float(np.float32(thresholds[1])))
        topk = int(topk)
        best, best_sim, labels, sims = [], [], [], []
        for r0 in range(0, x.shape[0], self.chunk_rows):
            b, bs, wb, bits, idx, sim = self._call(x[r0: r0 + self.chunk_rows], th0, th1, topk, want_sim)
            best.append(b.astype(np.int64))
            best_sim.append(bs)
            sims.append(sim)
            if topk <= 0:
                labels += [np.flatnonzero(row) for row in window_members(bits, self.classes_num)]
            elif idx is not None:
                labels += [row[row >= 0].astype(np.int64) for row in idx]
            else:
                labels += [np.array([w], dtype=np.int64) if w >= 0 else _EMPTY for w in wb]
        return LabelMapping(np.concatenate(best), np.concatenate(best_sim), labels, np.concatenate(sims) if want_sim else None)
