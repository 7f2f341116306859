"""Phrase occurrence statistics of weak phrase training: the ``phrase_count`` JSON that ``SamplePhrasesCountDataset`` loads and
``ClipBceLossFreqWeight`` / ``PriorAdjustedClipBceLoss`` read as ``output["counts"]``.

* ``phrase_count``      mirror of utils/data/calc_phrase_count.py in the reference: how many label entries name each phrase.
* ``phrase_sim_count``  mirror of utils/data/calc_phrase_sim_count.py: for every phrase the summed counts of all phrases whose
  embedding has cosine >= threshold with it.  The reference makes one 1 x N ``cosine_similarity`` call per phrase on the host;
  here the stacked table goes through ONE ``ops.phrase_sim_count`` call (phrase_sim.hip: fp32 products on the MFMA, no N x N
  matrix).  Both compute the cosine in fp32 from the fp32 embeddings, so a pair can differ only where its cosine lies within
  rounding (about D * 2^-24) of the threshold.
"""
from typing import Dict, Iterable, Mapping

import numpy as np
import torch


def phrase_count(label_data: Iterable[Mapping]) -> Dict[str, int]:
    """label_data: the strong label list (``{"phrases": [{"phrase": ...}, ...]}`` per clip) -> {phrase: occurrences}, keys in
    order of first appearance."""
    counts: Dict[str, int] = {}
    for clip in label_data:
        for entry in clip["phrases"]:
            counts[entry["phrase"]] = counts.get(entry["phrase"], 0) + 1
    return counts


def phrase_sim_count(phrase_to_emb: Mapping[str, np.ndarray], phrase_to_count: Mapping[str, int], threshold: float = 0.5,
                     device="cuda") -> Dict[str, int]:
    """{phrase: sum of phrase_to_count over the phrases with cosine >= threshold to it}, in phrase_to_emb's order, Python ints."""
    from .. import ops
    phrases = list(phrase_to_emb)
    table = np.stack([np.asarray(phrase_to_emb[p], dtype=np.float32).reshape(-1) for p in phrases])
    counts = np.array([int(phrase_to_count[p]) for p in phrases], dtype=np.int64)
    bank = torch.from_numpy(table).to(device)
    out = ops.phrase_sim_count(bank, bank, torch.from_numpy(counts).to(device), threshold=threshold, normalize=True)
    return {p: int(c) for p, c in zip(phrases, out.cpu().tolist())}
