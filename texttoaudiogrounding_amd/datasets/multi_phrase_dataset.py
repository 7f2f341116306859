"""Weakly supervised (clip, phrases) datasets (mirror of datasets/multi_phrase_dataset.py:51-339 in the reference): an item is a
clip, its positive phrases (cut to ``phrase_num``) and sampled negatives that fill up to ``phrase_num`` --
``{"waveform": float32 array, "phrases": list[str], "label": int array (1 positive, 0 negative)}``, plus ``"counts"`` for
``SamplePhrasesCountDataset`` (filled for the ``similarity`` strategy only, as in the reference).

Label JSON: a list of clips ``{"audio_id", "phrases": [str, ...]}``.  Negative strategies:

* ``random``      uniform over the pool without the clip's positives;
* ``clustering``  (``cluster_map``: JSON {cluster index: [phrases]}) one phrase from each of as many clusters that hold no
  positive; with fewer such clusters than negatives every cluster is drawn from several times;
* ``similarity``  (``phrase_embed``: pickle {phrase: vector}, ``sim_threshold``; optional ``negative_pool``: one phrase per
  line, replaces the pool) candidates in shuffled order whose largest cosine to a positive is below the threshold; too few
  passing candidates are repeated cyclically.

``fix_neg`` remembers a clip's negatives (pool indices) from its first visit.  The draws go through the same ``np.random`` /
``random`` calls in the same order as the reference, so under equal seeds (and an equal pool order) an item is identical to
the reference's.  Differences, all in INTEGRATION.md: the pool is sorted (the reference's ``list(set(...))`` order changes with
the process's string hash seed); the cosine is a numpy normalise-and-dot (no sklearn); waveforms come through
``WaveformStore``; the ``random`` strategy draws pool indices of the same count instead of copying the string pool per item;
and where the reference would loop forever (no candidate passes and there is nothing to repeat; no cluster without a positive;
an empty ``fix_neg`` memory that has to grow) a ValueError names the clip.
"""
import json
import pickle
import random
from typing import Dict, List, Tuple

import numpy as np

from .waveform_store import WaveformStore

STRATEGIES = ("random", "clustering", "similarity")


def _unit_rows(x: np.ndarray) -> np.ndarray:
    """Rows over their norms in the array's own precision (sklearn's normalize: an all-zero row stays zero)."""
    x = np.asarray(x)
    if not np.issubdtype(x.dtype, np.floating):
        x = x.astype(np.float64)
    norms = np.sqrt((x * x).sum(axis=1, keepdims=True))
    norms[norms == 0.0] = 1.0
    return x / norms


class AudioSamplePhrasesDataset:
    def __init__(self, audio, label, phrase_num: int, fix_neg: bool, neg_samp_stratg: str = "clustering",
                 max_phrase_length: int = None, sample_rate: int = 32000, max_audio_length: float = None, **kwargs):
        assert neg_samp_stratg in STRATEGIES
        self.store = audio if isinstance(audio, WaveformStore) else WaveformStore(audio)
        self.sample_rate = sample_rate
        self.max_audio_len = None if max_audio_length is None else int(max_audio_length * sample_rate)
        self.max_phrase_len = max_phrase_length
        self.phrase_num = phrase_num
        self.neg_samp_stratg = neg_samp_stratg
        self.fix_neg = fix_neg
        if fix_neg:
            self.aid_to_neg: Dict[str, List[int]] = {}

        clips = []
        for path in ([label] if isinstance(label, str) else list(label)):
            with open(path) as f:
                clips.extend(json.load(f))
        # clips without a phrase of admissible length are dropped; the pool is every admissible phrase
        pool = set()
        self.data = []
        for clip in clips:
            admitted = [p for p in clip["phrases"] if self._admits(p)]
            pool.update(admitted)
            if admitted:
                self.data.append(clip)
        self._set_pool(sorted(pool))

        if neg_samp_stratg == "clustering":
            assert "cluster_map" in kwargs, "cluster_map not provided"
            self.cluster_idx_to_phrases, self.phrase_to_cluster_idx = self.read_cluster_map(kwargs["cluster_map"])
            self.cluster_idxs = np.array(list(self.cluster_idx_to_phrases.keys()))
            self.cluster_idx_to_idx = {c: i for i, c in enumerate(self.cluster_idxs)}
        elif neg_samp_stratg == "similarity":
            assert "phrase_embed" in kwargs, "phrase_embed not provided"
            assert "sim_threshold" in kwargs, "sim_threshold not provided"
            self.sim_threshold = kwargs["sim_threshold"]
            self.phrase_to_emb = self._read_embeddings(kwargs["phrase_embed"])
            if "negative_pool" in kwargs:
                with open(kwargs["negative_pool"]) as f:
                    listed = [line.strip() for line in f.readlines()]
                self._set_pool([p for p in listed if self._admits(p)])      # in the file's order
            in_pool = set(self.phrases.tolist())
            self.phrase_to_emb = {p: e for p, e in self.phrase_to_emb.items() if p in in_pool}
            self.phrase_embs = np.stack([self.phrase_to_emb[p] for p in self.phrases])
            self._unit_embs = _unit_rows(self.phrase_embs)

    def _admits(self, phrase: str) -> bool:
        return self.max_phrase_len is None or len(phrase.split()) <= self.max_phrase_len

    def _set_pool(self, phrases: List[str]):
        self.phrases = np.array(phrases)
        self.phrase_to_idx = {p: i for i, p in enumerate(phrases)}

    def _read_embeddings(self, path: str) -> Dict[str, np.ndarray]:
        if path.endswith(".pkl"):
            with open(path, "rb") as f:
                return pickle.load(f)
        if path.endswith((".hdf5", ".h5")):
            try:
                import h5py
            except ImportError as e:
                raise RuntimeError(f"{path}: reading HDF5 phrase embeddings needs h5py; store them as a .pkl of "
                                   "{phrase: vector}") from e
            with h5py.File(path, "r") as store:
                return {p: store[p.replace("/", "%2F")][()] for p in self.phrases.tolist()}
        raise ValueError(f"phrase_embed {path!r}: expected a .pkl, .h5 or .hdf5 file")

    def read_cluster_map(self, cluster_map: str) -> Tuple[Dict[int, List[str]], Dict[str, int]]:
        """-> ({cluster: its phrases that are in the pool and admissible}, {every listed phrase: cluster}), in the file's order."""
        with open(cluster_map) as f:
            mapping = json.load(f)
        in_pool = set(self.phrases.tolist())
        members, owner = {}, {}
        for key, listed in mapping.items():
            cluster = int(key)
            for p in listed:
                owner[p] = cluster
            members[cluster] = [p for p in listed if p in in_pool and self._admits(p)]
        return members, owner

    # ---- negatives ----------------------------------------------------------------------------------------------------
    def sample_negative_phrases(self, pos_phrases: List[str], audio_id: str):
        want = max(0, self.phrase_num - len(pos_phrases))
        if self.fix_neg and audio_id in self.aid_to_neg:
            kept = self.aid_to_neg[audio_id]
            if len(kept) < want:
                if not kept:
                    raise ValueError(f"clip {audio_id!r}: {want} negatives wanted but none were found on its first visit")
                while len(kept) < want:
                    kept.extend(kept)               # (the remembered list itself grows, as in the reference)
            return [self.phrases[i] for i in kept[:want]]

        pos_idxs = [self.phrase_to_idx[p] for p in pos_phrases]
        cand_idxs = np.delete(np.arange(len(self.phrases)), pos_idxs)
        if self.neg_samp_stratg == "random":
            # the reference draws from the pool's strings with the positives deleted: the same positions of an equally long array
            negatives = self.phrases[np.random.choice(cand_idxs, size=want, replace=False)]
        elif self.neg_samp_stratg == "similarity":
            negatives = self.phrases[self._dissimilar(pos_idxs, cand_idxs, want, audio_id)]
        else:
            negatives = self._other_clusters(pos_phrases, want, audio_id)
        while len(negatives) < want:
            negatives.append(negatives[-1])
        if self.fix_neg:
            self.aid_to_neg[audio_id] = [self.phrase_to_idx[p] for p in negatives]
        return negatives

    def _dissimilar(self, pos_idxs, cand_idxs, want, audio_id) -> List[int]:
        pos = self._unit_embs[pos_idxs]
        np.random.shuffle(cand_idxs)
        found: List[int] = []
        at = 0
        while len(found) < want and at < len(cand_idxs):
            part = cand_idxs[at:at + want]
            closest = (pos @ self._unit_embs[part].T).max(axis=0)
            passing = np.where(closest < self.sim_threshold)[0]
            found.extend(part[passing[:want - len(found)]])
            at += want
        if want > 0 and not found:
            raise ValueError(f"clip {audio_id!r}: no phrase of the pool has every cosine to its positives below sim_threshold = "
                             f"{self.sim_threshold}, so there is no negative to sample or to repeat")
        while len(found) < want:
            found.extend(found[:want - len(found)])
        return found

    def _other_clusters(self, pos_phrases, want, audio_id) -> List[str]:
        taken = list({self.phrase_to_cluster_idx[p] for p in pos_phrases})
        cand = np.delete(self.cluster_idxs, [self.cluster_idx_to_idx[c] for c in taken])
        negatives: List[str] = []
        if want > 0 and len(cand) == 0:
            raise ValueError(f"clip {audio_id!r}: its positives lie in every cluster, so there is no cluster to draw {want} "
                             "negatives from")
        if len(cand) >= want:
            for cluster in np.random.choice(cand, size=want, replace=False):
                if len(self.cluster_idx_to_phrases[cluster]) > 0:
                    negatives.append(np.random.choice(self.cluster_idx_to_phrases[cluster]))
        else:
            # fewer clusters than negatives: every cluster gives floor((want - 1) / len) phrases, the remainder goes to clusters
            # drawn without replacement
            each, rest = np.zeros_like(cand), want
            while rest > len(cand):
                each += 1
                rest -= len(cand)
            if rest > 0:
                each[np.random.choice(np.arange(len(cand)), size=rest, replace=False)] += 1
            for cluster, n in zip(cand, each):
                negatives.extend(np.random.choice(self.cluster_idx_to_phrases[cluster], size=n, replace=False).tolist())
        return negatives

    # ---- items --------------------------------------------------------------------------------------------------------
    def __getitem__(self, index):
        clip = self.data[index]
        audio_id = clip["audio_id"]
        waveform = self.store[audio_id]
        if self.max_audio_len is not None and waveform.shape[0] > self.max_audio_len:
            start = random.randint(0, waveform.shape[0] - self.max_audio_len)
            waveform = waveform[start:start + self.max_audio_len]
        positives = [p for p in clip["phrases"][:self.phrase_num] if self._admits(p)]
        negatives = self.sample_negative_phrases(positives, audio_id)
        if isinstance(negatives, np.ndarray):
            negatives = negatives.tolist()
        return {"waveform": waveform, "phrases": positives + negatives,
                "label": np.array([1] * len(positives) + [0] * len(negatives))}

    def __len__(self):
        return len(self.data)


class SamplePhrasesCountDataset(AudioSamplePhrasesDataset):
    """... plus ``counts``: the ``phrase_count`` JSON's entry of every phrase of the item ({phrase: count}, written by
    tools/calc_phrase_count.py or tools/calc_phrase_sim_count.py); read by ClipBceLossFreqWeight / PriorAdjustedClipBceLoss."""

    def __init__(self, waveform, label, phrase_num: int, fix_neg: bool, neg_samp_stratg: str = "clustering",
                 max_phrase_length: int = None, sample_rate: int = 32000, max_audio_length: float = None, **kwargs):
        super().__init__(waveform, label, phrase_num, fix_neg, neg_samp_stratg, max_phrase_length, sample_rate,
                         max_audio_length, **kwargs)
        assert "phrase_count" in kwargs
        with open(kwargs["phrase_count"]) as f:
            self.phrase_to_count = json.load(f)

    def __getitem__(self, index):
        item = super().__getitem__(index)
        item["counts"] = ([self.phrase_to_count[p] for p in item["phrases"]] if self.neg_samp_stratg == "similarity" else [])
        return item
