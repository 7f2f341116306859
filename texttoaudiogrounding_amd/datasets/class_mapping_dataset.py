"""The cluster class-mapping datasets (mirror of ``KmeansMappingDataset``, ``KmeansMappingEvalDataset``, ``SpectralMappingDataset``
and ``SpectralMappingEvalDataset`` of datasets/class_mapping_dataset.py in the reference): phrases become class indices through a
k-means model over the phrase embeddings or through a cluster-map JSON, and ``AudioTagging`` / ``ClassMappingRunner`` train and
evaluate on those classes.

Label JSON: a list of clips ``{"audio_id", "audiocap_id", "tokens", "phrases": [{"phrase", "start_index", "end_index",
"segments": [[start, end], ...]}, ...]}``.

* ``KmeansMappingDataset``  one item per clip: ``audiocap_id``, ``audio_id``, ``text`` (the caption tokens), ``waveform`` (unless
  ``no_waveform``) and, for ``label_type="weak"``, ``label`` (classes_num,), or for ``"strong"``, ``weak_label`` and
  ``strong_label`` (n_frame, classes_num) with n_frame = floor(duration / time_resolution) + 1 and segments set from
  round(start / time_resolution) to round(end / time_resolution).  A phrase labels its cluster only when its distance to the
  cluster centre is <= the ``max_dist_percent`` percentile of all phrases' distances.  Clips longer than ``max_audio_length``
  seconds are cropped at ``random.randint``.
* ``KmeansMappingEvalDataset``  one item per (clip, phrase): the clip's fields plus ``text_idx`` (the phrase's cluster),
  ``start_index`` and ``end_index``.
* ``SpectralMappingDataset`` / ``SpectralMappingEvalDataset``  the same items from a ``cluster_map`` JSON ``{str(cluster index):
  [phrases ...]}`` of ANY clustering method (tools/kmeans_emb.py, tools/dbscan_emb.py, tools/agc_emb.py and tools/spectral_emb.py,
  the script the classes are named after, or the reference's own scripts): host-only, no model, no embeddings and no distance filter.  As in the reference ``classes_num`` is the number of
  keys, a DBSCAN map's ``"-1"`` key included, and the phrases under ``"-1"`` index class -1 (the last column).

Differences from the reference: waveforms come through ``WaveformStore``; ``cluster_model`` is read by
``utils.phrase_cluster.load_cluster_centers`` (an ``.npz`` of ``KMeans.save`` natively, a joblib checkpoint of sklearn's KMeans when
joblib is importable); labels and distances come from ONE assignment call on the device (``device`` keyword, csrc/kmeans.hip)
instead of ``predict`` plus ``transform(...).min(1)``; the distinct phrases are taken in order of first appearance (the
reference's ``list(set(...))`` order changes nothing it computes).
"""
import json
import math
import pickle
import random

import numpy as np

from .waveform_store import WaveformStore


class _MappingBase:
    """The clips and the items of all four datasets; a subclass sets ``phrase_to_label`` and ``classes_num``."""

    def _read_clips(self, waveform, label):
        self.store = waveform if isinstance(waveform, WaveformStore) else WaveformStore(waveform)
        with open(label) as f:
            self.data = json.load(f)

    def _read_cluster_map(self, cluster_map):
        with open(cluster_map) as f:
            self.cluster_map = json.load(f)
        self.phrase_to_label = {phrase: int(idx) for idx, phrases in self.cluster_map.items() for phrase in phrases}
        self.classes_num = len(self.cluster_map)

    def _keeps(self, phrase):
        return True

    def _phrase_item(self, index):
        audio_idx, phrase_idx = self.idxs[index]
        item = self.data[audio_idx]
        phrase_item = item["phrases"][phrase_idx]
        return {
            "audiocap_id": item["audiocap_id"],
            "audio_id": item["audio_id"],
            "text": item["tokens"],
            "waveform": self.store[item["audio_id"]],
            "text_idx": self.phrase_to_label[phrase_item["phrase"]],
            "start_index": phrase_item["start_index"],
            "end_index": phrase_item["end_index"],
        }

    def _clip_item(self, index):
        item = self.data[index]
        waveform = self.store[item["audio_id"]]
        if self.max_audio_len is not None and waveform.shape[0] > self.max_audio_len:
            start = random.randint(0, waveform.shape[0] - self.max_audio_len)
            waveform = waveform[start: start + self.max_audio_len]
        output = {"audiocap_id": item["audiocap_id"], "audio_id": item["audio_id"], "text": item["tokens"]}
        if not self.no_waveform:
            output["waveform"] = waveform
        kept = [p for p in item["phrases"] if self._keeps(p["phrase"])]
        if self.label_type == "weak":
            label = np.zeros(self.classes_num)
            for phrase_item in kept:
                label[self.phrase_to_label[phrase_item["phrase"]]] = 1
            output["label"] = label
        else:
            n_frame = math.floor(waveform.shape[0] / self.sample_rate / self.time_resolution) + 1
            weak_label = np.zeros(self.classes_num)
            strong_label = np.zeros((n_frame, self.classes_num))
            for phrase_item in kept:
                label_idx = self.phrase_to_label[phrase_item["phrase"]]
                weak_label[label_idx] = 1
                for start, end in phrase_item["segments"]:
                    onset = round(start / self.time_resolution)
                    offset = round(end / self.time_resolution)
                    strong_label[onset: offset, label_idx] = 1
            output["weak_label"] = weak_label
            output["strong_label"] = strong_label
        return output

    def _clip_settings(self, label_type, time_resolution, sample_rate, max_audio_length, no_waveform):
        assert label_type in ("weak", "strong")
        self.label_type = label_type
        self.time_resolution = time_resolution
        self.sample_rate = sample_rate
        self.no_waveform = no_waveform
        self.max_audio_len = None if max_audio_length is None else int(max_audio_length * sample_rate)


class _KmeansMappingBase(_MappingBase):
    def _read(self, waveform, label, phrase_embed, cluster_model, device):
        from ..utils.phrase_cluster import KMeans, load_cluster_centers
        self._read_clips(waveform, label)
        self.cluster_model = KMeans.from_centers(load_cluster_centers(cluster_model), device=device)
        self.classes_num = self.cluster_model.n_clusters
        with open(phrase_embed, "rb") as f:
            self.phrase_to_emb = pickle.load(f)

    def _phrase_labels(self):
        """-> (distinct phrases in order of first appearance, their labels, their distances to the assigned centre)"""
        phrases = list(dict.fromkeys(p["phrase"] for item in self.data for p in item["phrases"]))
        embs = np.stack([np.asarray(self.phrase_to_emb[p], dtype=np.float32).reshape(-1) for p in phrases])
        labels, distances = self.cluster_model.predict_min_distance(embs)
        return phrases, labels, distances


class KmeansMappingEvalDataset(_KmeansMappingBase):
    def __init__(self, waveform, label: str, phrase_embed: str, cluster_model: str, device="cuda:0"):
        self._read(waveform, label, phrase_embed, cluster_model, device)
        self.prepare_phrase_label()
        self.generate_index()

    def generate_index(self):
        self.idxs = [(a, p) for a, item in enumerate(self.data) for p in range(len(item["phrases"]))]

    def prepare_phrase_label(self):
        phrases, labels, _ = self._phrase_labels()
        self.phrase_to_label = dict(zip(phrases, labels))

    def __getitem__(self, index):
        return self._phrase_item(index)

    def __len__(self):
        return len(self.idxs)


class KmeansMappingDataset(_KmeansMappingBase):
    def __init__(self, waveform, label: str, phrase_embed: str, cluster_model: str, label_type: str = "weak",
                 max_dist_percent: float = 95.0, time_resolution: float = 0.02, sample_rate: int = 32000,
                 max_audio_length: float = None, no_waveform: bool = False, device="cuda:0"):
        self._read(waveform, label, phrase_embed, cluster_model, device)
        self._clip_settings(label_type, time_resolution, sample_rate, max_audio_length, no_waveform)
        self.max_dist_percent = max_dist_percent
        self.prepare_phrase_label()

    def prepare_phrase_label(self):
        phrases, labels, distances = self._phrase_labels()
        self.max_distance = np.percentile(distances, self.max_dist_percent)
        self.phrase_to_label = dict(zip(phrases, labels))
        self.phrase_to_distance = dict(zip(phrases, distances))

    def _keeps(self, phrase):
        return self.phrase_to_distance[phrase] <= self.max_distance

    def __getitem__(self, index):
        return self._clip_item(index)

    def __len__(self):
        return len(self.data)


class SpectralMappingEvalDataset(_MappingBase):
    def __init__(self, waveform, label: str, cluster_map: str):
        self._read_clips(waveform, label)
        self._read_cluster_map(cluster_map)
        self.phrase_to_idx = self.phrase_to_label           # (the reference's name)
        self.idxs = [(a, p) for a, item in enumerate(self.data) for p in range(len(item["phrases"]))]

    def __getitem__(self, index):
        return self._phrase_item(index)

    def __len__(self):
        return len(self.idxs)


class SpectralMappingDataset(_MappingBase):
    def __init__(self, waveform, label: str, cluster_map: str, label_type: str = "weak", time_resolution: float = 0.02,
                 sample_rate: int = 32000, max_audio_length: float = None, no_waveform: bool = False):
        self._read_clips(waveform, label)
        self._read_cluster_map(cluster_map)
        self.phrase_to_idx = self.phrase_to_label           # (the reference's name)
        self._clip_settings(label_type, time_resolution, sample_rate, max_audio_length, no_waveform)

    def __getitem__(self, index):
        return self._clip_item(index)

    def __len__(self):
        return len(self.data)
