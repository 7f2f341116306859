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

The AudioSet class-mapping datasets (mirror of ``ASMappingEvalDataset``, ``ASMappingWeakDataset``, ``ASMappingEvalLabelSimDataset``
and ``ASMappingStrongDataset``, class_mapping_dataset.py:15-293 in the reference): a phrase becomes AudioSet class indices through
the cosine similarity of its embedding (``phrase_embed`` pickle) to the label embeddings (``as_label_embed`` pickle, taken in
insertion order), inside the ``thresholds`` window.  Same constructor keywords plus ``device``, same item keys and dtypes.

* ``ASMappingEvalDataset``  one item per (clip, phrase): ``text_idx`` is the most similar label.
* ``ASMappingEvalLabelSimDataset``  the same items with ``label_sim``, the float32 similarities to all labels.
* ``ASMappingWeakDataset``  one item per clip: ``label`` (classes_num,) set at the labels of every phrase of at most
  ``max_phrase_words`` words and, with ``use_audioset_label``, at the clip's AudioSet labels (``audioset_label`` TSV, names joined
  by ``;``, indexed by ``label_encoder``: a pickle of anything with ``.classes_`` or a JSON list of names).  ``min_sim_percent``
  replaces ``thresholds`` by [that percentile of the best similarities of ALL phrases of ``phrase_embed``, 1.0].
* ``ASMappingStrongDataset``  ``weak_label``, ``strong_label`` (n_frame, classes_num) and ``strong_label_mask`` (classes_num,), the
  classes some phrase of the clip labels (the input of ``MaskedFrameBceLoss``); ``max_audio_length`` is accepted and, as in the
  reference, does not crop.

Differences from the reference: the reference calls sklearn's ``cosine_similarity`` for one phrase in every ``__getitem__``;
here ALL device work happens in ``__init__``, one ``utils.label_map.LabelMap`` call over the distinct phrases (csrc/label_map.hip),
and ``__getitem__`` is host-only lookups, so loader workers never open the GPU.  A phrase labels ONLY members of its window
(thresholds[0] <= sim <= thresholds[1], sim != 0), at most ``topk`` of them, in both datasets: the reference's
``np.argsort(sim)[::-1][:topk]`` also picks zero-valued entries, in an order that depends on numpy's sort, when fewer than
``topk`` labels lie in the window and, in the Strong dataset (which lacks the Weak one's guard), when none does.  The number of
label embeddings must equal ``classes_num`` (``ValueError``).
"""
import json
import math
import pickle
import random

import numpy as np

from ..utils.label_map import LabelMap, stack_embeddings
from .waveform_store import WaveformStore, load_dict_from_csv


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


class _ASMappingBase:
    """The files all four AudioSet mapping datasets read and their (clip, phrase) index."""

    def _read(self, waveform, label, phrase_embed, as_label_embed, device):
        self.store = waveform if isinstance(waveform, WaveformStore) else WaveformStore(waveform)
        with open(label) as f:
            self.data = json.load(f)
        with open(phrase_embed, "rb") as f:
            self.phrase_to_emb = pickle.load(f)
        with open(as_label_embed, "rb") as f:
            self.label_to_emb = pickle.load(f)
        self.label_embs = stack_embeddings(self.label_to_emb)
        self.label_map = LabelMap(self.label_embs, device=device)

    def generate_index(self):
        self.idxs = [(a, p) for a, item in enumerate(self.data) for p in range(len(item["phrases"]))]

    def _distinct_phrases(self, max_words=None):
        phrases = dict.fromkeys(p["phrase"] for item in self.data for p in item["phrases"])
        return [p for p in phrases if max_words is None or len(p.split()) <= max_words]

    def _map_phrases(self, phrases, thresholds=None, topk=1, want_sim=False):
        if not phrases:
            return None
        embs = np.stack([np.asarray(self.phrase_to_emb[p], dtype=np.float32).reshape(-1) for p in phrases])
        return self.label_map.map(embs, thresholds, topk, want_sim=want_sim)

    def __len__(self):
        return len(self.idxs)


class ASMappingEvalDataset(_ASMappingBase):
    def __init__(self, waveform, label: str, phrase_embed: str, as_label_embed: str, device="cuda:0"):
        self._read(waveform, label, phrase_embed, as_label_embed, device)
        self.generate_index()
        phrases = self._distinct_phrases()
        mapped = self._map_phrases(phrases)
        self.phrase_to_label = dict(zip(phrases, mapped.best)) if phrases else {}

    def __getitem__(self, index):
        audio_idx, phrase_idx = self.idxs[index]
        item = self.data[audio_idx]
        phrase_item = item["phrases"][phrase_idx]
        return {
            "audio_id": item["audio_id"],
            "audiocap_id": item["audiocap_id"],
            "start_index": phrase_item["start_index"],
            "end_index": phrase_item["end_index"],
            "waveform": self.store[item["audio_id"]],
            "text": item["tokens"],
            "text_idx": self.phrase_to_label[phrase_item["phrase"]],
        }


class ASMappingEvalLabelSimDataset(_ASMappingBase):
    def __init__(self, waveform, label: str, phrase_embed: str, as_label_embed: str, device="cuda:0"):
        self._read(waveform, label, phrase_embed, as_label_embed, device)
        self.generate_index()
        phrases = self._distinct_phrases()
        mapped = self._map_phrases(phrases, want_sim=True)
        self.phrase_to_sim = dict(zip(phrases, mapped.sim)) if phrases else {}

    def __getitem__(self, index):
        audio_idx, phrase_idx = self.idxs[index]
        item = self.data[audio_idx]
        phrase_item = item["phrases"][phrase_idx]
        return {
            "audiocap_id": item["audiocap_id"],
            "start_index": phrase_item["start_index"],
            "end_index": phrase_item["end_index"],
            "waveform": self.store[item["audio_id"]],
            "label_sim": self.phrase_to_sim[phrase_item["phrase"]],
        }


def _read_classes(label_encoder):
    """The class names of a label encoder: a JSON list of names, or a pickle of anything with ``.classes_``."""
    if str(label_encoder).endswith(".json"):
        with open(label_encoder) as f:
            return list(json.load(f))
    with open(label_encoder, "rb") as f:
        return list(pickle.load(f).classes_)


class ASMappingWeakDataset(_ASMappingBase):
    def __init__(self, waveform, label: str, audioset_label: str, phrase_embed: str, as_label_embed: str, label_encoder: str,
                 thresholds=(0.5, 1.0), min_sim_percent: float = None, use_audioset_label: bool = True, topk: int = 1,
                 max_phrase_words: int = 10, max_audio_length: float = None, sample_rate: int = 32000, device="cuda:0"):
        self._read(waveform, label, phrase_embed, as_label_embed, device)
        self.thresholds = thresholds
        self.min_sim_percent = min_sim_percent
        self.topk = topk
        self.max_phrase_words = max_phrase_words
        self.classes = _read_classes(label_encoder)
        self.classes_num = len(self.classes)
        if len(self.label_embs) != self.classes_num:
            raise ValueError(f"as_label_embed holds {len(self.label_embs)} label embeddings, label_encoder {self.classes_num} classes")
        self.label_to_idx = {lbl: idx for idx, lbl in enumerate(self.classes)}
        self.aid_to_aslabel = load_dict_from_csv(audioset_label, ("audio_id", "event_labels"))
        self.use_audioset_label = use_audioset_label
        self.max_audio_len = None if max_audio_length is None else int(max_audio_length * sample_rate)
        self.sample_rate = sample_rate

        msg = "either one of 'thresholds' or 'min_sim_percent' can be set"
        if min_sim_percent is not None:
            assert thresholds is None, msg
            assert topk == 1, "currently only support topk = 1 when setting similarity percent"
            self.calc_thresholds()
        if thresholds is not None:
            assert min_sim_percent is None, msg
        self.prepare_phrase_label()

    def calc_thresholds(self):
        sims = self.label_map.map(stack_embeddings(self.phrase_to_emb)).best_sim
        self.thresholds = [np.percentile(sims, self.min_sim_percent), 1.0]

    def prepare_phrase_label(self):
        phrases = self._distinct_phrases(self.max_phrase_words)
        mapped = self._map_phrases(phrases, self.thresholds, self.topk)
        self.phrase_to_labels = dict(zip(phrases, mapped.labels)) if phrases else {}

    def _kept(self, item):
        return [p for p in item["phrases"] if len(p["phrase"].split()) <= self.max_phrase_words]

    def _add_audioset_label(self, item, label):
        if self.use_audioset_label:
            for as_label in self.aid_to_aslabel[item["audio_id"]].split(";"):
                label[self.label_to_idx[as_label]] = 1

    def __getitem__(self, index):
        item = self.data[index]
        waveform = self.store[item["audio_id"]]
        if self.max_audio_len is not None and waveform.shape[0] > self.max_audio_len:
            start = random.randint(0, waveform.shape[0] - self.max_audio_len)
            waveform = waveform[start: start + self.max_audio_len]
        label = np.zeros(self.classes_num)
        for phrase_item in self._kept(item):
            label[self.phrase_to_labels[phrase_item["phrase"]]] = 1
        self._add_audioset_label(item, label)
        return {"audiocap_id": item["audiocap_id"], "audio_id": item["audio_id"], "text": item["tokens"], "waveform": waveform,
                "label": label}

    def __len__(self):
        return len(self.data)


class ASMappingStrongDataset(ASMappingWeakDataset):
    def __init__(self, waveform, label: str, audioset_label: str, phrase_embed: str, as_label_embed: str, label_encoder: str,
                 time_resolution: float = 0.02, sample_rate: int = 32000, thresholds=(0.5, 1.0), use_audioset_label: bool = True,
                 topk: int = 1, max_phrase_words: int = 10, max_audio_length: float = None, device="cuda:0"):
        super().__init__(waveform=waveform, label=label, audioset_label=audioset_label, phrase_embed=phrase_embed,
                         as_label_embed=as_label_embed, label_encoder=label_encoder, thresholds=thresholds, min_sim_percent=None,
                         use_audioset_label=use_audioset_label, topk=topk, max_phrase_words=max_phrase_words,
                         max_audio_length=max_audio_length, sample_rate=sample_rate, device=device)
        self.time_resolution = time_resolution

    def __getitem__(self, index):
        item = self.data[index]
        waveform = self.store[item["audio_id"]]
        weak_label = np.zeros(self.classes_num)
        n_frame = math.floor(waveform.shape[0] / self.sample_rate / self.time_resolution) + 1
        strong_label = np.zeros((n_frame, self.classes_num))
        strong_label_mask = np.zeros(self.classes_num)
        for phrase_item in self._kept(item):
            indices = self.phrase_to_labels[phrase_item["phrase"]]
            weak_label[indices] = 1
            strong_label_mask[indices] = 1
            for start, end in phrase_item["segments"]:
                onset = round(start / self.time_resolution)
                offset = round(end / self.time_resolution)
                strong_label[onset: offset, indices] = 1
        self._add_audioset_label(item, weak_label)
        return {"audiocap_id": item["audiocap_id"], "audio_id": item["audio_id"], "text": item["tokens"], "waveform": waveform,
                "weak_label": weak_label, "strong_label": strong_label, "strong_label_mask": strong_label_mask}
