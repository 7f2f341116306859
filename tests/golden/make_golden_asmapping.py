#!/usr/bin/env python3
"""tests/golden/asmapping/: what the REFERENCE's own AudioSet mapping datasets (``ASMappingEvalDataset``, ``ASMappingWeakDataset``,
``ASMappingEvalLabelSimDataset``, ``ASMappingStrongDataset`` of datasets/class_mapping_dataset.py, imported through ref_import) make
of kmeans/mapping_label.json (4 clips, 13 distinct phrases) and multi_phrase/phrase_emb.pkl (33 phrases, D = 8) --

* inputs written here: ``as_label_emb.pkl`` (9 seeded Gaussian label embeddings, float32, a dict in class order), ``classes.json``
  (their names: the label encoder as a JSON list), ``audioset_label.tsv`` (one or two class names per clip) and ``config.json``
  (the thresholds: quantiles of the fixture's own 13 x 9 similarities; the recorded configurations).
* ``items.npz``: the items of every configuration in CONFIGS (Weak with thresholds and topk 1, 2, 0, with ``min_sim_percent``, with
  a crop under ``random.seed`` and a word limit; Strong with topk 1, 2, 0 and a word limit), of the Eval dataset (``text_idx``)
  and of the LabelSim one (``label_sim``), and ``sims``, sklearn's float32 similarities of the 13 phrases.

h5py is not installed: the module's ``read_from_h5`` is replaced by a function over the waveforms of kmeans.npz.  The label
encoder is a pickled namespace with ``classes_`` in a temporary directory.

The reference's ``np.argsort(sim)[::-1][:topk]`` picks zero-valued entries when fewer than ``topk`` labels lie in the window
(the module docstring of datasets/class_mapping_dataset.py here).  The generator ASSERTS that the fixture never gets there: every
phrase the reference labels (within the word limit and, in the Weak dataset, past its guard) has at least ``topk`` window
members in every recorded configuration; no similarity lies within 1e-4 of a threshold; the gaps between the top window members
(and between the two most similar labels of every phrase) exceed 1e-4.

Only recorded data is committed.  The generator needs the reference checkout (ref_import.REF), sklearn and pandas."""
import json
import os
import pickle
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
FIX = os.path.join(HERE, "multi_phrase")
OUT = os.path.join(HERE, "asmapping")
LABEL = os.path.join(HERE, "kmeans", "mapping_label.json")

CLASSES = ["Bark", "Bell", "Bird", "Car", "Crowd", "Door", "Rain", "Speech", "Wind"]
AUDIOSET = {"K0.wav": "Bird;Speech", "K1.wav": "Rain", "K2.wav": "Wind;Bell", "K3.wav": "Door"}
SR, RES = 100, 0.1
CROP_S, CROP_SEED = 1.0, 3
MARGIN = 1e-4
LOW_Q, MID_Q, HIGH_Q = 0.6, 0.7, 0.97
MIN_SIM_PERCENT = 20
#: name -> (dataset, keywords, which thresholds); "mid" leaves phrases below the window (the Weak guard drops them)
CONFIGS = {
    "weak_top1": ("weak", dict(topk=1), "mid"),
    "weak_top2": ("weak", dict(topk=2, use_audioset_label=False), "low"),
    "weak_all": ("weak", dict(topk=0), "mid"),
    "weak_percent": ("weak", dict(topk=1, min_sim_percent=MIN_SIM_PERCENT), None),
    "weak_crop": ("weak", dict(topk=1, max_phrase_words=5, max_audio_length=CROP_S, use_audioset_label=False), "mid"),
    "strong_top1": ("strong", dict(topk=1, max_phrase_words=5), "low"),
    "strong_top2": ("strong", dict(topk=2, use_audioset_label=False, max_audio_length=CROP_S), "low"),
    "strong_all": ("strong", dict(topk=0), "low"),
}
ITEM_KEYS = {"weak": ("label",), "strong": ("weak_label", "strong_label", "strong_label_mask")}


def load_ref(name):
    import importlib.util
    import ref_import
    spec = importlib.util.spec_from_file_location("ref_" + name.replace("/", "_"), os.path.join(ref_import.REF, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_window(sims, phrases, th, topk, max_words, guard):
    """The asserted properties of one configuration; -> the number of phrases the reference labels."""
    assert (np.abs(sims - th[0]) > MARGIN).all() and (np.abs(sims - th[1]) > MARGIN).all(), "a similarity is at a threshold"
    labelled = 0
    for phrase, s in zip(phrases, sims):
        if len(phrase.split()) > max_words or (guard and (s.max() < th[0] or s.min() > th[1])):
            continue
        members = np.sort(s[(s >= th[0]) & (s <= th[1]) & (s != 0)])[::-1]
        need = max(topk, 1)
        assert len(members) >= need, (phrase, topk, len(members))
        assert (np.abs(np.diff(members[: need + 1])) > MARGIN).all(), (phrase, "window gap")
        labelled += 1
    return labelled


if __name__ == "__main__":
    import ref_import
    from sklearn.metrics.pairwise import cosine_similarity
    ref_import.install()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(FIX, "phrase_emb.pkl"), "rb") as f:
        phrase_to_emb = pickle.load(f)
    with open(LABEL) as f:
        label = json.load(f)
    with np.load(os.path.join(HERE, "kmeans.npz")) as f:
        clips = {c["audio_id"]: f[f"wave/{c['audio_id']}"] for c in label}

    g = np.random.RandomState(31)
    label_embs = g.randn(len(CLASSES), 8).astype(np.float32)
    emb_path = os.path.join(OUT, "as_label_emb.pkl")
    with open(emb_path, "wb") as f:
        pickle.dump({name: label_embs[i] for i, name in enumerate(CLASSES)}, f)
    with open(os.path.join(OUT, "classes.json"), "w") as f:
        json.dump(CLASSES, f)
    as_tsv = os.path.join(OUT, "audioset_label.tsv")
    with open(as_tsv, "w") as f:
        f.write("audio_id\tevent_labels\n" + "".join(f"{aid}\t{names}\n" for aid, names in AUDIOSET.items()))

    phrases = list(dict.fromkeys(p["phrase"] for c in label for p in c["phrases"]))
    sims = cosine_similarity(np.stack([phrase_to_emb[p] for p in phrases]), label_embs)
    top = np.sort(sims, axis=1)
    assert (top[:, -1] - top[:, -2] > MARGIN).all(), "two labels tie for a phrase's best"
    thresholds = {"low": [float(np.quantile(sims, LOW_Q)), float(np.quantile(sims, HIGH_Q))],
                  "mid": [float(np.quantile(sims, MID_Q)), float(np.quantile(sims, HIGH_Q))]}

    out = {"sims": sims.astype(np.float32)}
    ds_mod = load_ref("datasets/class_mapping_dataset")
    ds_mod.read_from_h5 = lambda key, key_to_h5, cache: clips[key]
    config = {"phrases": phrases, "thresholds": thresholds, "sample_rate": SR, "time_resolution": RES, "crop_seed": CROP_SEED,
              "configs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        enc = os.path.join(tmp, "label_encoder.pkl")
        with open(enc, "wb") as f:
            pickle.dump(types.SimpleNamespace(classes_=np.array(CLASSES)), f)
        tsv = os.path.join(tmp, "wave.csv")
        with open(tsv, "w") as f:
            f.write("audio_id\thdf5_path\n" + "".join(f"{aid}\tnone.h5\n" for aid in clips))
        common = dict(waveform=tsv, label=LABEL, phrase_embed=os.path.join(FIX, "phrase_emb.pkl"), as_label_embed=emb_path)
        for name, (kind, kw, which) in CONFIGS.items():
            th = None if which is None else thresholds[which]
            if kind == "weak":
                ds = ds_mod.ASMappingWeakDataset(audioset_label=as_tsv, label_encoder=enc, thresholds=th, sample_rate=SR, **common, **kw)
            else:
                ds = ds_mod.ASMappingStrongDataset(audioset_label=as_tsv, label_encoder=enc, thresholds=th, sample_rate=SR,
                                                   time_resolution=RES, **common, **kw)
            used = [float(t) for t in ds.thresholds]
            labelled = check_window(sims, phrases, used, kw["topk"], kw.get("max_phrase_words", 10), guard=kind == "weak")
            if which is None:
                out[f"{name}/threshold"] = np.float64(used[0])
            if which == "mid":
                assert labelled < len([p for p in phrases if len(p.split()) <= kw.get("max_phrase_words", 10)]), "no phrase is outside"
            assert ds.classes_num == len(CLASSES) and len(ds) == len(label)
            random.seed(CROP_SEED)
            for i in range(len(ds)):
                item = ds[i]
                assert item["audiocap_id"] == label[i]["audiocap_id"] and item["text"] == label[i]["tokens"]
                if "max_audio_length" in kw:
                    out[f"{name}/{i}/waveform"] = np.asarray(item["waveform"])
                for k in ITEM_KEYS[kind]:
                    assert item[k].dtype == np.float64
                    out[f"{name}/{i}/{k}"] = item[k]
            config["configs"][name] = {"dataset": kind, "keywords": kw, "thresholds": which, "labelled_phrases": labelled}
            print(f"{name}: thresholds {used}, {labelled} phrases labelled")
        ev = ds_mod.ASMappingEvalDataset(**common)
        assert len(ev) == 16
        items = [ev[i] for i in range(len(ev))]
        assert list(items[0]) == ["audio_id", "audiocap_id", "start_index", "end_index", "waveform", "text", "text_idx"]
        out["eval/text_idx"] = np.array([int(it["text_idx"]) for it in items], dtype=np.int32)
        out["eval/start_index"] = np.array([int(it["start_index"]) for it in items], dtype=np.int32)
        out["eval/end_index"] = np.array([int(it["end_index"]) for it in items], dtype=np.int32)
        ls = ds_mod.ASMappingEvalLabelSimDataset(**common)
        items = [ls[i] for i in range(len(ls))]
        assert list(items[0]) == ["audiocap_id", "start_index", "end_index", "waveform", "label_sim"]
        assert items[0]["label_sim"].dtype == np.float32 and items[0]["waveform"].dtype == np.float32
        out["labelsim/label_sim"] = np.stack([it["label_sim"] for it in items])
    with open(os.path.join(OUT, "config.json"), "w") as f:
        json.dump(config, f, indent=1)
    np.savez_compressed(os.path.join(OUT, "items.npz"), **out)
    print("wrote", OUT, {n: os.path.getsize(os.path.join(OUT, n)) for n in sorted(os.listdir(OUT))})
