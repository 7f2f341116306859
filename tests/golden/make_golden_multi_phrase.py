#!/usr/bin/env python3
"""tests/golden/multi_phrase/: a tiny weak-phrase corpus in the reference's on-disk formats, and what the REFERENCE's own code
(imported through ref_import: datasets/multi_phrase_dataset.py, datasets/collate_function.py, utils/data/calc_phrase_count.py,
utils/data/calc_phrase_sim_count.py) makes of it --

* ``label.json``          12 clips with 1..5 phrases each out of 30 distinct ones, some longer than the ``max_phrase_length`` used
* ``phrase_emb.pkl``      {phrase: fp32 vector of 8} for every phrase and three more; no cosine within 1e-4 of a threshold
* ``cluster_map.json`` / ``cluster_map_small.json`` / ``cluster_map_hole.json``   6 clusters, 3 clusters (fewer than the negatives
  wanted), and 6 clusters plus one whose phrases are all outside the pool
* ``negative_pool.txt``   a pool file: every phrase the clips name and four that no clip names, in another order
* ``phrase_count.json``   {phrase: count}
* ``strong_label.json`` -> ``strong_phrase_count.json``   the count script's input and output
* ``sim40_emb.pkl`` + ``sim40_count.json`` -> ``sim40_sim_count.json``   the similarity-count script's inputs and output (40 phrases)
* ``../multi_phrase.json`` per case (strategy x fix_neg x negative_pool x max_phrase_length x phrase_num ...) the items of two or
  three passes over the data under recorded seeds: phrases and counts as indices into ``all_phrases``, labels, and the crop
  offset; a case that changes ``phrase_num`` between passes cuts and extends the ``fix_neg`` memory
* ``../multi_phrase.npz`` VarNumTextCollate and TextCollate (List[List[str]]) outputs with DictTokenizer(formats/vocab.pkl)

The reference orders its pool by ``list(set(...))``, which changes from process to process; the generator imposes the sorted order
on the reference instance (``phrases``, ``phrase_to_idx``, ``phrase_embs``), which is the order the mirror uses.  h5py and
torchaudio are stubbed and ``load_audio`` reads the seeded float16 clips.  ``run_reference`` is also what the live test calls
when the reference is present.  The generator needs the reference checkout (ref_import.REF)."""
import argparse
import importlib.util
import json
import os
import pickle
import random
import signal
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "multi_phrase")
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

SR = 100                          # a small sample rate keeps the clips tiny; the crop arithmetic is rate-agnostic
MAX_AUDIO_S = 2.0
MAX_PHRASE_LEN = 3
GAP = 1e-4
SIM_THRESHOLDS = (0.5, 0.2)       # the second one lets few candidates pass: the cyclic fill
D = 8

WORDS = ["dog", "bird", "rain", "wind", "door", "man", "car", "bell", "water", "crowd"]
VERBS = ["barks", "sings", "falls", "blows", "slams", "speaks", "passes", "rings", "drips", "cheers"]


def all_label_phrases():
    """30 distinct phrases; every fifth has more than MAX_PHRASE_LEN words."""
    out = []
    for i in range(30):
        w, v = WORDS[i % 10], VERBS[(i * 3 + i // 10) % 10]
        p = f"a {w} {v}" if i < 10 else (f"{w} {v}" if i < 20 else f"the {w} {v}")
        if i % 5 == 4:
            p += " loudly in the distance"
        out.append(p)
    assert len(set(out)) == 30
    return out


def make_label():
    phrases = all_label_phrases()
    g = np.random.RandomState(7)
    label = []
    for c in range(12):
        n = 1 + c % 5
        idx = g.choice(30, size=n, replace=False)
        label.append({"audio_id": f"Y{c:02d}.wav", "phrases": [phrases[i] for i in idx]})
    label[5]["phrases"] = [phrases[4], phrases[9]]               # long phrases only: dropped under max_phrase_length
    label[8]["phrases"] = [phrases[14], phrases[2], phrases[3]]  # a long phrase first: fewer positives under max_phrase_length
    return label


def synthetic_clips():
    g = np.random.RandomState(11)
    return [(f"Y{c:02d}.wav", (0.3 * g.randn(150 + 23 * c)).astype(np.float16)) for c in range(12)]


def unit64(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.sqrt((x * x).sum(1, keepdims=True))


def gapped_embeddings(names, seed, thresholds):
    """fp32 rows; vectors are re-drawn until no pairwise cosine lies within GAP of a threshold."""
    g = np.random.RandomState(seed)
    emb = g.randn(len(names), D)
    for _ in range(200):
        e32 = emb.astype(np.float32)
        sims = unit64(e32) @ unit64(e32).T
        bad = np.zeros(len(names), dtype=bool)
        for t in thresholds:
            near = np.abs(sims - t) < GAP
            np.fill_diagonal(near, False)
            bad |= near.any(0)
        if not bad.any():
            return {n: e32[i].copy() for i, n in enumerate(names)}
        emb[bad] = g.randn(int(bad.sum()), D)
    raise AssertionError("no gapped embeddings found")


def passing_counts(label, emb, pool, max_len, thr):
    """per clip: how many pool phrases outside its positives have every cosine to the positives below thr (phrase_num large)."""
    out = []
    for clip in label:
        pos = [p for p in clip["phrases"] if max_len is None or len(p.split()) <= max_len]
        if not pos:
            continue
        cand = [p for p in pool if p not in pos and (max_len is None or len(p.split()) <= max_len)]
        up, uc = unit64(np.stack([emb[p] for p in pos])), unit64(np.stack([emb[p] for p in cand]))
        out.append(int(((up @ uc.T).max(0) < thr).sum()))
    return out


def write_fixture(out=OUT):
    os.makedirs(out, exist_ok=True)
    label = make_label()
    phrases = all_label_phrases()
    extra = ["a whale sings", "thunder rolls", "a kettle whistles"]
    g = np.random.RandomState(3)
    used = {p for clip in label for p in clip["phrases"]}
    unused = [p for p in phrases if p not in used]
    assert len(unused) >= 5, len(unused)
    # the pool file: every phrase a clip names (the reference looks every positive up in the pool) and four that no clip names
    pool_file = sorted(used | set(unused[:4]), key=lambda p: (len(p), p[::-1]))
    label_pool = sorted(used)
    for seed in range(1000):
        emb = gapped_embeddings(phrases + extra, seed, SIM_THRESHOLDS)
        ok = True
        few = False
        for pool in (label_pool, pool_file):
            for max_len in (None, MAX_PHRASE_LEN):
                ok &= min(passing_counts(label, emb, pool, max_len, 0.5)) >= 1
                tight = passing_counts(label, emb, pool, max_len, SIM_THRESHOLDS[1])
                ok &= min(tight) >= 1
                few |= min(tight) < 3
        if ok and few:
            break
    else:
        raise AssertionError("no embedding seed leaves every clip a negative")
    json.dump(label, open(os.path.join(out, "label.json"), "w"), indent=1)
    pickle.dump(emb, open(os.path.join(out, "phrase_emb.pkl"), "wb"))
    with open(os.path.join(out, "negative_pool.txt"), "w") as f:
        f.write("".join(p + "\n" for p in pool_file))
    clusters = {str(10 + c): [phrases[i] for i in range(30) if i % 6 == c] for c in range(6)}
    clusters["10"].append("a whale sings")                       # listed, but outside the pool
    json.dump(clusters, open(os.path.join(out, "cluster_map.json"), "w"), indent=1)
    json.dump({str(c): [phrases[i] for i in range(30) if i % 3 == c] for c in range(3)},
              open(os.path.join(out, "cluster_map_small.json"), "w"), indent=1)
    json.dump({**clusters, "99": ["thunder rolls", "a kettle whistles"]}, open(os.path.join(out, "cluster_map_hole.json"), "w"), indent=1)
    json.dump({p: int(g.randint(1, 400)) for p in phrases + extra}, open(os.path.join(out, "phrase_count.json"), "w"), indent=1)
    # the count scripts' inputs
    strong = [{"audio_id": c["audio_id"], "phrases": [{"phrase": p, "start_index": 0, "end_index": 1, "segments": []}
                                                       for p in c["phrases"] + c["phrases"][:1]]} for c in label]
    json.dump(strong, open(os.path.join(out, "strong_label.json"), "w"), indent=1)
    names40 = [f"{w} {v}" for w in WORDS[:8] for v in VERBS[:5]]
    emb40 = gapped_embeddings(names40, 5, (0.5,))
    rows = np.stack([emb40[n] for n in names40])
    for j in range(1, 40, 4):                                    # near-duplicates, so that counts exceed the phrase's own
        rows[j] = rows[j - 1] + 0.3 * np.random.RandomState(j).randn(D).astype(np.float32)
    sims = unit64(rows) @ unit64(rows).T
    assert (np.abs(sims - 0.5) >= GAP).all(), "re-seed: a cosine of the 40-phrase table is within the gap"
    pickle.dump({n: rows[i] for i, n in enumerate(names40)}, open(os.path.join(out, "sim40_emb.pkl"), "wb"))
    json.dump({n: int(g.randint(1, 50)) for n in names40}, open(os.path.join(out, "sim40_count.json"), "w"), indent=1)


def write_audio(tmp_dir):
    """the seeded clips as an .npz pack and the reference's ``audio_id<TAB>file_path`` TSV -> path of the TSV"""
    pack = os.path.join(tmp_dir, "pack.npz")
    np.savez(pack, **dict(synthetic_clips()))
    tsv = os.path.join(tmp_dir, "audio.tsv")
    with open(tsv, "w") as f:
        f.write("audio_id\tfile_path\n" + "".join(f"{aid}\t{pack}\n" for aid, _ in synthetic_clips()))
    return tsv


def cases():
    """[{name, cls, strategy, fix_neg, pool, max_len, phrase_nums (one per pass), sim_threshold, cluster_map, crop}]"""
    out = []
    for fix in (False, True):
        for max_len in (None, MAX_PHRASE_LEN):
            # 2 / 4 / 7: below, equal to and above the clips' numbers of positives, twice (the second pass hits the fix_neg
            # memory); 9 -> 12 -> 5 (more than any clip has positives, so that every clip remembers at least one negative: the
            # reference does not return from extending an empty memory): the memory is extended, then cut
            for nums in ([2, 2], [4, 4], [7, 7]) + (([9, 12, 5],) if fix else ()):
                pn = nums[0]
                base = dict(fix_neg=fix, max_len=max_len, phrase_nums=nums, crop=(pn == 4))
                out.append(dict(base, strategy="random", cls="AudioSamplePhrasesDataset"))
                out.append(dict(base, strategy="clustering", cluster_map="cluster_map.json", cls="AudioSamplePhrasesDataset"))
                for pool in (False, True):
                    out.append(dict(base, strategy="similarity", pool=pool, sim_threshold=0.5, cls="SamplePhrasesCountDataset"))
            out.append(dict(fix_neg=fix, max_len=max_len, phrase_nums=[7, 7], crop=False, strategy="clustering",
                            cluster_map="cluster_map_small.json", cls="SamplePhrasesCountDataset"))
            out.append(dict(fix_neg=fix, max_len=max_len, phrase_nums=[7, 7], crop=False, strategy="similarity", pool=True,
                            sim_threshold=SIM_THRESHOLDS[1], cls="SamplePhrasesCountDataset"))
            out.append(dict(fix_neg=fix, max_len=max_len, phrase_nums=[6, 6], crop=False, strategy="similarity", pool=False,
                            sim_threshold=SIM_THRESHOLDS[1], cls="AudioSamplePhrasesDataset"))
    out.append(dict(fix_neg=False, max_len=None, phrase_nums=[4, 4], crop=False, strategy="clustering",
                    cluster_map="cluster_map_hole.json", cls="AudioSamplePhrasesDataset"))
    for i, c in enumerate(out):
        c.setdefault("pool", False)
        c["seed"] = 100 + i
        c["name"] = f"{i:02d}_{c['strategy']}_fix{int(c['fix_neg'])}_pool{int(c['pool'])}_len{c['max_len']}_n{c['phrase_nums'][0]}"
    return out


def dataset_kwargs(case, fixture, tsv):
    kw = dict(label=os.path.join(fixture, "label.json"), phrase_num=case["phrase_nums"][0], fix_neg=case["fix_neg"],
              neg_samp_stratg=case["strategy"], max_phrase_length=case["max_len"], sample_rate=SR,
              max_audio_length=MAX_AUDIO_S if case["crop"] else None)
    if case["strategy"] == "clustering":
        kw["cluster_map"] = os.path.join(fixture, case["cluster_map"])
    if case["strategy"] == "similarity":
        kw.update(phrase_embed=os.path.join(fixture, "phrase_emb.pkl"), sim_threshold=case["sim_threshold"])
        if case["pool"]:
            kw["negative_pool"] = os.path.join(fixture, "negative_pool.txt")
    if case["cls"] == "SamplePhrasesCountDataset":
        kw["phrase_count"] = os.path.join(fixture, "phrase_count.json")
    return kw


def crop_start(waveform, audio_id):
    full = dict(synthetic_clips())[audio_id].astype(np.float32)
    for s in range(full.shape[0] - waveform.shape[0] + 1):
        if np.array_equal(full[s:s + waveform.shape[0]], waveform):
            return s
    raise AssertionError("the item's waveform is no crop of its clip")


class NoReturn(BaseException):
    pass


def _no_return(signum, frame):
    raise NoReturn()


def run_passes(ds, case, index_of, no_return_after=None):
    """Items of every pass of a case under its seed -> list of passes, an item as plain data (or {"error": exception type}).
    no_return_after (seconds; for the reference only, the mirror's tests leave it off): the reference does not return where
    nothing can be sampled or repeated; the mirror documents a ValueError there, and an alarm records the same for the
    reference (neither has drawn from np.random at that point of the item)."""
    np.random.seed(case["seed"])
    random.seed(case["seed"])
    if no_return_after is not None:
        signal.signal(signal.SIGALRM, _no_return)
    passes = []
    for pn in case["phrase_nums"]:
        ds.phrase_num = pn
        items = []
        for i in range(len(ds)):
            if no_return_after is not None:
                signal.setitimer(signal.ITIMER_REAL, no_return_after)
            try:
                item = ds[i]
            except (IndexError, ValueError, KeyError) as e:
                items.append({"error": type(e).__name__})
                continue
            except NoReturn:
                items.append({"error": "ValueError", "reference_did_not_return": True})
                continue
            finally:
                if no_return_after is not None:
                    signal.setitimer(signal.ITIMER_REAL, 0.0)
            assert item["waveform"].dtype == np.float32
            rec = {"phrases": [index_of[str(p)] for p in item["phrases"]], "label": [int(v) for v in item["label"]],
                   "start": crop_start(item["waveform"], ds.data[i]["audio_id"]), "samples": int(item["waveform"].shape[0])}
            if "counts" in item:
                rec["counts"] = [int(v) for v in item["counts"]]
            items.append(rec)
        passes.append(items)
    return passes


def load_ref(name):
    import ref_import
    spec = importlib.util.spec_from_file_location("ref_" + name.replace("/", "_"), os.path.join(ref_import.REF, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_REF = {}


def reference_module():
    if "ds" not in _REF:
        import ref_import
        ref_import.install()                     # stubs (h5py, torchaudio ...) and the reference on sys.path for ``utils.*``
        _REF["ds"] = load_ref("datasets/multi_phrase_dataset")
    return _REF["ds"]


def run_reference(case, fixture, tsv, index_of):
    mod = reference_module()
    clips = {aid: w for aid, w in synthetic_clips()}
    cls = getattr(mod, case["cls"])
    kw = dataset_kwargs(case, fixture, tsv)
    first = kw.pop("label")
    ds = cls(tsv, first, **kw)
    ds.load_audio = lambda audio_id, file_path: clips[audio_id]
    if not (case["strategy"] == "similarity" and case["pool"]):
        ds.phrases = np.array(sorted(ds.phrases.tolist()))                     # the mirror's pool order
        ds.phrase_to_idx = {p: i for i, p in enumerate(ds.phrases.tolist())}
        if case["strategy"] == "similarity":
            ds.phrase_embs = np.stack([ds.phrase_to_emb[p] for p in ds.phrases.tolist()])
    return run_passes(ds, case, index_of, no_return_after=2.0)


def phrase_index():
    names = all_label_phrases() + ["a whale sings", "thunder rolls", "a kettle whistles"]
    return names, {p: i for i, p in enumerate(names)}


COLLATE_ITEMS = [
    {"waveform": np.arange(5, dtype=np.float32), "phrases": ["a dog barks", "rain falls", "unknownword"], "label": np.array([1, 0, 0])},
    {"waveform": np.arange(3, dtype=np.float32), "phrases": ["birds chirp in the background"], "label": np.array([1])},
    {"waveform": np.arange(7, dtype=np.float32), "phrases": ["a", "wind blows and a door slams loudly"], "label": np.array([1, 0])},
]
FIXED_ITEMS = [{"waveform": np.arange(4 + i, dtype=np.float32), "phrases": ps, "label": np.array([1, 0, 0]), "counts": [3, 1, 4]}
               for i, ps in enumerate([["a dog barks", "rain falls", "unknownword"], ["birds chirp", "a", "a door slams"]])]


def collate_outputs(col_mod, tok):
    out = {}
    b = col_mod.VarNumTextCollate(tok, text_key="phrases", pad_keys=["waveform", "label"])([dict(i) for i in COLLATE_ITEMS])
    assert b["text_key"] == "phrases"
    out["var/phrases"], out["var/phrases_len"] = np.asarray(b["phrases"]), np.asarray(b["phrases_len"])
    out["var/phrases_num"] = np.asarray(b["phrases_num"])
    for k in ("waveform", "waveform_len", "label", "label_len"):
        out[f"var/{k}"] = np.asarray(b[k])
    b = col_mod.VarNumTextCollate(tok, text_key="phrases", pad_keys=["waveform", "label"], sort_key="waveform")(
        [dict(i) for i in COLLATE_ITEMS])
    out["var_sorted/phrases"], out["var_sorted/phrases_num"] = np.asarray(b["phrases"]), np.asarray(b["phrases_num"])
    b = col_mod.TextCollate(tok, text_key="phrases", pad_keys=["waveform"])([dict(i) for i in FIXED_ITEMS])
    for k in ("text", "text_len", "label", "counts", "waveform", "waveform_len"):
        out[f"fixed/{k}"] = np.asarray(b[k])
    return out


if __name__ == "__main__":
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    write_fixture(a.out)
    names, index_of = phrase_index()
    with tempfile.TemporaryDirectory() as tmp:
        tsv = write_audio(tmp)
        recorded = {c["name"]: run_reference(c, a.out, tsv, index_of) for c in cases()}
    n_err = sum("error" in it for ps in recorded.values() for p in ps for it in p)
    json.dump({"all_phrases": names, "cases": recorded}, open(os.path.join(HERE, "multi_phrase.json"), "w"), separators=(",", ":"))
    # the two count scripts
    cnt = load_ref("utils/data/calc_phrase_count")
    cnt.main(argparse.Namespace(input=os.path.join(a.out, "strong_label.json"), output=os.path.join(a.out, "strong_phrase_count.json")))
    sim = load_ref("utils/data/calc_phrase_sim_count")
    sim.main(argparse.Namespace(phrase_count_path=os.path.join(a.out, "sim40_count.json"), embedding_path=os.path.join(a.out, "sim40_emb.pkl"),
                                threshold=0.5, output_path=os.path.join(a.out, "sim40_sim_count.json")))
    tok = load_ref("datasets/text_tokenizer").DictTokenizer(os.path.join(HERE, "formats", "vocab.pkl"))
    np.savez_compressed(os.path.join(HERE, "multi_phrase.npz"), **collate_outputs(load_ref("datasets/collate_function"), tok))
    print("wrote", a.out, {f: os.path.getsize(os.path.join(a.out, f)) for f in sorted(os.listdir(a.out))}, "items with errors:", n_err)
