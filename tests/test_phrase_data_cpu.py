"""CPU: the weak-phrase data path -- AudioSamplePhrasesDataset / SamplePhrasesCountDataset, VarNumTextCollate and the phrase
count -- against what the REFERENCE's own code produced on the same files under the same seeds (tests/golden/multi_phrase/,
multi_phrase.json and multi_phrase.npz, written by tests/golden/make_golden_multi_phrase.py), plus the documented differences."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests.golden import make_golden_multi_phrase as G
from tests.golden import ref_import

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_phrase")
CASES = G.cases()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(FIX), "multi_phrase.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def audio_tsv(tmp_path_factory):
    return G.write_audio(str(tmp_path_factory.mktemp("multi_phrase_audio")))


def drop_aliases():
    """what install_aliases() registered: the top-level names of the reference and the ``datasets.*`` sub-module names"""
    import sys
    for k, m in list(sys.modules.items()):
        if (k.split(".")[0] in ("models", "losses", "utils") or k.startswith("datasets.")) and \
                getattr(m, "__name__", "").startswith("texttoaudiogrounding_amd"):
            del sys.modules[k]


def mirror_passes(case, tsv):
    from texttoaudiogrounding_amd.datasets import multi_phrase_dataset as M
    ds = getattr(M, case["cls"])(tsv, **G.dataset_kwargs(case, FIX, tsv))
    return G.run_passes(ds, case, G.phrase_index()[1])


def plain(passes):
    """items as recorded, without the generator's note on how an error was observed"""
    return [[{k: v for k, v in item.items() if k != "reference_did_not_return"} for item in items] for items in passes]


def test_the_cases_cover_what_they_claim(recorded):
    assert recorded["all_phrases"] == G.phrase_index()[0] and set(recorded["cases"]) == {c["name"] for c in CASES}
    assert {(c["strategy"], c["fix_neg"], c["pool"], c["max_len"]) for c in CASES} >= {
        (s, f, False, m) for s in ("random", "clustering", "similarity") for f in (False, True) for m in (None, G.MAX_PHRASE_LEN)}
    items = [it for c in recorded["cases"].values() for p in c for it in p]
    ok = [it for it in items if "error" not in it]
    assert len(ok) > 1000 and any(it["start"] > 0 for it in ok) and any(it.get("counts") for it in ok)
    assert any(sum(it["label"]) == len(it["label"]) for it in ok) and any(sum(it["label"]) == 1 < len(it["label"]) for it in ok)
    # the cyclic fill (a negative more than once) and the reference's endless loops (recorded as the mirror's ValueError)
    assert any(len(set(it["phrases"])) < len(it["phrases"]) for it in ok)
    assert any(it.get("reference_did_not_return") for it in items)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_items_equal_the_reference(case, recorded, audio_tsv):
    """identical phrases, labels, counts and crop offsets in every pass, the fix_neg memory extended and cut included"""
    assert mirror_passes(case, audio_tsv) == plain(recorded["cases"][case["name"]])


@pytest.mark.skipif(not ref_import.available(), reason="the reference checkout is not present")
@pytest.mark.parametrize("case", [c for c in CASES if c["strategy"] != "clustering" or "small" not in c["cluster_map"]][::5],
                         ids=lambda c: c["name"])
def test_items_equal_the_live_reference(case, audio_tsv):
    got = mirror_passes(case, audio_tsv)
    assert got == plain(G.run_reference(case, FIX, audio_tsv, G.phrase_index()[1]))


def test_item_layout(audio_tsv):
    from texttoaudiogrounding_amd.datasets import SamplePhrasesCountDataset
    case = next(c for c in CASES if c["strategy"] == "similarity" and c["cls"] == "SamplePhrasesCountDataset")
    ds = SamplePhrasesCountDataset(audio_tsv, **G.dataset_kwargs(case, FIX, audio_tsv))
    np.random.seed(0)
    item = ds[0]
    assert set(item) == {"waveform", "phrases", "label", "counts"} and item["waveform"].dtype == np.float32
    assert all(type(p) is str for p in item["phrases"]) and item["label"].dtype.kind == "i"
    assert len(item["phrases"]) == len(item["label"]) == len(item["counts"]) == case["phrase_nums"][0]
    assert len(ds.phrase_to_emb) == len(ds.phrases) < 33                     # embeddings outside the pool are dropped
    assert ds.phrases.tolist() == sorted(ds.phrases.tolist())                # the documented pool order


def test_endless_loops_of_the_reference_raise(tmp_path, audio_tsv):
    """No candidate below the threshold and nothing to repeat: the reference never returns, the mirror names the clip."""
    from texttoaudiogrounding_amd.datasets import AudioSamplePhrasesDataset
    with open(os.path.join(FIX, "phrase_emb.pkl"), "rb") as f:
        emb = pickle.load(f)
    same = {p: np.ones(8, dtype=np.float32) for p in emb}                    # every cosine is 1
    path = str(tmp_path / "same.pkl")
    with open(path, "wb") as f:
        pickle.dump(same, f)
    ds = AudioSamplePhrasesDataset(audio_tsv, os.path.join(FIX, "label.json"), 4, False, "similarity", sample_rate=G.SR,
                                   phrase_embed=path, sim_threshold=0.5)
    with pytest.raises(ValueError, match="Y00.wav"):
        ds[0]
    small = AudioSamplePhrasesDataset(audio_tsv, os.path.join(FIX, "label.json"), 9, False, "clustering", sample_rate=G.SR,
                                      cluster_map=os.path.join(FIX, "cluster_map_small.json"))
    full = next(i for i, c in enumerate(small.data) if len({small.phrase_to_cluster_idx[p] for p in c["phrases"]}) == 3)
    with pytest.raises(ValueError, match=small.data[full]["audio_id"]):
        small[full]


def test_waveform_tsv_headers(tmp_path, audio_tsv):
    from texttoaudiogrounding_amd.datasets.waveform_store import WaveformStore, write_waveform_pack
    by_file_path = WaveformStore(audio_tsv)
    by_hdf5_path = WaveformStore(write_waveform_pack(str(tmp_path / "p.npz"), G.synthetic_clips()))
    for aid, w in G.synthetic_clips():
        assert np.array_equal(by_file_path[aid], w.astype(np.float32)) and np.array_equal(by_hdf5_path[aid], by_file_path[aid])


def test_collates_equal_the_reference(golden_dir):
    from texttoaudiogrounding_amd.datasets import collate_function, text_tokenizer
    want = np.load(os.path.join(golden_dir, "multi_phrase.npz"))
    tok = text_tokenizer.DictTokenizer(os.path.join(golden_dir, "formats", "vocab.pkl"))
    got = G.collate_outputs(collate_function, tok)
    assert set(got) == set(want.files)
    for k in want.files:
        assert np.array_equal(np.asarray(got[k]), want[k]), k
    b = collate_function.VarNumTextCollate(tok, text_key="phrases", pad_keys=["waveform", "label"])([dict(i) for i in G.COLLATE_ITEMS])
    assert b["phrases_num"] == [3, 1, 2] and torch.is_tensor(b["waveform"]) and b["text_key"] == "phrases"


def test_phrase_count_equals_the_reference_script():
    from texttoaudiogrounding_amd.utils.phrase_stats import phrase_count
    with open(os.path.join(FIX, "strong_label.json")) as f:
        label = json.load(f)
    with open(os.path.join(FIX, "strong_phrase_count.json")) as f:
        want = json.load(f)
    got = phrase_count(label)
    assert got == want and list(got) == list(want) and max(got.values()) > 1


def test_count_tool_writes_the_reference_format(tmp_path):
    import subprocess
    import sys
    out = tmp_path / "count.json"
    tool = os.path.join(os.path.dirname(os.path.dirname(FIX)), "..", "tools", "calc_phrase_count.py")
    subprocess.check_call([sys.executable, tool, "--input", os.path.join(FIX, "strong_label.json"), "--output", str(out)])
    assert out.read_text() == open(os.path.join(FIX, "strong_phrase_count.json")).read()


def test_alias_resolves():
    import importlib
    import sys
    import texttoaudiogrounding_amd as pkg
    pkg.install_aliases(force=True)
    try:
        mod = importlib.import_module("datasets.multi_phrase_dataset")
        assert mod.SamplePhrasesCountDataset.__module__.startswith("texttoaudiogrounding_amd")
        assert hasattr(importlib.import_module("datasets.collate_function"), "VarNumTextCollate")
    finally:
        drop_aliases()


def test_no_cpu_fallback():
    from texttoaudiogrounding_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.phrase_sim_count(torch.zeros(3, 4), torch.zeros(5, 4))


def test_integration_yaml_block_builds_as_written(audio_tsv, golden_dir):
    """The weak-phrase ``data:`` block of INTEGRATION.md, with its file names pointed at the fixtures, through the reference's
    plugin mechanism after install_aliases()."""
    import re
    import sys
    import yaml
    import texttoaudiogrounding_amd as pkg
    from texttoaudiogrounding_amd.utils.train_util import init_obj_from_str
    text = open(os.path.join(os.path.dirname(os.path.dirname(FIX)), "..", "INTEGRATION.md")).read()
    block = next(b for b in re.findall(r"```yaml\n(.*?)```", text, flags=re.S) if "SamplePhrasesCountDataset" in b)
    cfg = yaml.safe_load(block)["data"]["train"]
    files = {"data/train/waveform.csv": audio_tsv, "data/train/label.json": os.path.join(FIX, "label.json"),
             "data/train/phrase_emb.pkl": os.path.join(FIX, "phrase_emb.pkl"),
             "data/train/phrase_sim_count.json": os.path.join(FIX, "phrase_count.json"),
             "data/train/vocab.pkl": os.path.join(golden_dir, "formats", "vocab.pkl")}
    args = cfg["dataset"]["args"]
    for k, v in list(args.items()):
        args[k] = files.get(v, v) if isinstance(v, str) else v
    cfg["collate_fn"]["tokenizer"]["args"]["vocabulary"] = files[cfg["collate_fn"]["tokenizer"]["args"]["vocabulary"]]
    args["sample_rate"] = G.SR
    pkg.install_aliases(force=True)
    try:
        ds, collate = init_obj_from_str(cfg["dataset"]), init_obj_from_str(cfg["collate_fn"])
        np.random.seed(1)
        batch = collate([ds[0], ds[1]])
    finally:
        drop_aliases()
    assert type(ds).__module__.startswith("texttoaudiogrounding_amd") and batch["text"].shape[:2] == (2, 8)
    assert np.asarray(batch["counts"]).shape == (2, 8) and tuple(batch["label"].shape) == (2, 8)
