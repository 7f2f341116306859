"""Host-side checks of the phrase-to-label map (csrc/label_map.hip, utils/label_map.py, the ASMapping datasets): the fp64 oracle
of tests/label_map_ref.py, wrapped in a host stand-in of LabelMap, reproduces the items the reference's datasets gave
(tests/golden/make_golden_asmapping.py); the documented difference from the reference; the build plumbing; and the argument
checks of the loaded library, which refuse before any launch."""
import ctypes
import json
import os
import pickle
import re

import numpy as np
import pytest

from tests import label_map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["tag_label_map", "tag_label_map_topk", "tag_label_map_ws_bytes"]
TAG_EINVAL = -1                      # include/tag_hip.h


@pytest.fixture()
def host_map(monkeypatch):
    from texttoaudiogrounding_amd.datasets import class_mapping_dataset
    cls = R.host_label_map_class()
    monkeypatch.setattr(class_mapping_dataset, "LabelMap", cls)
    return cls


def test_oracle_selection_rules_on_a_hand_made_case():
    s = np.array([[0.5, 0.9, 0.9, 0.0, -0.2, 0.7],
                  [0.1, 0.0, 0.05, 0.0, 0.0, 0.0],
                  [1.0, 0.6, 0.6, 0.6, 0.95, 0.3]], dtype=np.float32)
    sel = R.select(s, 0.5, 0.9)
    assert sel["best"].tolist() == [1, 0, 0] and sel["win_best"].tolist() == [1, -1, 1]
    assert sel["win_count"].tolist() == [4, 0, 3] and sel["min_sim"].tolist() == [np.float32(-0.2), 0.0, np.float32(0.3)]
    assert sel["win_bits"].tolist() == [[0b100111], [0], [0b001110]]
    assert R.topk(s, 0.5, 0.9, 3).tolist() == [[1, 2, 5], [-1, -1, -1], [1, 2, 3]]
    assert R.topk(s, 0.5, 0.9, 6)[0].tolist() == [1, 2, 5, 0, -1, -1]
    assert R.select(s, 0.9, 0.5)["win_count"].tolist() == [0, 0, 0]                 # th0 > th1: an empty window
    z = R.cosine64(np.array([[0.0, 0.0], [3.0, 4.0]]), np.array([[0.0, 0.0], [6.0, 8.0], [-4.0, 3.0]]))
    assert np.array_equal(z[0], [0.0, 0.0, 0.0]) and z[1, 0] == 0.0 and abs(z[1, 1] - 1.0) <= 1e-15 and abs(z[1, 2]) <= 1e-15
    mask = np.zeros((2, 70), dtype=bool)
    mask[0, [0, 31, 32, 69]] = True
    assert R.pack_bits(mask).tolist() == [[0x80000001, 1, 1 << 5], [0, 0, 0]]
    from texttoaudiogrounding_amd.utils.label_map import window_members
    assert np.array_equal(window_members(R.pack_bits(mask).view(np.int32), 70), mask)


def test_oracle_cosine_equals_sklearn(golden_dir):
    sk = pytest.importorskip("sklearn.metrics.pairwise")
    g = np.random.RandomState(5)
    x, e = g.randn(40, 33).astype(np.float32), g.randn(17, 33).astype(np.float32)
    x[3] = 0
    assert np.abs(R.cosine64(x, e) - sk.cosine_similarity(x.astype(np.float64), e.astype(np.float64))).max() <= 1e-14
    with np.load(os.path.join(golden_dir, "asmapping", "items.npz")) as f:
        sims = f["sims"]
    with open(os.path.join(golden_dir, "asmapping", "config.json")) as f:
        phrases = json.load(f)["phrases"]
    with open(os.path.join(golden_dir, "multi_phrase", "phrase_emb.pkl"), "rb") as f:
        emb = pickle.load(f)
    with open(os.path.join(golden_dir, "asmapping", "as_label_emb.pkl"), "rb") as f:
        labels = pickle.load(f)
    ours = R.cosine64(np.stack([emb[p] for p in phrases]), np.stack(list(labels.values())))
    assert np.abs(ours - sims).max() <= 1e-6


def test_datasets_on_the_host_stand_in_equal_the_reference(host_map, golden_dir, tmp_path):
    assert R.check_datasets_against_golden(golden_dir, tmp_path, device="none", sim_tol=1e-6) >= 4 * 8 + 32


def _tiny_files(tmp_path, phrase_vecs, label_vecs, clip_phrases):
    from texttoaudiogrounding_amd.datasets import write_waveform_pack
    tsv = write_waveform_pack(str(tmp_path / "pack.npz"), [("a.wav", np.zeros(50, dtype=np.float16))])
    paths = {k: str(tmp_path / k) for k in ("label.json", "phrase.pkl", "labels.pkl", "classes.json", "as.tsv")}
    with open(paths["label.json"], "w") as f:
        json.dump([{"audio_id": "a.wav", "audiocap_id": 1, "tokens": "t",
                    "phrases": [{"phrase": p, "start_index": 0, "end_index": 1, "segments": [[0.0, 0.2]]} for p in clip_phrases]}], f)
    with open(paths["phrase.pkl"], "wb") as f:
        pickle.dump({p: np.asarray(v, dtype=np.float32) for p, v in phrase_vecs.items()}, f)
    with open(paths["labels.pkl"], "wb") as f:
        pickle.dump({f"L{i}": np.asarray(v, dtype=np.float32) for i, v in enumerate(label_vecs)}, f)
    with open(paths["classes.json"], "w") as f:
        json.dump([f"L{i}" for i in range(len(label_vecs))], f)
    with open(paths["as.tsv"], "w") as f:
        f.write("audio_id\tevent_labels\na.wav\tL2\n")
    return dict(waveform=tsv, label=paths["label.json"], audioset_label=paths["as.tsv"], phrase_embed=paths["phrase.pkl"],
                as_label_embed=paths["labels.pkl"], label_encoder=paths["classes.json"], sample_rate=100, device="none")


def test_a_phrase_labels_only_window_members(host_map, tmp_path):
    """The documented difference: the reference's argsort picks zero-valued entries when the window holds fewer than topk labels
    (and, in the Strong dataset, when it is empty); here such a phrase labels the members alone, or nothing."""
    from texttoaudiogrounding_amd.datasets import ASMappingStrongDataset, ASMappingWeakDataset
    labels = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    phrases = {"far": [1, 1, 1], "near": [1, 0.1, 0], "two": [1, 0.9, 0]}      # cos: far 0.577 x 3; near 0.995, 0.0995, 0
    files = _tiny_files(tmp_path, phrases, labels, ["far", "near"])
    item = ASMappingStrongDataset(thresholds=[0.9, 1.0], time_resolution=0.1, use_audioset_label=False, topk=1, **files)[0]
    assert item["strong_label_mask"].tolist() == [1, 0, 0] and item["weak_label"].tolist() == [1, 0, 0]
    assert item["strong_label"].shape == (6, 3) and item["strong_label"][:2].tolist() == [[1, 0, 0]] * 2 and item["strong_label"][2:].sum() == 0
    only_far = _tiny_files(tmp_path, phrases, labels, ["far"])
    item = ASMappingStrongDataset(thresholds=[0.9, 1.0], time_resolution=0.1, use_audioset_label=True, topk=1, **only_far)[0]
    assert item["strong_label_mask"].sum() == 0 and item["strong_label"].sum() == 0 and item["weak_label"].tolist() == [0, 0, 1]
    # fewer members than topk: the members alone, in both datasets
    two = _tiny_files(tmp_path, phrases, labels, ["two"])
    assert ASMappingWeakDataset(thresholds=[0.5, 1.0], use_audioset_label=False, topk=3, **two)[0]["label"].tolist() == [1, 1, 0]
    assert ASMappingStrongDataset(thresholds=[0.5, 1.0], use_audioset_label=False, topk=3, **two)[0]["strong_label_mask"].tolist() == [1, 1, 0]
    assert ASMappingWeakDataset(thresholds=[0.5, 1.0], use_audioset_label=False, topk=0, **two)[0]["label"].tolist() == [1, 1, 0]
    # the word limit, and the two assertion messages of the reference
    assert ASMappingWeakDataset(thresholds=[0.5, 1.0], use_audioset_label=False, max_phrase_words=0, **two)[0]["label"].sum() == 0
    with pytest.raises(AssertionError, match="either one of 'thresholds' or 'min_sim_percent' can be set"):
        ASMappingWeakDataset(thresholds=[0.5, 1.0], min_sim_percent=50, **two)
    with pytest.raises(AssertionError, match="currently only support topk = 1 when setting similarity percent"):
        ASMappingWeakDataset(thresholds=None, min_sim_percent=50, topk=2, **two)
    ds = ASMappingWeakDataset(thresholds=None, min_sim_percent=50, **two)
    assert ds.thresholds[1] == 1.0 and ds.thresholds[0] == np.percentile(R.cosine64(np.float32(list(phrases.values())), labels).astype(np.float32).max(1), 50)
    with open(two["label_encoder"], "w") as f:
        json.dump(["L0", "L1"], f)
    with pytest.raises(ValueError, match="3 label embeddings, label_encoder 2 classes"):
        ASMappingWeakDataset(**two)


def test_label_encoder_pickle_and_topk_limit(host_map, tmp_path):
    import types
    from texttoaudiogrounding_amd.datasets import ASMappingWeakDataset
    files = _tiny_files(tmp_path, {"p": [1, 0.5, 0]}, [[1, 0, 0], [0, 1, 0], [0, 0, 1]], ["p"])
    enc = str(tmp_path / "enc.pkl")
    with open(enc, "wb") as f:
        pickle.dump(types.SimpleNamespace(classes_=np.array(["L0", "L1", "L2"])), f)
    files["label_encoder"] = enc
    assert ASMappingWeakDataset(thresholds=[0.1, 1.0], topk=2, **files)[0]["label"].tolist() == [1, 1, 1]      # + AudioSet's L2
    from texttoaudiogrounding_amd import dispatch
    header = open(os.path.join(ROOT, "include", "tag_hip.h")).read()
    assert int(re.search(r"#define TAG_LABEL_MAP_MAX_TOPK (\d+)", header).group(1)) == dispatch.LABEL_MAP_MAX_TOPK == 32


def test_label_map_hip_is_built_declared_and_checks_its_arguments():
    from texttoaudiogrounding_amd import lib
    header = open(os.path.join(ROOT, "include", "tag_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(tag_label_map[a-z_]*)\s*\(", code))) == SYMBOLS
    assert sorted(s for s in lib.declared_symbols() if s.startswith("tag_label_map")) == SYMBOLS
    make = open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "Makefile")).read()
    assert "label_map.hip" in re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    h = lib.load()
    big = 2**31 - 128
    assert lib.query("tag_label_map_ws_bytes", 300, 527, 384) == 4 * (300 + 527)
    assert lib.query("tag_label_map_ws_bytes", big - 1, big - 1, 1) == 4 * (2 * big - 2)
    for shape in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (big, 4, 4), (4, big, 4)):
        assert lib.query("tag_label_map_ws_bytes", *shape) == 0, shape
    # refused with a message before any launch (no GPU is touched): the pointers below are never dereferenced on the host
    a = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)

    def args(x=a, ldx=8, e=a, lde=8, outs=(a,) * 6, sim=None, lds=4, N=4, C=4, D=8, ws=a):
        return (x, ldx, e, lde, 0.5, 1.0) + tuple(outs) + (sim, lds, N, C, D, ws, None)
    bad = [(args(N=0), b"N, C, D must be >= 1 (got 0, 4, 8)"), (args(C=0), b"(got 4, 0, 8)"), (args(D=-2, ldx=8), b"(got 4, 4, -2)"),
           (args(ldx=7), b"ldx = 7, lde = 8 must be >= D = 8"), (args(lde=3), b"ldx = 8, lde = 3 must be >= D = 8"),
           (args(sim=a, lds=3), b"lds = 3 of sim must be >= C = 4"), (args(N=big), b"N = 2147483520 exceeds 2147483519"),
           (args(C=big), b"C = 2147483520 exceeds 2147483519"), (args(x=None), b"argument check failed"),
           (args(e=None), b"argument check failed"), (args(ws=None), b"argument check failed")]
    bad += [(args(outs=(a,) * i + (None,) + (a,) * (5 - i)), b"argument check failed") for i in range(6)]
    for call_args, message in bad:
        assert h.tag_label_map(*call_args) == TAG_EINVAL and message in h.tag_last_error(), (message, h.tag_last_error())
    bad_topk = [((None, 4, 0.5, 1.0, a, 4, 4, 2), b"argument check failed"), ((a, 4, 0.5, 1.0, None, 4, 4, 2), b"argument check failed"),
                ((a, 4, 0.5, 1.0, a, 0, 4, 2), b"(got 0, 4, 1)"), ((a, 3, 0.5, 1.0, a, 4, 4, 2), b"lds = 3 of sim must be >= C = 4"),
                ((a, 4, 0.5, 1.0, a, 4, 4, 0), b"k = 0 must lie in [1, 32]"), ((a, 4, 0.5, 1.0, a, 4, 4, 33), b"k = 33 must lie in [1, 32]")]
    for call_args, message in bad_topk:
        assert h.tag_label_map_topk(*call_args, None) == TAG_EINVAL and message in h.tag_last_error(), (message, h.tag_last_error())


def test_ops_and_tool_refuse_without_a_device(tmp_path):
    import importlib.util
    import torch
    from texttoaudiogrounding_amd import ops
    x = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="expected a tensor on the MI355X"):
        ops.label_map(x, x, 0.5, 1.0)
    spec = importlib.util.spec_from_file_location("map_phrase_to_event_tool", os.path.join(ROOT, "tools", "map_phrase_to_event.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.build_parser().parse_args(["--phrase_emb", "p.pkl", "--label_emb", "l.pkl", "--output", "o.tsv"])
    assert (args.phrase_emb, args.label_emb, args.output, args.device) == ("p.pkl", "l.pkl", "o.tsv", "cuda:0")
    out = str(tmp_path / "o.tsv")
    tool.write_table([("a dog", 3, np.float32(0.25)), ("b", 0, np.float32(1 / 3))], out)
    assert open(out).read() == "phrase\tindex\tsim\na dog\t3\t0.25\nb\t0\t0.33333334\n"
