"""fp64 numpy oracle of the contract of csrc/label_map.hip (include/tag_hip.h, tag_label_map / tag_label_map_topk).

``cosine64``      s[i][c] = x_i . e_c / (||x_i|| ||e_c||) in fp64, a zero row's norm taken as 1.
``select``        the selection rules applied to ANY similarity array (the oracle's fp64 one, or the fp32 one the op returned: the
                  GPU tests demand that the op's other outputs equal these rules on its own ``sim`` exactly): first argmax, its
                  value, the minimum, the window th0 <= s <= th1 && s != 0 with the thresholds as float32, the window's first
                  argmax (-1 when empty), its size and its bit words.
``topk``          the window members in descending s, ties to the lowest index, padded with -1.
``bound(D)``      (D + 8) 2^-24: what an fp32 implementation may differ from ``cosine64`` by.  A D-term fp32 dot product, in any
                  order of additions, errs by at most gamma_D sum |x_d e_d| <= gamma_D ||x|| ||e|| (Cauchy-Schwarz), gamma_D =
                  D u / (1 - D u), u = 2^-24: D u after the division by the norms (plus D^2 u^2, below u / 100 for D < 1000).
                  The two norm factors and the two scalings add a few u more; 8 u covers them.
``decided``       where the oracle decides a selection by more than 2 bound(D), so that every implementation within the bound
                  must agree with it.
``HostLabelMap``  ``utils.label_map.LabelMap`` with the device call replaced by this oracle (for the tests without a GPU).
"""
import numpy as np

U = 2.0 ** -24


def bound(D):
    return (D + 8) * U


def cosine64(x, e):
    x, e = np.asarray(x, dtype=np.float64), np.asarray(e, dtype=np.float64)
    nx, ne = np.sqrt((x * x).sum(1)), np.sqrt((e * e).sum(1))
    nx[nx == 0] = 1.0
    ne[ne == 0] = 1.0
    return (x / nx[:, None]) @ (e / ne[:, None]).T


def thresholds32(th0, th1):
    return np.float32(th0), np.float32(th1)


def window(s, th0, th1):
    th0, th1 = thresholds32(th0, th1)
    s = np.asarray(s)
    return (s >= s.dtype.type(th0)) & (s <= s.dtype.type(th1)) & (s != 0)


def pack_bits(mask):
    N, C = mask.shape
    W = (C + 31) // 32
    padded = np.zeros((N, W * 32), dtype=np.uint32)
    padded[:, :C] = mask
    return (padded.reshape(N, W, 32) << np.arange(32, dtype=np.uint32)).sum(2, dtype=np.uint32)


def select(s, th0, th1):
    s = np.asarray(s)
    rows = np.arange(s.shape[0])
    best = s.argmax(1)                                   # numpy's argmax is the first of equal values
    mask = window(s, th0, th1)
    masked = np.where(mask, s, -np.inf)
    win_best = np.where(mask.any(1), masked.argmax(1), -1)
    return {"best": best.astype(np.int32), "best_sim": s[rows, best], "min_sim": s.min(1), "mask": mask,
            "win_best": win_best.astype(np.int32), "win_count": mask.sum(1).astype(np.int32), "win_bits": pack_bits(mask)}


def topk(s, th0, th1, k):
    s = np.asarray(s)
    mask = window(s, th0, th1)
    order = np.argsort(-np.where(mask, s, -np.inf), axis=1, kind="stable")[:, :k]     # stable: ties keep ascending index
    taken = np.arange(order.shape[1])[None, :] < mask.sum(1)[:, None]
    idx = np.full((s.shape[0], k), -1, dtype=np.int32)
    idx[:, :order.shape[1]] = np.where(taken, order, -1)
    return idx


def decided(s64, th0, th1, D):
    """-> (bit_ok (N, C) bool, best_ok (N,) bool, win_ok (N,) bool): the window bits, ``best`` and ``win_best`` that every
    implementation within bound(D) of s64 shares with the oracle."""
    g = 2.0 * bound(D)
    th0, th1 = (np.float64(t) for t in thresholds32(th0, th1))
    sure_in = (s64 > th0 + g) & (s64 < th1 - g) & (np.abs(s64) > g)
    sure_out = (s64 < th0 - g) | (s64 > th1 + g)
    bit_ok = sure_in | sure_out
    top = np.sort(s64, axis=1)
    best_ok = np.ones(len(s64), dtype=bool) if s64.shape[1] == 1 else (top[:, -1] - top[:, -2] > g)
    # win_best: the oracle's pick is surely a member and beats every label that may be one by more than g
    mask = window(s64, th0, th1)
    masked = np.where(mask, s64, -np.inf)
    w = masked.argmax(1)
    rows = np.arange(len(s64))
    rivals = np.where(~sure_out, s64, -np.inf)
    rivals[rows, w] = -np.inf
    has = mask.any(1)
    win_ok = np.where(has, sure_in[rows, w] & (s64[rows, w] - rivals.max(1) > g), sure_out.all(1))
    return bit_ok, best_ok, win_ok


def host_label_map_class():
    """``LabelMap`` whose rows go through this oracle instead of the device (the similarities rounded to float32)."""
    from texttoaudiogrounding_amd.utils.label_map import LabelMap

    class HostLabelMap(LabelMap):
        def _call(self, x, th0, th1, topk_, want_sim):
            s = cosine64(x, self.label_embs).astype(np.float32)
            sel = select(s, th0, th1)
            k = min(topk_, s.shape[1])
            idx = topk(s, th0, th1, k) if k >= 2 else None
            return (sel["best"], sel["best_sim"], sel["win_best"], sel["win_bits"].view(np.int32), idx, s if want_sim else None)

    return HostLabelMap


def check_datasets_against_golden(golden_dir, tmp_path, device, sim_tol):
    """All four ASMapping datasets of the package on tests/golden/asmapping (make_golden_asmapping.py: the items of the
    reference's datasets) -- every label array exactly, ``label_sim`` to ``sim_tol``.  -> the number of items compared."""
    import json
    import os
    import random
    from texttoaudiogrounding_amd.datasets import (ASMappingEvalDataset, ASMappingEvalLabelSimDataset, ASMappingStrongDataset,
                                                   ASMappingWeakDataset, write_waveform_pack)
    fix = os.path.join(golden_dir, "asmapping")
    with np.load(os.path.join(fix, "items.npz")) as f:
        G = {k: f[k] for k in f.files}
    with open(os.path.join(fix, "config.json")) as f:
        cfg = json.load(f)
    label = os.path.join(golden_dir, "kmeans", "mapping_label.json")
    with open(label) as f:
        clips = json.load(f)
    with np.load(os.path.join(golden_dir, "kmeans.npz")) as f:
        waves = {c["audio_id"]: f[f"wave/{c['audio_id']}"] for c in clips}
    tsv = write_waveform_pack(str(tmp_path / "pack.npz"), list(waves.items()))
    common = dict(waveform=tsv, label=label, phrase_embed=os.path.join(golden_dir, "multi_phrase", "phrase_emb.pkl"),
                  as_label_embed=os.path.join(fix, "as_label_emb.pkl"), device=device)
    train = dict(audioset_label=os.path.join(fix, "audioset_label.tsv"), label_encoder=os.path.join(fix, "classes.json"),
                 sample_rate=cfg["sample_rate"])
    keys = {"weak": ("label",), "strong": ("weak_label", "strong_label", "strong_label_mask")}
    compared = 0
    for name, c in cfg["configs"].items():
        th = None if c["thresholds"] is None else cfg["thresholds"][c["thresholds"]]
        if c["dataset"] == "weak":
            ds = ASMappingWeakDataset(thresholds=th, **common, **train, **c["keywords"])
        else:
            ds = ASMappingStrongDataset(thresholds=th, time_resolution=cfg["time_resolution"], **common, **train, **c["keywords"])
        assert ds.classes_num == 9 and len(ds) == len(clips)
        if th is None:
            assert abs(float(ds.thresholds[0]) - float(G[f"{name}/threshold"])) <= sim_tol and ds.thresholds[1] == 1.0
        random.seed(cfg["crop_seed"])
        for i, clip in enumerate(clips):
            item = ds[i]
            assert (item["audiocap_id"], item["audio_id"], item["text"]) == (clip["audiocap_id"], clip["audio_id"], clip["tokens"])
            assert list(item) == ["audiocap_id", "audio_id", "text", "waveform"] + list(keys[c["dataset"]])
            assert item["waveform"].dtype == np.float32
            want = G.get(f"{name}/{i}/waveform", waves[clip["audio_id"]].astype(np.float32))
            assert np.array_equal(item["waveform"], want), (name, i)
            for k in keys[c["dataset"]]:
                assert item[k].dtype == np.float64 and np.array_equal(item[k], G[f"{name}/{i}/{k}"]), (name, i, k)
                compared += 1
    ev = ASMappingEvalDataset(**common)
    items = [ev[i] for i in range(len(ev))]
    assert len(ev) == len(G["eval/text_idx"]) and list(items[0]) == ["audio_id", "audiocap_id", "start_index", "end_index", "waveform",
                                                                    "text", "text_idx"]
    assert [int(it["text_idx"]) for it in items] == G["eval/text_idx"].tolist()
    assert [it["start_index"] for it in items] == G["eval/start_index"].tolist()
    assert [it["end_index"] for it in items] == G["eval/end_index"].tolist()
    ls = ASMappingEvalLabelSimDataset(**common)
    items = [ls[i] for i in range(len(ls))]
    assert len(ls) == len(G["labelsim/label_sim"]) and list(items[0]) == ["audiocap_id", "start_index", "end_index", "waveform",
                                                                         "label_sim"]
    for it, want in zip(items, G["labelsim/label_sim"]):
        assert it["label_sim"].dtype == np.float32 and it["label_sim"].shape == want.shape
        assert np.abs(it["label_sim"].astype(np.float64) - want).max() <= sim_tol
    return compared + len(ev) + len(ls)
