#!/usr/bin/env python3
"""Fixture of the IMPORTED REFERENCE's early-fusion CrossCDur (models/audio_text_model.py:461-568) with an EmbeddingAgg(5221, 256)
text encoder.  Data only; weights and inputs are regenerated from seeds by tests/cross_cdur_state.py (which does not touch the
reference), loaded into the reference here and into this package's model by the tests.

    python tests/golden/make_golden_cross_cdur.py        (build container only: needs the reference)

Writes tests/golden/cross_cdur.npz:
(a) the reference's state-dict keys and shapes;
(b) eval, B = 2 x 10 s (second clip 8 s, zero-padded): frame_sim of the fp64 twin and of the fp32 reference, ``length``, the
    segments utils/eval_util.py's own functions produce from the fp32 scores at the 50 thresholds (window 1, n_connect =
    ceil(0.5 / 0.08)), ``margin``: the distance of the nearest fp64 score to each threshold; the same pass with upsample=True;
(c) one training step, B = 2, S = 64 000, dropout off, FrameBceLoss on a Bernoulli(0.5) label: fp64 loss, per parameter the fp64
    gradient as norm, largest magnitude and seeded sampled entries, the fp32 reference's own distance from it (the ``floor``),
    and the BatchNorm buffers after the step.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import tag_oracle as O  # noqa: E402
from make_golden import DropoutReplay, mods  # noqa: E402  (installs the reference import)
from tests import cross_cdur_state as CS  # noqa: E402

RM, TE, EU, LOSS = mods["models.audio_text_model"], mods["models.text_encoder"], mods["utils.eval_util"], mods["losses"]


def reference(st, dtype, upsample=False):
    m = RM.CrossCDur(32000, TE.EmbeddingAgg(CS.VOCAB, CS.D_TEXT), upsample=upsample)
    m.load_state_dict(st, strict=True)
    return m.to(dtype)


def inputs(b, dtype):
    return {"waveform": b["waveform"].to(dtype), "waveform_len": b["waveform_len"], "text": b["text"],
            "text_len": b["text_len"]}                          # no specaug / mixup_lambda keys: the forward reads neither


def main():
    torch.set_num_threads(8)
    out = {}
    ref0 = RM.CrossCDur(32000, TE.EmbeddingAgg(CS.VOCAB, CS.D_TEXT))
    sd0 = ref0.state_dict()
    keys = [(k, tuple(v.shape)) for k, v in sd0.items()]
    assert keys == CS.reference_keys(), "tests/cross_cdur_state.reference_keys() is not the reference's state dict"
    assert len(keys) == 53
    assert sum(p.numel() for n, p in ref0.named_parameters() if not n.startswith("text_encoder")) == 884355
    out["keys"] = np.array([k for k, _ in keys])
    out["shapes"] = np.array([",".join(map(str, s)) for _, s in keys])

    eb = CS.eval_batch()
    lm = O.logmel(eb["waveform"].double(), "crnn")
    stats = (float(lm.mean()), float(lm.var(unbiased=False)))
    out["block1_bn_running"] = np.array(stats)
    st = CS.draw_state(stats)
    out["state_checksum"] = CS.state_checksum(st)
    out["input_checksum"] = np.array(CS.checksum(eb["waveform"]) + CS.checksum(eb["text"].float()))

    # ---- (b) eval ----
    thresholds = np.arange(1 / 100, 1, 1 / 50)
    n_connect = int(np.ceil(0.5 / 0.08))
    fs = {}
    for up in (False, True):
        for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            m = reference(st, dtype, up).eval()
            with torch.no_grad():
                o = m(inputs(eb, dtype))
            fs[(up, tag)] = o["frame_sim"].double().numpy()
            fs[(up, "len")] = o["length"].numpy()
    assert fs[(False, "f32")].shape == (2, 125) and fs[(True, "f32")].shape == (2, 500)
    assert fs[(False, "len")].tolist() == [125, 100] and fs[(True, "len")].tolist() == [500, 400]
    f32, f64 = fs[(False, "f32")], fs[(False, "f64")]
    ref_err = float(np.abs(f32 - f64).max())
    seg_rows, margin = [], np.zeros((2, len(thresholds)))
    for b in range(2):
        for ti, th in enumerate(thresholds):
            filt = EU.median_filter(torch.from_numpy(f32[b]).float().unsqueeze(0), window_size=1, threshold=th)[0]
            reg = EU.find_contiguous_regions(EU.connect_clusters(filt, n_connect))
            margin[b, ti] = np.abs(f64[b] - th).min()
            for on, off in reg:
                seg_rows.append((b, ti, int(on), int(off)))
    n4 = int((margin > 4 * ref_err).sum())
    n2 = int((margin > 2 * (1e-4 + ref_err)).sum())
    print(f"eval: scores {f64.min():.4g} .. {f64.max():.4g}; fp32 reference {ref_err:.2e} from fp64; {len(seg_rows)} segments; "
          f"margins above 4 x that error {n4}/100, above 2 x (1e-4 + error) {n2}/100")
    assert n4 == 100 and n2 >= 95, "the drawn weights put scores on thresholds: change STATE_SEED"
    out.update(frame_sim_f64=f64, frame_sim_f32=f32.astype(np.float32), frame_sim_ref_err=np.array(ref_err),
               length=fs[(False, "len")], frame_sim_up_f64=fs[(True, "f64")], length_up=fs[(True, "len")],
               frame_sim_up_ref_err=np.array(float(np.abs(fs[(True, "f32")] - fs[(True, "f64")]).max())),
               thresholds=thresholds, n_connect=np.array(n_connect), segments=np.asarray(seg_rows, dtype=np.int64).reshape(-1, 4),
               margin=margin)

    # ---- (c) one training step, dropout off ----
    tb = CS.train_batch()
    out["train_input_checksum"] = np.array(CS.checksum(tb["waveform"]) + CS.checksum(tb["label"]))
    res = {}
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        m = reference(st, dtype).train()
        with DropoutReplay(off=True):
            o = m(inputs(tb, dtype))
            fsim = o["frame_sim"]
            label = tb["label"].to(dtype)
            tt = min(fsim.size(1), label.size(1))
            loss = LOSS.FrameBceLoss()({"frame_sim": fsim[..., :tt], "label": label[..., :tt],
                                        "length": torch.clamp(o["length"], 1, tt)})
            loss.backward()
        res[tag] = (float(loss.item()), {k: p.grad.detach().double() for k, p in m.named_parameters()},
                    {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k},
                    fsim.detach().double().numpy())
    out["loss_f64"], out["loss_f32"] = np.array(res["f64"][0]), np.array(res["f32"][0])
    out["train_frame_sim_f64"] = res["f64"][3]
    print(f"train: loss fp64 {res['f64'][0]:.9f}, fp32 {res['f32'][0]:.9f} ({abs(res['f64'][0] - res['f32'][0]):.2e} apart)")
    worst = 0.0
    for name, g in res["f64"][1].items():
        flat, f32g = g.flatten(), res["f32"][1][name].flatten()
        idx = CS.sample_index(name, tuple(g.shape), tb["text"])
        scale = flat.abs().max().item() + 1e-300
        out[f"grad/{name}"] = np.concatenate([[flat.norm().item(), flat.abs().max().item()], flat[idx].numpy()])
        out[f"floor/{name}"] = np.array([(f32g - flat).abs().max().item() / scale,
                                         abs(f32g.norm().item() - flat.norm().item()) / (flat.norm().item() + 1e-300)])
        worst = max(worst, out[f"floor/{name}"].max())
        print(f"  {name:40s} |g| {flat.norm().item():.3e}  fp32 floor {out[f'floor/{name}'][0]:.2e} (norm {out[f'floor/{name}'][1]:.2e})")
    print(f"  worst gradient floor {worst:.2e}")
    assert len(res["f64"][1]) == 38
    for k, v in res["f64"][2].items():
        out[f"after/{k}"] = v.numpy()
    path = os.path.join(HERE, "cross_cdur.npz")
    np.savez_compressed(path, **out)
    print("wrote cross_cdur.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
