#!/usr/bin/env python3
"""Generate tests/golden/cnn8rnn_specaug_train.npz and cnn8rnn_specaug_mixup_train.npz: one training step of the IMPORTED
REFERENCE's Cnn8Rnn (models/audio_encoder.py:88-232) with SpecAugment, and with SpecAugment + mixup, at the encoder level.

    python tests/golden/make_golden_specaug.py

torchlibrosa is not installed: ``models.audio_encoder.SpecAugmentation`` is replaced by the test-side twin
(tests/torchlibrosa_twin.py) BEFORE the encoder is built, so that the widths come from the reference's own constructor call
(:126-131); the twin records the stripes it draws.  Dropout off (DropoutReplay(off=True)), train-mode BatchNorm, B = 4 clips of
1.5 s with ragged lengths, the oracle's init_state weights, loss = sum(embedding * R) for a fixed random R (regenerated from
R_SEED by the tests).  Mixup: lambda = the reference's Mixup(1.).get_lambda(4), do_mixup on the bn0 output and on `length`.

Stored per case: the torch seed and the stripes drawn, lambda, the embedding (fp64 run, stored as float32) and the fp32 run's
max distance from it, `length` with its dtype, per-parameter gradient summaries of the fp64 and fp32 runs (make_golden.py's
grad_summary), the running statistics after the step (fp64 run).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_import  # noqa: E402
from make_golden import DropoutReplay, grad_summary  # noqa: E402
from oracle import tag_oracle as O  # noqa: E402
from tests import torchlibrosa_twin  # noqa: E402

torch.set_num_threads(8)
mods = ref_import.install()
AE = mods["models.audio_encoder"]
import importlib  # noqa: E402
TU = importlib.import_module("utils.train_util")

B, S = 4, 48000
LENS = np.array([S, S - 7000, S - 16123, S - 3200])
R_SEED = 31
CASES = (("cnn8rnn_specaug_train", 2024, False), ("cnn8rnn_specaug_mixup_train", 2025, True))


def make_inputs():
    b = O.synthetic_batch(B, S, seed=1234, ragged=False, hop=320)
    wave = b["waveform"].clone()
    for i in range(B):
        wave[i, LENS[i]:] = 0.0
    return wave


def encoder_state():
    st = O.init_state(seed=7, text_dim=512, shared_dim=512, logit_gain=120.0)
    return {k[len("audio_encoder."):]: v for k, v in st.items() if k.startswith("audio_encoder.")}


def build_encoder(dtype):
    AE.SpecAugmentation = torchlibrosa_twin.SpecAugmentation        # before the constructor runs (:126-131)
    enc = AE.Cnn8Rnn(sample_rate=32000)
    missing = enc.load_state_dict(encoder_state(), strict=False)
    assert not missing.unexpected_keys and all("melspec_extractor" in k for k in missing.missing_keys), missing
    assert isinstance(enc.spec_augmenter, torchlibrosa_twin.SpecAugmentation)
    return enc.to(dtype).train(True)


def r_tensor(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(R_SEED), dtype=torch.float64)


def run(dtype, seed, lam):
    enc = build_encoder(dtype)
    wave = make_inputs().to(dtype)
    d = {"waveform": wave, "waveform_len": LENS, "specaug": True}
    if lam is not None:
        d["mixup_lambda"] = lam
    torch.manual_seed(seed)
    with DropoutReplay(off=True):
        out = enc(d)
    emb = out["embedding"]
    loss = (emb * r_tensor(emb.shape).to(dtype)).sum()
    loss.backward()
    grads = {k: p.grad for k, p in enc.named_parameters() if p.grad is not None}
    stripes = enc.spec_augmenter.table(B)
    running = {k: v.detach().double().numpy() for k, v in enc.state_dict().items() if "running_" in k}
    return emb.detach(), out["length"], grads, stripes, running, float(loss)


def main():
    for name, seed, mixup in CASES:
        lam = TU.Mixup(1.).get_lambda(B) if mixup else None
        e64, len64, g64, st64, run64, l64 = run(torch.float64, seed, lam)
        e32, len32, g32, st32, _, l32 = run(torch.float32, seed, lam)
        assert torch.equal(st64, st32), "the two runs drew different stripes"
        assert torch.equal(len64, len32) and len64.dtype == len32.dtype
        assert e64.shape[0] == (B // 2 if mixup else B)
        store = {"seed": np.array(seed), "r_seed": np.array(R_SEED), "lens": LENS, "stripes": st64.numpy(),
                 "n_time": np.array(2), "loss_f64": np.array(l64), "loss_f32": np.array(l32),
                 "embedding_f64_as_f32": e64.float().numpy(),
                 "embedding_f32_err": np.array((e32.double() - e64).abs().max().item()),
                 "length": len64.numpy(), "length_dtype": np.array(str(len64.dtype))}
        if lam is not None:
            store["mixup_lambda"] = np.asarray(lam, dtype=np.float64)
        for k, v in grad_summary(g64).items():
            store[f"grad_f64/{k}"] = v
        for k, v in grad_summary(g32).items():
            store[f"grad_f32/{k}"] = v
        for k, v in run64.items():
            store[f"after/{k}"] = v.astype(np.float32)
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **store)
        print(name, "stripes", st64.tolist(), "lambda", None if lam is None else list(lam), "length", len64.tolist(),
              "loss", l64, "emb err f32", store["embedding_f32_err"])


if __name__ == "__main__":
    main()
