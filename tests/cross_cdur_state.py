"""Seeded weights and inputs of the CrossCDur fixture (tests/golden/cross_cdur.npz), shared by the script that makes the fixture
and the tests that read it.  Nothing here touches the reference: the state dict is drawn in the reference's key order from one
seeded generator; the fixture carries a checksum of what was drawn.

The drawn values follow the constructor's distributions (kaiming-normal convs, kaiming-uniform linears and embedding, nn.GRU's
uniform) except that every bias and every BatchNorm parameter and buffer is non-trivial (all biases are zero at init, which would
hide a missing term), ``block1.bn``'s running statistics are the log-mel's own (passed in: the fixture stores them) so that eval
activations are sane, and ``fc_output.weight`` is scaled by 6 so that the scores span the evaluation thresholds."""
import math

import numpy as np
import torch

from oracle import tag_oracle as O

VOCAB, D_TEXT = 5221, 256
STATE_SEED = 4179
EVAL_SEED, TRAIN_SEED = 5101, 5102
HOP = 640
N_SAMPLE = 512
CHANNELS = [(1, 32), (32, 128), (128, 128), (128, 128), (128, 128)]


def reference_keys():
    """[(key, shape)] of the reference CrossCDur's state dict with an EmbeddingAgg text encoder, in module order
    (models/audio_text_model.py:482-514): 53 entries."""
    keys = [("text_encoder.embedding.core.weight", (VOCAB, D_TEXT))]
    for i, (cin, cout) in enumerate(CHANNELS, start=1):
        p = f"block{i}."
        keys += [(p + "bn.weight", (cin,)), (p + "bn.bias", (cin,)), (p + "bn.running_mean", (cin,)),
                 (p + "bn.running_var", (cin,)), (p + "bn.num_batches_tracked", ()), (p + "conv.weight", (cout, cin, 3, 3)),
                 (p + "fc_text.weight", (cout, D_TEXT)), (p + "fc_text.bias", (cout,))]
    for sfx in ("", "_reverse"):
        keys += [(f"gru.weight_ih_l0{sfx}", (384, 128)), (f"gru.weight_hh_l0{sfx}", (384, 128)),
                 (f"gru.bias_ih_l0{sfx}", (384,)), (f"gru.bias_hh_l0{sfx}", (384,))]
    keys += [("fc_text.weight", (256, D_TEXT)), ("fc_text.bias", (256,)), ("fc_output.weight", (1, 256)), ("fc_output.bias", (1,))]
    return keys


def draw_state(block1_stats, seed=STATE_SEED):
    """The fixture's state dict (fp32), keyed by the reference's names.  block1_stats: (mean, var) of the log-mel."""
    g = torch.Generator().manual_seed(seed)
    randn = lambda shape: torch.randn(shape, generator=g)
    uni = lambda shape, b: (torch.rand(shape, generator=g) * 2 - 1) * b
    st = {}
    for key, shape in reference_keys():
        if key.endswith("num_batches_tracked"):
            v = torch.tensor(3, dtype=torch.long)
        elif key.endswith("bn.weight"):
            v = 1 + 0.2 * randn(shape)
        elif key.endswith("running_mean"):
            v = 0.1 * randn(shape)
        elif key.endswith("running_var"):
            v = 0.5 + torch.rand(shape, generator=g)
        elif key.startswith("gru."):
            v = uni(shape, 1.0 / math.sqrt(128))
        elif key.endswith("bias"):
            v = 0.2 * randn(shape)
        elif key.endswith("conv.weight"):
            v = randn(shape) * math.sqrt(2.0 / (shape[1] * 9))
        else:                                                   # linear / embedding weight: kaiming-uniform over fan_in
            v = uni(shape, math.sqrt(6.0 / shape[1]))
        st[key] = v
    st["block1.bn.running_mean"] = torch.tensor([float(block1_stats[0])])
    st["block1.bn.running_var"] = torch.tensor([float(block1_stats[1])])
    st["fc_output.weight"] = st["fc_output.weight"] * 6
    return st


def checksum(t):
    t = t.detach().double().flatten()
    return [float(t.sum()), float(t.abs().max()), float(t[:: max(1, t.numel() // 7)][:7].sum())]


def state_checksum(st):
    return np.array([c for k, _ in reference_keys() if st[k].is_floating_point() for c in checksum(st[k])])


def eval_batch():
    """B = 2 clips of 10 s @ 32 kHz, the second 8 s long and zero-padded."""
    S = 320000
    b = O.synthetic_batch(2, S, seed=EVAL_SEED, ragged=False, hop=HOP, vocab_size=VOCAB)
    lens = np.array([S, 256000])
    b["waveform"][1, lens[1]:] = 0.0
    b["waveform_len"] = lens
    return b


def train_batch():
    """B = 2 clips of 2 s, the second ragged; label: Bernoulli(0.5) over the (64000 // 640 + 1) // 4 = 25 output frames."""
    S = 64000
    b = O.synthetic_batch(2, S, seed=TRAIN_SEED, ragged=False, hop=HOP, vocab_size=VOCAB)
    lens = np.array([S, 50000])
    b["waveform"][1, lens[1]:] = 0.0
    b["waveform_len"] = lens
    return b


def sample_index(name, shape, text=None):
    """Entries of a gradient tensor the fixture stores: N_SAMPLE seeded positions; for the embedding table every entry of the
    rows of the tokens the batch uses (a random sample of the 5221 x 256 table would be zeros)."""
    numel = int(np.prod(shape)) if len(shape) else 1
    if name.endswith("embedding.core.weight") and text is not None:
        rows = torch.unique(torch.as_tensor(text).flatten())
        return (rows[:, None] * shape[1] + torch.arange(shape[1])[None]).flatten()
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return torch.randint(0, numel, (min(N_SAMPLE, numel),), generator=g)
