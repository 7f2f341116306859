"""Launch traces of the whole-encoder autograd nodes, shared by the script that records the fixture
(tests/golden/make_golden_launch_trace.py) and the test that replays it (tests/test_gpu_encoder_launch_trace.py).

A trace is the sequence of launching C-ABI calls of one case: ``[entry name, arguments, "main" | "side"]`` where an integer or
float argument is recorded by value, a pointer argument only as "ptr" / "null", and the last element says whether the launch
went to the device's default stream.  It is taken by replacing ``lib._lib`` with a proxy, so a call is seen whichever module
imported ``call`` by name.  Only ``lib._lib`` and the public model classes are used: the same code records a trace before and
after a change of the autograd nodes, and equal traces mean the GPU was handed the same work in the same order.
"""
import contextlib
import ctypes

import torch

from oracle import tag_oracle as O

SEED = 6000011                      # every dropout seed of a traced step
_NOT_LAUNCHES = ("tag_gru_timed_out", "tag_stream_create_cu_mask")
_QUERY_SUFFIXES = ("_ws_bytes", "_rows", "_ok", "_pack_bytes", "_can_reuse_v")


def launch_entries():
    """Entry points that launch: int-returning, the stream as their last argument."""
    from texttoaudiogrounding_amd import lib
    return {name for name, (res, args) in lib._SIGS.items()
            if res is ctypes.c_int and args and args[-1] is ctypes.c_void_p and name not in _NOT_LAUNCHES
            and not name.endswith(_QUERY_SUFFIXES)}


class _Proxy:
    def __init__(self, real, sigs, names, main_stream, events):
        self._real, self._sigs, self._names, self._main, self._events = real, sigs, names, main_stream, events

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._names:
            return fn
        kinds = self._sigs[name][1][:-1]
        events, main = self._events, self._main

        def recorded(*args):
            vals = [("ptr" if a else "null") if k is ctypes.c_void_p else (a if isinstance(a, float) else int(a))
                    for k, a in zip(kinds, args)]
            events.append([name, vals, "main" if (args[-1] or 0) == main else "side"])
            return fn(*args)
        return recorded


@contextlib.contextmanager
def recording(dev):
    """Yields the list that receives the launches made inside the block; dropout seeds are fixed to SEED."""
    from texttoaudiogrounding_amd import functions, lib
    real = lib.load()
    events = []
    old_seed = functions.new_seed
    lib._lib = _Proxy(real, lib._SIGS, launch_entries(), torch.cuda.default_stream(dev).cuda_stream, events)
    functions.new_seed = lambda: SEED
    try:
        yield events
        torch.cuda.synchronize(dev)
    finally:
        lib._lib = real
        functions.new_seed = old_seed


@contextlib.contextmanager
def _settings(**kw):
    from texttoaudiogrounding_amd import settings
    old = {k: getattr(settings, k) for k in kw}
    for k, v in kw.items():
        setattr(settings, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(settings, k, v)


def build_model(name, **kw):
    """-> (model with seeded initial weights, hop length): 'cnn8rnn' / 'crnn' in a BiEncoder, 'cross_cnn8rnn', 'cross_cdur'."""
    from texttoaudiogrounding_amd.models import audio_encoder as AE, audio_text_model as M, match, text_encoder as TE
    torch.manual_seed(0)
    if name == "cnn8rnn":
        return M.BiEncoder(AE.Cnn8Rnn(32000, **kw), TE.EmbeddingAgg(5221, 512), match.DotProduct(), 512), 320
    if name == "crnn":
        return M.BiEncoder(AE.CrnnEncoder(32000, 256), TE.EmbeddingAgg(5221, 256), match.ExpNegL2(), 256), 640
    if name == "cross_cnn8rnn":
        return M.CrossCnn8_Rnn(32000, TE.EmbeddingAgg(5221, 512)), 320
    return M.CrossCDur(32000, TE.EmbeddingAgg(5221, 256)), 640


def device_inputs(dev, hop):
    """The B = 2 x 1 s batch of the cases as the input dict of a model's forward."""
    b = O.synthetic_batch(2, 32000, seed=5, hop=hop)
    return {"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"], "text": b["text"].to(dev),
            "text_len": torch.as_tensor(b["text_len"]).to(dev), "specaug": False}


def _train(dev, name, freeze=(), specaug=False, **kw):
    """One training step of B = 2 clips of 1 s through StrongRunner.forward_backward (direct-gradient sinks live)."""
    from texttoaudiogrounding_amd.runner import StrongRunner
    model, hop = build_model(name, **kw)
    for k, p in model.named_parameters():
        if k in freeze:
            p.requires_grad_(False)
    runner = StrongRunner(model, device=str(dev))
    runner.model.train()
    batch = O.synthetic_batch(2, 32000, seed=5, hop=hop)
    batch["specaug"] = specaug
    with recording(dev) as ev:
        runner.forward_backward(batch)
    return ev


def _eval(dev, name):
    model, hop = build_model(name)
    model = model.to(dev).eval()
    inp = device_inputs(dev, hop)
    with recording(dev) as ev, torch.no_grad():
        model(inp)
    return ev


def _augmented(dev):
    """The Cnn8Rnn encoder alone (the pairing heads refuse a halved batch, so no StrongRunner and no direct-gradient sinks:
    cnn8rnn_specaug has those): SpecAugment + mixup on B = 4 clips of 1 s."""
    from texttoaudiogrounding_amd.models.audio_encoder import Cnn8Rnn
    torch.manual_seed(0)
    m = Cnn8Rnn(32000).to(dev).train()
    wave = O.synthetic_batch(4, 32000, seed=5)["waveform"].to(dev)
    with recording(dev) as ev:
        out = m({"waveform": wave, "waveform_len": [32000] * 4, "specaug": True, "mixup_lambda": [0.3, 0.7, 0.1, 0.9]})
        out["embedding"].sum().backward()
    return ev


def _with(fn, **settings):
    def run(dev):
        with _settings(**settings):
            return fn(dev)
    return run


CASES = {}
for _n in ("cnn8rnn", "crnn", "cross_cnn8rnn", "cross_cdur"):
    CASES[f"{_n}_train"] = lambda dev, n=_n: _train(dev, n)
    CASES[f"{_n}_eval"] = lambda dev, n=_n: _eval(dev, n)
CASES["cnn8rnn_specaug_mixup"] = _augmented
CASES["cnn8rnn_specaug"] = lambda dev: _train(dev, "cnn8rnn", specaug=True)
CASES["cnn8rnn_freeze_cnn"] = lambda dev: _train(dev, "cnn8rnn", freeze_cnn=True)
CASES["cnn8rnn_wino_forced"] = _with(lambda dev: _train(dev, "cnn8rnn"), WINO_MIN_WORK=1)
CASES["cnn8rnn_x3"] = _with(lambda dev: _train(dev, "cnn8rnn"), CONV_MATH="x3")
CASES["crnn_x3"] = _with(lambda dev: _train(dev, "crnn"), CONV_MATH="x3")
CASES["cross_cdur_frozen_block3_conv"] = lambda dev: _train(dev, "cross_cdur", freeze=("block3.conv.weight",))

#: so that the fixture cannot be vacuous: each group must appear in the union of the traces (one of the names is enough)
COVERAGE = [("tag_conv3x3_wino_forward",),
            ("tag_conv3x3_dgrad_poolsums", "tag_conv3x3_wino_dgrad_poolsums"),
            ("tag_conv3x3_dgrad_bnsums", "tag_conv3x3_wino_dgrad_bnsums"),
            ("tag_conv3x3_c1_backward_bnrelu",),
            ("tag_conv3x3_forward_bnrelu_pool_eval", "tag_conv3x3_wino_forward_bnrelu_pool_eval"),
            ("tag_augment_backward",),
            ("tag_bias_bnrelu_pool_backward",),
            ("tag_bn_act_backward_clip",)]
