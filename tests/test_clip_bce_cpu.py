"""The clip-level BCE objectives without a GPU: the statements of tests/clip_bce_ref.py against the fixture made from the
imported reference, the analytic derivative the kernels evaluate against autograd of the statements (end points included), the
reference-shaped loss classes, operator registration with fake kernels, the wrappers' and the C ABI's argument checks."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import clip_bce_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_bce.npz")
SYMBOLS = ("tag_clip_bce_ws_bytes", "tag_clip_bce_forward", "tag_clip_bce_backward")
TAG_EINVAL = -1                      # include/tag_hip.h


@pytest.fixture(scope="module")
def cases():
    return R.load_golden(GOLDEN)


def test_fixture_case_names_are_complete(cases):
    assert sorted(cases) == sorted(R.golden_names()) and len(cases) == 6 * 9
    for name, c in cases.items():
        assert c["cfg"] in [tuple(float(v) for v in cfg) for cfg in R.GOLDEN_CONFIGS[c["kind"]]], name
        assert c["p"].dtype == np.float64 and c["p"].shape == c["label"].shape == c["counts"].shape == c["dp_f64"].shape
        assert c["p"].min() >= 0.01 and c["p"].max() <= 0.99 and c["counts"].min() >= 1 and c["counts"].max() <= 499
        assert np.isfinite(c["dp_f64"]).all() and np.isfinite(c["dp_f32"]).all() and c["dp_f32"].dtype == np.float32
        fractional = bool(((c["label"] != 0) & (c["label"] != 1)).any())
        assert fractional == ("_soft_" in name) or c["p"].size == 1, name


def test_statement_equals_the_reference(cases):
    for name, c in cases.items():
        aux = R.aux_from_counts(c["kind"], c["cfg"], c["counts"])
        fn = R.statement(c["kind"], c["cfg"], torch.from_numpy(c["label"]), aux)
        loss, dp = R.loss_and_grad(fn, torch.from_numpy(c["p"]))
        assert abs(float(loss) - float(c["loss_f64"])) <= 1e-12 * max(1.0, abs(float(loss))), name
        assert np.abs(dp.numpy() - c["dp_f64"]).max() <= 1e-12 * max(1.0, np.abs(c["dp_f64"]).max()), name


def _derivative_cases():
    for kind in R.KINDS:
        for cfg in R.SWEEP_CONFIGS[kind]:
            yield kind, cfg
    yield "focal", (0, 0.5)
    yield "focal", (0.5, 0.3)            # gamma < 1: (1 - p)^(gamma - 1) is infinite at p = 1 without the guard
    yield "freq", (100, 0)
    yield "origin", (1, 0, 1e-3)
    yield "prior", (1000, 0)


def test_analytic_derivative_equals_autograd_of_the_statement():
    inputs = [R.make_inputs(5, 7, 3), R.make_inputs(3, 64, 4, soft=True), R.end_point_inputs()]
    assert {(float(p), float(y)) for p, y in zip(inputs[2][0][0], inputs[2][1][0])} == {(0.0, 0.0), (0.0, 1.0), (0.0, 0.3),
                                                                                        (1.0, 0.0), (1.0, 1.0), (1.0, 0.3)}
    for kind, cfg in _derivative_cases():
        for p, label, counts in inputs:
            aux = R.aux_from_counts(kind, cfg, counts)
            aux = None if aux is None else torch.from_numpy(aux)
            loss, dp = R.loss_and_grad(R.statement(kind, cfg, label, aux), p)
            want = R.dterm(kind, cfg, p, label, aux) / p.numel()
            assert torch.isfinite(loss) and torch.isfinite(dp).all() and torch.isfinite(want).all(), (kind, cfg)
            assert (dp - want).abs().max().item() <= 1e-10 * max(1.0, want.abs().max().item()), (kind, cfg)


def test_identities_of_the_statements():
    """What the GPU test asserts of the kernels holds of the statements, with an exact 1.0 in the input."""
    p, label, counts = R.end_point_inputs()
    bce = lambda q: torch.nn.functional.binary_cross_entropy(q, label)          # noqa: E731
    want = R.loss_and_grad(bce, p)
    for kind, cfg, factor in (("focal", (0, 0.5), 2.0), ("freq", (100, 0), 1.0), ("origin", (1, 0, 1e-3), 1.0),
                              ("prior", (1000, 0), 1.0)):
        aux = R.aux_from_counts(kind, cfg, counts)
        got = R.loss_and_grad(R.statement(kind, cfg, label, None if aux is None else torch.from_numpy(aux)), p)
        assert abs(factor * float(got[0]) - float(want[0])) <= 1e-12 * float(want[0]), kind
        assert (factor * got[1] - want[1]).abs().max() <= 1e-12 * want[1].abs().max(), kind


def test_loss_classes_have_the_reference_signatures():
    from texttoaudiogrounding_amd import losses
    expect = {"FocalClipBceLoss": (("gamma", 2), ("alpha", 0.25)),
              "ClipBceLossFreqWeight": (("C", inspect.Parameter.empty), ("gamma", inspect.Parameter.empty)),
              "SymmetricClipBceLoss": (("a", 1), ("b", 1), ("eps", 1e-3)),
              "OriginSymmetricClipBceLoss": (("a", 1), ("b", 1), ("eps", 1e-3)),
              "PriorAdjustedClipBceLoss": (("data_size", inspect.Parameter.empty), ("tau", 1)),
              "VectorQuantizeLoss": (("loss_fn", inspect.Parameter.empty), ("vq_weight", 1.0))}
    for cls, params in expect.items():
        sig = inspect.signature(getattr(losses, cls).__init__)
        assert [(k, v.default) for k, v in sig.parameters.items()][1:] == list(params), cls
    assert vars(losses.FocalClipBceLoss(1.5, 0.4)).items() >= {"gamma": 1.5, "alpha": 0.4}.items()
    assert vars(losses.ClipBceLossFreqWeight(100, 0.5)).items() >= {"C": 100, "gamma": 0.5}.items()
    assert vars(losses.SymmetricClipBceLoss(0.7, 1.3, 1e-2)).items() >= {"a": 0.7, "b": 1.3, "eps": 1e-2}.items()
    o = losses.OriginSymmetricClipBceLoss(0.7, 1.3, 1e-2)
    assert (o.a, o.b, o.A) == (0.7, 1.3, math.log(1e-2)) and not hasattr(o, "eps")
    assert vars(losses.PriorAdjustedClipBceLoss(1000, 0.5)).items() >= {"data_size": 1000, "tau": 0.5}.items()
    assert not hasattr(losses, "MaskedClipBceLoss")
    for kind, (cls, args) in R.CLASSES.items():
        assert set(args) <= set(inspect.signature(getattr(losses, cls).__init__).parameters), kind


def test_signatures_and_attributes_equal_the_imported_reference():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import ref_import
    if not ref_import.available():
        pytest.skip("the reference is not on this machine")
    from texttoaudiogrounding_amd import losses
    ref = ref_import.install()["losses"]
    try:
        args = {"ClipBceLossFreqWeight": (100, 0.5), "PriorAdjustedClipBceLoss": (1000,),
                "VectorQuantizeLoss": (torch.nn.Identity(),)}
        for cls in [c for c, _ in R.CLASSES.values()] + ["VectorQuantizeLoss"]:
            ours, theirs = getattr(losses, cls), getattr(ref, cls)
            assert str(inspect.signature(ours.__init__)) == str(inspect.signature(theirs.__init__)), cls
            a, b = ours(*args.get(cls, ())), theirs(*args.get(cls, ()))
            keep = lambda o: {k: v for k, v in vars(o).items() if not k.startswith("_") and k != "training"}   # noqa: E731
            assert keep(a) == keep(b), cls
        assert hasattr(ref.VectorQuantizeLoss, "get_separate_loss")
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "losses", "utils")]:
            del sys.modules[k]


def test_yaml_style_construction_and_aliases():
    import sys
    import texttoaudiogrounding_amd as pkg
    from texttoaudiogrounding_amd.utils.train_util import init_obj_from_str
    pkg.install_aliases(force=True)
    try:
        loss = init_obj_from_str({"type": "losses.FocalClipBceLoss", "args": {"gamma": 2, "alpha": 0.25}})
        assert type(loss).__module__ == "texttoaudiogrounding_amd.losses" and (loss.gamma, loss.alpha) == (2, 0.25)
        import losses as aliased
        for cls in [c for c, _ in R.CLASSES.values()] + ["VectorQuantizeLoss"]:
            assert hasattr(aliased, cls), cls
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "losses", "utils")]:
            del sys.modules[k]


def test_operators_registered_with_schemas_and_fake_kernels():
    import texttoaudiogrounding_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("clip_bce", "clip_bce_backward"):
        assert name in T.OP_NAMES and hasattr(torch.ops.tag, name)
        assert "Tensor? aux" in str(getattr(torch.ops.tag, name).default._schema)
    with FakeTensorMode():
        y = torch.empty(5, 7)
        assert torch.ops.tag.clip_bce(torch.empty(5, 7), y, None, 0, 2.0, 0.25, 0.0).shape == ()
        assert torch.ops.tag.clip_bce(torch.empty(5, 7), y, torch.empty(5, 7), 4, 1.0, 0.0, 0.0).shape == ()
        dp = torch.ops.tag.clip_bce_backward(torch.empty(7, 5).t(), y, None, 2, 1e-3, 0.0, 0.0, torch.empty(()))
        assert dp.shape == (5, 7) and dp.is_contiguous()
        # the autograd formula runs through the backward operator's fake kernel; label and aux get no gradient
        c = torch.empty(5, 7, requires_grad=True)
        label, aux = torch.empty(5, 7, requires_grad=True), torch.empty(5, 7, requires_grad=True)
        (torch.ops.tag.clip_bce(c, label, aux, 1, 0.0, 0.0, 0.0) + torch.ops.tag.clip_bce(c.t().t(), label, None, 3, 1.0, 1.0, -6.9)
         ).backward()
        assert c.grad.shape == (5, 7) and label.grad is None and aux.grad is None


def test_wrappers_check_their_arguments_before_any_call(monkeypatch):
    from texttoaudiogrounding_amd import dispatch, losses

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(dispatch, "call", no_call)
    monkeypatch.setattr(dispatch, "query", no_call)
    assert dispatch.CLIP_BCE_MODES == {"focal": 0, "freq_weight": 1, "symmetric": 2, "origin_symmetric": 3, "prior_adjusted": 4}
    p, y = torch.rand(3, 4), torch.rand(3, 4)
    one = torch.ones(())
    for fwd in (True, False):
        def run(*args):
            return dispatch.clip_bce_forward(*args) if fwd else dispatch.clip_bce_backward(*args, one)
        with pytest.raises(RuntimeError, match="mode 5"):
            run(p, y, None, 5, 0.0, 0.0, 0.0)
        with pytest.raises(RuntimeError, match="NaN"):
            run(p, y, None, 0, float("nan"), 0.25, 0.0)
        with pytest.raises(RuntimeError, match=r"label \(4, 3\): expected clip_sim's shape \(3, 4\)"):
            run(p, y.t(), None, 0, 2.0, 0.25, 0.0)
        with pytest.raises(RuntimeError, match=r"aux \(3, 1\)"):
            run(p, y, torch.rand(3, 1), 1, 0.0, 0.0, 0.0)
        for mode in (1, 4):
            with pytest.raises(RuntimeError, match="needs aux"):
                run(p, y, None, mode, 1.0, 0.0, 0.0)
        with pytest.raises(RuntimeError, match=r"\(B,N\) matrix"):
            run(p[0], y[0], None, 0, 2.0, 0.25, 0.0)
        with pytest.raises(RuntimeError, match=r"\(B,N\) matrix"):
            run(p[:0], y[:0], None, 0, 2.0, 0.25, 0.0)
        with pytest.raises(RuntimeError, match="label: expected float32"):
            run(p, y.double(), None, 0, 2.0, 0.25, 0.0)
        with pytest.raises(RuntimeError, match="clip_sim: expected float32"):
            run(p.double(), y, None, 0, 2.0, 0.25, 0.0)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            run(p, y, None, 0, 2.0, 0.25, 0.0)
    # the modules: counts of another shape (the dataset's empty lists) -> ValueError naming both shapes; CPU tensors raise
    out = {"clip_sim": p, "label": y, "counts": [[], [], []]}
    for loss in (losses.ClipBceLossFreqWeight(100, 0.5), losses.PriorAdjustedClipBceLoss(1000)):
        with pytest.raises(ValueError, match=r"counts \(3, 0\).*\(3, 4\)"):
            loss(out)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            loss({"clip_sim": p, "label": y, "counts": np.ones((3, 4), dtype=np.int64)})
    for loss in (losses.FocalClipBceLoss(), losses.SymmetricClipBceLoss(), losses.OriginSymmetricClipBceLoss()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            loss(out)


def test_modules_hand_the_reference_expression_to_the_operator(monkeypatch):
    """What reaches tag::clip_bce: mode, constants, and the weight / prior formed on the host from numpy or tensor counts."""
    from texttoaudiogrounding_amd import losses, ops
    seen = []
    # (the operator looks its body up in the ops namespace, whose re-exports cannot be assigned: replace the binding itself)
    monkeypatch.setitem(vars(ops), "clip_bce_forward", lambda *a: seen.append(a) or torch.zeros(()))
    p, label, counts = (t.float() for t in R.make_inputs(3, 4, 9))
    cn = counts.numpy().astype(np.int64)
    out = {"clip_sim": p, "label": label.double(), "counts": cn}
    losses.FocalClipBceLoss(1.5, 0.4)(out)
    losses.ClipBceLossFreqWeight(100, 0.5)(out)
    losses.SymmetricClipBceLoss(eps=1e-2)(out)
    losses.OriginSymmetricClipBceLoss(0.7, 1.3, 1e-2)(out)
    losses.PriorAdjustedClipBceLoss(1000, 0.5)(out)
    losses.PriorAdjustedClipBceLoss(torch.full((1, 4), 1000.0, dtype=torch.float64), 1)(dict(out, counts=torch.from_numpy(cn)))
    assert [(a[3], a[4:]) for a in seen] == [(0, (1.5, 0.4, 0.0)), (1, (0.0, 0.0, 0.0)), (2, (1e-2, 0.0, 0.0)),
                                            (3, (0.7, 1.3, math.log(1e-2))), (4, (0.5, 0.0, 0.0)), (4, (1.0, 0.0, 0.0))]
    assert all(a[1].dtype == torch.float32 and torch.equal(a[1], label) for a in seen)
    assert [a[2] is None for a in seen] == [True, False, True, True, False, False]
    w = torch.from_numpy((100 / (100 + cn)) ** 0.5).float()
    assert seen[1][2].dtype == torch.float32 and torch.equal(seen[1][2], w)
    assert torch.equal(seen[4][2], torch.from_numpy(cn / 1000).float()) and torch.equal(seen[5][2], seen[4][2])


class _Stub(torch.nn.Module):
    def forward(self, output):
        return output["u"] * 2.0


def test_vector_quantize_loss():
    from texttoaudiogrounding_amd.losses import VectorQuantizeLoss
    m = VectorQuantizeLoss(_Stub(), 0.25)
    assert isinstance(m.loss_fn, _Stub) and m.vq_weight == 0.25 and dict(m.named_children()) == {"loss_fn": m.loss_fn}
    u, vq = torch.tensor(1.5, requires_grad=True), torch.tensor(4.0, requires_grad=True)
    out = m({"u": u, "vq_loss": vq})
    assert out.item() == 0.25 * 4.0 + 3.0
    out.backward()
    assert (float(u.grad), float(vq.grad)) == (2.0, 0.25)
    sep = m.get_separate_loss({"u": u, "vq_loss": vq})
    assert set(sep) == {"cls_loss", "vq_loss"} and sep["cls_loss"].item() == 3.0 and sep["vq_loss"] is vq
    assert VectorQuantizeLoss(_Stub()).vq_weight == 1.0


def test_symbols_declared_and_arguments_checked():
    from texttoaudiogrounding_amd import dispatch, lib
    header = open(os.path.join(ROOT, "include", "tag_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(tag_clip_bce_[a-z_]+)\s*\(", code))) == sorted(SYMBOLS)
    assert sorted(s for s in lib.declared_symbols() if s.startswith("tag_clip_bce")) == sorted(SYMBOLS)
    src = open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "clip_bce.hip")).read()
    assert int(re.search(r"long ONE_LAUNCH_MAX = (\d+);", src).group(1)) == dispatch.CLIP_BCE_ONE_LAUNCH_MAX
    assert "clip_bce.hip" in open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "Makefile")).read()
    h = lib.load()
    assert h.tag_abi_version() == lib.ABI_VERSION == 3
    L = dispatch.CLIP_BCE_ONE_LAUNCH_MAX
    assert lib.query("tag_clip_bce_ws_bytes", 0) == 0 and lib.query("tag_clip_bce_ws_bytes", -3) == 0
    sizes = [lib.query("tag_clip_bce_ws_bytes", M) for M in (1, L, L + 1, 1 << 33)]
    assert all(s >= 8 and s % 8 == 0 for s in sizes)
    # refused with a message before any launch (no GPU is touched): the pointers below are never dereferenced on the host
    import ctypes
    buf = (ctypes.c_float * 4)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    nan = float("nan")
    bad_fwd = [(a, a, None, 0, 0, 2.0, 0.25, 0.0, a, a), (a, a, None, 4, -1, 2.0, 0.25, 0.0, a, a),
               (a, a, None, 4, 5, 2.0, 0.25, 0.0, a, a), (None, a, None, 4, 0, 2.0, 0.25, 0.0, a, a),
               (a, None, None, 4, 0, 2.0, 0.25, 0.0, a, a), (a, a, None, 4, 0, 2.0, 0.25, 0.0, None, a),
               (a, a, None, 4, 1, 0.0, 0.0, 0.0, a, a), (a, a, None, 4, 4, 1.0, 0.0, 0.0, a, a),
               (a, a, None, 4, 0, nan, 0.25, 0.0, a, a), (a, a, None, 4, 0, 2.0, nan, 0.0, a, a),
               (a, a, None, 4, 3, 1.0, 1.0, nan, a, a), (a, a, None, L + 1, 0, 2.0, 0.25, 0.0, a, None)]
    for args in bad_fwd:
        assert h.tag_clip_bce_forward(*args, None) == TAG_EINVAL and b"argument check failed" in h.tag_last_error(), args
    b = ctypes.cast((ctypes.c_float * 4)(), ctypes.c_void_p)
    bad_bwd = [(a, a, None, 0, 0, 2.0, 0.25, 0.0, a, b), (a, a, None, 4, 7, 2.0, 0.25, 0.0, a, b),
               (None, a, None, 4, 0, 2.0, 0.25, 0.0, a, b), (a, None, None, 4, 0, 2.0, 0.25, 0.0, a, b),
               (a, a, None, 4, 0, 2.0, 0.25, 0.0, None, b), (a, a, None, 4, 0, 2.0, 0.25, 0.0, a, None),
               (a, a, None, 4, 1, 0.0, 0.0, 0.0, a, b), (a, a, None, 4, 4, 1.0, 0.0, 0.0, a, b),
               (a, a, None, 4, 2, nan, 0.0, 0.0, a, b), (a, a, None, 4, 0, 2.0, 0.25, 0.0, a, a)]
    for args in bad_bwd:
        assert h.tag_clip_bce_backward(*args, None) == TAG_EINVAL and b"argument check failed" in h.tag_last_error(), args
