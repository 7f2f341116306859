"""CPU: SpecAugment's stripe draw (models/augmentation.py) against the torchlibrosa twin and the reference fixtures, the mixup host
helpers against the reference, the host-side refusals of Cnn8Rnn's augmentation inputs, and the augmentation kernels' build."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import torchlibrosa_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("cnn8rnn_specaug_train", "cnn8rnn_specaug_mixup_train")


def twin_stripes(seed, B, T, F, widths):
    """The stripes torchlibrosa's SpecAugmentation draws on a (B, 1, T, F) input after torch.manual_seed(seed)."""
    twin = torchlibrosa_twin.SpecAugmentation(*widths).train()
    torch.manual_seed(seed)
    twin(torch.zeros(B, 1, T, F))
    return twin.table(B)


@pytest.mark.parametrize("seed,B,T,F,widths", [
    (0, 2, 151, 64, (64, 2, 8, 2)),          # the reference's settings (models/audio_encoder.py:126-131)
    (1, 5, 1001, 64, (64, 2, 8, 2)),
    (2, 3, 40, 16, (1, 3, 1, 1)),            # drop_width 1: every width is 0
    (3, 4, 65, 64, (64, 1, 64, 4)),          # widths up to T - 1 / F - 1
    (4, 2, 100, 64, (10, 0, 8, 3)),          # no time stripes
])
def test_draw_matches_torchlibrosa_twin(seed, B, T, F, widths):
    from texttoaudiogrounding_amd.models.augmentation import SpecAugmentation
    want = twin_stripes(seed, B, T, F, widths)
    sa = SpecAugmentation(*widths)
    torch.manual_seed(seed)
    got = sa.draw(B, T, F)
    assert got.dtype == torch.int32 and got.shape == (B, widths[1] + widths[3], 2)
    assert torch.equal(got, want)
    # the generator advanced exactly as far as the twin's
    torch.manual_seed(seed)
    sa.draw(B, T, F)
    a = torch.rand(3)
    torch.manual_seed(seed)
    twin_stripes(seed, B, T, F, widths)
    assert torch.equal(a, torch.rand(3))
    assert (got[..., 1] >= 0).all() and (got[..., 0] >= 0).all()
    assert (got[:, :widths[1]].sum(-1) <= T).all() and (got[:, widths[1]:].sum(-1) <= F).all()


def test_draw_raises_like_torchlibrosa_when_no_room():
    """A width that leaves no room (T <= distance): torch.randint raises, in the twin and in the port, with the same type."""
    from texttoaudiogrounding_amd.models.augmentation import SpecAugmentation
    widths, B, T, F = (64, 2, 8, 2), 3, 5, 64
    errs = []
    for fn in (lambda: twin_stripes(11, B, T, F, widths),
               lambda: (torch.manual_seed(11), SpecAugmentation(*widths).draw(B, T, F))):
        with pytest.raises(Exception) as e:
            for s in range(11, 40):                       # some seed draws a distance >= T = 5
                torch.manual_seed(s)
                fn()
        errs.append(type(e.value))
    assert errs[0] is errs[1]


def test_module_has_reference_widths_and_no_state():
    from texttoaudiogrounding_amd.models.audio_encoder import Cnn8Rnn
    m = Cnn8Rnn(32000)
    sa = m.spec_augmenter
    assert (sa.time_dropper.dim, sa.time_dropper.drop_width, sa.time_dropper.stripes_num) == (2, 64, 2)
    assert (sa.freq_dropper.dim, sa.freq_dropper.drop_width, sa.freq_dropper.stripes_num) == (3, 8, 2)
    assert not any("spec_augmenter" in k for k in m.state_dict())


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_stripes_reproduced_from_seed(name):
    """The reference fixtures' stripes (drawn by the reference's Cnn8Rnn through the torchlibrosa twin) come out of the
    module's draw for the fixture's seed, at the encoder's frame count."""
    from texttoaudiogrounding_amd.models.audio_encoder import Cnn8Rnn
    gold = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    m = Cnn8Rnn(32000)
    B = gold["lens"].shape[0]
    frames = 48000 // m.hop_length + 1
    torch.manual_seed(int(gold["seed"]))
    got = m.spec_augmenter.draw(B, frames, 64)
    assert np.array_equal(got.numpy(), gold["stripes"])


def test_mixup_helpers_match_reference(tmp_path):
    """utils.train_util.Mixup / do_mixup against the live reference's (run in a child process: importing the reference
    registers its module names)."""
    sys.path.insert(0, os.path.join(GOLDEN))
    try:
        import ref_import
    finally:
        sys.path.pop(0)
    if not ref_import.available():
        pytest.skip("the reference is not on this machine")
    from texttoaudiogrounding_amd.utils.train_util import Mixup, do_mixup
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 3, 7, generator=g)
    n = torch.randint(1, 300, (6,), generator=g)
    out = tmp_path / "ref.npz"
    code = ("import sys, numpy as np, torch, importlib\n"
            f"sys.path.insert(0, {GOLDEN!r})\n"
            "import ref_import\nref_import.install()\n"
            "TU = importlib.import_module('utils.train_util')\n"
            f"x = torch.from_numpy(np.load({str(tmp_path / 'in.npz')!r})['x'])\n"
            f"n = torch.from_numpy(np.load({str(tmp_path / 'in.npz')!r})['n'])\n"
            "m = TU.Mixup(0.4)\nl8 = m.get_lambda(8)\nl6 = m.get_lambda(6)\nm1 = TU.Mixup(1., random_seed=7).get_lambda(4)\n"
            f"np.savez({str(out)!r}, l8=l8, l6=l6, m1=m1, x=TU.do_mixup(x, l8).numpy(), n=TU.do_mixup(n, l6).numpy())\n")
    np.savez(tmp_path / "in.npz", x=x.numpy(), n=n.numpy())
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.DEVNULL)
    ref = np.load(out)
    m = Mixup(0.4)
    l8, l6 = m.get_lambda(8), m.get_lambda(6)
    assert np.array_equal(l8, ref["l8"]) and np.array_equal(l6, ref["l6"])
    assert np.array_equal(Mixup(1., random_seed=7).get_lambda(4), ref["m1"])
    xm, nm = do_mixup(x, l8), do_mixup(n, l6)
    assert xm.dtype == torch.float32 and nm.dtype == torch.float32 and nm.shape == (3,)
    assert np.array_equal(xm.numpy(), ref["x"]) and np.array_equal(nm.numpy(), ref["n"])


@pytest.mark.parametrize("B,lam", [(3, [0.5, 0.5, 1.0]), (4, [0.5, 0.5]), (4, [[0.5, 0.5], [0.5, 0.5]])])
def test_cnn8rnn_refuses_bad_mixup_before_any_launch(monkeypatch, B, lam):
    """An odd batch or a lambda of the wrong length is a ValueError from the module, raised before the encoder operator (or any
    kernel) is reached -- here on a CPU tensor, which the operator itself would refuse with a RuntimeError."""
    from texttoaudiogrounding_amd import torch_ops
    from texttoaudiogrounding_amd.models.audio_encoder import Cnn8Rnn

    def reached(*a, **k):
        raise AssertionError("the encoder operator was reached")

    monkeypatch.setattr(torch_ops, "run_encoder", reached)
    m = Cnn8Rnn(32000).train()
    d = {"waveform": torch.zeros(B, 16000), "waveform_len": [16000] * B, "specaug": True, "mixup_lambda": lam}
    state = torch.random.get_rng_state()
    with pytest.raises(ValueError, match="mixup"):
        m(d)
    assert torch.equal(state, torch.random.get_rng_state())          # refused before the stripes were drawn


def test_eval_mode_reads_and_ignores_both_keys(monkeypatch):
    """Eval mode: no stripes drawn, no lambda checked, the operator called exactly as without augmentation."""
    from texttoaudiogrounding_amd import torch_ops
    from texttoaudiogrounding_amd.models.audio_encoder import Cnn8Rnn
    seen = []
    monkeypatch.setattr(torch_ops, "run_encoder", lambda op, mod, w, p, *aug: (seen.append(aug), torch.zeros(3, 12, 512))[1])
    m = Cnn8Rnn(32000).eval()
    out = m({"waveform": torch.zeros(3, 16000), "waveform_len": [16000] * 3, "specaug": True, "mixup_lambda": [1.0, 0.0, 2.0]})
    assert seen == [()] and out["length"].dtype == torch.int64 and out["length"].shape == (3,)
    assert m._last_specaug is None


def test_augment_kernels_build_clean_without_scratch(tmp_path):
    """csrc/augment.hip is part of the library build and compiles for gfx950 with the Makefile's flags with no warning; neither
    kernel uses scratch."""
    csrc = os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS = .*\baugment\.hip\b", mk, flags=re.M)
    flags = re.search(r"^CXXFLAGS = (.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", "augment.hip", "-o",
                        str(tmp_path / "augment.o")], cwd=csrc, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr
    report = {}
    for name, scratch in re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, flags=re.S):
        report[name] = int(scratch)
    kernels = {k: v for k, v in report.items() if "augment_fwd_kernel" in k or "augment_bwd_kernel" in k}
    assert len(kernels) == 2, report
    assert all(v == 0 for v in kernels.values()), kernels
