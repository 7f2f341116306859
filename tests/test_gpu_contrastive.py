"""The sentence-level contrastive objectives on the GPU (csrc/contrastive.hip through losses.py): the fixture made from the
imported reference, a sweep over the edge sizes against the fp64 statement of tests/contrastive_ref.py, bit-equal repeats,
torch.library.opcheck, and AudioTextAlignByPhrase driven by WeakSentenceRunner against the fp64 twin.

Tolerance of the sweep and of the fixture, per case and separately for the loss and the gradient (max abs): the kernel's error
against fp64 is at most the larger of 4 x the error of the SAME statement run in fp32 by torch on the CPU (both accumulate the
same n terms, in another order) and 16 * 2^-24 * scale, scale = max(|loss|, 1) for the loss and max |dx_fp64| for the gradient
(a handful of fp32 roundings on a result that is returned in fp32; the fp32 statement is sometimes exact by luck)."""
import numpy as np
import pytest
import torch

from tests import contrastive_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 1025)
MIL_N = (1, 63, 64, 65, 257)
KINDS = ("infonce", "max", "weighted", "random")
# (tau, margin, transposed non-contiguous input, upstream gradient)
CONFIGS = ((0.07, 0.2, False, 1.0), (1.0, 1.0, True, -1.7))
FLOOR = 16 * 2.0 ** -24


def loss_module(kind, cfg):
    from texttoaudiogrounding_amd import losses
    return {"infonce": losses.InfoNceLoss, "max": losses.MaxTripletLoss, "weighted": losses.WeightedTripletLoss,
            "random": losses.RandomTripletLoss, "milnce": losses.MilNceLoss}[kind](cfg)


def run_module(kind, cfg, x32, dev, upstream=1.0, transposed=False, label=None, seed=None):
    """The loss module on the device -> (loss, dx) on the host.  transposed: the module sees a non-contiguous view."""
    xd = (x32.t().contiguous().to(dev).t() if transposed else x32.to(dev)).requires_grad_(True)
    assert xd.is_contiguous() != transposed or xd.shape[0] == 1
    out = {"clip_sim": xd, "label": label} if kind == "milnce" else {"sim": xd}
    if seed is not None:
        np.random.seed(seed)
    loss = loss_module(kind, cfg)(out)
    (loss * upstream).backward()
    return loss.detach().cpu(), xd.grad.cpu()


def sweep_input(kind, n, ci, margin):
    """fp32 input (raised diagonals) and the random mode's draws, redrawn until the precondition holds -> (x, seed, s, a, ok)."""
    for attempt in range(50):
        seed = 1000 * n + 10 * ci + 100000 * attempt
        x = R.raised_diagonal_input(n, seed, torch.float32)
        np.random.seed(seed)
        s_index, a_index = np.random.randint(n, size=n), np.random.randint(n, size=n)
        if kind == "infonce":
            ok = True
        elif kind == "random":
            ok = R.random_precondition(x, margin, s_index, a_index)
        else:
            ok = R.triplet_precondition(x, margin, weighted=kind == "weighted")
        if ok:
            break
    return x, seed, s_index, a_index, ok


def check(tag, fn, x32, got_loss, got_dx, upstream=1.0, ref32=None):
    """fn: the statement as a function of the input.  ref32: (loss, dx) of an fp32 run made elsewhere (the fixture)."""
    loss64, dx64 = R.loss_and_grad(fn, x32.double(), upstream=upstream)
    loss32, dx32 = ref32 if ref32 is not None else R.loss_and_grad(fn, x32, upstream=upstream)
    ref_l, ref_d = abs(float(loss32) - float(loss64)), (dx32.double() - dx64).abs().max().item()
    err_l, err_d = abs(float(got_loss) - float(loss64)), (got_dx.double() - dx64).abs().max().item()
    tol_l = max(4 * ref_l, FLOOR * max(abs(float(loss64)), 1.0))
    tol_d = max(4 * ref_d, FLOOR * dx64.abs().max().item())
    print(f"{tag}: loss {float(loss64):.6g} err {err_l:.2e} (fp32 statement {ref_l:.2e}, bound {tol_l:.2e}); "
          f"dx max {dx64.abs().max().item():.3g} err {err_d:.2e} (fp32 statement {ref_d:.2e}, bound {tol_d:.2e})")
    assert torch.isfinite(got_dx).all() and got_dx.shape == x32.shape and got_loss.shape == ()
    assert err_l <= tol_l, (tag, "loss", err_l, tol_l)
    assert err_d <= tol_d, (tag, "dx", err_d, tol_d)
    return err_l, err_d


def test_golden_cases(dev, golden_dir):
    fx = np.load(f"{golden_dir}/contrastive.npz")
    for name in (str(n) for n in fx["names"]):
        kind = name.split("_")[0]
        cfg = float(fx[f"{name}/cfg"])
        extra = {k: torch.from_numpy(fx[f"{name}/{k}"]) for k in ("label", "s_index", "a_index") if f"{name}/{k}" in fx}
        x32 = torch.from_numpy(fx[f"{name}/x"]).float()
        label = extra["label"].float() if kind == "milnce" else None
        seed = int(fx[f"{name}/seed"]) if kind == "random" else None
        loss, dx = run_module(kind, cfg, x32, dev, label=label, seed=seed)
        # the fixture's input is fp64 and its fp32 run rounded it as the kernel's caller does: both errors are against that fp64 run
        loss64, dx64 = torch.from_numpy(fx[f"{name}/loss_f64"]), torch.from_numpy(fx[f"{name}/dx_f64"])
        ref_l = abs(float(fx[f"{name}/loss_f32"]) - float(loss64))
        ref_d = np.abs(fx[f"{name}/dx_f32"].astype(np.float64) - fx[f"{name}/dx_f64"]).max()
        err_l, err_d = abs(float(loss) - float(loss64)), (dx.double() - dx64).abs().max().item()
        tol_l = max(4 * ref_l, FLOOR * max(abs(float(loss64)), 1.0))
        tol_d = max(4 * ref_d, FLOOR * dx64.abs().max().item())
        print(f"golden {name}: loss err {err_l:.2e} (reference fp32 {ref_l:.2e}); dx err {err_d:.2e} (reference fp32 {ref_d:.2e})")
        assert torch.isfinite(dx).all()
        assert err_l <= tol_l and err_d <= tol_d, (name, err_l, tol_l, err_d, tol_d)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_sweep(dev, kind, n):
    for ci, (tau, margin, transposed, upstream) in enumerate(CONFIGS):
        cfg = tau if kind == "infonce" else margin
        x, seed, s_index, a_index, ok = sweep_input(kind, n, ci, margin)
        assert ok, "input precondition (not the kernel)"
        fn = R.statement(kind, cfg, s_index=s_index, a_index=a_index)
        sd = seed if kind == "random" else None
        loss, dx = run_module(kind, cfg, x, dev, upstream, transposed, seed=sd)
        check(f"{kind} n={n} cfg={cfg}{' transposed' if transposed else ''}", fn, x, loss, dx, upstream)
        loss2, dx2 = run_module(kind, cfg, x, dev, upstream, transposed, seed=sd)
        assert torch.equal(loss, loss2) and torch.equal(dx, dx2), "two runs on the same input differ"
        if n == 1:
            assert float(loss) == 0 and not dx.any()


@pytest.mark.parametrize("N", MIL_N)
def test_milnce_sweep(dev, N):
    B = 3
    for ci, (tau, _, transposed, upstream) in enumerate(CONFIGS):
        g = torch.Generator().manual_seed(77 * N + ci)
        c = torch.rand(N, B, generator=g).t() if transposed else torch.rand(B, N, generator=g)
        label = (torch.rand(B, N, generator=g) < 0.4).float()
        cd = c.to(dev).requires_grad_(True)
        from texttoaudiogrounding_amd.losses import MilNceLoss
        res = []
        for _ in range(2):
            cd.grad = None
            loss = MilNceLoss(tau)({"clip_sim": cd, "label": label})
            (loss * upstream).backward()
            res.append((loss.detach().cpu(), cd.grad.cpu()))
        check(f"milnce B={B} N={N} tau={tau}", R.statement("milnce", tau, label=label), c.contiguous(), *res[0], upstream)
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "two runs on the same input differ"


def test_milnce_many_rows(dev):
    """More rows than one launch folds (B > 128): the two-launch forward, one wave per row."""
    from texttoaudiogrounding_amd.losses import MilNceLoss
    g = torch.Generator().manual_seed(5)
    c, label = torch.rand(131, 5, generator=g), (torch.rand(131, 5, generator=g) < 0.4).float()
    cd = c.to(dev).requires_grad_(True)
    loss = MilNceLoss(0.5)({"clip_sim": cd, "label": label.to(dev)})
    loss.backward()
    check("milnce B=131 N=5", R.statement("milnce", 0.5, label=label), c, loss.detach().cpu(), cd.grad.cpu())


def test_infonce_wide_range_is_finite(dev):
    g = torch.Generator().manual_seed(3)
    for n in (9, 129):
        x = torch.randn(n, n, generator=g) * 40
        loss, dx = run_module("infonce", 0.07, x, dev)
        assert torch.isfinite(loss) and torch.isfinite(dx).all()
        check(f"infonce wide n={n}", R.statement("infonce", 0.07), x, loss, dx)


def test_backward_without_the_saved_workspace(dev, monkeypatch):
    """A traced backward has no workspace handed over: the backward operator refills it with one more forward launch and gives
    the same bits.  Under eager autograd the workspace of the forward IS handed over: nothing is refilled."""
    from texttoaudiogrounding_amd import dispatch
    refills = []
    for name in ("infonce_forward", "triplet_forward", "milnce_forward"):
        def counted(*args, _fn=getattr(dispatch, name), _name=name):
            refills.append(_name)
            return _fn(*args)
        monkeypatch.setattr(dispatch, name, counted)          # the backward wrappers look the forward up in their own module
    g = torch.Generator().manual_seed(11)
    x = torch.rand(65, 65, generator=g).to(dev)
    one = torch.ones((), device=dev)
    for fwd, bwd in ((lambda t: torch.ops.tag.infonce(t, 0.07), lambda: torch.ops.tag.infonce_backward(x, 0.07, one, None)),
                     (lambda t: torch.ops.tag.triplet(t, 1, 0.2, None, None),
                      lambda: torch.ops.tag.triplet_backward(x, 1, 0.2, None, None, one, None))):
        xr = x.clone().requires_grad_(True)
        fwd(xr).backward()
        assert refills == [], "the eager backward re-ran the forward"
        assert torch.equal(xr.grad, bwd()) and len(refills) == 1
        refills.clear()
    c, lab = torch.rand(4, 9, generator=g).to(dev), (torch.rand(4, 9, generator=g) < 0.5).float().to(dev)
    cr = c.clone().requires_grad_(True)
    torch.ops.tag.milnce(cr, lab, 0.3).backward()
    assert refills == [], "the eager backward re-ran the forward"
    assert torch.equal(cr.grad, torch.ops.tag.milnce_backward(c, lab, 0.3, one, None)) and refills == ["milnce_forward"]


def test_opcheck(dev):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(7, 7, generator=g).to(dev).requires_grad_(True)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.tag.infonce.default, (x, 0.07), test_utils=utils)
    torch.library.opcheck(torch.ops.tag.triplet.default, (x, 0, 0.2, None, None), test_utils=utils)
    idx = torch.tensor([1, 0, 3, 3, 6, 2, 5], dtype=torch.int32, device=dev)
    torch.library.opcheck(torch.ops.tag.triplet.default, (x, 2, 0.2, idx, idx.flip(0)), test_utils=utils)


@pytest.fixture(scope="module")
def align_setup():
    from oracle import tag_oracle as O
    st = O.init_state(seed=19, logit_gain=60.0)
    batch = O.synthetic_batch(3, 48000, seed=5, ragged=True)
    g = torch.Generator().manual_seed(1)
    nums, L = [2, 1, 3], 4
    phrases = torch.randint(2, 5221, (sum(nums), L), generator=g)
    phrases_len = torch.randint(1, L + 1, (sum(nums),), generator=g)
    for r in range(sum(nums)):
        phrases[r, phrases_len[r]:] = 0
    # the fp64 twin up to the (B,B) matrix: the oracle's pieces as AudioTextAlignByPhrase.forward composes them (eval-mode
    # BatchNorm: well conditioned at B = 3)
    s64 = O.state_to(st, torch.float64, requires_grad=True)
    ao = O.cnn8rnn_forward(s64, batch["waveform"].double(), batch["waveform_len"], training=False)
    seq = O.embedding_agg_mean(s64, phrases, phrases_len)["seq_emb"]
    seq = torch.nn.utils.rnn.pad_sequence(torch.split(seq, nums, dim=0), batch_first=True)
    sim = O.audio_mean_text_mean(O.align_dot_product(ao["embedding"], seq), ao["length"], torch.as_tensor(nums))
    return st, batch, phrases, phrases_len, nums, s64, sim


@pytest.mark.parametrize("kind,cfg", [("infonce", 0.07), ("max", 0.2)])
def test_align_by_phrase_through_weak_sentence_runner(dev, align_setup, kind, cfg):
    from texttoaudiogrounding_amd.models import align, audio_encoder, audio_text_model, sim_pooling, text_encoder
    from texttoaudiogrounding_amd.runner import WeakSentenceRunner
    st, batch, phrases, phrases_len, nums, s64, sim64 = align_setup
    model = audio_text_model.AudioTextAlignByPhrase(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512),
                                                    align.DotProduct(), sim_pooling.AudioMeanTextMean(), 512)
    missing = model.load_state_dict(st, strict=False)
    assert not missing.unexpected_keys and all("melspec" in k for k in missing.missing_keys)
    runner = WeakSentenceRunner(model, loss_fn=loss_module(kind, cfg), device=dev)
    runner.model.eval()

    def fresh():
        return {"waveform": batch["waveform"].clone(), "waveform_len": batch["waveform_len"], "phrases": phrases.clone(),
                "phrases_len": phrases_len.clone(), "phrases_num": list(nums), "text_key": "phrases"}
    loss = runner.forward_backward(fresh())
    names = ("text_encoder.embedding.core.weight", "audio_encoder.fc1.weight", "audio_encoder.rnn.weight_ih_l0")
    for v in s64.values():
        v.grad = None
    lo = R.statement(kind, cfg)(sim64)
    lo.backward(retain_graph=True)
    params = dict(runner.model.named_parameters())
    rel = {k: (params[k].grad.cpu().double() - s64[k].grad).abs().max().item() / (s64[k].grad.abs().max().item() + 1e-30)
           for k in names}
    print(f"AlignByPhrase + {kind}: loss {loss.item():.6f} vs {lo.item():.6f}; gradient rel err", {k: f"{v:.1e}" for k, v in rel.items()})
    assert abs(loss.item() - lo.item()) < 2e-5
    assert all(s64[k].grad.abs().max().item() > 0 for k in names)
    assert all(v < 1e-4 for v in rel.values()), rel
    before = runner.flat.flat.clone()
    loss = runner.train_step(fresh())
    assert torch.isfinite(loss) and torch.isfinite(runner.flat.flat).all()
    assert (runner.flat.flat != before).any()
