"""csrc/gru.hip over its edge shapes and its three recurrence forms, tag_gru_forward / tag_gru_backward called directly through the C
ABI and compared with the fp64 statement of tests/gru_ref.py on the same seeded CPU inputs (gradients from autograd on that
statement).  The case tables, with the form, placement and tail each row reaches, live beside the statement because
tests/test_gru_ref_cpu.py checks on the CPU that every case is conditioned well enough for the bounds used here.

Every output is allocated with NaN in it and a sentinel region behind it that must survive the launch; the scratch has exactly
tag_gru_ws_bytes bytes, zero-filled as the header asks, with a sentinel behind it; the sticky error word is read after every launch
and must be zero; every launch runs twice and must repeat bit for bit; tag_gru_last_form must name the form the table row names.

Tolerances are those of test_gru_forward_backward: max-normalised ``relerr`` of 5e-6 for y and the saved gates, 2e-5 for dgi and dgh;
hprev is exact (the predecessor's y, zero at the first step) and so are the r and z thirds of dgi against dgh.  Every comparison
also evaluates the same statement in fp32 on the CPU and prints that floor.  The rule of assert_crnn_grad_close (bound = max(plain,
4 x max(floor, 1e-6))) is available to gradients named in FLOOR_RULE only; the table is empty: no comparison needed it (worst cases
in docs/experiments_gru_sweep.md).

The launcher's options are read once per process, so the 16-row persistent form (TAG_GRU_TILE=16) and write-through publishing on
the remapped placement (TAG_GRU_XCD=0) run in two child processes, one after the other, at the end of the module.  Tests and ids
with "persistent" in their name run in every process, on whichever persistent form that process selects.  Nothing here launches a
persistent kernel without the cooperative launch, makes an exchange time out or hands over a misaligned pointer."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import gru_ref as R

pytestmark = pytest.mark.gpu

D64 = torch.float64
NAN = float("nan")
SENTINEL, GUARD = 12345.0, 256
TILE16 = os.environ.get("TAG_GRU_TILE") == "16"
XCD_OFF = os.environ.get("TAG_GRU_XCD") == "0"
# name of a comparison -> why its arithmetic is ill-conditioned at that shape.  Gradients only, at most 5 % of the comparisons.
FLOOR_RULE = {}


@pytest.fixture(scope="module")
def ops(dev):
    from texttoaudiogrounding_amd import ops as _ops
    return _ops


def form_here(form):
    """the persistent form this process runs for a table row that names one"""
    if form == R.STEP:
        return form
    return R.P16 if TILE16 else R.P4


def close(name, got, ref64, ref32, bound):
    got, ref64, ref32 = (torch.as_tensor(v).detach().double().cpu() for v in (got, ref64, ref32))
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    err, floor = R.relerr(got, ref64), R.relerr(ref32, ref64)
    if name in FLOOR_RULE:
        assert bound == R.GRAD and name.endswith(("dgi", "dgh")), name
        bound = max(bound, 4.0 * max(floor, 1e-6))
    print(f"  {name:72s} err {err:.2e}  fp32 floor {floor:.2e}  bound {bound:.2e}")
    assert err <= bound, (name, err, floor, bound)


class Out:
    """an output the kernel must fill completely and must not overrun: NaN inside, a sentinel region behind it that is at least one
    batch row long (row b = B of a partly filled tile is what a wrong mask writes, and it starts right behind the output)"""

    def __init__(self, dev, *shape, fill=NAN):
        self.n = int(math.prod(shape))
        self.buf = torch.full((self.n + max(GUARD, self.n // shape[0]),), fill, device=dev, dtype=torch.float32)
        self.buf[self.n:] = SENTINEL
        self.t = self.buf[:self.n].view(*shape)

    def ptr(self):
        return self.buf.data_ptr()

    def done(self, filled=True):
        """guard intact; returns the output on the CPU (filled=False: the launch was refused, every element is still NaN; None: NaN is
        allowed by the case, the caller looks)"""
        assert (self.buf[self.n:] == SENTINEL).all(), "the kernel wrote behind its output"
        t = self.t.cpu()
        if filled is not None:
            assert (not torch.isnan(t).any()) if filled else torch.isnan(t).all()
        return t


class Scratch(Out):
    """exactly tag_gru_ws_bytes bytes, zero-filled once by the caller as include/tag_hip.h asks, a sentinel behind them"""

    def __init__(self, ops, dev, B, T, H):
        self.nbytes = ops.query("tag_gru_ws_bytes", B, T, H)
        assert self.nbytes % 256 == 0 and self.nbytes > 256
        super().__init__(dev, self.nbytes // 4, fill=0.0)
        self.off_x = (6 * H * H * 4 + 255) // 256 * 256          # the exchange granules lie between the transposed weights ...
        self.off_err = self.nbytes - 256                         # ... and the sticky error word

    def check(self):
        """after a launch: nothing behind the scratch, no bounded spin ran out"""
        assert (self.buf[self.n:] == SENTINEL).all(), "the kernel wrote behind its scratch"
        assert int(self.t.view(torch.int32)[self.off_err // 4].item()) == 0, "a persistent kernel timed out on its exchange"

    def poison_exchange(self, lo=None):
        """every granule between lo (default: the exchange region) and the error word: epoch tag 1, 2 or 3, value 1e30"""
        w = self.t.view(torch.int32)[(self.off_x if lo is None else lo) // 4:self.off_err // 4]
        i = torch.arange(w.numel() // 2, device=w.device, dtype=torch.int32)
        w[0::2] = torch.tensor([1e30]).view(torch.int32).item()
        w[1::2] = 1 + i % 3


def forward(ops, dev, d, B, T, H, ws=None, gates=True, filled=True, form=None):
    """one tag_gru_forward on device inputs d = (gi, w_hh, b_hh, ...) -> (y Out, gates Out or None)"""
    ws = ws or Scratch(ops, dev, B, T, H)
    y, g = Out(dev, B, T, 2 * H), (Out(dev, B, T, 2, 4 * H) if gates else None)
    ops.call("tag_gru_forward", ops.ptr(d[0]), ops.ptr(d[1]), ops.ptr(d[2]), y.ptr(), g.ptr() if gates else None, ws.ptr(), B, T, H)
    torch.cuda.synchronize()
    ws.check()
    if form is not None:
        assert ops.query("tag_gru_last_form", 0) == form, (ops.query("tag_gru_last_form", 0), form)
    y.done(filled)
    if gates:
        g.done(filled)
    return y, g


def backward(ops, dev, d, y, g, B, T, H, scratch=None, filled=True, form=None):
    """one tag_gru_backward on the outputs of ``forward`` -> (dgi, dgh, hprev) on the CPU"""
    scratch = scratch or Scratch(ops, dev, B, T, H)
    outs = [Out(dev, B, T, 2, 3 * H), Out(dev, B, T, 2, 3 * H), Out(dev, B, T, 2, H)]
    ops.call("tag_gru_backward", ops.ptr(d[3]), y.ptr(), g.ptr(), ops.ptr(d[1]), *(o.ptr() for o in outs), scratch.ptr(), B, T, H)
    torch.cuda.synchronize()
    scratch.check()
    if form is not None:
        assert ops.query("tag_gru_last_form", 1) == form, (ops.query("tag_gru_last_form", 1), form)
    return [o.done(filled) for o in outs]


def run(ops, dev, inputs, H, form=None, with_backward=True, filled=True, ws=None, scratch=None, twice=True):
    """forward and backward on CPU inputs, each twice on fresh outputs (bit-equal) -> dict of CPU tensors"""
    B, T = inputs[0].shape[:2]
    d = [t.to(dev).contiguous() for t in inputs]
    y, g = forward(ops, dev, d, B, T, H, ws=ws, filled=filled, form=form)
    got = {"y": y.t.cpu(), "gates": g.t.cpu()}
    if twice:
        y2, g2 = forward(ops, dev, d, B, T, H, filled=filled, form=form)
        assert torch.equal(y2.t.cpu().view(torch.int32), got["y"].view(torch.int32)), "forward does not repeat"
        assert torch.equal(g2.t.cpu().view(torch.int32), got["gates"].view(torch.int32)), "forward does not repeat"
    if with_backward:
        b1 = backward(ops, dev, d, y, g, B, T, H, scratch=scratch, filled=filled, form=form)
        if twice:
            for a, b in zip(b1, backward(ops, dev, d, y, g, B, T, H, filled=filled, form=form)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "backward does not repeat"
        got.update(zip(("dgi", "dgh", "hprev"), b1))
    return got


def same(a, b, names=None, rows=None):
    for n in names or a:
        x, y = (a[n], b[n]) if rows is None else (a[n][rows], b[n][rows])
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), n


@functools.lru_cache(maxsize=None)
def reference(B, T, H, sat=False):
    """inputs, fp64 statement and fp32 floor of a table case: computed once, shared, never written to"""
    inputs = R.case_inputs(B, T, H, sat)
    return inputs, R.gru_ref(*inputs, D64), R.gru_ref(*inputs, torch.float32)


def exact_relations(got, B, T, H):
    """hprev is the predecessor's y bit for bit and zero at the first step; dgi and dgh share their r and z thirds"""
    y = got["y"].view(B, T, 2, H)
    hp = got["hprev"]
    assert torch.equal(hp[:, 1:, 0], y[:, :-1, 0]) and torch.equal(hp[:, :-1, 1], y[:, 1:, 1])
    assert (hp[:, 0, 0] == 0).all() and (hp[:, -1, 1] == 0).all()
    assert torch.equal(got["dgi"][..., :2 * H].contiguous().view(torch.int32), got["dgh"][..., :2 * H].contiguous().view(torch.int32))


def check_case(ops, dev, case, sat=False, with_backward=True):
    B, T, H, form, what = case
    form = form_here(form)
    inputs, r64, r32 = reference(B, T, H, sat)
    tag = f"({B},{T},{H}){' sat' if sat else ''} form {form}"
    print(f"{tag}: {what}")
    got = run(ops, dev, inputs, H, form=form, with_backward=with_backward)
    for n in ("y", "gates") + (("dgi", "dgh") if with_backward else ()):
        close(f"{tag} {n}", got[n], r64[n], r32[n], R.FWD if n in ("y", "gates") else R.GRAD)
    if with_backward:
        exact_relations(got, B, T, H)
    return got, r64


def ids(cases):
    return [f"{B}x{T}x{H}" for B, T, H, _, _ in cases]


# ------------------------------------------------------------------------------------------------ 1. the forms against fp64
@pytest.mark.parametrize("case", R.P4_CASES, ids=ids(R.P4_CASES))
def test_p4_cases(ops, dev, case):
    check_case(ops, dev, case)


def test_p4_long_sequence(ops, dev):
    check_case(ops, dev, R.LONG_CASE)


@pytest.mark.parametrize("case", R.STEP0_CASES, ids=ids(R.STEP0_CASES))
def test_step_runtime_h_cases(ops, dev, case):
    check_case(ops, dev, case)


@pytest.mark.parametrize("case", R.STEPT_CASES, ids=ids(R.STEPT_CASES))
def test_step_templated_cases(ops, dev, case):
    check_case(ops, dev, case)


@pytest.mark.parametrize("key", ["step", "persistent"])
def test_saturated_update_gates(ops, dev, key):
    case = R.SAT_CASES["step"] if key == "step" else R.SAT_CASES["p16" if TILE16 else "p4"]
    got, r64 = check_case(ops, dev, case, sat=True)
    H = case[2]
    assert R.saturated_share(got["gates"][..., H:2 * H]) > 0.25


def test_occupancy_ladder(ops, dev):
    """H = 256, B rising through the sizes at which the launcher changes form under one occupancy or another.  Which form a B takes is
    the runtime's answer, not asserted; asserted are agreement with fp64 whatever ran, and that a larger B never moves to a form with
    a larger grid (4-row -> 16-row -> per-step)."""
    last = [R.P4, R.P4]
    for B in R.LADDER_B:
        inputs, r64, r32 = reference(B, 2, 256)
        got = run(ops, dev, inputs, 256, twice=False)
        forms = [ops.query("tag_gru_last_form", 0), ops.query("tag_gru_last_form", 1)]
        print(f"ladder H 256 B {B:4d}: 4-row grid {16 * ((B + 3) // 4):5d}, 16-row grid {32 * ((B + 15) // 16):5d} -> forward form "
              f"{forms[0]}, backward form {forms[1]}")
        for n in ("y", "gates", "dgi", "dgh"):
            close(f"ladder ({B},2,256) forms {forms} {n}", got[n], r64[n], r32[n], R.FWD if n in ("y", "gates") else R.GRAD)
        exact_relations(got, B, 2, 256)
        for i in range(2):
            assert 1 <= forms[i] <= last[i], (B, forms, last)
        last = forms


# ------------------------------------------------------------------------------------------------ 2. exact properties, per form
# id -> (H, T, form of the table); "persistent" ids run on the process's persistent form, "step" ids on the per-step kernels
EXACT = {"persistent128": (128, 3, R.P4), "persistent256": (256, 4, R.P4), "step64": (64, 5, R.STEP), "step288": (288, 2, R.STEP)}


@pytest.mark.parametrize("key", list(EXACT))
def test_forward_without_gates(ops, dev, key):
    H, T, form = EXACT[key]
    inputs = R.gru_inputs(5, T, H, 11)
    d = [t.to(dev) for t in inputs]
    y, _ = forward(ops, dev, d, 5, T, H, form=form_here(form))
    y0, _ = forward(ops, dev, d, 5, T, H, gates=False, form=form_here(form))
    assert torch.equal(y.t.cpu().view(torch.int32), y0.t.cpu().view(torch.int32))


def test_forward_without_gates_single_step_templated(ops, dev):
    d = [t.to(dev) for t in R.gru_inputs(5, 1, 256, 12)]
    y, _ = forward(ops, dev, d, 5, 1, 256, form=R.STEP)
    y0, _ = forward(ops, dev, d, 5, 1, 256, gates=False, form=R.STEP)
    assert torch.equal(y.t.cpu().view(torch.int32), y0.t.cpu().view(torch.int32))


@pytest.mark.parametrize("key", list(EXACT))
def test_mirror(ops, dev, key):
    """gi reversed in time with the directions' weights and biases swapped gives the mirrored y and gates bit for bit: both
    directions run the same arithmetic"""
    H, T, form = EXACT[key]
    gi, w, b, dy = R.gru_inputs(5, T, H, 13)
    a = run(ops, dev, (gi, w, b, dy), H, form=form_here(form), with_backward=False, twice=False)
    m = run(ops, dev, (gi.flip(1).flip(2).contiguous(), w.flip(0).contiguous(), b.flip(0).contiguous(), dy), H,
            form=form_here(form), with_backward=False, twice=False)
    assert torch.equal(m["y"].view(5, T, 2, H).flip(1).flip(2).contiguous().view(torch.int32), a["y"].view(5, T, 2, H).view(torch.int32))
    assert torch.equal(m["gates"].flip(1).flip(2).contiguous().view(torch.int32), a["gates"].view(torch.int32))


@pytest.mark.parametrize("key", list(EXACT))
def test_rows_are_independent(ops, dev, key):
    """rows 0..4 of a B = 5 run are the same rows of a B = 8 run bit for bit, forward and backward"""
    H, T, form = EXACT[key]
    big = R.gru_inputs(8, T, H, 14)
    small = (big[0][:5].contiguous(), big[1], big[2], big[3][:5].contiguous())
    a = run(ops, dev, small, H, form=form_here(form), twice=False)
    b = run(ops, dev, big, H, form=form_here(form), twice=False)
    same(a, b, rows=slice(0, 5))


@pytest.mark.parametrize("key", list(EXACT))
def test_nan_stays_in_its_row(ops, dev, key):
    """a NaN in one row's gi makes that row NaN and leaves every other row as it was; it is data, not a timeout (error word zero)"""
    H, T, form = EXACT[key]
    gi, w, b, dy = R.gru_inputs(5, T, H, 15)
    clean = run(ops, dev, (gi, w, b, dy), H, form=form_here(form), twice=False)
    bad = gi.clone()
    bad[2, 1, 0, 7] = NAN
    bad[2, T - 1, 1, H + 3] = NAN
    dirty = run(ops, dev, (bad, w, b, dy), H, form=form_here(form), filled=None, twice=False)      # (run checks the error word)
    others = [0, 1, 3, 4]
    same(clean, dirty, rows=others)
    for n in ("y", "gates", "dgi", "dgh"):
        assert torch.isnan(dirty[n][2]).any(), n
    yd = dirty["y"].view(5, T, 2, H)
    assert torch.isnan(yd[2, 1, 0, 7]) and torch.isnan(yd[2, 2:, 0]).all()     # direction 0: unit 7 at t = 1, every unit after it
    assert not torch.isnan(yd[2, 0, 0]).any()                                  # ... and nothing before it


@pytest.mark.parametrize("H", [128, 256], ids=["persistent128", "persistent256"])
def test_scratch_reuse_persistent(ops, dev, H):
    """T = 40, then T = 3, then T = 40 on ONE scratch that is never cleared by the caller (dispatch._gru_ws keeps one scratch per
    (B, H, pass) across T), other inputs each time: the granules the T = 3 launch leaves carry epochs 2 and 3 in the very slots
    steps 2 and 3 of the next launch poll.  Bit-equal to fresh-scratch runs, forward and backward: the launcher clears the exchange."""
    B, form = 13, form_here(R.P4)
    ws, scratch = Scratch(ops, dev, B, 40, H), Scratch(ops, dev, B, 40, H)
    for T, seed in ((40, 21), (3, 22), (40, 23)):
        assert ops.query("tag_gru_ws_bytes", B, T, H) == ws.nbytes
        inputs = R.gru_inputs(B, T, H, seed)
        fresh = run(ops, dev, inputs, H, form=form, twice=False)
        same(fresh, run(ops, dev, inputs, H, form=form, ws=ws, scratch=scratch, twice=False))


@pytest.mark.parametrize("key", list(EXACT))
def test_scratch_poisoned_exchange(ops, dev, key):
    """every granule of the exchange region tagged epoch 1, 2 or 3 and holding 1e30 before the launch (the error word untouched;
    per-step kernels: the whole scratch up to the error word): the results do not change"""
    H, T, form = EXACT[key]
    inputs = R.gru_inputs(5, T, H, 16)
    fresh = run(ops, dev, inputs, H, form=form_here(form), twice=False)
    ws, scratch = Scratch(ops, dev, 5, T, H), Scratch(ops, dev, 5, T, H)
    for s in (ws, scratch):
        s.poison_exchange(lo=0 if form == R.STEP else None)
    same(fresh, run(ops, dev, inputs, H, form=form_here(form), ws=ws, scratch=scratch, twice=False))


# ------------------------------------------------------------------------------------------------ 3. the gate functions
GATE_FORMS = {"persistent128": (4, 2, 128, R.P4), "persistent256": (4, 2, 256, R.P4), "step96": (16, 2, 96, R.STEP)}


@pytest.mark.parametrize("key", list(GATE_FORMS))
def test_gate_functions(ops, dev, key):
    """w_hh = 0, b_hh = 0: the saved gates are sigmoid(gi_r), sigmoid(gi_z), tanh(gi_n) of the inputs.  The 4-row forward kernel uses
    the hardware forms (v_exp_f32, v_rcp_f32, an odd series below |x| = 0.2), every other kernel the library's expf / tanhf: all within
    3e-7 absolute of fp64 (the kernel comment's claim), exact at +-inf, finite everywhere.  The worst relative error over
    |ref| >= 1e-30 is printed; for |x| <= 20 it must stay below gru_ref.GATE_REL = 2e-6.  (The comment used to claim 4e-7 relative;
    measured on an MI355X: 9.2e-7 for the sigmoid at x = -44, 7.7e-7 within |x| <= 20, 6.2e-7 for tanh next to the series switch.)"""
    B, T, H, form = GATE_FORMS[key]
    form = form_here(form)
    gi, w, b, col = R.gate_case(B, T, H)
    d = [t.to(dev) for t in (gi, w, b)]
    _, g = forward(ops, dev, d, B, T, H, form=form)
    g = g.t.cpu()
    x = col.double()
    kind = "hardware gates" if form == R.P4 else "libm gates"
    for name, got, ref in (("sigmoid (r)", g[..., :H], torch.sigmoid(x)), ("sigmoid (z)", g[..., H:2 * H], torch.sigmoid(x)),
                           ("tanh (n)", g[..., 2 * H:3 * H], torch.tanh(x))):
        assert torch.isfinite(got).all(), name
        e = (got.double() - ref).abs()
        big = ref.abs() >= 1e-30
        rel = (e[big] / ref[big].abs())
        central = big & (x.abs() <= 20)
        relc = (e[central] / ref[central].abs())
        i, j = int(e.argmax()), int(rel.argmax())
        print(f"  gates form {form} H {H} ({kind}) {name:12s} worst abs {e.max().item():.3e} at x = {x.flatten()[i].item():+.8g}; worst rel "
              f"{rel.max().item():.3e} at x = {x[big][j].item():+.8g}; worst rel over |x| <= 20: {relc.max().item():.3e}")
        assert e.max().item() <= R.GATE_ABS, (name, e.max().item())
        assert relc.max().item() <= R.GATE_REL, (name, relc.max().item())
        inf = torch.isinf(x)
        assert torch.equal(got[inf].double(), ref[inf]), name                  # exactly 0 / 1 / +-1
    assert (g[..., 3 * H:] == 0).all()                                          # gh_n = 0: zero weights, zero bias


# ------------------------------------------------------------------------------------------------ 4. refused calls
def _dummies(dev, B, T, H):
    B, T, H = max(B, 1), max(T, 1), max(H, 32)
    z = torch.zeros(B * T * 2 * 4 * H + 6 * H * H + 64, device=dev)
    return z, [Out(dev, B, T, 2 * H), Out(dev, B, T, 2, 4 * H)], [Out(dev, B, T, 2, 3 * H), Out(dev, B, T, 2, 3 * H), Out(dev, B, T, 2, H)], \
        Out(dev, 6 * H * H + 16 * B * H * H + 64)


def _refused(ops, name, *args):
    with pytest.raises(RuntimeError, match="argument check failed"):          # (the text of tag_last_error)
        ops.call(name, *args)
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,T,H", [(0, 3, 32), (3, 0, 32), (3, 3, 0), (3, 3, 8), (3, 3, 24), (0, 3, 256), (3, 0, 128)])
def test_refused_shapes_leave_the_outputs_untouched(ops, dev, B, T, H):
    z, fo, bo, ws = _dummies(dev, B, T, H)
    _refused(ops, "tag_gru_forward", ops.ptr(z), ops.ptr(z), ops.ptr(z), fo[0].ptr(), fo[1].ptr(), ws.ptr(), B, T, H)
    _refused(ops, "tag_gru_backward", ops.ptr(z), ops.ptr(z), ops.ptr(z), ops.ptr(z), *(o.ptr() for o in bo), ws.ptr(), B, T, H)
    for o in fo + bo + [ws]:
        o.done(filled=False)


@pytest.mark.parametrize("H", [64, 256])
def test_refused_null_pointers_leave_the_outputs_untouched(ops, dev, H):
    B, T = 3, 3
    z, fo, bo, ws = _dummies(dev, B, T, H)
    fargs = [ops.ptr(z), ops.ptr(z), ops.ptr(z), fo[0].ptr(), fo[1].ptr(), ws.ptr()]
    for i in (0, 1, 2, 3, 5):                                                   # gates (4) may be NULL
        _refused(ops, "tag_gru_forward", *[None if k == i else a for k, a in enumerate(fargs)], B, T, H)
    bargs = [ops.ptr(z)] * 4 + [o.ptr() for o in bo] + [ws.ptr()]
    for i in range(8):
        _refused(ops, "tag_gru_backward", *[None if k == i else a for k, a in enumerate(bargs)], B, T, H)
    for o in fo + bo + [ws]:
        o.done(filled=False)


@pytest.mark.parametrize("case", R.FWD_ONLY_CASES, ids=ids(R.FWD_ONLY_CASES))
def test_hidden_sizes_forward_takes_and_backward_refuses(ops, dev, case):
    """H = 16 and H = 48: forward runs (H % 16 == 0) and agrees with fp64; backward needs (3H) % 32 == 0 as well and refuses, its
    outputs untouched.  Stated in include/tag_hip.h: a model of such a width runs in inference and cannot be trained."""
    B, T, H, form, _ = case
    check_case(ops, dev, case, with_backward=False)
    z, fo, bo, ws = _dummies(dev, B, T, H)
    _refused(ops, "tag_gru_backward", ops.ptr(z), ops.ptr(z), ops.ptr(z), ops.ptr(z), *(o.ptr() for o in bo), ws.ptr(), B, T, H)
    for o in bo + [ws]:
        o.done(filled=False)


# ------------------------------------------------------------------------------------------------ 5. the other processes' cases
@pytest.mark.parametrize("case", R.P16_CASES, ids=ids(R.P16_CASES))
def test_tile16_cases(ops, dev, case):
    """the 16-row persistent form in the TAG_GRU_TILE=16 child (the 4-row form at the same shapes in a default process)"""
    check_case(ops, dev, case)


@pytest.mark.parametrize("case", R.XCD_CASES, ids=ids(R.XCD_CASES))
def test_xcd_cases(ops, dev, case):
    """the remapped placement; in the TAG_GRU_XCD=0 child every group publishes write-through"""
    check_case(ops, dev, case)


def test_xcd_option_of_this_process(ops, dev):
    """the child started with TAG_GRU_XCD=0 really has L2-resident publishing off (the query returns the previous setting; it is only
    asked there, because it also switches the setting off)"""
    if XCD_OFF:
        assert ops.query("tag_gru_disable_xcd_fast") == 0


def _child(env, select):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", select],
                           env=dict(os.environ, **env), cwd=root, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the child process did not end within its time limit:\n{str(e.stdout)[-3000:]}\n{str(e.stderr)[-2000:]}")
    print(r.stdout)                                             # (the child's comparison lines, for a run with -s)
    assert r.returncode >= 0, f"the child process ended on signal {-r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


def test_zz_child_process_tile16(dev):
    """TAG_GRU_TILE=16: the 16-row persistent kernels on their table, their saturated case, scratch reuse and every exact property
    (tag_gru_last_form must report 2 in each)"""
    if TILE16 or XCD_OFF:
        return                                                  # (a child selects no child test; nothing to start from here)
    _child({"TAG_GRU_TILE": "16"}, "(tile16 or persistent) and not child_process")


def test_zz_child_process_xcd_off(dev):
    """TAG_GRU_XCD=0: the remapped 4-row placement with write-through publishing"""
    if TILE16 or XCD_OFF:
        return
    _child({"TAG_GRU_XCD": "0"}, "(xcd or persistent) and not child_process")
