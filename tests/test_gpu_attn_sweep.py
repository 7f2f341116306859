"""csrc/mha.hip, csrc/cross.hip and csrc/text_tower.hip over their edge shapes, every entry point called directly through the C ABI
and compared with the fp64 statement of the same operation in tests/attn_ref.py on the same seeded CPU inputs (gradients from
autograd on those statements; the dropout masks are the kernels' own, exported with tag_dropout_mask and imposed on the reference).
The shape tables, with the instantiation, grid and tail each row reaches, live beside the statements in tests/attn_ref.py because
tests/test_attn_ref_cpu.py checks on the CPU that every case is conditioned well enough for the bounds used here.

Every output is allocated with NaN in it and a sentinel region behind it that must survive the launch; workspaces have exactly the
size the library's query returns (and a sentinel behind that); every backward runs twice and must repeat bit for bit.

Tolerances are the project's, not the kernels': max-normalised ``relerr`` of 2e-6 for forward outputs, 2e-5 for gradients (the
bounds of tests/test_gpu_heads_sweep.py), exact for masks, position ids, determinism and the bit-identity checks.  Every comparison
also evaluates the same statement in fp32 on the CPU and prints that floor.  The rule of assert_crnn_grad_close (bound = max(plain,
4 x max(floor, 1e-6))) is available to gradients named in FLOOR_RULE only; the table is empty: no comparison needed it (worst cases
in docs/experiments_attn_sweep.md)."""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu

FWD, GRAD = R.FWD, R.GRAD
D64 = torch.float64
NAN = float("nan")
SENTINEL, GUARD = 12345.0, 256
# name of a comparison -> why its arithmetic is ill-conditioned at that shape.  Gradients only, at most 5 % of the comparisons.
FLOOR_RULE = {}
FORWARD_NAMES = ("attn", "ctx", "sim", "mu", "rstd", "out")


@pytest.fixture(scope="module")
def ops(dev):
    from texttoaudiogrounding_amd import ops as _ops
    return _ops


def close(name, got, ref64, ref32, bound):
    """got (HIP) against ref64 within ``bound``; floor = the fp32 CPU statement's own distance from ref64.  A reference that is
    zero to fp64 rounding has no scale to normalise by: the same bound then holds for the absolute values (inputs of order one)."""
    got, ref64, ref32 = (torch.as_tensor(v).detach().double().cpu() for v in (got, ref64, ref32))
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    if ref64.abs().max().item() < 1e-12:
        err, floor, how = got.abs().max().item(), ref32.abs().max().item(), "abs (zero reference)"
    else:
        err, floor, how = R.relerr(got, ref64), R.relerr(ref32, ref64), "rel"
    if name in FLOOR_RULE:
        assert bound == GRAD and not name.endswith(FORWARD_NAMES), name
        bound = max(bound, 4.0 * max(floor, 1e-6))
    print(f"  {name:64s} err {err:.2e}  fp32 floor {floor:.2e}  bound {bound:.2e}  {how}")
    assert err <= bound, (name, err, floor, bound)


class Out:
    """an output the kernel must fill completely and must not overrun: NaN inside, a sentinel region behind it"""

    def __init__(self, dev, *shape, dtype=torch.float32, fill=NAN):
        self.n = int(math.prod(shape))
        self.buf = torch.full((self.n + GUARD,), fill, device=dev, dtype=dtype)
        self.buf[self.n:] = SENTINEL
        self.t = self.buf[:self.n].view(*shape)

    def ptr(self):
        return self.buf.data_ptr()

    def done(self, filled=True):
        """guard intact; returns the output on the CPU (filled=False: the launch was refused, every element is still NaN)"""
        assert (self.buf[self.n:] == SENTINEL).all(), "the kernel wrote behind its output"
        t = self.t.cpu()
        if filled is not None:                                  # (None: partly written by contract, the caller looks)
            assert (not torch.isnan(t).any()) if filled else torch.isnan(t).all()
        return t


def workspace(ops, dev, query, *dims):
    """exactly the bytes the library asks for, a sentinel behind them"""
    n = ops.query(query, *dims)
    assert n % 4 == 0 and n > 0
    return Out(dev, n // 4), n


def refused(ops, name, *args):
    with pytest.raises(RuntimeError, match="argument check failed"):
        ops.call(name, *args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 1. attention core
def run_mha(ops, dev, q, k, v, dctx, klen, H, p, seed, forward_only=False):
    """tag_mha_cross_forward / _backward on CPU inputs -> attn, ctx, dq, dk, dv on the CPU.  attn and ctx of a clip with klen 0 are
    NaN by contract, so the forward outputs must be NaN-free on the other clips only."""
    B, T, E = q.shape
    L = k.shape[1]
    qd, kd, vd, gd, ld = (t.to(dev).contiguous() for t in (q, k, v, dctx, klen))
    attn, ctx = Out(dev, B, T, H, L), Out(dev, B, T, E)
    ops.call("tag_mha_cross_forward", ops.ptr(qd), ops.ptr(kd), ops.ptr(vd), ops.ptr(ld), attn.ptr(), ctx.ptr(), B, T, L, E, H,
             float(p), seed)
    live = (klen != 0).to(dev)
    for o in (attn, ctx):
        assert (o.buf[o.n:] == SENTINEL).all(), "the kernel wrote behind its output"
        assert not torch.isnan(o.t[live]).any()
    if forward_only:
        return attn.t.cpu(), ctx.t.cpu()
    nbytes = ops.query("tag_mha_cross_backward_ws_bytes", B, T, L, E)
    assert nbytes == 2 * B * R.cdiv(T, 8) * L * E * 4            # partials per tile of QT = 8 frames (the MFMA path uses fewer)
    runs = []
    for _ in range(2):
        ws, _ = workspace(ops, dev, "tag_mha_cross_backward_ws_bytes", B, T, L, E)
        dq, dk, dv = Out(dev, B, T, E), Out(dev, B, L, E), Out(dev, B, L, E)
        ops.call("tag_mha_cross_backward", ops.ptr(qd), ops.ptr(kd), ops.ptr(vd), attn.ptr(), ops.ptr(gd), ops.ptr(ld), dq.ptr(),
                 dk.ptr(), dv.ptr(), B, T, L, E, H, float(p), seed, ws.ptr())
        assert (ws.buf[ws.n:] == SENTINEL).all(), "the kernel wrote behind its workspace"
        runs.append([o.done() for o in (dq, dk, dv)])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "backward is not deterministic"
    return [attn.t.cpu(), ctx.t.cpu()] + runs[0]


def check_mha(ops, dev, tag, q, k, v, dctx, klen, H, p, seed):
    B, T, E = q.shape
    L = k.shape[1]
    got = run_mha(ops, dev, q, k, v, dctx, klen, H, p, seed)
    keep = ops.dropout_mask(seed, (B, T, H, L), p, dev).cpu() if p > 0 else None
    if keep is not None and keep.numel() >= 64:
        assert 0 < keep.float().mean().item() < 1
    ref = R.mha_ref(q, k, v, dctx, klen, H, keep, p, D64)
    r32 = R.mha_ref(q, k, v, dctx, klen, H, keep, p, torch.float32)
    for b in range(B):                                          # the mask is exact: nothing on a token >= klen
        assert (got[0][b, :, :, int(klen[b]):] == 0).all()
    for i, name in enumerate(("attn", "ctx", "dq", "dk", "dv")):
        close(f"{tag} {name}", got[i], ref[i], r32[i], FWD if i < 2 else GRAD)


@pytest.mark.parametrize("pi", range(len(R.MHA_DROP)), ids=[f"p{p}" for p in R.MHA_DROP])
@pytest.mark.parametrize("si", range(len(R.MHA_SHAPES)), ids=["x".join(map(str, s)) for s in R.MHA_SHAPES])
def test_mha_core_sweep(ops, dev, si, pi):
    (B, T, L, E, H, p), (q, k, v, dctx), klen = R.mha_case(si, pi)
    check_mha(ops, dev, f"mha ({B},{T},{L},{E},{H}) p {p}", q, k, v, dctx, klen, H, p, 900 + si)


def test_mha_core_saturated_scores(ops, dev):
    """scores over +-30 (exact in fp32 by construction, see attn_ref.mha_saturated_inputs): the max subtraction and expf over the
    whole range; <64> / VALU <2,64>, two tiles"""
    B, T, L, E, H = R.SAT_SHAPE
    check_mha(ops, dev, "mha saturated", *R.mha_saturated_inputs(), torch.tensor([L, 17]), H, 0.0, 1)


# (B, T, L, E, H) with L < 32 so that klen > L names tokens the MFMA tile has rows for: <32>, <64>, <128>, and the VALU <4,16>
KLEN_EDGE_SHAPES = [(2, 33, 5, 96, 3), (2, 9, 5, 128, 2), (2, 31, 7, 128, 1), (3, 11, 4, 64, 4)]


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("shape", KLEN_EDGE_SHAPES, ids=["x".join(map(str, s)) for s in KLEN_EDGE_SHAPES])
def test_mha_core_klen_above_L_is_klen_L(ops, dev, shape, p):
    """klen[b] > L masks nothing, as arange(L) >= text_len in the reference: bit-equal to klen[b] = L, forward and backward, on the
    MFMA and on the VALU path.  (The MFMA kernels used to count the tile's rows L .. klen - 1 as tokens with a score of 0.)"""
    B, T, L, E, H = shape
    q, k, v, dctx = R.mha_inputs(B, T, L, E, H, 31)
    exact = run_mha(ops, dev, q, k, v, dctx, torch.tensor([L, 2, L][:B]), H, p, 5)
    above = run_mha(ops, dev, q, k, v, dctx, torch.tensor([L + 1, 2, 4000][:B]), H, p, 5)
    assert (exact[0].sum(-1) - 1).abs().max() < 1e-5 and (above[0].sum(-1) - 1).abs().max() < 1e-5
    for name, a, b in zip(("attn", "ctx", "dq", "dk", "dv"), exact, above):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("shape", KLEN_EDGE_SHAPES, ids=["x".join(map(str, s)) for s in KLEN_EDGE_SHAPES])
def test_mha_core_klen_zero(ops, dev, shape, p):
    """A clip without a valid token: forward is NaN on that clip only (attn; ctx wherever a kept weight enters it, which without
    dropout is everywhere); backward returns exact zeros for that clip's dq, dk, dv (include/tag_hip.h); every other clip is
    bit-equal to a run in which that clip had a valid length."""
    B, T, L, E, H = shape
    q, k, v, dctx = R.mha_inputs(B, T, L, E, H, 32)
    lens = torch.tensor([L, 2, 3][:B])
    valid = run_mha(ops, dev, q, k, v, dctx, lens, H, p, 6)
    lens[1] = 0
    empty = run_mha(ops, dev, q, k, v, dctx, lens, H, p, 6)
    others = [b for b in range(B) if b != 1]
    assert torch.isnan(empty[0][1]).all() and (p > 0 or torch.isnan(empty[1][1]).all())
    if p > 0:                                                   # NaN for every (frame, head) that kept a weight, 0 where all were dropped
        kept = (ops.dropout_mask(6, (B, T, H, L), p, dev).cpu()[1] != 0).any(-1)             # (T, H)
        assert torch.equal(torch.isnan(empty[1][1]).view(T, H, E // H).all(-1), kept)
        assert torch.equal((empty[1][1] == 0).view(T, H, E // H).all(-1), ~kept)
    for name, a, b in zip(("attn", "ctx", "dq", "dk", "dv"), valid, empty):
        assert torch.equal(a[others], b[others]), name
    for name, t in zip(("dq", "dk", "dv"), empty[2:]):
        assert (t[1] == 0).all(), name


def test_mha_core_refusals_leave_the_outputs_untouched(ops, dev):
    """L = 33, E = 1088, E % H != 0, a head of 48, a head of 16 with E = 1024, drop_p = 1: refused before any launch"""
    for (B, T, L, E, H), p in [((1, 3, 33, 64, 4), 0.0), ((1, 3, 4, 1088, 17), 0.0), ((1, 3, 4, 64, 3), 0.0), ((1, 3, 4, 96, 2), 0.0),
                               ((1, 3, 4, 1024, 64), 0.0), ((1, 3, 4, 64, 4), 1.0)]:
        z = torch.zeros(B * max(T, L) * E + 64, device=dev)
        klen = torch.ones(B, dtype=torch.long, device=dev)
        attn, ctx, dq, dk, dv = (Out(dev, n) for n in (B * T * H * L, B * T * E, B * T * E, B * L * E, B * L * E))
        ws = Out(dev, 2 * B * R.cdiv(T, 8) * L * E)
        refused(ops, "tag_mha_cross_forward", ops.ptr(z), ops.ptr(z), ops.ptr(z), ops.ptr(klen), attn.ptr(), ctx.ptr(), B, T, L, E, H,
                p, 1)
        refused(ops, "tag_mha_cross_backward", ops.ptr(z), ops.ptr(z), ops.ptr(z), ops.ptr(z), ops.ptr(z), ops.ptr(klen), dq.ptr(),
                dk.ptr(), dv.ptr(), B, T, L, E, H, p, 1, ws.ptr())
        for o in (attn, ctx, dq, dk, dv, ws):
            o.done(filled=False)


def test_mha_core_runs_on_the_path_the_process_asks_for(ops, dev):
    """Which kernels a process launches is told by the workspace: the VALU backward writes partials for cdiv(T, 8) tiles and fills
    the whole workspace, the MFMA backward for cdiv(T, 32) tiles and leaves the rest as it was.  The default process must be on
    the MFMA path and a process started with TAG_MHA_MFMA=0 (the child below) on the VALU path -- otherwise the child would repeat
    the MFMA cases and pass."""
    B, T, L, E, H = 1, 33, 5, 96, 3                             # a head of 32; 5 tiles of 8 frames, 2 tiles of 32
    q, k, v, dctx = (t.to(dev) for t in R.mha_inputs(B, T, L, E, H, 41))
    klen = torch.full((B,), L, dtype=torch.long, device=dev)
    attn, ctx, dq, dk, dv = Out(dev, B, T, H, L), Out(dev, B, T, E), Out(dev, B, T, E), Out(dev, B, L, E), Out(dev, B, L, E)
    ws, _ = workspace(ops, dev, "tag_mha_cross_backward_ws_bytes", B, T, L, E)
    ops.call("tag_mha_cross_forward", ops.ptr(q), ops.ptr(k), ops.ptr(v), ops.ptr(klen), attn.ptr(), ctx.ptr(), B, T, L, E, H, 0.0, 1)
    ops.call("tag_mha_cross_backward", ops.ptr(q), ops.ptr(k), ops.ptr(v), attn.ptr(), ops.ptr(dctx), ops.ptr(klen), dq.ptr(),
             dk.ptr(), dv.ptr(), B, T, L, E, H, 0.0, 1, ws.ptr())
    written = int((~torch.isnan(ws.done(filled=None))).sum())
    valu = os.environ.get("TAG_MHA_MFMA") == "0"
    assert written == 2 * B * (5 if valu else 2) * L * E, (written, "VALU" if valu else "MFMA")


def test_mha_core_valu_kernels_in_child_process(dev):
    """The mha_mfma option is read once per process, so the VALU kernels at the head sizes the MFMA path takes (every HL 32 and HL 64
    instantiation of MHA_DISPATCH, attn_ref.FORCED_SHAPES) run in ONE child process with the option off: the attention-core tests of
    this module, this one excluded; test_mha_core_runs_on_the_path_the_process_asks_for fails there if the option did not arrive."""
    if os.environ.get("TAG_MHA_MFMA") == "0":
        pytest.skip("this process already runs with TAG_MHA_MFMA=0: the VALU kernels run here and the MFMA kernels are NOT covered")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k",
                        "test_mha_core and not child_process"], env=dict(os.environ, TAG_MHA_MFMA="0"), cwd=root, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout and "deselected" in r.stdout


# ------------------------------------------------------------------------------------------------ 2. LayerNorm head
LN_NAMES = ("sim", "mu", "rstd", "dx", "dr", "gw", "gg", "gb", "ds")


def run_resln(ops, dev, x, r, gamma, beta, w, bias, dsim, p, seed):
    rows, E = x.shape
    d = [t.to(dev).contiguous() for t in (x, r, gamma, beta, w, bias, dsim)]
    sim, mu, rstd = Out(dev, rows), Out(dev, rows), Out(dev, rows)
    ops.call("tag_resln_head_forward", *(ops.ptr(t) for t in d[:6]), sim.ptr(), mu.ptr(), rstd.ptr(), rows, E, R.LN_EPS, float(p), seed)
    fwd = [o.done() for o in (sim, mu, rstd)]
    runs = []
    for _ in range(2):
        outs = [Out(dev, rows, E) for _ in range(5)] + [Out(dev, rows)]
        ops.call("tag_resln_head_backward", *(ops.ptr(t) for t in d[:5]), mu.ptr(), rstd.ptr(), sim.ptr(), ops.ptr(d[6]),
                 *(o.ptr() for o in outs), rows, E, float(p), seed)
        runs.append([o.done() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    return dict(zip(LN_NAMES, fwd + runs[0]))


@pytest.mark.parametrize("p", R.LN_DROP)
@pytest.mark.parametrize("E", R.LN_E)
def test_resln_head_sweep(ops, dev, E, p):
    for rows in R.LN_ROWS:
        args = R.resln_inputs(rows, E, 3000 + E + rows)
        got = run_resln(ops, dev, *args, p, 70 + rows)
        keep = ops.dropout_mask(70 + rows, (rows, E), p, dev).cpu() if p > 0 else None
        ref, r32 = R.resln_ref(*args, keep, p, D64), R.resln_ref(*args, keep, p, torch.float32)
        for name in LN_NAMES:
            close(f"resln rows {rows} E {E} p {p} {name}", got[name], ref[name], r32[name], FWD if name in ("sim", "mu", "rstd") else GRAD)
        if E == 1:                                              # the zero-variance row, exactly: xhat = 0 and no gradient reaches z
            assert (got["dx"] == 0).all() and (got["dr"] == 0).all() and (got["gg"] == 0).all()


def test_resln_head_refuses_e_above_1024(ops, dev):
    rows, E = 2, 1025
    z = torch.zeros(rows * E, device=dev)
    outs = [Out(dev, rows * E) for _ in range(5)] + [Out(dev, rows) for _ in range(4)]
    refused(ops, "tag_resln_head_forward", *([ops.ptr(z)] * 6), outs[5].ptr(), outs[6].ptr(), outs[7].ptr(), rows, E, R.LN_EPS, 0.0, 1)
    refused(ops, "tag_resln_head_backward", *([ops.ptr(z)] * 9), *(o.ptr() for o in outs[:5]), outs[8].ptr(), rows, E, 0.0, 1)
    for o in outs:
        o.done(filled=False)


# ------------------------------------------------------------------------------------------------ 3. additive attention
ADD_NAMES = ("attn", "ctx", "daq", "dak", "dkv", "dv")


def run_addattn(ops, dev, aq, ak, v, kv, dctx, qlen, klen, backward=True):
    B, T, Da = aq.shape
    L, Dk = kv.shape[1], kv.shape[2]
    d = [t.to(dev).contiguous() for t in (aq, ak, v, kv, qlen, klen, dctx)]
    attn, ctx = Out(dev, B, T, L), Out(dev, B, T, Dk)
    ops.call("tag_addattn_forward", *(ops.ptr(t) for t in d[:6]), attn.ptr(), ctx.ptr(), B, T, L, Da, Dk)
    fwd = [attn.done(), ctx.done()]
    if not backward:
        return dict(zip(ADD_NAMES, fwd))
    nbytes = ops.query("tag_addattn_backward_ws_bytes", B, T, L, Da, Dk)
    assert nbytes == B * R.cdiv(T, 8) * (L * Da + L * Dk + Da) * 4
    runs = []
    for _ in range(2):
        ws, _ = workspace(ops, dev, "tag_addattn_backward_ws_bytes", B, T, L, Da, Dk)
        outs = [Out(dev, B, T, Da), Out(dev, B, L, Da), Out(dev, B, L, Dk), Out(dev, Da)]
        ops.call("tag_addattn_backward", *(ops.ptr(t) for t in d[:4]), attn.ptr(), ops.ptr(d[6]), ops.ptr(d[4]), ops.ptr(d[5]),
                 *(o.ptr() for o in outs), B, T, L, Da, Dk, ws.ptr())
        assert (ws.buf[ws.n:] == SENTINEL).all(), "the kernel wrote behind its workspace"
        runs.append([o.done() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "backward is not deterministic"
    return dict(zip(ADD_NAMES, fwd + runs[0]))


@pytest.mark.parametrize("si", range(len(R.ADD_SHAPES)), ids=["x".join(map(str, s)) for s in R.ADD_SHAPES])
def test_addattn_sweep(ops, dev, si):
    (B, T, L, Da, Dk), inputs, (qlen, klen) = R.add_case(si)
    got = run_addattn(ops, dev, *inputs, qlen, klen)
    ref, r32 = R.add_ref(*inputs, qlen, klen, D64), R.add_ref(*inputs, qlen, klen, torch.float32)
    for name in ADD_NAMES:
        close(f"addattn ({B},{T},{L},{Da},{Dk}) {name}", got[name], ref[name], r32[name], FWD if name in ("attn", "ctx") else GRAD)
    uniform = torch.full((L,), 1.0, dtype=torch.float32) / L
    for b in range(B):
        kl = int(klen[b])
        ql = min(int(qlen[b]), T) if kl > 0 else 0             # frames from ql on are fully filled rows
        # a fully filled row: exp(0) = 1 for every token, padding included, times 1 / L -- exactly; and no score gradient
        assert torch.equal(got["attn"][b, ql:], uniform.expand(T - ql, L))
        assert (got["daq"][b, ql:] == 0).all()
        assert (got["attn"][b, :ql, kl:] == 0).all() and (got["dak"][b, kl:] == 0).all()


def test_addattn_guards_as_they_are(ops, dev):
    """Forward streams Da and Dk and takes any size: Da = Dk = 1025 is computed, and correctly.  Backward holds a row in registers
    and refuses Da or Dk above 1024 with its outputs untouched.  L = 33 is refused by both."""
    B, T, L, D = 1, 3, 2, 1025
    inputs = R.add_inputs(B, T, L, D, D, 8)
    qlen, klen = torch.tensor([T]), torch.tensor([L])
    got = run_addattn(ops, dev, *inputs, qlen, klen, backward=False)
    ref, r32 = R.add_ref(*inputs, qlen, klen, D64), R.add_ref(*inputs, qlen, klen, torch.float32)
    close("addattn Da = Dk = 1025 attn", got["attn"], ref["attn"], r32["attn"], FWD)
    close("addattn Da = Dk = 1025 ctx", got["ctx"], ref["ctx"], r32["ctx"], FWD)
    z, lens = torch.zeros(4 * 33 * D, device=dev), torch.ones(1, dtype=torch.long, device=dev)
    for (L_, Da, Dk) in [(2, 1025, 64), (2, 64, 1025), (33, 64, 64)]:
        outs = [Out(dev, B * T * Da), Out(dev, B * L_ * Da), Out(dev, B * L_ * Dk), Out(dev, Da), Out(dev, B * (L_ * Da + L_ * Dk + Da))]
        refused(ops, "tag_addattn_backward", *([ops.ptr(z)] * 6), ops.ptr(lens), ops.ptr(lens), *(o.ptr() for o in outs[:4]), B, T, L_,
                Da, Dk, outs[4].ptr())
        for o in outs:
            o.done(filled=False)
    attn, ctx = Out(dev, B * T * 33), Out(dev, B * T * 64)
    refused(ops, "tag_addattn_forward", *([ops.ptr(z)] * 4), ops.ptr(lens), ops.ptr(lens), attn.ptr(), ctx.ptr(), B, T, 33, 64, 64)
    attn.done(filled=False), ctx.done(filled=False)


# ------------------------------------------------------------------------------------------------ 4. gating
@pytest.mark.parametrize("n", R.GATE_N)
def test_mul_and_gate_backward_sweep(ops, dev, n):
    dout, x, g, dx_in = R.gate_inputs(n, n % 1000)
    d = [t.to(dev) for t in (dout, x, g)]
    out = Out(dev, n)
    ops.call("tag_mul", ops.ptr(d[1]), ops.ptr(d[2]), out.ptr(), n)
    prod = out.done()
    close(f"mul n {n}", prod, x.double() * g.double(), x * g, FWD)
    assert torch.equal(prod, x * g)                             # one correctly rounded product per element
    for accumulate in (0, 1):
        dx, dz = Out(dev, n), Out(dev, n)
        if accumulate:
            dx.t.copy_(dx_in)
        ops.call("tag_gate_backward", ops.ptr(d[0]), ops.ptr(d[1]), ops.ptr(d[2]), dx.ptr(), accumulate, dz.ptr(), n)
        r64 = R.gate_backward(dout.double(), x.double(), g.double(), dx_in.double() if accumulate else None)
        r32 = R.gate_backward(dout, x, g, dx_in if accumulate else None)
        close(f"gate_backward n {n} accumulate {accumulate} dx", dx.done(), r64[0], r32[0], GRAD)
        close(f"gate_backward n {n} accumulate {accumulate} dz", dz.done(), r64[1], r32[1], GRAD)


def test_mul_and_gate_backward_refuse_n_0_and_n_6(ops, dev):
    z = torch.zeros(8, device=dev)
    for n in (0, 6):
        a, b = Out(dev, 8), Out(dev, 8)
        refused(ops, "tag_mul", ops.ptr(z), ops.ptr(z), a.ptr(), n)
        refused(ops, "tag_gate_backward", ops.ptr(z), ops.ptr(z), ops.ptr(z), a.ptr(), 0, b.ptr(), n)
        a.done(filled=False), b.done(filled=False)


# ------------------------------------------------------------------------------------------------ 5. row heads
def run_rows(ops, dev, entry, a, b, dsim, kind, l2norm, scale):
    rows, D = a.shape
    ad, bd, gd = (t.to(dev).contiguous() for t in (a, b, dsim))
    mode = (scale,) if entry == "rowdot" else (kind, l2norm, scale)
    fwd, bwd = ("tag_rowdot_sigmoid_forward", "tag_rowdot_sigmoid_backward") if entry == "rowdot" else ("tag_rowpair_forward",
                                                                                                        "tag_rowpair_backward")
    sim = Out(dev, rows)
    ops.call(fwd, ops.ptr(ad), ops.ptr(bd), sim.ptr(), rows, D, *mode)
    runs = []
    for _ in range(2):
        da, db = Out(dev, rows, D), Out(dev, rows, D)
        ops.call(bwd, ops.ptr(ad), ops.ptr(bd), ops.ptr(gd), da.ptr(), db.ptr(), rows, D, *mode)
        runs.append([da.done(), db.done()])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    return [sim.done()] + runs[0]


@pytest.mark.parametrize("mi", range(len(R.ROW_MODES)), ids=[f"{e}-kind{k}-l2{n}-scale{s}" for e, k, n, s in R.ROW_MODES])
@pytest.mark.parametrize("D", R.ROW_D)
def test_row_heads_sweep(ops, dev, D, mi):
    entry, kind, l2norm, scale = R.ROW_MODES[mi]
    for rows in R.ROW_ROWS:
        a, b, dsim = R.row_inputs(rows, D, kind, l2norm, scale, 4000 + 10 * D + mi)
        got = run_rows(ops, dev, entry, a, b, dsim, kind, l2norm, scale)
        ref, r32 = R.row_ref(a, b, dsim, kind, l2norm, scale, D64), R.row_ref(a, b, dsim, kind, l2norm, scale, torch.float32)
        tag = f"{entry} rows {rows} D {D} kind {kind} l2norm {l2norm} scale {scale}"
        close(tag + " sim", got[0], ref[0], r32[0], FWD)
        close(tag + " da", got[1], ref[1], r32[1], GRAD)
        close(tag + " db", got[2], ref[2], r32[2], GRAD)


@pytest.mark.parametrize("entry", ["rowdot", "rowpair"])
def test_row_heads_saturated_clamp_and_its_backward(ops, dev, entry):
    """logits of -30 / +30 / order one in turn: sigmoid(-30) = 9.4e-14 is clamped to exactly 1e-7f and passes exactly no gradient,
    sigmoid(+30) rounds to 1.0f.  rows 9 (a last block of one wave), D 65 (a second trip of one lane)."""
    rows, D = 9, 65
    g = torch.Generator().manual_seed(7)
    b = torch.randn(rows, D, generator=g)
    unit = b / (b * b).sum(-1, keepdim=True) * math.sqrt(D)       # unit . b / sqrt(D) = 1
    a = 0.5 * torch.randn(rows, D, generator=g)
    low, high = torch.arange(rows) % 3 == 0, torch.arange(rows) % 3 == 1
    a[low], a[high] = -30.0 * unit[low], 30.0 * unit[high]
    dsim = torch.randn(rows, generator=g)
    got = run_rows(ops, dev, entry, a, b, dsim, 0, 0, 1)
    ref, r32 = R.row_ref(a, b, dsim, 0, 0, 1, D64), R.row_ref(a, b, dsim, 0, 0, 1, torch.float32)
    assert torch.equal(got[0][low], torch.full((int(low.sum()),), 1e-7)) and torch.equal(got[0][high], torch.ones(int(high.sum())))
    assert (got[1][low] == 0).all() and (got[2][low] == 0).all()
    for i, name in enumerate(("sim", "da", "db")):
        close(f"{entry} saturated {name}", got[i], ref[i], r32[i], FWD if i == 0 else GRAD)


@pytest.mark.parametrize("l2norm", [0, 1])
def test_rowpair_exp_neg_l2_identical_rows_and_a_zero_row(ops, dev, l2norm):
    """kind 1 at a distance of exactly 0 (identical rows): similarity 1 and the ZERO gradient the kernel documents (rr > 0 ? ... :
    0; autograd's is 0 / 0).  A zero row under l2norm: F.normalize's eps keeps every output finite."""
    rows, D = 5, 65
    g = torch.Generator().manual_seed(3)
    a = torch.randn(rows, D, generator=g)
    b = a.clone()
    b[3] = torch.randn(D, generator=g)
    if l2norm:
        a[4] = 0.0
    sim, da, db = run_rows(ops, dev, "rowpair", a, b, torch.ones(rows), 1, l2norm, 0)
    same = [0, 1, 2] if l2norm else [0, 1, 2, 4]
    assert torch.equal(sim[same], torch.ones(len(same))) and (da[same] == 0).all() and (db[same] == 0).all()
    assert torch.isfinite(sim).all() and torch.isfinite(da).all() and torch.isfinite(db).all()
    assert 0 < sim[3] < 1 and (da[3] != 0).any()
    if l2norm:                                                  # u = 0, w a unit vector: exp(-1)
        assert abs(sim[4].item() - math.exp(-1.0)) < 1e-6


@pytest.mark.parametrize("scale", [0, 1])
def test_rowdot_and_rowpair_kind0_agree_bit_for_bit(ops, dev, scale):
    """tag_rowdot_sigmoid_* is tag_rowpair_* with kind 0 and no l2norm: the same sums in the same order (include/tag_hip.h)"""
    a, b, dsim = R.row_inputs(1001, 300, 0, 0, scale, 12)
    for x, y in zip(run_rows(ops, dev, "rowdot", a, b, dsim, 0, 0, scale), run_rows(ops, dev, "rowpair", a, b, dsim, 0, 0, scale)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 6. text tower
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("D", R.ALN_D)
def test_add_layernorm_sweep(ops, dev, D, with_res):
    for rows in R.ALN_ROWS:
        x, res, gamma, beta = R.aln_inputs(rows, D, 5000 + D)
        res = res if with_res else None
        d = [None if t is None else t.to(dev) for t in (x, res, gamma, beta)]
        out = Out(dev, rows, D)
        ops.call("tag_add_layernorm", *(ops.ptr(t) for t in d), R.LN_EPS, out.ptr(), rows, D)
        ref = R.add_layernorm(x.double(), None if res is None else res.double(), gamma.double(), beta.double())
        close(f"add_layernorm rows {rows} D {D} res {with_res} out", out.done(), ref, R.add_layernorm(x, res, gamma, beta), FWD)


def test_text_tower_refusals(ops, dev):
    z, ids = torch.zeros(4 * 1025, device=dev), torch.zeros(65 * 4, dtype=torch.long, device=dev)
    out = Out(dev, 2 * 1025)
    refused(ops, "tag_add_layernorm", ops.ptr(z), None, ops.ptr(z), ops.ptr(z), R.LN_EPS, out.ptr(), 2, 1025)
    refused(ops, "tag_roberta_embed_ln", ops.ptr(ids), ops.ptr(z), ops.ptr(z), ops.ptr(z), ops.ptr(z), ops.ptr(z), R.LN_EPS, out.ptr(),
            1, 2, 1025, 1)
    out.done(filled=False)
    qkv, small = torch.zeros(65 * 3 * 64, device=dev), Out(dev, 65 * 64)
    refused(ops, "tag_mha_small", ops.ptr(qkv), ops.ptr(ids), small.ptr(), 1, 65, 1, 16)          # L = 65
    refused(ops, "tag_mha_small", ops.ptr(qkv), ops.ptr(ids), small.ptr(), 1, 4, 1, 48)           # dh = 48
    small.done(filled=False)


@pytest.mark.parametrize("D", R.EMB_D)
@pytest.mark.parametrize("L", R.EMB_L)
def test_roberta_embed_ln_sweep(ops, dev, L, D):
    ids, word, type0, pos, gamma, beta = R.emb_inputs(L, D, 6000 + L)
    d = [t.to(dev) for t in (ids, word, type0, pos, gamma, beta)]
    out = Out(dev, 4 * L, D)
    ops.call("tag_roberta_embed_ln", *(ops.ptr(t) for t in d), R.LN_EPS, out.ptr(), 4, L, D, R.EMB_PAD)
    got = out.done()
    ref = R.roberta_embed_ln(ids, *(t.double() for t in (word, type0, pos, gamma, beta)), R.EMB_PAD)
    close(f"roberta_embed_ln L {L} D {D} out", got, ref, R.roberta_embed_ln(ids, word, type0, pos, gamma, beta, R.EMB_PAD), FWD)
    # the position rows by value: with the word and type rows zeroed and a plain LayerNorm, an output row is LayerNorm(pos[p]) of
    # exactly one row p of the table -- decode p and compare it with the rule
    zero_w, zero_t, one, zero_b = torch.zeros_like(d[1]), torch.zeros_like(d[2]), torch.ones_like(d[4]), torch.zeros_like(d[5])
    out = Out(dev, 4 * L, D)
    ops.call("tag_roberta_embed_ln", ops.ptr(d[0]), ops.ptr(zero_w), ops.ptr(zero_t), ops.ptr(d[3]), ops.ptr(one), ops.ptr(zero_b),
             R.LN_EPS, out.ptr(), 4, L, D, R.EMB_PAD)
    table = R.layer_norm_rows(pos.double(), 1.0, 0.0)[0]                                  # (P, D)
    decoded = torch.cdist(out.done().double(), table).argmin(-1).view(4, L)
    assert torch.equal(decoded, R.position_ids(ids, R.EMB_PAD))


@pytest.mark.parametrize("dh", R.SMALL_DH)
@pytest.mark.parametrize("L", R.SMALL_L)
def test_mha_small_sweep(ops, dev, L, dh):
    for heads in R.SMALL_HEADS:
        for B in R.SMALL_B:
            qkv, mask = R.small_inputs(B, L, heads, dh), R.small_mask(B, L, heads)
            out, qd, md = Out(dev, B * L, heads * dh), qkv.to(dev), mask.to(dev)
            ops.call("tag_mha_small", ops.ptr(qd), ops.ptr(md), out.ptr(), B, L, heads, dh)
            ref = R.mha_small(qkv.double(), mask, heads, dh)
            close(f"mha_small B {B} L {L} heads {heads} dh {dh} out", out.done().view(B, L, -1), ref, R.mha_small(qkv, mask, heads, dh), FWD)


def test_mha_small_fully_masked_sequence_is_nan_and_alone(ops, dev):
    """a sequence without a valid key: every output of that sequence is NaN (include/tag_hip.h); the others are bit-equal to a run in
    which it had one"""
    B, L, heads, dh = 3, 9, 3, 32
    qkv, mask = R.small_inputs(B, L, heads, dh).to(dev), R.small_mask(B, L, 0)
    outs = []
    for dead in (False, True):
        m = mask.clone()
        if dead:
            m[1] = 0
        out, md = Out(dev, B, L, heads * dh), m.to(dev)
        ops.call("tag_mha_small", ops.ptr(qkv), ops.ptr(md), out.ptr(), B, L, heads, dh)
        assert (out.buf[out.n:] == SENTINEL).all()
        outs.append(out.t.cpu())
    assert torch.isfinite(outs[0]).all() and torch.isnan(outs[1][1]).all() and torch.equal(outs[0][[0, 2]], outs[1][[0, 2]])
