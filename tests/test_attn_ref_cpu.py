"""The CPU statements of the attention sweep (tests/attn_ref.py) against torch's own modules and the oracle -- a reference that
is wrong would make the GPU sweep assert the wrong thing -- and the sweep's INPUT CONDITION for every case of its tables: the
same statement evaluated in fp32 on the CPU (the floor) stays below a quarter of the plain bound, so that a kernel as good as
plain fp32 passes with room and a case that fails says something about the kernel."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import tag_oracle as O
from tests import attn_ref as R

D64 = torch.float64


def rel(a, b):
    """max-normalised, with a scale of at least one: a gradient that vanishes identically (LayerNorm over one element) is
    compared absolutely -- torch's own module leaves 1e-17 there"""
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1.0)


# ------------------------------------------------------------------------------------------------ the statements
@pytest.mark.parametrize("B,T,L,E,H", [(3, 5, 6, 32, 2), (2, 4, 32, 64, 1), (1, 3, 1, 48, 3)])
def test_mha_core_is_nn_multihead_attention(B, T, L, E, H):
    """with identity projections nn.MultiheadAttention IS the core: same weights (per head), same context, same gradients"""
    q, k, v, dctx = (t.double() for t in R.mha_inputs(B, T, L, E, H, 5))
    klen = torch.tensor([L, 1, max(L // 2, 1)][:B])
    m = torch.nn.MultiheadAttention(E, H, 0.0, batch_first=True).double()
    with torch.no_grad():
        m.in_proj_weight.copy_(torch.eye(E, dtype=D64).repeat(3, 1))
        m.in_proj_bias.zero_()
        m.out_proj.weight.copy_(torch.eye(E, dtype=D64))
        m.out_proj.bias.zero_()
    qa, ka, va = (R.leaf(t, D64) for t in (q, k, v))
    want, w = m(qa, ka, va, key_padding_mask=torch.arange(L)[None, :] >= klen[:, None], average_attn_weights=False)
    want.backward(dctx)
    attn, ctx, dq, dk, dv = R.mha_ref(q, k, v, dctx, klen, H, None, 0.0, D64)
    assert rel(ctx, want) < 1e-12 and rel(attn, w.permute(0, 2, 1, 3)) < 1e-12
    assert rel(dq, qa.grad) < 1e-12 and rel(dk, ka.grad) < 1e-12 and rel(dv, va.grad) < 1e-12
    assert (attn.sum(-1) - 1).abs().max() < 1e-12
    for b in range(B):
        assert (attn[b, :, :, int(klen[b]):] == 0).all()


def test_mha_core_klen_edges_and_keep_mask():
    """klen > L masks nothing (equal to klen = L bit for bit), klen = 0 is NaN on that clip alone, and the keep mask is applied to
    the weights AFTER the softmax (the returned attn is the undropped one) -- the same as the oracle's match_cross_attention with
    identity projections does through its out_proj"""
    B, T, L, E, H = 3, 4, 5, 32, 2
    q, k, v, _ = (t.double() for t in R.mha_inputs(B, T, L, E, H, 9))
    a0, c0 = R.mha_core(q, k, v, torch.tensor([5, 3, 5]), H)
    a1, c1 = R.mha_core(q, k, v, torch.tensor([9, 3, 40]), H)
    assert torch.equal(a0, a1) and torch.equal(c0, c1)
    a2, c2 = R.mha_core(q, k, v, torch.tensor([5, 0, 5]), H)
    assert torch.isnan(a2[1]).all() and torch.isnan(c2[1]).all() and torch.equal(c2[[0, 2]], c0[[0, 2]])
    keep = (torch.rand(B, T, H, L, generator=torch.Generator().manual_seed(1)) > 0.3)
    a3, c3 = R.mha_core(q, k, v, torch.tensor([5, 3, 5]), H, keep.double(), 0.3)
    assert torch.equal(a3, a0)
    dh = E // H
    want = torch.einsum("bthl,blhd->bthd", a0 * keep / 0.7, v.view(B, L, H, dh)).reshape(B, T, E)
    assert rel(c3, want) < 1e-12


@pytest.mark.parametrize("E,H,p", [(32, 2, 0.0), (64, 4, 0.3)])
def test_core_plus_head_is_the_oracle_cross_attention(E, H, p):
    """projections (F.linear) + mha_core + out_proj + resln_head == O.match_cross_attention, outputs and every gradient, with both
    keep masks imposed"""
    B, T, L = 2, 5, 4
    g = torch.Generator().manual_seed(E)
    names = {"attn.in_proj_weight": (3 * E, E), "attn.in_proj_bias": (3 * E,), "attn.out_proj.weight": (E, E),
             "attn.out_proj.bias": (E,), "norm.weight": (E,), "norm.bias": (E,), "linear.weight": (1, E), "linear.bias": (1,)}
    vals = {k: (torch.randn(*s, generator=g) / math.sqrt(s[-1])).double() for k, s in names.items()}
    audio, token = torch.randn(B, T, E, generator=g).double(), torch.randn(B, L, E, generator=g).double()
    dsim, text_len = torch.randn(B, T, generator=g).double(), torch.tensor([4, 2])
    ak = rk = None
    if p > 0:
        ak, rk = (torch.rand(B, T, H, L, generator=g) > p).double(), (torch.rand(B, T, E, generator=g) > p).double()
    grads = []
    for mine in (False, True):
        st = {"match_fn." + k: R.leaf(v, D64) for k, v in vals.items()}
        a, t = R.leaf(audio, D64), R.leaf(token, D64)
        if mine:
            w, b = st["match_fn.attn.in_proj_weight"], st["match_fn.attn.in_proj_bias"]
            q, k, v = F.linear(a, w[:E], b[:E]), F.linear(t, w[E:2 * E], b[E:2 * E]), F.linear(t, w[2 * E:], b[2 * E:])
            _, ctx = R.mha_core(q, k, v, text_len, H, ak, p)
            r = F.linear(ctx, st["match_fn.attn.out_proj.weight"], st["match_fn.attn.out_proj.bias"])
            sim, _, _ = R.resln_head(a.reshape(B * T, E), r.reshape(B * T, E), st["match_fn.norm.weight"], st["match_fn.norm.bias"],
                                     st["match_fn.linear.weight"][0], st["match_fn.linear.bias"][0],
                                     None if rk is None else rk.reshape(B * T, E), p)
            sim = sim.view(B, T)
        else:
            sim = O.match_cross_attention(st, a, t, text_len, H, attn_keep=ak, res_keep=rk, p_drop=p)
        sim.backward(dsim)
        grads.append([sim.detach(), a.grad, t.grad] + [st["match_fn." + k].grad for k in names])
    for x, y in zip(*grads):
        assert rel(y, x) < 1e-12


@pytest.mark.parametrize("rows,E", [(1, 1), (5, 65), (7, 256)])
def test_resln_head_is_f_layer_norm_and_its_per_row_terms_sum_to_the_parameter_gradients(rows, E):
    x, r, gamma, beta, w, bias, dsim = (t.double() for t in R.resln_inputs(rows, E, 3))
    keep = (torch.rand(rows, E, generator=torch.Generator().manual_seed(2)) > 0.3).double()
    ls = [R.leaf(t, D64) for t in (x, r, gamma, beta, w, bias)]
    z = ls[0] + ls[1] * keep / 0.7
    want = torch.sigmoid(F.linear(F.layer_norm(z, (E,), ls[2], ls[3], R.LN_EPS), ls[4][None, :], ls[5])).squeeze(-1)
    want.backward(dsim)
    ref = R.resln_ref(x, r, gamma, beta, w, bias, dsim, keep, 0.3, D64)
    assert rel(ref["sim"], want) < 1e-12 and rel(ref["dx"], ls[0].grad) < 1e-12 and rel(ref["dr"], ls[1].grad) < 1e-12
    assert rel(ref["gg"].sum(0), ls[2].grad) < 1e-12 and rel(ref["gb"].sum(0), ls[3].grad) < 1e-12
    assert rel(ref["gw"].sum(0), ls[4].grad) < 1e-12 and rel(ref["ds"].sum(0, keepdim=True), ls[5].grad) < 1e-12
    assert torch.equal(ref["dr"], ref["dx"] * keep / 0.7)
    assert rel(ref["mu"], z.detach().mean(-1)) < 1e-12
    assert rel(ref["rstd"], 1 / torch.sqrt(z.detach().var(-1, unbiased=False) + R.LN_EPS)) < 1e-12
    if E == 1:                                                 # the zero-variance row: xhat = 0, the output is beta, dx vanishes
        assert (ref["dx"] == 0).all() and (ref["gg"] == 0).all() and rel(ref["rstd"], torch.full((rows,), R.LN_EPS ** -0.5, dtype=D64)) < 1e-12


def test_addattn_is_the_oracle_seq2seq_attention():
    B, T, L, Dq, Dkv, Da = 3, 6, 5, 8, 12, 7
    g = torch.Generator().manual_seed(4)
    st = {"cross_encoder.attn.h2attn.weight": torch.randn(Da, Dq + Dkv, generator=g).double(),
          "cross_encoder.attn.h2attn.bias": torch.randn(Da, generator=g).double(),
          "cross_encoder.attn.v": torch.randn(Da, generator=g).double()}
    query, kv = torch.randn(B, T, Dq, generator=g).double(), torch.randn(B, L, Dkv, generator=g).double()
    qlen, klen = torch.tensor([6, 3, 9]), torch.tensor([5, 0, 2])
    want = O.seq2seq_attention(st, query, kv, qlen, klen)
    W = st["cross_encoder.attn.h2attn.weight"]
    aq, ak = F.linear(query, W[:, :Dq]), F.linear(kv, W[:, Dq:], st["cross_encoder.attn.h2attn.bias"])
    attn, ctx = R.addattn(aq, ak, st["cross_encoder.attn.v"], kv, qlen, klen)
    assert rel(ctx, want) < 1e-12 and (attn.sum(-1) - 1).abs().max() < 1e-12
    # a fully filled row is uniform over ALL L tokens, padding included: frames >= qlen, and every frame of the clip with klen 0
    assert torch.equal(attn[1], torch.full((T, L), 1.0 / L, dtype=D64)) and (attn[0] > 0).all()     # clip 0: nothing filled
    assert (attn[2, :, 2:] == 0).all() and (attn[2, :, :2] > 0).all()
    # ... and passes no score gradient
    ref = R.add_ref(aq, ak, st["cross_encoder.attn.v"], kv, torch.randn(B, T, Dkv, generator=g).double(), qlen, klen, D64)
    assert (ref["daq"][1] == 0).all() and (ref["dak"][1] == 0).all() and (ref["daq"][0] != 0).any()
    assert (ref["dkv"][1] != 0).all()                          # the attn @ kv term reaches every token of a uniform row


def test_gate_backward_is_autograd_of_x_times_sigmoid():
    g = torch.Generator().manual_seed(6)
    x, z = R.leaf(torch.randn(40, generator=g), D64), R.leaf(torch.randn(40, generator=g), D64)
    dout, dx_in = torch.randn(40, generator=g).double(), torch.randn(40, generator=g).double()
    (x * torch.sigmoid(z)).backward(dout)
    dx, dz = R.gate_backward(dout, x.detach(), torch.sigmoid(z.detach()), None)
    assert rel(dx, x.grad) < 1e-12 and rel(dz, z.grad) < 1e-12
    assert rel(R.gate_backward(dout, x.detach(), torch.sigmoid(z.detach()), dx_in)[0], x.grad + dx_in) < 1e-12


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("l2norm", [False, True])
def test_rowpair_is_the_oracle_token_heads(l2norm, scale):
    g = torch.Generator().manual_seed(8)
    a, b = torch.randn(3, 7, 20, generator=g).double(), torch.randn(3, 7, 20, generator=g).double()
    if not l2norm:
        assert rel(R.rowpair(a, b, 0, 0, scale), O.match_dot_product_token(a, b, scale)) < 1e-12
    an, bn = (F.normalize(a, dim=-1), F.normalize(b, dim=-1)) if l2norm else (a, b)
    assert rel(R.rowpair(a, b, 0, l2norm, scale), O.match_dot_product_token(an, bn, scale)) < 1e-12
    assert rel(R.rowpair(a, b, 1, l2norm, scale), torch.exp(-(an - bn).norm(dim=-1))) < 1e-12
    # the clamp: sigmoid(-30) -> exactly 1e-7 with a zero gradient
    al = R.leaf(torch.full((1, 4), 30.0), D64)
    s = R.rowpair(al, torch.full((1, 4), -1.0, dtype=D64), 0, 0, True)
    s.backward(torch.ones(1, dtype=D64))
    assert s.item() == 1e-7 and (al.grad == 0).all()
    # a zero row under l2norm stays finite (F.normalize's eps)
    assert torch.isfinite(R.rowpair(torch.zeros(1, 4, dtype=D64), torch.ones(1, 4, dtype=D64), 1, 1, 0)).all()


def test_position_ids_are_the_hf_rule_and_the_embedding_is_f_layer_norm():
    ids, word, type0, pos, gamma, beta = R.emb_inputs(9, 12, 1)
    m = ids.ne(R.EMB_PAD).int()
    want = (torch.cumsum(m, dim=1).type_as(m) * m).long() + R.EMB_PAD         # create_position_ids_from_input_ids
    assert torch.equal(R.position_ids(ids, R.EMB_PAD), want)
    assert (want[3] == R.EMB_PAD).all() and want[0, 3] == R.EMB_PAD + 1 and want.max() == R.EMB_PAD + 9 - 2
    e = F.embedding(ids, word.double()) + type0.double() + F.embedding(want, pos.double())
    ln = F.layer_norm(e, (12,), gamma.double(), beta.double(), R.LN_EPS).reshape(-1, 12)
    assert rel(R.roberta_embed_ln(ids, *(t.double() for t in (word, type0, pos, gamma, beta)), R.EMB_PAD), ln) < 1e-12
    x, res, gamma, beta = (t.double() for t in R.aln_inputs(5, 65, 2))
    assert rel(R.add_layernorm(x, res, gamma, beta), F.layer_norm(x + res, (65,), gamma, beta, R.LN_EPS)) < 1e-12
    assert rel(R.add_layernorm(x, None, gamma, beta), F.layer_norm(x, (65,), gamma, beta, R.LN_EPS)) < 1e-12
    for L in R.EMB_L:                                          # every pattern the sweep asks for is really in the inputs
        ids = R.emb_inputs(L, 65, L)[0]
        assert (ids[3] == R.EMB_PAD).all() and ids.max() < R.EMB_VOCAB
        if L >= 4:
            assert ids[0, 0] == R.EMB_PAD and ids[0, -1] != R.EMB_PAD and ids[2, -1] == R.EMB_PAD and ids[2, 0] != R.EMB_PAD
            assert ids[1, 0] != R.EMB_PAD and ids[1, -1] != R.EMB_PAD and (ids[1] == R.EMB_PAD).any()


@pytest.mark.parametrize("B,L,heads,dh", [(3, 9, 2, 16), (1, 2, 3, 8)])
def test_mha_small_is_scaled_dot_product_attention(B, L, heads, dh):
    qkv = R.small_inputs(B, L, heads, dh).double()
    mask = R.small_mask(B, L, 1)
    q, k, v = (t.reshape(B, L, heads, dh).transpose(1, 2) for t in qkv.split(heads * dh, dim=-1))
    want = F.scaled_dot_product_attention(q, k, v, attn_mask=(mask != 0)[:, None, None, :]).transpose(1, 2).reshape(B, L, heads * dh)
    assert rel(R.mha_small(qkv, mask, heads, dh), want) < 1e-12
    dead = mask.clone()
    dead[0] = 0
    out = R.mha_small(qkv, dead, heads, dh)
    assert torch.isnan(out[0]).all() and torch.equal(out[1:], R.mha_small(qkv, mask, heads, dh)[1:])
    for L_ in R.SMALL_L:
        m3 = R.small_mask(3, L_, 0)
        assert (m3.sum(1) >= 1).all() and (m3[0] == 1).all()
        if L_ >= 3:
            assert m3[2, 0] == 1 and m3[2, -1] == 1 and (m3[2] == 0).any() and m3[1, -1] == 0


# ------------------------------------------------------------------------------------------------ the input condition
def floors(ref64, ref32, names_fwd):
    """every entry of the two reference results: (name, floor, a quarter of its plain bound)"""
    items = ref64.items() if isinstance(ref64, dict) else enumerate(ref64)
    out = []
    for key, want in items:
        got = ref32[key]
        if want.abs().max().item() < 1e-12:
            fl = got.abs().max().item()
        else:
            fl = R.relerr(got, want)
        out.append((key, fl, (R.FWD if key in names_fwd else R.GRAD) / 4))
    return out


def assert_condition(tag, ref64, ref32, names_fwd):
    for key, fl, quarter in floors(ref64, ref32, names_fwd):
        assert fl < quarter, f"{tag} {key}: fp32 floor {fl:.2e} >= {quarter:.2e} -- take another seed for this case"


@pytest.mark.parametrize("si", range(len(R.MHA_SHAPES)), ids=["x".join(map(str, s)) for s in R.MHA_SHAPES])
def test_input_condition_attention_core(si):
    for pi, p in enumerate(R.MHA_DROP):
        (B, T, L, E, H, p), (q, k, v, dctx), klen = R.mha_case(si, pi)
        keep = None
        if p > 0:                                              # any mask of the right density: the sweep's is the kernel's own
            keep = (torch.rand(B, T, H, L, generator=torch.Generator().manual_seed(si)) >= p).float()
        assert_condition(f"mha {R.MHA_SHAPES[si]} p {p}", R.mha_ref(q, k, v, dctx, klen, H, keep, p, D64),
                         R.mha_ref(q, k, v, dctx, klen, H, keep, p, torch.float32), (0, 1))


def test_input_condition_saturated_attention():
    B, T, L, E, H = R.SAT_SHAPE
    q, k, v, dctx = R.mha_saturated_inputs()
    klen = torch.tensor([L, 17])
    score = torch.einsum("bthd,blhd->bthl", q.view(B, T, H, -1).double(), k.view(B, L, H, -1).double()) / 8.0
    assert score.min() < -30 and score.max() > 30 and score.abs().max() < 200
    s32 = torch.einsum("bthd,blhd->bthl", q.view(B, T, H, -1), k.view(B, L, H, -1)) / 8.0
    assert torch.equal(s32.double(), score), "the scores of the saturated case are exact in fp32"
    assert_condition("mha saturated", R.mha_ref(q, k, v, dctx, klen, H, None, 0.0, D64),
                     R.mha_ref(q, k, v, dctx, klen, H, None, 0.0, torch.float32), (0, 1))


@pytest.mark.parametrize("E", R.LN_E)
def test_input_condition_layernorm_head(E):
    for rows in R.LN_ROWS:
        for p in R.LN_DROP:
            args = R.resln_inputs(rows, E, 3000 + E + rows)
            keep = None if p == 0 else (torch.rand(rows, E, generator=torch.Generator().manual_seed(E)) >= p).float()
            assert_condition(f"resln rows {rows} E {E} p {p}", R.resln_ref(*args, keep, p, D64),
                             R.resln_ref(*args, keep, p, torch.float32), ("sim", "mu", "rstd"))


@pytest.mark.parametrize("si", range(len(R.ADD_SHAPES)), ids=["x".join(map(str, s)) for s in R.ADD_SHAPES])
def test_input_condition_additive_attention(si):
    shape, inputs, (qlen, klen) = R.add_case(si)
    assert_condition(f"addattn {shape}", R.add_ref(*inputs, qlen, klen, D64), R.add_ref(*inputs, qlen, klen, torch.float32),
                     ("attn", "ctx"))


def test_additive_attention_lengths_cover_every_value_the_sweep_asks_for():
    q_seen, k_seen = set(), set()
    for si, (B, T, L, Da, Dk) in enumerate(R.ADD_SHAPES):
        qlen, klen = R.add_lens(B, T, L, si)
        q_seen |= {"0" if v == 0 else "below" if v < T else "T" if v == T else "above" for v in qlen.tolist()}
        k_seen |= {"0" if v == 0 else "1" if v == 1 else "L" if v == L else "mid" for v in klen.tolist()}
    assert q_seen == {"0", "below", "T", "above"} and {"0", "1", "L"} <= k_seen
    assert {R.cdiv(T, 8) * B for B, T, *_ in R.ADD_SHAPES} >= {1, 15, 16, 17, 40}
    assert {L for _, _, L, _, _ in R.ADD_SHAPES} >= {1, 4, 5, 8, 9, 16, 17, 32}
    assert {T for _, T, *_ in R.ADD_SHAPES} >= {1, 7, 8, 9, 17}
    assert {(Da, Dk) for *_, Da, Dk in R.ADD_SHAPES} >= {(1, 1), (64, 64), (65, 64), (64, 65), (256, 257), (512, 513), (1024, 1024)}
    assert {Da for *_, Da, _ in R.ADD_SHAPES} >= {1, 17, 65}


@pytest.mark.parametrize("D", R.ROW_D)
def test_input_condition_row_heads(D):
    for mi, (entry, kind, l2norm, scale) in enumerate(R.ROW_MODES):
        for rows in R.ROW_ROWS:
            a, b, dsim = R.row_inputs(rows, D, kind, l2norm, scale, 4000 + 10 * D + mi)
            r64 = R.row_ref(a, b, dsim, kind, l2norm, scale, D64)
            if not (D == 1 and kind == 1 and l2norm):          # (there u, w = +-1 and the similarity is exactly 1 or e^-2)
                assert 0.02 <= r64[0].min().item() and r64[0].max().item() <= 0.98, (D, mi, rows)
            assert_condition(f"row D {D} mode {mi} rows {rows}", r64, R.row_ref(a, b, dsim, kind, l2norm, scale, torch.float32), (0,))


def test_input_condition_gating():
    for n in R.GATE_N:
        dout, x, g, dx_in = R.gate_inputs(n, n % 1000)
        assert_condition(f"mul n {n}", [x.double() * g.double()], [x * g], (0,))
        for acc in (None, dx_in):
            assert_condition(f"gate n {n}", list(R.gate_backward(dout.double(), x.double(), g.double(), None if acc is None else acc.double())),
                             list(R.gate_backward(dout, x, g, acc)), ())


# The remaining inputs of the sweep take no condition: the klen edge cases, the refusals, the bit-identity of rowdot and rowpair,
# the fully masked sequence and the path check compare one kernel run with another, or an output with an exact value (NaN, 0,
# 1 / L, 1e-7f), and no fp64 reference with a tolerance enters; the saturated row heads and identical rows assert exact values
# first and reuse the conditioned draw of the heads sweep for the rest.
def test_input_condition_text_tower():
    for D in R.ALN_D:
        for rows in R.ALN_ROWS:
            x, res, gamma, beta = R.aln_inputs(rows, D, 5000 + D)
            for r_ in (None, res):
                w = R.add_layernorm(x.double(), None if r_ is None else r_.double(), gamma.double(), beta.double())
                assert_condition(f"add_layernorm {rows}x{D}", [w], [R.add_layernorm(x, r_, gamma, beta)], (0,))
    for L in R.EMB_L:
        for D in R.EMB_D:
            ids, *tabs = R.emb_inputs(L, D, 6000 + L)
            assert_condition(f"embed L {L} D {D}", [R.roberta_embed_ln(ids, *(t.double() for t in tabs), R.EMB_PAD)],
                             [R.roberta_embed_ln(ids, *tabs, R.EMB_PAD)], (0,))
    for L in R.SMALL_L:
        for dh in R.SMALL_DH:
            for heads in R.SMALL_HEADS:
                for B in R.SMALL_B:
                    qkv, mask = R.small_inputs(B, L, heads, dh), R.small_mask(B, L, heads)
                    assert_condition(f"mha_small {B} {L} {heads} {dh}", [R.mha_small(qkv.double(), mask, heads, dh)],
                                     [R.mha_small(qkv, mask, heads, dh)], (0,))
