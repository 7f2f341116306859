"""CPU: the GRU statement of tests/gru_ref.py is nn.GRU and the oracle's gru_bidir seen from the kernels' interface (to 1e-12 in
fp64, values and every gradient the caller forms from the kernels' outputs), and every case of the sweep's tables is conditioned
well enough: the same statement in fp32 stays below a quarter of the bound tests/test_gpu_gru_sweep.py uses on the GPU."""
import pytest
import torch

from oracle import tag_oracle as O
from tests import gru_ref as R

D64 = torch.float64


@pytest.mark.parametrize("B,T,I,H", [(3, 5, 24, 32), (5, 4, 16, 128), (2, 1, 8, 48)])
def test_statement_is_nn_gru_and_the_oracle(B, T, I, H):
    g = torch.Generator().manual_seed(H + T)
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    shapes = [(3 * H, I), (3 * H, H), (3 * H,), (3 * H,)]
    st = {"rnn." + n + sfx: ((torch.rand(s, generator=g, dtype=D64) * 2 - 1) * 0.2).requires_grad_(True)
          for sfx in ("", "_reverse") for n, s in zip(names, shapes)}
    x = torch.randn(B, T, I, generator=g, dtype=D64).requires_grad_(True)
    dy = torch.randn(B, T, 2 * H, generator=g, dtype=D64)
    y_o = O.gru_bidir(x, st, "rnn.")
    y_o.backward(dy)
    rnn = torch.nn.GRU(I, H, bidirectional=True, batch_first=True).double()
    rnn.load_state_dict({k[4:]: v.detach() for k, v in st.items()})
    y_t, _ = rnn(x.detach())
    # the kernels' interface: gi = x W_ih^T + b_ih of both directions
    w_ih = torch.stack([st["rnn.weight_ih_l0"], st["rnn.weight_ih_l0_reverse"]]).detach()                     # (2,3H,I)
    b_ih = torch.stack([st["rnn.bias_ih_l0"], st["rnn.bias_ih_l0_reverse"]]).detach()
    w_hh = torch.stack([st["rnn.weight_hh_l0"], st["rnn.weight_hh_l0_reverse"]]).detach()
    b_hh = torch.stack([st["rnn.bias_hh_l0"], st["rnn.bias_hh_l0_reverse"]]).detach()
    gi = torch.einsum("bti,dki->btdk", x.detach(), w_ih) + b_ih
    r = R.gru_ref(gi, w_hh, b_hh, dy, D64)
    assert (r["y"] - y_t).abs().max().item() < 1e-12 and (r["y"] - y_o).abs().max().item() < 1e-12
    dx = torch.einsum("btdk,dki->bti", r["dgi"], w_ih)
    assert (dx - x.grad).abs().max().item() < 1e-12
    for d, sfx in enumerate(("", "_reverse")):
        dw_hh = torch.einsum("btk,bth->kh", r["dgh"][:, :, d], r["hprev"][:, :, d])
        assert (dw_hh - st["rnn.weight_hh_l0" + sfx].grad).abs().max().item() < 1e-12
        assert (r["dgh"][:, :, d].sum((0, 1)) - st["rnn.bias_hh_l0" + sfx].grad).abs().max().item() < 1e-12
        dw_ih = torch.einsum("btk,bti->ki", r["dgi"][:, :, d], x.detach())
        assert (dw_ih - st["rnn.weight_ih_l0" + sfx].grad).abs().max().item() < 1e-12
    # what the kernels promise beyond the values: hprev is the predecessor's y, r and z thirds of dgi and dgh coincide
    yv = r["y"].view(B, T, 2, H)
    assert torch.equal(r["hprev"][:, 1:, 0], yv[:, :-1, 0]) and torch.equal(r["hprev"][:, :-1, 1], yv[:, 1:, 1])
    assert (r["hprev"][:, 0, 0] == 0).all() and (r["hprev"][:, -1, 1] == 0).all()
    assert torch.equal(r["dgi"][..., :2 * H], r["dgh"][..., :2 * H])


def test_every_case_is_conditioned():
    """fp32 floor of every (B, T, H) of the tables <= a quarter of the GPU bound; a case that is not takes another seed
    (gru_ref.SEEDS).  The saturated cases must also be saturated."""
    worst = {n: 0.0 for n in R.NAMES}
    for B, T, H, sat in R.all_cases():
        gi, w, b, dy = R.case_inputs(B, T, H, sat)
        r64, r32 = R.gru_ref(gi, w, b, dy, D64), R.gru_ref(gi, w, b, dy, torch.float32)
        for n in R.NAMES:
            fl = R.relerr(r32[n], r64[n])
            worst[n] = max(worst[n], fl)
            quarter = (R.FWD if n in ("y", "gates", "hprev") else R.GRAD) / 4
            assert fl <= quarter, f"({B},{T},{H}) sat {sat} {n}: fp32 floor {fl:.2e} > {quarter:.2e} -- take another seed"
        if sat:
            share = R.saturated_share(r64["gates"][..., H:2 * H])
            assert share > 0.25, (B, T, H, share)
    print("worst fp32 floors:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_tables_reach_what_they_name():
    assert len(R.P4_CASES) == 54 and len(R.STEP0_CASES) == 36 and len(R.P16_CASES) == 30 and len(R.XCD_CASES) == 6
    lay = {B: R.p4_placement(B) for B in (1, 3, 4, 5, 13, 16, 17, 61, 64)}
    assert {B for B, v in lay.items() if v[0] == "remapped"} == {13, 16, 61, 64}
    assert lay[13][1] == 1 and lay[61][1] == 1 and lay[3][1] == 3 and lay[17][1] == 1 and lay[64][1] == 4
    # neither persistent grid of the two big step cases fits (8 - 1) x 256 workgroups
    for B, T, H, form, _ in R.STEPT_CASES:
        if T > 1:
            assert (H // 16) * ((B + 15) // 16) * 2 > 7 * 256 and (H // 32) * ((B + 3) // 4) * 2 > 7 * 256
            assert (H // 16) * ((B - 16 + 15) // 16) * 2 <= 7 * 256      # and B is the smallest multiple-of-16 tile count that does not


def test_gate_points():
    p = R.gate_points()
    assert p.dtype == torch.float32 and p.numel() <= 4 * 2 * 2 * 128
    assert (p == 0).sum() == 1 and torch.isinf(p).sum() == 2 and ((p.abs() > 0) & (p.abs() < 1.17e-38)).sum() == 4
    near = p[(p - 0.2).abs() < 1e-5]
    assert near.numel() == 129 and (near < 0.2).sum() == 64
    gi, w, b, col = R.gate_case(4, 2, 128)
    assert gi.shape == (4, 2, 2, 384) and set(p.tolist()) == set(col.flatten().tolist())
