"""CPU checks of tests/logmel_ref.py, the fp64 reference of tests/test_gpu_logmel_sweep.py (no GPU):

* the restatement (explicit reflected frame indices, hand-padded window, torch.fft.rfft) against oracle.tag_oracle
  (torch.stft) for both production parameter sets at every clip length of the sweep, and against torch.stft for the
  synthetic hop / window cases: 1e-12 of the clip maximum in the power domain, 1e-9 dB after the clamp;
* analytic known answers that depend on neither: constant, alternating and single-cosine signals under a window of ones;
* the premises of the sweep's rule, measured on the reference alone: the share of entries a dB comparison leaves out is below
  5 % for every case built here, the fp32 run of the restatement deviates by less than 1.25e-6, and the filterbank builders
  have the band widths their names promise.
"""
import math

import pytest
import torch

from oracle import tag_oracle as O
from tests import logmel_ref as R

LENGTHS = {"cnn8rnn": [513, 514, 640, 641, 959, 960, 1023, 1024, 1025, 3333],
           "crnn": [1025, 1281, 2047, 2048, 2049, 3333]}
SYNTH = [(161, 1024, 2001), (320, 1023, 1500), (160, 401, 1500)]          # (hop, win_length, S) at n_fft 1024


@pytest.mark.parametrize("kind,S", [(k, s) for k, v in LENGTHS.items() for s in v])
def test_restatement_equals_the_oracle(kind, S):
    p = O.FRONTEND[kind]
    window, fb = O.frontend_tables(kind)
    wave = R.noise(3, S, seed=S)
    mine = R.mel_power(wave, p["n_fft"], p["hop_length"], window, fb)
    ref = O.mel_spectrogram(wave.double(), kind).transpose(1, 2)
    assert mine.shape == ref.shape == (3, S // p["hop_length"] + 1, 64)
    err = R.rel_err(mine, ref)
    ddb = (R.to_db(mine) - O.amplitude_to_db(ref)).abs().max().item()
    dev32 = R.rel_err(R.mel_power(wave, p["n_fft"], p["hop_length"], window, fb, torch.float32), mine)
    print(f"{kind} S={S}: restatement vs oracle {err:.1e}, dB {ddb:.1e}; fp32 restatement vs fp64 {dev32:.2e}")
    assert err < 1e-12 and ddb < 1e-9
    assert dev32 < R.DEV_LIMIT


@pytest.mark.parametrize("hop,win_length,S", SYNTH)
def test_restatement_equals_torch_stft_on_odd_hops_and_windows(hop, win_length, S):
    window = torch.hann_window(win_length)
    wave = R.noise(3, S, seed=S + hop)
    mine = R.spectrum(wave, 1024, hop, window)
    ref = torch.stft(wave.double(), 1024, hop, win_length, window=window.double(), center=True, pad_mode="reflect",
                     return_complex=True).abs().pow(2.0).transpose(1, 2)
    assert mine.shape == ref.shape == (3, S // hop + 1, 513)
    assert R.rel_err(mine, ref) < 1e-12


@pytest.mark.parametrize("n_fft,hop", [(1024, 320), (2048, 640)])
def test_analytic_known_answers(n_fft, hop):
    k0, c = 37, 0.25
    S = n_fft + 3 * hop + 1
    wave = R.analytic_signals(n_fft, S, k0, c)
    P = R.spectrum(wave, n_fft, hop, torch.ones(n_fft))
    inner = R.interior_frames(S, n_fft, hop)
    assert len(inner) >= 2
    NC = n_fft // 2
    for row, (peak, value) in enumerate([(0, (c * n_fft) ** 2), (NC, (c * n_fft) ** 2), (k0, (n_fft / 2) ** 2)]):
        for t in inner:
            assert abs(P[row, t, peak].item() - value) < 1e-12 * value
            rest = torch.cat([P[row, t, :peak], P[row, t, peak + 1:]])
            assert rest.max().item() < 1e-20 * value
    picked = P[:, inner][:, :, R.analytic_bins(n_fft, k0)]
    expect = R.analytic_expected(n_fft, k0, c).unsqueeze(1).expand_as(picked)
    assert R.rel_err(picked, expect) < 1e-12


def test_frame_indices_reflect_at_both_ends():
    s = R.frame_indices(700, 1024, 320)                     # n_fft/2 < S < n_fft: frame 1 reflects at both ends
    assert s.shape == (3, 1024)
    assert s[1, 0].item() == 192 and s[1, 192].item() == 0 and s[1, 1023].item() == 2 * 699 - 831
    assert s[0, 0].item() == 512 and s[2, 1023].item() == 2 * 699 - (640 - 512 + 1023)
    s = R.frame_indices(513, 1024, 320)                     # the shortest clip torch.stft and the kernel accept
    assert s[0, 0].item() == 512 and s[1, 1023].item() == 2 * 512 - 831


def test_rel_err_and_db_check_notice():
    ref = torch.rand(2, 5, 4, dtype=torch.float64) + 0.5
    a = ref.clone()
    a[1, 2, 3] += 1e-3 * ref[1].max()
    assert abs(R.rel_err(a, ref) - 1e-3) < 1e-9
    ref[0] = 0.0
    with pytest.raises(AssertionError):
        R.rel_err(a, ref)                                   # a silent reference clip must be silent
    db = R.to_db(ref)
    assert R.db_check(db, ref)[:2] == (0.0, 0.0) and R.db_check(db, ref)[2] == 20
    db[0, 0, 0] = -99.99
    with pytest.raises(AssertionError):
        R.db_check(db, ref)
    assert R.bound_for(3e-7) == 5e-6 and R.bound_for(2e-6) == 8e-6


@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_filterbank_builders(n_fft):
    def band(col):
        nz = col.nonzero().flatten()
        return (int(nz[0]), int(nz[-1])) if nz.numel() else None
    w, NC = R.WCAP[n_fft], n_fft // 2
    fb = R.fb_dense(n_fft, 1)
    assert fb.shape == (NC + 1, 5) and bool((fb > 0).all()) and NC + 1 > w
    fb = R.fb_wcap_bands(n_fft, 2)
    widths = [band(fb[:, j])[1] - band(fb[:, j])[0] + 1 for j in range(3)]
    assert widths == [w, w + 1, w - 1] and band(fb[:, 2])[1] == NC
    fb = R.fb_holes(n_fft, 3)
    assert fb.shape[1] == 37 and band(fb[:, 11]) is None and band(fb[:, 23]) == (200, 259)
    assert bool((fb[215:231, 23] == 0).all()) and all(band(fb[:, j]) is not None for j in range(37) if j != 11)
    fb = R.fb_edge_columns(n_fft, 4)
    assert band(fb[:, 0]) == (0, 0) and band(fb[:, 63]) == (NC, NC) and fb.shape == (NC + 1, 64)
    groups = R.bin_groups(n_fft)
    assert len(groups) == NC // 64 + 1 and groups[-1] == [NC] and sum(groups, []) == list(range(NC + 1))
    hot = R.one_hot_fb(n_fft, groups[1])
    assert hot.shape == (NC + 1, 64) and hot.sum().item() == 64 and hot[64, 0] == 1 and hot[127, 63] == 1
    # the production tables never show the DC and Nyquist bins and never reach WCAP (why the sweep brings its own tables)
    for kind in ("cnn8rnn", "crnn"):
        p = O.FRONTEND[kind]
        if p["n_fft"] != n_fft:
            continue
        _, pfb = O.frontend_tables(kind)
        assert bool((pfb[0] == 0).all()) and bool((pfb[NC] == 0).all())
        assert max(band(pfb[:, j])[1] - band(pfb[:, j])[0] + 1 for j in range(64)) < w


@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_premises_of_the_db_rule(n_fft):
    """Measured on the fp64 reference alone, on the very inputs the sweep uses: what a dB comparison leaves out stays below 5 %
    for the per-bin spectrum of the DC + Nyquist + noise wave, for every filterbank shape, for the floor-and-range batch without
    its full-scale row, and for the short full-scale clip.  The full-scale row of the long batch is the exception the sweep
    documents: frames without the 65504 sample sit 1e-7 below the clip maximum, so most of that row is below the gate."""
    p = R.PARAMS[n_fft]
    hop = p["hop"]
    window, fb = O.frontend_tables(p["kind"])
    S = n_fft + 3 * hop + 1
    P = R.spectrum(R.dc_nyquist_wave(2, S, seed=3), n_fft, hop, window)
    _, left, _ = R.db_check(R.to_db(P), P)
    print(f"n_fft {n_fft}: left out per bin {left:.3%}")
    assert left < R.LEAVE_OUT_MAX
    P = R.spectrum(R.noise(2, 3333, seed=5), n_fft, hop, window)
    for name, tab in R.fb_cases(n_fft).items():
        M = P @ tab.double()
        _, left, zeros = R.db_check(R.to_db(M), M)
        print(f"n_fft {n_fft} fb {name}: left out {left:.3%}, exact zeros {zeros}")
        assert left < R.LEAVE_OUT_MAX and zeros == (M[..., 0].numel() if name == "holes37" else 0)
    batch = R.floor_range_batch(R.FLOOR_S, seed=7)
    M = R.mel_power(batch, n_fft, hop, window, fb)
    _, left_g, zeros = R.db_check(R.to_db(M[:3]), M[:3])
    _, left_full, _ = R.db_check(R.to_db(M[3:]), M[3:])
    Ms = R.mel_power(R.full_scale_short(n_fft, seed=8), n_fft, hop, window, fb)
    _, left_short, _ = R.db_check(R.to_db(Ms), Ms)
    print(f"n_fft {n_fft}: floor batch rows 0-2 left out {left_g:.3%} ({zeros} exact zeros), full-scale row {left_full:.1%}, "
          f"short full-scale clip {left_short:.3%}")
    assert left_g < R.LEAVE_OUT_MAX and left_short < R.LEAVE_OUT_MAX
    assert bool((M[1] == 0).all()) and zeros > M[1].numel()          # the zero tail of row 2 gives exact zeros too
    assert left_full > 0.5 and math.isfinite(M[3].max().item())
