"""Edge-shape sweep of the log-mel frontend kernel (csrc/logmel.hip: STFT, real-FFT unpack, mel projection, dB) against the fp64
restatement of tests/logmel_ref.py, which does not go through torch.stft (checked on the CPU by tests/test_logmel_ref_cpu.py).

Bounds (the rule of tests/test_gpu_text_rnn.py and tests/test_gpu_text_clap.py, unchanged): the power-domain error, relative to the
clip's largest fp64 entry, is below 5e-6 where the SAME restatement run in fp32 on the CPU deviates from fp64 by less than 1.25e-6,
else below 4 x that deviation (measured inside the test, never taken from the kernel).  dB is compared at 1e-3 dB where the
reference power exceeds 1e-4 of the clip maximum; entries whose fp64 power is exactly 0 must be exactly -100.0; what neither
covers may be at most 5 % of a case (asserted).  Every measured figure is printed.

Groups: a per-bin spectrum through one-hot filterbanks (DC and Nyquist on their own), b analytic known answers, c clip-length,
hop and window edges, d load paths / alignment / repeatability (bit equality), e filterbank shapes (bands at and beyond WCAP,
n_mels < 64, empty and holed columns), f more frames than the persistent grid holds, g floor and range, h refused arguments and
the table checks of ops.logmel.

The one exception to the 5 % rule is the full-scale row of g: its clip maximum comes from the frames that hold the single 65504
sample, every other frame sits 1e-7 below it and therefore below the dB gate (86 % / 91 % of the row, by construction of the
clip).  That row is held to the power bound, to finiteness and to row isolation; the dB rule with its 5 % is asserted on the three
other rows and on a SHORT full-scale clip in which every frame holds the 65504 sample (tests/logmel_ref.full_scale_short).

Worst measured on an MI355X (256 CUs), power error relative to the clip's largest fp64 entry, the CPU fp32 deviation of the same
case in brackets, then the largest dB difference and the share left out of the dB comparison (the full table, the planted-defect
runs and the findings are in docs/experiments_logmel_sweep.md):
  a  per-bin spectrum   n_fft 1024: 1.4e-7 [1.4e-7], 1.5e-5 dB, 3.5 %;  n_fft 2048: 1.9e-7 [1.9e-7], 1.4e-5 dB, 4.6 %
     DC / Nyquist bin alone   1024: 8.5e-8 [8.5e-8] / 1.6e-7 [1.6e-7];  2048: 1.3e-7 [1.3e-7] / 1.9e-7 [1.9e-7];  dB <= 4.4e-6
  b  closed forms       1.8e-7 [1.2e-7] / 6.0e-8 [1.2e-7], 5.5e-6 dB at the peaks
  c  lengths            cnn8rnn 2.3e-7 [1.0e-7] (S 1024), crnn 5.1e-7 [2.4e-7] (S 2048), hop / window 1.9e-7 [1.9e-7];  5.6e-6 dB, 0 %
  d  load paths         3.6e-7 [2.0e-7] (n_fft 2048, S 2001), 4.7e-6 dB, 0 %;  every equality bit for bit
  e  filterbank shapes  1.1e-6 [1.1e-6] (dense, n_fft 2048: the largest CPU deviation of the sweep, below 1.25e-6), 1.6e-5 dB, 0.26 %
  f  beyond the grid    3172 frames on 3072 (n_fft 1024): 2.4e-7 [2.1e-7], 1.0e-5 dB;  2196 on 2048 (n_fft 2048): 6.1e-7 [5.2e-7], 6.3e-6 dB;  0 %
  g  floor and range    rows 0-2 3.1e-7 [2.6e-7], 5.5e-6 dB, 3.0 %;  full-scale row 2.3e-7 [2.3e-7], 1.4e-5 dB, 85.7 % / 90.9 % (not asserted);
     short full-scale clip 3.6e-7 [3.6e-7], 1.8e-5 dB, 0 %
No arithmetic defect found.  Fixed with this sweep: the vector-load guard of logmel.hip tested the parity of the sample index, not the
alignment of the address; ops.logmel read window and fb as they lay (strides, shapes and dtype unchecked).
"""
import math

import pytest
import torch

from oracle import tag_oracle as O
from tests import logmel_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from texttoaudiogrounding_amd import ops as _ops
    return _ops


def _unaligned(t):
    """The same values in a view that is only 4-byte aligned (offset 1 of a flat buffer); tests/test_gpu_text_clap.py."""
    buf = torch.zeros(t.numel() + 1, device=t.device, dtype=t.dtype)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view_as(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def run(ops, dev, wave, n_fft, hop, window, fb):
    db, power = ops.logmel(wave.to(dev), n_fft, window.numel(), hop, window.to(dev), fb.to(dev), want_power=True)
    assert db.shape == power.shape == (wave.shape[0], wave.shape[1] // hop + 1, fb.shape[1])
    return db.cpu(), power.cpu()


def check(label, db, power, ref, ref32, leave_out_max=R.LEAVE_OUT_MAX):
    """The rule of the module docstring for one case; returns the measured figures."""
    dev32 = R.rel_err(ref32, ref)
    bound = R.bound_for(dev32)
    err = R.rel_err(power, ref)
    ddb, left, zeros = R.db_check(db, ref)
    print(f"LOGMEL {label}: power err {err:.2e} (CPU fp32 {dev32:.2e}, bound {bound:.1e}); dB {ddb:.2e}; left out {left:.3%}; "
          f"exact floor entries {zeros}")
    assert bool(torch.isfinite(power).all()) and bool(torch.isfinite(db).all())
    assert err < bound, (label, err, bound)
    assert ddb < R.DB_TOL, (label, ddb)
    assert left <= leave_out_max, (label, left)
    return err, dev32, ddb, left


def tables(n_fft):
    p = R.PARAMS[n_fft]
    window, fb = O.frontend_tables(p["kind"])
    return p["hop"], window, fb


# ------------------------------------------------------------------------------------------------ a. per-bin spectrum
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_a_spectrum_bin_by_bin(ops, dev, n_fft):
    hop, window, _ = tables(n_fft)
    NC = n_fft // 2
    S = n_fft + 3 * hop + 1
    wave = R.dc_nyquist_wave(2, S, seed=3)
    groups = R.bin_groups(n_fft)
    assert len(groups) == {1024: 9, 2048: 17}[n_fft] and groups[-1] == [NC]
    F = S // hop + 1
    P, DB = torch.zeros(2, F, NC + 1), torch.zeros(2, F, NC + 1)
    for bins in groups:
        db, power = run(ops, dev, wave, n_fft, hop, window, R.one_hot_fb(n_fft, bins))
        P[..., bins], DB[..., bins] = power, db
    ref = R.spectrum(wave, n_fft, hop, window)
    ref32 = R.spectrum(wave, n_fft, hop, window, torch.float32)
    check(f"a n_fft {n_fft} all bins", DB, P, ref, ref32)
    for name, k in (("DC", 0), ("Nyquist", NC)):             # each on its own scale: nothing may hide under another bin's maximum
        dev32 = R.rel_err(ref32[..., k], ref[..., k])
        err = R.rel_err(P[..., k], ref[..., k])
        ddb = (DB[..., k].double() - R.to_db(ref[..., k])).abs().max().item()
        print(f"LOGMEL a n_fft {n_fft} {name} bin alone: power err {err:.2e} (CPU fp32 {dev32:.2e}); dB {ddb:.2e}")
        assert err < R.bound_for(dev32) and ddb < R.DB_TOL
        assert ref[..., k].min() > 1e-2 * ref.amax()           # the 0.05 offsets make both bins strong in every frame


# ------------------------------------------------------------------------------------------------ b. analytic known answers
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_b_analytic_known_answers(ops, dev, n_fft):
    hop, k0, c = R.PARAMS[n_fft]["hop"], 37, 0.25
    S = n_fft + 3 * hop + 1
    wave64 = R.analytic_signals(n_fft, S, k0, c)
    wave = wave64.float()
    bins = R.analytic_bins(n_fft, k0)
    ones = torch.ones(n_fft)
    db, power = run(ops, dev, wave, n_fft, hop, ones, R.one_hot_fb(n_fft, bins))
    inner = R.interior_frames(S, n_fft, hop)
    assert len(inner) >= 2
    expect = R.analytic_expected(n_fft, k0, c).unsqueeze(1).expand(3, len(inner), 7)
    cpu32 = R.spectrum(wave, n_fft, hop, ones, torch.float32)[:, inner][:, :, bins]
    dev32 = R.rel_err(cpu32, expect)
    err = R.rel_err(power[:, inner], expect)
    peak = expect > 0
    ddb = (db[:, inner].double() - R.to_db(expect))[peak].abs().max().item()
    print(f"LOGMEL b n_fft {n_fft}: power err vs closed forms {err:.2e} (CPU fp32 {dev32:.2e}, bound {R.bound_for(dev32):.1e}); "
          f"dB at the peaks {ddb:.2e}")
    assert err < R.bound_for(dev32) and ddb < R.DB_TOL


# ------------------------------------------------------------------------------------------------ c. lengths, hops, windows
C_CASES = ([("cnn8rnn", S) for S in (513, 514, 640, 641, 959, 960, 1023, 1024, 1025, 3333)]
           + [("crnn", S) for S in (1025, 1281, 2047, 2048, 2049, 3333)])


@pytest.mark.parametrize("kind,S", C_CASES)
def test_c_clip_length_edges(ops, dev, kind, S):
    p = O.FRONTEND[kind]
    n_fft, hop = p["n_fft"], p["hop_length"]
    window, fb = O.frontend_tables(kind)
    wave = R.noise(3, S, seed=S)
    db, power = run(ops, dev, wave, n_fft, hop, window, fb)
    assert db.shape[1] == S // hop + 1
    check(f"c {kind} S {S}", db, power, R.mel_power(wave, n_fft, hop, window, fb),
          R.mel_power(wave, n_fft, hop, window, fb, torch.float32))


@pytest.mark.parametrize("hop,win_length,S", [(161, 1024, 2001), (320, 1023, 1500), (160, 401, 1500)])
def test_c_hop_and_window_edges(ops, dev, hop, win_length, S):
    window, fb = torch.hann_window(win_length), R.slaney_fb(1024)
    wave = R.noise(3, S, seed=S + hop)
    db, power = run(ops, dev, wave, 1024, hop, window, fb)
    assert db.shape[1] == S // hop + 1
    check(f"c hop {hop} win {win_length} S {S}", db, power, R.mel_power(wave, 1024, hop, window, fb),
          R.mel_power(wave, 1024, hop, window, fb, torch.float32))


# ------------------------------------------------------------------------------------------------ d. load paths give the same bits
@pytest.mark.parametrize("n_fft", [1024, 2048])
@pytest.mark.parametrize("S", [2001, 3333])
def test_d_load_paths_alignment_and_repeats(ops, dev, n_fft, S):
    hop, window, fb = tables(n_fft)
    wave = R.noise(3, S, seed=S + n_fft)
    wave[1] = wave[0]                       # odd S: interior frames of row 0 take the 8-byte loads, those of row 1 the scalar loads
    # (S 2001 at n_fft 2048 has no interior frame: S < n_fft, every frame reflects and takes the scalar loads in both rows)
    assert len(R.interior_frames(S, n_fft, hop)) >= (1 if S >= n_fft else 0)
    wd, win_d, fb_d = wave.to(dev), window.to(dev), fb.to(dev)
    assert wd.data_ptr() % 8 == 0
    args = (n_fft, window.numel(), hop, win_d, fb_d)
    db, power = ops.logmel(wd, *args, want_power=True)
    assert torch.equal(db[0], db[1]) and torch.equal(power[0], power[1])
    # the same batch where only 4-byte alignment holds: now row 1 is the 8-byte aligned one
    wu = _unaligned(wd)
    dbu, pu = ops.logmel(wu, *args, want_power=True)
    assert torch.equal(dbu, db) and torch.equal(pu, power)
    dbt, pt = ops.logmel(wd[1:], *args, want_power=True)     # batch[1:] of an odd-length batch: contiguous, base 4 mod 8
    assert wd[1:].data_ptr() % 8 == 4 and torch.equal(dbt, db[1:]) and torch.equal(pt, power[1:])
    db2, p2 = ops.logmel(wd, *args, want_power=True)
    assert torch.equal(db2, db) and torch.equal(p2, power)
    assert torch.equal(ops.logmel(wd, *args), db)
    check(f"d n_fft {n_fft} S {S}", db.cpu(), power.cpu(), R.mel_power(wave, n_fft, hop, window, fb),
          R.mel_power(wave, n_fft, hop, window, fb, torch.float32))


# ------------------------------------------------------------------------------------------------ e. filterbank shapes
@pytest.mark.parametrize("n_fft", [1024, 2048])
@pytest.mark.parametrize("name", ["dense5", "wcap", "holes37", "edges64"])
def test_e_filterbank_shapes(ops, dev, n_fft, name):
    hop, window, _ = tables(n_fft)
    fb = R.fb_cases(n_fft)[name]
    assert fb.shape[1] == {"dense5": 5, "wcap": 3, "holes37": 37, "edges64": 64}[name]
    wave = R.noise(2, 3333, seed=5)
    db, power = run(ops, dev, wave, n_fft, hop, window, fb)
    ref = R.spectrum(wave, n_fft, hop, window) @ fb.double()
    ref32 = R.spectrum(wave, n_fft, hop, window, torch.float32) @ fb
    check(f"e n_fft {n_fft} fb {name}", db, power, ref, ref32)
    if name == "holes37":
        assert bool((db[..., 11] == -100.0).all()) and bool((power[..., 11] == 0).all())


# ------------------------------------------------------------------------------------------------ f. beyond the persistent grid
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_f_more_frames_than_the_grid_holds(ops, dev, n_fft):
    hop, window, fb = tables(n_fft)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    grid_frames = {1024: 3 * cus * 4, 2048: cus * 8}[n_fft]           # workgroups per CU x CUs x waves (= frames) per workgroup
    S = {1024: 19201, 2048: 38407}[n_fft]
    B = math.ceil({1024: 52, 2048: 36}[n_fft] * cus / 256)
    F = S // hop + 1
    assert F == 61 and B * F > grid_frames, (cus, B, F, grid_frames)
    wave = R.noise(B, S, seed=n_fft + 1)
    db, power = run(ops, dev, wave, n_fft, hop, window, fb)
    print(f"LOGMEL f n_fft {n_fft}: {cus} CUs, grid holds {grid_frames} frames, launched B {B} x F {F} = {B * F}")
    check(f"f n_fft {n_fft}", db, power, R.mel_power(wave, n_fft, hop, window, fb),
          R.mel_power(wave, n_fft, hop, window, fb, torch.float32))
    dbl, pl = run(ops, dev, wave[B - 1:].clone(), n_fft, hop, window, fb)
    assert torch.equal(dbl[0], db[B - 1]) and torch.equal(pl[0], power[B - 1])


# ------------------------------------------------------------------------------------------------ g. floor and range
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_g_floor_and_range(ops, dev, n_fft):
    hop, window, fb = tables(n_fft)
    wave = R.floor_range_batch(R.FLOOR_S, seed=7)
    db, power = run(ops, dev, wave, n_fft, hop, window, fb)
    ref = R.mel_power(wave, n_fft, hop, window, fb)
    ref32 = R.mel_power(wave, n_fft, hop, window, fb, torch.float32)
    assert bool((ref[1] == 0).all()) and int((ref[2] == 0).all(dim=1).sum()) >= 3      # silent frames beyond the all-zero clip
    check(f"g n_fft {n_fft} rows 0-2", db[:3], power[:3], ref[:3], ref32[:3])
    assert bool((db[1] == -100.0).all()) and bool((power[1] == 0).all())
    # the full-scale row: see the module docstring for why its dB gate leaves most of it out
    check(f"g n_fft {n_fft} full-scale row", db[3:], power[3:], ref[3:], ref32[3:], leave_out_max=1.0)
    for b in range(4):                                       # no row is disturbed by its neighbours
        dbb, pb = run(ops, dev, wave[b:b + 1].clone(), n_fft, hop, window, fb)
        assert torch.equal(dbb[0], db[b]) and torch.equal(pb[0], power[b]), b
    short = R.full_scale_short(n_fft, seed=8)
    dbs, ps = run(ops, dev, short, n_fft, hop, window, fb)
    check(f"g n_fft {n_fft} short full-scale clip", dbs, ps, R.mel_power(short, n_fft, hop, window, fb),
          R.mel_power(short, n_fft, hop, window, fb, torch.float32))


# ------------------------------------------------------------------------------------------------ h. refused arguments, table checks
def test_h_refused_arguments(ops, dev):
    def call(S=4000, n_fft=1024, win_length=1024, hop=320, n_mels=64):
        return ops.logmel(torch.zeros(1, S, device=dev), n_fft, win_length, hop, torch.ones(win_length, device=dev),
                          torch.ones(n_fft // 2 + 1, n_mels, device=dev))
    assert call().shape == (1, 13, 64)
    assert call(S=513).shape == (1, 2, 64)
    for bad in (dict(S=512), dict(S=1024, n_fft=2048, win_length=1280, hop=640), dict(n_fft=512, win_length=512),
                dict(n_mels=65), dict(win_length=1025), dict(hop=0)):
        with pytest.raises(RuntimeError):
            call(**bad)
    torch.cuda.synchronize()


def test_h_tables_are_validated_and_made_contiguous(ops, dev):
    window, fb = O.frontend_tables("cnn8rnn")
    wave = R.noise(2, 3333, seed=9).to(dev)
    win_d, fb_d = window.to(dev), fb.to(dev)
    db, power = ops.logmel(wave, 1024, 1024, 320, win_d, fb_d, want_power=True)
    fb_t = fb_d.t().contiguous().t()                         # the same values, strides (1, 513)
    assert not fb_t.is_contiguous() and torch.equal(fb_t, fb_d)
    db_t, power_t = ops.logmel(wave, 1024, 1024, 320, win_d, fb_t, want_power=True)
    assert torch.equal(db_t, db) and torch.equal(power_t, power)
    win_s = torch.stack([win_d, win_d], 1)[:, 0]             # strided window
    assert not win_s.is_contiguous()
    assert torch.equal(ops.logmel(wave, 1024, 1024, 320, win_s, fb_d), db)
    for w, f, shape in ((win_d[:-1], fb_d, "(1023,)"), (win_d, fb_d[:-1], "(512, 64)"), (win_d, fb_d.t(), "(64, 513)"),
                        (win_d, fb_d[:, 0], "(513,)")):
        with pytest.raises(RuntimeError, match=shape.replace("(", r"\(").replace(")", r"\)")):
            ops.logmel(wave, 1024, 1024, 320, w, f)
    with pytest.raises(RuntimeError, match="float32"):
        ops.logmel(wave, 1024, 1024, 320, win_d, fb_d.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.logmel(wave, 1024, 1024, 320, win_d, fb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.logmel(wave, 1024, 1024, 320, window, fb_d)
