"""Plain restatement of the log-mel frontend (csrc/logmel.hip) that does NOT go through torch.stft: explicit frame
indices with the reflection written out, the window zero-padded by hand, torch.fft.rfft of the framed product, |X|^2,
the filterbank product and the dB clamp.  TEST INFRASTRUCTURE ONLY.

Run in float64 it is the reference of tests/test_gpu_logmel_sweep.py; run in float32 it is the "CPU deviation" that
test's bound rule needs.  tests/test_logmel_ref_cpu.py checks it against oracle.tag_oracle (torch.stft) and against
closed forms that depend on neither.  The case builders of the sweep live here too, so that the CPU test can check the
claims the sweep's bounds rest on (deviation of the fp32 restatement, share of entries left out of a dB comparison).
"""
import math

import torch

BOUND, DEV_LIMIT = 5e-6, 1.25e-6       # the rule of tests/test_gpu_text_rnn.py / test_gpu_text_clap.py
DB_TOL, DB_GATE, LEAVE_OUT_MAX = 1e-3, 1e-4, 0.05
WCAP = {1024: 96, 2048: 192}           # Plan<NFFT>::WCAP of csrc/logmel.hip (widest band held in LDS)
# clip length of the floor-and-range batch: odd, and long enough that the ONE frame of the zero-tailed clip whose window only
# grazes the signal (at n_fft 2048 its power is below 1e-4 of the clip maximum) is 1 / 33 of the three ordinary rows, not 1 / 18
FLOOR_S = 6401


def bound_for(dev32):
    return BOUND if dev32 < DEV_LIMIT else 4.0 * dev32


def frame_indices(S, n_fft, hop):
    """(F, n_fft) sample index of every frame position: t hop - n_fft/2 + n, reflected about 0 and about S - 1."""
    F = S // hop + 1
    s = torch.arange(F).unsqueeze(1) * hop - n_fft // 2 + torch.arange(n_fft).unsqueeze(0)
    s = s.abs()
    s = torch.where(s >= S, 2 * (S - 1) - s, s)
    assert int(s.min()) >= 0 and int(s.max()) < S, (S, n_fft, hop, int(s.min()), int(s.max()))
    return s


def padded_window(window, n_fft):
    win_length = window.numel()
    assert win_length <= n_fft
    left = (n_fft - win_length) // 2
    w = torch.zeros(n_fft, dtype=window.dtype)
    w[left:left + win_length] = window
    return w


def spectrum(wave, n_fft, hop, window, dtype=torch.float64):
    """(B, F, n_fft/2 + 1) power spectrum |X|^2 of every frame, computed in ``dtype``."""
    wave = wave.to(dtype)
    idx = frame_indices(wave.shape[1], n_fft, hop)
    frames = wave[:, idx] * padded_window(window.to(dtype), n_fft)          # (B, F, n_fft)
    X = torch.fft.rfft(frames, dim=-1)
    return X.real ** 2 + X.imag ** 2


def mel_power(wave, n_fft, hop, window, fb, dtype=torch.float64):
    """(B, F, n_mels) = spectrum @ fb in ``dtype``."""
    return spectrum(wave, n_fft, hop, window, dtype) @ fb.to(dtype)


def to_db(power):
    return 10.0 * torch.log10(torch.clamp(power, min=1e-10))


def rel_err(a, ref):
    """max over clips of (largest |a - ref| of the clip / the clip's largest |ref|); a clip whose reference is all zero must be
    all zero itself (then it contributes 0)."""
    a, ref = a.double().cpu(), ref.double().cpu()
    B = ref.shape[0]
    diff = (a - ref).abs().reshape(B, -1).amax(1)
    scale = ref.abs().reshape(B, -1).amax(1)
    dead = scale == 0
    assert bool((diff[dead] == 0).all()), "a clip whose reference is exactly zero is not exactly zero"
    return float((diff[~dead] / scale[~dead]).max()) if bool((~dead).any()) else 0.0


def db_check(db, ref_power):
    """The dB rule: entries whose reference power exceeds DB_GATE of the clip maximum are compared (-> largest difference in
    dB); entries whose reference power is exactly 0 must be exactly -100.0 (also counted as compared).  Returns (largest dB
    difference, share of the entries that neither comparison covers, number of exact-floor entries)."""
    db, ref_power = db.double().cpu(), ref_power.double().cpu()
    scale = ref_power.abs().amax(dim=tuple(range(1, ref_power.dim())), keepdim=True)
    big = ref_power > DB_GATE * scale
    zero = ref_power == 0
    assert bool((db[zero] == -100.0).all()), "an entry whose fp64 power is exactly 0 is not exactly -100.0 dB"
    ddb = float((db - to_db(ref_power))[big].abs().max()) if bool(big.any()) else 0.0
    left_out = 1.0 - float((big | zero).double().mean())
    return ddb, left_out, int(zero.sum())


# ------------------------------------------------------------------------------------------------ case builders
def noise(B, S, seed, amp=0.1):
    return amp * torch.randn(B, S, generator=torch.Generator().manual_seed(seed))


def one_hot_fb(n_fft, bins):
    """(n_fft/2 + 1, len(bins)) table whose column j selects spectrum bin bins[j]."""
    fb = torch.zeros(n_fft // 2 + 1, len(bins))
    for j, k in enumerate(bins):
        fb[k, j] = 1.0
    return fb


def bin_groups(n_fft):
    """groups of 64 consecutive bins; the last one is the Nyquist bin alone (n_mels = 1)."""
    nb = n_fft // 2 + 1
    return [list(range(k, min(k + 64, nb))) for k in range(0, nb, 64)]


def dc_nyquist_wave(B, S, seed):
    n = torch.arange(S)
    return noise(B, S, seed) + 0.05 + 0.05 * (1.0 - 2.0 * (n % 2).float())


def analytic_signals(n_fft, S, k0, c=0.25):
    """rows: constant c, c (-1)^n, cos(2 pi k0 n / n_fft)."""
    n = torch.arange(S, dtype=torch.float64)
    return torch.stack([torch.full((S,), c, dtype=torch.float64), c * (1.0 - 2.0 * (n % 2)),
                        torch.cos(2 * math.pi * k0 * n / n_fft)])


def analytic_bins(n_fft, k0):
    return [0, 1, k0 - 1, k0, k0 + 1, n_fft // 2 - 1, n_fft // 2]


def analytic_expected(n_fft, k0, c=0.25):
    """(3, 7) closed-form |X|^2 on analytic_bins for an interior frame under a window of ones."""
    e = torch.zeros(3, 7, dtype=torch.float64)
    e[0, 0] = (c * n_fft) ** 2
    e[1, 6] = (c * n_fft) ** 2
    e[2, 3] = (n_fft / 2) ** 2
    return e


def interior_frames(S, n_fft, hop):
    """frames that touch neither clip edge."""
    F = S // hop + 1
    return [t for t in range(F) if t * hop - n_fft // 2 >= 0 and t * hop + n_fft // 2 <= S]


def slaney_fb(n_fft, n_mels=64):
    from oracle import tag_oracle as O
    return O.melscale_fbanks(n_fft // 2 + 1, 50.0, 14000.0, n_mels, 32000, "slaney", "slaney")


def fb_dense(n_fft, seed):
    """n_mels = 5, every entry rand + 0.1: each band is the whole spectrum (wloop = WCAP and the tail loop)."""
    return torch.rand(n_fft // 2 + 1, 5, generator=torch.Generator().manual_seed(seed)) + 0.1


def fb_wcap_bands(n_fft, seed):
    """three columns whose bands hold exactly WCAP, WCAP + 1 and WCAP - 1 bins."""
    w = WCAP[n_fft]
    g = torch.Generator().manual_seed(seed)
    fb = torch.zeros(n_fft // 2 + 1, 3)
    for j, (lo, width) in enumerate([(7, w), (100, w + 1), (n_fft // 2 + 1 - (w - 1), w - 1)]):
        fb[lo:lo + width, j] = torch.rand(width, generator=g) + 0.1
    return fb


def fb_holes(n_fft, seed):
    """n_mels = 37: random bands of 3 .. 40 bins; column 11 is all zero, column 23 has zeros strictly inside its band."""
    g = torch.Generator().manual_seed(seed)
    nb = n_fft // 2 + 1
    fb = torch.zeros(nb, 37)
    for j in range(37):
        width = int(torch.randint(3, 41, (1,), generator=g))
        lo = int(torch.randint(0, nb - width, (1,), generator=g))
        fb[lo:lo + width, j] = torch.rand(width, generator=g) + 0.1
    fb[:, 11] = 0.0
    fb[:, 23] = 0.0
    fb[200:260, 23] = torch.rand(60, generator=g) + 0.1
    fb[215:231, 23] = 0.0
    return fb


def fb_edge_columns(n_fft, seed):
    """n_mels = 64 slaney-like table whose column 0 is non-zero only at bin 0 and column 63 only at bin n_fft/2."""
    fb = slaney_fb(n_fft).clone()
    top = fb.max().item()
    fb[:, 0] = 0.0
    fb[:, 63] = 0.0
    fb[0, 0] = 0.75 * top
    fb[n_fft // 2, 63] = 1.5 * top
    return fb


def fb_cases(n_fft):
    return {"dense5": fb_dense(n_fft, 21), "wcap": fb_wcap_bands(n_fft, 22), "holes37": fb_holes(n_fft, 23),
            "edges64": fb_edge_columns(n_fft, 24)}


PARAMS = {1024: dict(kind="cnn8rnn", hop=320, win_length=1024), 2048: dict(kind="crnn", hop=640, win_length=1280)}


def floor_range_batch(S, seed):
    """rows: a normal clip, an all-zero clip, a clip that is zero from sample 700 on, a full-scale clip (amplitude 1.0 plus one
    65504 sample, the largest float16)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(4, S)
    w[0] = 0.1 * torch.randn(S, generator=g)
    w[2, :700] = 0.1 * torch.randn(700, generator=g)
    w[3] = 2.0 * torch.rand(S, generator=g) - 1.0
    w[3, S // 2] = 65504.0
    return w


def full_scale_short(n_fft, seed):
    """A full-scale clip short enough that EVERY frame holds the 65504 sample well inside the window, so that the dB comparison
    sees all of it: S = 801 at n_fft 1024 / hop 320 / window 1024 (three frames, the sample at window positions 832, 512, 192)
    and S = 1201 at n_fft 2048 / hop 640 / window 1280 (two frames, the sample at positions 960 and 320 of the 1280)."""
    S = {1024: 801, 2048: 1201}[n_fft]
    g = torch.Generator().manual_seed(seed)
    w = (2.0 * torch.rand(1, S, generator=g) - 1.0)
    w[0, 320] = 65504.0
    return w
