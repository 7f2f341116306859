"""Functional wrappers over the C ABI of libtag_hip.so -- one Python function per kernel family, no autograd -- and the
DISPATCH RULES between kernel forms (direct / Winograd convolution, fused / two-pass epilogues, fp32 / bf16-MFMA arithmetics;
the switches live in settings.py).  Also what the per-kernel parity tests call.  PyTorch is plumbing here: device memory and
the current HIP stream; there is no eager fallback -- a CPU tensor or a missing library raises.
"""
from __future__ import annotations

import collections
import math
from typing import Optional

import torch

from . import settings as cfg
from .lib import call, ptr, query
from .engine import (F32, _chk, _empty, _timed, _ws)

# ------------------------------------------------------------------------------------------------
# thin functional wrappers (no autograd) -- also what the per-kernel parity tests call
# ------------------------------------------------------------------------------------------------

def waveform_f16_to_f32_padded(clips, device, length=None):
    """Ragged float16 clips (a list of 1-D numpy / torch float16 arrays, as WaveformStore.fetch_f16 returns them) ->
    (waveform (B,S) float32 zero-padded on ``device``, waveform_len (B,) int64 on ``device``), S = ``length`` or the longest
    clip.  The float16 samples are copied to the device back to back (half the bytes of the padded float32 batch the
    reference's collate function builds on the host) and widened + padded there (tag_waveform_f16_to_f32_padded)."""
    import numpy as np
    arrs = [c.numpy() if isinstance(c, torch.Tensor) else np.asarray(c) for c in clips]
    if any(a.dtype != np.float16 or a.ndim != 1 for a in arrs):
        raise RuntimeError("waveform_f16_to_f32_padded: clips must be 1-D float16 arrays (the pack's storage type)")
    lens = [a.shape[0] for a in arrs]
    S = int(length) if length is not None else max(lens)
    off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.long)
    packed = torch.from_numpy(np.concatenate(arrs) if len(arrs) > 1 else arrs[0].copy())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("waveform_f16_to_f32_padded: the target must be the MI355X (cuda) device; no CPU fallback")
    packed_d, off_d = packed.to(dev, non_blocking=True), off.to(dev, non_blocking=True)
    out = torch.empty(len(arrs), S, device=dev, dtype=F32)
    lens_d = torch.empty(len(arrs), device=dev, dtype=torch.long)
    call("tag_waveform_f16_to_f32_padded", ptr(packed_d), ptr(off_d), len(arrs), S, ptr(out), ptr(lens_d))
    return out, lens_d


def logmel(wave, n_fft, win_length, hop, window, fb, want_power=False):
    wave = _chk(wave, "waveform")
    window, fb = _chk(window, "window"), _chk(fb, "fb")      # the kernel reads both as dense row-major tables
    if wave.dim() != 2:
        raise RuntimeError(f"logmel: waveform must be (B, S), got {tuple(wave.shape)}")
    if window.numel() != win_length:
        raise RuntimeError(f"logmel: window must hold win_length = {win_length} values, got {tuple(window.shape)}")
    if fb.dim() != 2 or fb.shape[0] != n_fft // 2 + 1:
        raise RuntimeError(f"logmel: fb must be (n_fft // 2 + 1, n_mels) = ({n_fft // 2 + 1}, n_mels), got {tuple(fb.shape)}")
    if hop <= 0:
        raise RuntimeError(f"logmel: hop must be positive, got {hop}")
    B, S = wave.shape
    Fr = S // hop + 1
    n_mels = fb.shape[1]
    out = _empty(B, Fr, n_mels, like=wave)
    power = _empty(B, Fr, n_mels, like=wave) if want_power else None
    call("tag_logmel_forward", ptr(wave), B, S, n_fft, win_length, hop, ptr(window), ptr(fb), n_mels, ptr(out),
         ptr(power))
    return (out, power) if want_power else out


class BNStat:
    """Per-channel statistics / fused affine of one BatchNorm application."""
    __slots__ = ("mean", "invstd", "scale", "shift", "train")


def bn_stats(x2d, gamma, beta, running_mean, running_var, training, eps=1e-5, momentum=0.1, pre_op=0,
             partials=None) -> BNStat:
    """x2d: (rows, C) view of a channels-last tensor.  partials = (P, buffer) from conv3x3(..., want_stats=True): the batch
    statistics come from the conv kernel's epilogue instead of another pass over x2d."""
    rows, C = x2d.shape
    st = BNStat()
    st.train = bool(training)
    st.scale = _empty(C, like=x2d)
    st.shift = _empty(C, like=x2d)
    if training:
        st.mean = _empty(C, like=x2d)
        st.invstd = _empty(C, like=x2d)
        if x2d.dtype != F32 and not (partials is not None and pre_op == 0):
            raise RuntimeError("bf16 activations: BatchNorm batch statistics come from the producing conv kernel's epilogue")
        if partials is not None and pre_op == 0:
            ws = _ws(query("tag_bn_stats_from_partials_ws_bytes", partials[0], C), x2d)
            call("tag_bn_stats_from_partials", ptr(partials[1]), partials[0], C, ptr(gamma), ptr(beta), eps, momentum,
                 ptr(running_mean), ptr(running_var), ptr(st.mean), ptr(st.invstd), ptr(st.scale), ptr(st.shift), ptr(ws))
        else:
            ws = _ws(query("tag_bn_stats_ws_bytes", rows, C), x2d)
            call("tag_bn_stats", ptr(x2d), rows, C, pre_op, ptr(gamma), ptr(beta), eps, momentum, ptr(running_mean),
                 ptr(running_var), ptr(st.mean), ptr(st.invstd), ptr(st.scale), ptr(st.shift), ptr(ws))
    else:
        call("tag_bn_eval_affine", ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), eps, C, ptr(st.scale),
             ptr(st.shift))
        st.mean = running_mean
        st.invstd = _empty(C, like=x2d)
        dummy = _empty(C, like=x2d)
        call("tag_bn_eval_affine", None, None, ptr(running_mean), ptr(running_var), eps, C, ptr(st.invstd), ptr(dummy))
    return st


def _dg_db(dg_out, db_out, C, like):
    """The (dgamma, dbeta) destinations of a BatchNorm backward: the caller's flat-gradient views, or fresh (C,) tensors."""
    return (dg_out if dg_out is not None else _empty(C, like=like)), (db_out if db_out is not None else _empty(C, like=like))


_X3_PRODUCTS = {"x3": 6, "x9": 9, "bf16": 1}
BF16 = torch.bfloat16


def gemm_bf16() -> bool:
    return cfg.GEMM_MATH == "bf16" or (cfg.GEMM_MATH == "auto" and cfg.ACT_DTYPE == "bf16")


def act_bf16() -> bool:
    return cfg.CONV_MATH == "bf16" and cfg.ACT_DTYPE == "bf16"


def _sfx(t) -> str:
    """Entry-point suffix for an activation tensor: '' (fp32) or '_bf16'."""
    return "_bf16" if t.dtype == BF16 else ""


def _x3_ok(W, K, N):
    return cfg.CONV_MATH in _X3_PRODUCTS and W in (8, 16, 32, 64) and K % 32 == 0 and N % 64 == 0


class _X3Pack:
    """Weight pack of the bf16-MFMA kernels: the byte blob + the product count it was made for."""
    dtype = torch.uint8

    def __init__(self, blob, products):
        self.blob, self.products = blob, products


def pack_conv_weight(w, want_dgrad=True, W=None):
    """(Cout,Cin,3,3) -> (forward pack, dgrad pack).  A pack is fp32 (9,K,N) for the exact kernels or a uint8 blob of
    pre-split bf16 fragments for the x3 kernels (when CONV_MATH == "x3" and the layer shape allows it)."""
    Cout, Cin = w.shape[0], w.shape[1]
    fx3, dx3 = _x3_ok(W, Cin, Cout), want_dgrad and _x3_ok(W, Cout, Cin)
    wf = wd = None
    if fx3 or dx3:
        nbytes = query("tag_conv3x3_x3_pack_bytes", Cin, Cout)
        xf = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        xd = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        npr = _X3_PRODUCTS[cfg.CONV_MATH]
        call("tag_pack_conv_weight_x3", ptr(w), ptr(xf), ptr(xd), Cin, Cout, npr)
        wf, wd = (_X3Pack(xf, npr) if fx3 else None), (_X3Pack(xd, npr) if dx3 else None)
    if wf is None or (want_dgrad and wd is None):
        pf = _empty(9, Cin, Cout, like=w)
        pd = _empty(9, Cout, Cin, like=w) if want_dgrad else None
        call("tag_pack_conv_weight", ptr(w), ptr(pf), ptr(pd), Cin, Cout)
        wf = pf if wf is None else wf
        wd = pd if wd is None else wd
        if W is not None and _wino_shape(W, Cin, Cout) and wf is pf and (not want_dgrad or wd is pd):
            # the direct packs stay what they are (inference, pool-sum epilogues, fallbacks); the Winograd-domain weights ride along
            uf = _empty(16, Cin, Cout, like=w)
            ud = _empty(16, Cout, Cin, like=w) if want_dgrad else None
            call("tag_pack_conv_weight_wino", ptr(w), ptr(uf), ptr(ud), Cin, Cout)
            pf.wino_u = uf
            if want_dgrad:
                pd.wino_u = ud
    return wf, (wd if want_dgrad else None)


def _wino_shape(W, Cin, Cout) -> bool:
    return (cfg.CONV_WINOGRAD and cfg.CONV_MATH == "fp32" and W in (8, 16, 32, 64) and min(Cin, Cout) >= cfg.WINO_MIN_C
            and max(Cin, Cout) >= cfg.WINO_MIN_CMAX)


def _wino_flop(B, H, W, Cin, Cout) -> float:
    """FLOP a Winograd launch EXECUTES on the matrix pipe (16 products of T x Cin x Cout; bench.py's roofline counts these, not the
    2.25 x larger direct-convolution figure)."""
    return 2.0 * 16 * B * ((H + 1) // 2) * ((W + 1) // 2) * Cin * Cout


def _wino_u(wpack, x, Cout, count=True, any_size=False):
    """The Winograd-domain weights riding on a direct pack (pack_conv_weight) when this launch may use them, else None.
    any_size: the inference forward -- no tile threshold (see CONV_WINOGRAD_EVAL)."""
    u = getattr(wpack, "wino_u", None)
    if u is None or not cfg.CONV_WINOGRAD or cfg.CONV_MATH != "fp32" or x.dtype != F32:
        return None
    B, H, W, Cin = x.shape
    if any_size and not cfg.CONV_WINOGRAD_EVAL:
        return None
    if ((not any_size and B * ((H + 1) // 2) * ((W + 1) // 2) * Cout < cfg.WINO_MIN_WORK)
            or not query("tag_conv3x3_wino_ok", 1 if any_size else B, H, W, Cin, Cout)):     # (inference launches are cut by batch)
        return None
    if count:
        cfg.WINO_LAUNCHES += 1
    return u


def conv3x3(x, wpack, Cout, prologue=0, scale=None, shift=None, training_launch=False):
    """y = conv(prologue(x)).  training_launch: a launch of the training step (a dgrad conv): may take the Winograd form."""
    return conv3x3_stats(x, wpack, Cout, prologue, scale, shift, want_stats=False, training_launch=training_launch)[0]


def _batch_chunks(B, bytes_per_clip):
    """Batch slices [b0, b1) whose tensors stay under WINO_MAX_BYTES (the fused Winograd kernels' descriptor range)."""
    nb = max(1, min(B, cfg.WINO_MAX_BYTES // max(1, bytes_per_clip)))
    return [(b0, min(B, b0 + nb)) for b0 in range(0, B, nb)]


def conv3x3_stats(x, wpack, Cout, prologue=0, scale=None, shift=None, want_stats=True, training_launch=False, inference=False):
    """(y, partials): y = conv(prologue(x)) and, when want_stats, the BatchNorm partial statistics of y that the kernel
    writes in its epilogue ((P, buffer), or None when this shape has no fused statistics) -> bn_stats(..., partials=...)."""
    B, H, W, Cin = x.shape
    y = _empty(B, H, W, Cout, like=x, dtype=x.dtype)
    x3 = wpack.dtype == torch.uint8
    part = None
    u = None
    if not x3 and inference and not want_stats:
        u = _wino_u(wpack, x, Cout, any_size=True)
        if u is not None:                      # inference forward: batch cuts keep every tensor inside the descriptor range
            for b0, b1 in _batch_chunks(B, H * W * max(Cin, Cout) * 4):
                ws = _ws(query("tag_conv3x3_wino_ws_bytes", b1 - b0, H, W, Cin, Cout), x)
                with _timed(("conv3x3_wino", b1 - b0, H, W, Cin, Cout), _wino_flop(b1 - b0, H, W, Cin, Cout)):
                    call("tag_conv3x3_wino_forward", ptr(x[b0:b1]), ptr(u), prologue, ptr(scale), ptr(shift), ptr(y[b0:b1]), None,
                         b1 - b0, H, W, Cin, Cout, ptr(ws), None)
            return y, None
    elif ((want_stats and cfg.FUSE_BN_STATS) or training_launch) and not x3:
        u = _wino_u(wpack, x, Cout)
    if u is not None:
        if want_stats and cfg.FUSE_BN_STATS:
            P = query("tag_conv3x3_wino_stats_rows", B, H, W, Cout)
            part = (P, _empty(P * (3 * Cout + 1), like=x))
        ws = _ws(query("tag_conv3x3_wino_ws_bytes", B, H, W, Cin, Cout), x)
        with _timed(("conv3x3_wino", B, H, W, Cin, Cout), _wino_flop(B, H, W, Cin, Cout)):
            call("tag_conv3x3_wino_forward", ptr(x), ptr(u), prologue, ptr(scale), ptr(shift), ptr(y), ptr(part[1]) if part else None,
                 B, H, W, Cin, Cout, ptr(ws), None)
        return y, part
    if want_stats and cfg.FUSE_BN_STATS:
        if x3 and x.dtype == BF16:
            P = query("tag_conv3x3_x3_bf16_stats_rows", B, H, W, Cin, Cout, prologue)
        else:
            P = query("tag_conv3x3_x3_stats_rows" if x3 else "tag_conv3x3_stats_rows", B, H, W, Cout)
        if P > 0:
            part = (P, _empty(P * (3 * Cout + 1), like=x))
    sp = ptr(part[1]) if part else None
    if x.dtype == BF16:
        if not (x3 and wpack.products == 1):
            raise RuntimeError("bf16 activations need the one-product bf16 conv kernels (CONV_MATH='bf16') and an image width "
                               "of 8/16/32/64")
        with _timed(("conv3x3_x3_kernel", B, H, W, Cin, Cout), 2.0 * B * H * W * 9 * Cin * Cout):
            call("tag_conv3x3_forward_x3_bf16", ptr(x), ptr(wpack.blob), prologue, ptr(scale), ptr(shift), ptr(y), sp, B, H,
                 W, Cin, Cout)
    elif x3:
        with _timed(("conv3x3_x3_kernel", B, H, W, Cin, Cout), 2.0 * B * H * W * 9 * Cin * Cout):
            call("tag_conv3x3_forward_x3", ptr(x), ptr(wpack.blob), prologue, ptr(scale), ptr(shift), ptr(y), sp, B, H, W,
                 Cin, Cout, wpack.products)
    else:
        kname = "conv3x3_halo_kernel" if W in (4, 8, 16, 32, 64) else "conv3x3_fwd_kernel"   # dispatch rule of the C side
        with _timed((kname, B, H, W, Cin, Cout), 2.0 * B * H * W * 9 * Cin * Cout):
            call("tag_conv3x3_forward", ptr(x), ptr(wpack), prologue, ptr(scale), ptr(shift), ptr(y), sp, B, H, W, Cin,
                 Cout)
    return y, part


def conv3x3_dgrad_bnrelu_backward(dy_in, wpack, yref, st: BNStat, gamma, dg_out=None, db_out=None, after_conv=None,
                                  defer_apply=False):
    """The dgrad convolution da = conv(dy_in, wpack) followed by the backward of relu(bn(yref)):
    returns (dy_ref, dgamma, dbeta) with dy_ref = dL/d yref (written in place over da).  Exact-fp32 halo-tile shapes
    fold the per-channel sums into the conv epilogue; other shapes / arithmetics run the conv and tag_bnrelu_backward.
    defer_apply: a 4-tuple (t, dgamma, dbeta, applied) comes back; on the fused paths applied is False and t is still da --
    the caller's next kernel applies the BatchNorm + ReLU backward itself (conv3x3_c1_backward(bn_bwd=...))."""
    B, H, W, Cin = dy_in.shape
    C = yref.shape[3]
    fused = (cfg.FUSE_BN_BWD_SUMS and wpack.dtype != torch.uint8 and st.train and W in (8, 16, 32, 64)
             and query("tag_conv3x3_stats_rows", B, H, W, C) > 0)
    if (cfg.FUSE_BN_BWD_SUMS and dy_in.dtype == BF16 and wpack.dtype == torch.uint8 and wpack.products == 1 and st.train
            and yref.dtype == BF16 and W in (8, 16, 32, 64)):
        # BASELINE configs[2] mode: the same fusion on the one-product bf16 kernels (sums from the fp32 accumulators)
        P = query("tag_conv3x3_x3_bf16_stats_rows", B, H, W, Cin, C, 0)
        da = _empty(B, H, W, C, like=dy_in, dtype=BF16)
        part = _empty(P * 2 * C, like=dy_in)
        with _timed(("conv3x3_x3_kernel", B, H, W, Cin, C), 2.0 * B * H * W * 9 * Cin * C):
            call("tag_conv3x3_dgrad_bnsums_bf16", ptr(dy_in), ptr(wpack.blob), ptr(da), ptr(yref), ptr(st.scale), ptr(st.shift),
                 ptr(st.mean), ptr(st.invstd), ptr(part), B, H, W, Cin, C)
        if after_conv is not None:
            after_conv()
        dg, db = _dg_db(dg_out, db_out, C, da)
        ws = _ws(query("tag_bn_grad_from_partials_ws_bytes", P, C), da)
        call("tag_bn_grad_from_partials", ptr(part), P, C, ptr(dg), ptr(db), ptr(ws))
        if defer_apply:
            return da, dg, db, False
        call("tag_bnrelu_backward_apply_bf16", ptr(yref), ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.invstd),
             ptr(gamma), ptr(da), ptr(da), ptr(dg), ptr(db), B * H * W, C, int(st.train))
        return da, dg, db
    if not fused:
        da = conv3x3(dy_in, wpack, C)
        if after_conv is not None:
            after_conv()
        res = bnrelu_backward(yref, st, gamma, da, dg_out=dg_out, db_out=db_out)
        return (*res, True) if defer_apply else res
    u = _wino_u(wpack, dy_in, C)
    da = _empty(B, H, W, C, like=dy_in)
    if u is not None:
        P = query("tag_conv3x3_wino_stats_rows", B, H, W, C)
        part = _empty(P * 2 * C, like=dy_in)
        ws = _ws(query("tag_conv3x3_wino_ws_bytes", B, H, W, Cin, C), dy_in)
        with _timed(("conv3x3_wino", B, H, W, Cin, C), _wino_flop(B, H, W, Cin, C)):
            call("tag_conv3x3_wino_dgrad_bnsums", ptr(dy_in), ptr(u), ptr(da), ptr(yref), ptr(st.scale), ptr(st.shift),
                 ptr(st.mean), ptr(st.invstd), ptr(part), B, H, W, Cin, C, ptr(ws))
    else:
        P = query("tag_conv3x3_stats_rows", B, H, W, C)
        part = _empty(P * 2 * C, like=dy_in)
        with _timed(("conv3x3_halo_kernel", B, H, W, Cin, C), 2.0 * B * H * W * 9 * Cin * C):
            call("tag_conv3x3_dgrad_bnsums", ptr(dy_in), ptr(wpack), ptr(da), ptr(yref), ptr(st.scale), ptr(st.shift),
                 ptr(st.mean), ptr(st.invstd), ptr(part), B, H, W, Cin, C)
    if after_conv is not None:
        after_conv()
    dg, db = _dg_db(dg_out, db_out, C, da)
    ws = _ws(query("tag_bn_grad_from_partials_ws_bytes", P, C), da)
    call("tag_bn_grad_from_partials", ptr(part), P, C, ptr(dg), ptr(db), ptr(ws))
    if defer_apply:
        return da, dg, db, False
    rows = B * H * W
    call("tag_bnrelu_backward_apply", ptr(yref), ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.invstd), ptr(gamma),
         ptr(da), ptr(da), ptr(dg), ptr(db), rows, C, int(st.train))
    return da, dg, db


def pool_sums_fusable(dy_in, wpack, yref, ph, pw):
    """Can the dgrad conv of (dy_in, wpack) carry the pool-backward sums of the block below (raw output yref, window ph x pw)?
    Exact-fp32 halo-tile shapes, windows 1x2 / 2x2."""
    B, H, W, Cin = dy_in.shape
    if not (cfg.FUSE_POOL_BWD_SUMS and W in (8, 16, 32, 64) and pw == 2 and ph in (1, 2) and H == yref.shape[1] // ph
            and W == yref.shape[2] // pw):
        return False
    if dy_in.dtype == BF16:       # BASELINE configs[2] mode: the one-product bf16 tile kernel with the staged output tile
        return (cfg.FUSE_POOL_BWD_SUMS_BF16 and yref.dtype == BF16 and wpack.dtype == torch.uint8 and getattr(wpack, "products", 0) == 1
                and query("tag_conv3x3_dgrad_poolsums_bf16_rows", B, H, W, Cin, yref.shape[3]) > 0)
    return (dy_in.dtype == F32 and yref.dtype == F32 and wpack.dtype != torch.uint8
            and query("tag_conv3x3_stats_rows", B, H, W, yref.shape[3]) > 0)


def conv3x3_dgrad_poolsums(dy_in, wpack, yref, st: BNStat, ph, pw, drop_p=0.0, seed=0, pool=0):
    """dx = conv(dy_in, wpack) -- the gradient of the pooled (and dropped-out) output of the block whose second conv produced
    yref -- and, from the conv's epilogue, the partial sums (P, buffer) of that block's BatchNorm+ReLU+pool backward
    -> bnrelu_pool_backward(..., partials=...)."""
    B, H, W, Cin = dy_in.shape
    _, Hf, Wf, C = yref.shape
    if dy_in.dtype == BF16:
        P = query("tag_conv3x3_dgrad_poolsums_bf16_rows", B, H, W, Cin, C)
        dx = _empty(B, H, W, C, like=dy_in, dtype=BF16)
        part = _empty(P * 2 * C, like=dy_in)
        with _timed(("conv3x3_x3_kernel", B, H, W, Cin, C), 2.0 * B * H * W * 9 * Cin * C):
            call("tag_conv3x3_dgrad_poolsums_bf16", ptr(dy_in), ptr(wpack.blob), ptr(dx), ptr(yref), ptr(st.scale), ptr(st.shift),
                 ptr(st.mean), ptr(st.invstd), ptr(part), B, H, W, Cin, C, Hf, Wf, ph, pw, int(pool), float(drop_p), seed)
        return dx, (P, part)
    u = _wino_u(wpack, dy_in, C)
    if u is not None:                  # Winograd dgrad: the sums come from its output transform (conv_wino.hip, EPI == 2)
        P = query("tag_conv3x3_wino_stats_rows", B, H, W, C)
        dx = _empty(B, H, W, C, like=dy_in)
        part = _empty(P * 2 * C, like=dy_in)
        ws = _ws(query("tag_conv3x3_wino_ws_bytes", B, H, W, Cin, C), dy_in)
        with _timed(("conv3x3_wino", B, H, W, Cin, C), _wino_flop(B, H, W, Cin, C)):
            call("tag_conv3x3_wino_dgrad_poolsums", ptr(dy_in), ptr(u), ptr(dx), ptr(yref), ptr(st.scale), ptr(st.shift), ptr(st.mean),
                 ptr(st.invstd), ptr(part), B, H, W, Cin, C, Hf, Wf, ph, pw, int(pool), float(drop_p), seed, ptr(ws))
        return dx, (P, part)
    P = query("tag_conv3x3_stats_rows", B, H, W, C)
    dx = _empty(B, H, W, C, like=dy_in)
    part = _empty(P * 2 * C, like=dy_in)
    with _timed(("conv3x3_halo_kernel", B, H, W, Cin, C), 2.0 * B * H * W * 9 * Cin * C):
        call("tag_conv3x3_dgrad_poolsums", ptr(dy_in), ptr(wpack), ptr(dx), ptr(yref), ptr(st.scale), ptr(st.shift), ptr(st.mean),
             ptr(st.invstd), ptr(part), B, H, W, Cin, C, Hf, Wf, ph, pw, int(pool), float(drop_p), seed)
    return dx, (P, part)


def eval_pool_fusable(x, wpack, ph, pw, pool=0):
    """Exact-fp32 halo-tile shapes, windows 1x2 / 2x2, the three pool types."""
    B, H, W, _ = x.shape
    return (cfg.FUSE_EVAL_POOL and x.dtype == F32 and wpack.dtype != torch.uint8 and W in (8, 16, 32, 64) and pw == 2 and ph in (1, 2)
            and H // ph > 0 and pool in (0, 2, 3) and query("tag_conv3x3_stats_rows", B, H, W, 64) > 0)


def conv3x3_bnrelu_pool_eval(x, wpack, Cout, st: BNStat, ph, pw, prologue=0, scale=None, shift=None, pool=0):
    """pool(relu(bn_eval(conv(prologue(x))))) in ONE kernel: nothing of the (B,H,W,Cout) conv output touches HBM."""
    B, H, W, Cin = x.shape
    out = _empty(B, H // ph, W // pw, Cout, like=x)
    u = _wino_u(wpack, x, Cout, any_size=True)
    if u is not None:
        for b0, b1 in _batch_chunks(B, H * W * max(Cin, Cout) * 4):
            ws = _ws(query("tag_conv3x3_wino_ws_bytes", b1 - b0, H, W, Cin, Cout), x)
            with _timed(("conv3x3_wino", b1 - b0, H, W, Cin, Cout), _wino_flop(b1 - b0, H, W, Cin, Cout)):
                call("tag_conv3x3_wino_forward_bnrelu_pool_eval", ptr(x[b0:b1]), ptr(u), prologue, ptr(scale), ptr(shift),
                     ptr(out[b0:b1]), ptr(st.scale), ptr(st.shift), b1 - b0, H, W, Cin, Cout, ph, pw, int(pool), ptr(ws))
        return out
    with _timed(("conv3x3_halo_kernel", B, H, W, Cin, Cout), 2.0 * B * H * W * 9 * Cin * Cout):
        call("tag_conv3x3_forward_bnrelu_pool_eval", ptr(x), ptr(wpack), prologue, ptr(scale), ptr(shift), ptr(out), ptr(st.scale),
             ptr(st.shift), B, H, W, Cin, Cout, ph, pw, int(pool))
    return out


def conv3x3_wgrad(x, dy, prologue=0, scale=None, shift=None, out=None):
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    dw = out if out is not None else _empty(Cout, Cin, 3, 3, like=x)
    if x.dtype == BF16:
        if dy.dtype != BF16 or not (W in (8, 16, 32, 64) and Cin % 64 == 0 and Cout % 64 == 0):
            raise RuntimeError("bf16 wgrad: both operands must be bf16, width 8/16/32/64, channels multiples of 64")
        ws = _ws(query("tag_conv3x3_wgrad_x3_ws_bytes", B, H, W, Cin, Cout), x)
        with _timed(("conv3x3_wgrad_x3_kernel", B, H, W, Cin, Cout), 2.0 * B * H * W * 9 * Cin * Cout):
            call("tag_conv3x3_wgrad_x3_bf16", ptr(x), prologue, ptr(scale), ptr(shift), ptr(dy), ptr(dw), B, H, W, Cin, Cout,
                 ptr(ws))
        return dw
    if cfg.CONV_MATH in _X3_PRODUCTS and W in (8, 16, 32, 64) and Cin % 64 == 0 and Cout % 64 == 0:
        ws = _ws(query("tag_conv3x3_wgrad_x3_ws_bytes", B, H, W, Cin, Cout), x)
        with _timed(("conv3x3_wgrad_x3_kernel", B, H, W, Cin, Cout), 2.0 * B * H * W * 9 * Cin * Cout):
            call("tag_conv3x3_wgrad_x3", ptr(x), prologue, ptr(scale), ptr(shift), ptr(dy), ptr(dw), B, H, W, Cin, Cout,
                 _X3_PRODUCTS[cfg.CONV_MATH], ptr(ws))
        return dw
    if (x.dtype == F32 and dy.dtype == F32 and _wino_shape(W, Cin, Cout)
            and B * ((H + 1) // 2) * ((W + 1) // 2) * max(Cin, Cout) >= cfg.WINO_MIN_WORK and query("tag_conv3x3_wino_ok", B, H, W, Cin, Cout)):
        cfg.WINO_LAUNCHES += 1
        ws = _ws(query("tag_conv3x3_wino_wgrad_ws_bytes", B, H, W, Cin, Cout), x)
        with _timed(("conv3x3_wino_wgrad", B, H, W, Cin, Cout), _wino_flop(B, H, W, Cin, Cout)):
            call("tag_conv3x3_wino_wgrad", ptr(x), prologue, ptr(scale), ptr(shift), ptr(dy), ptr(dw), B, H, W, Cin, Cout, ptr(ws),
                 None)
        return dw
    ws = _ws(query("tag_conv3x3_wgrad_ws_bytes", B, H, W, Cin, Cout), x)
    # profile family: the all-taps decomposition (conv3x3_wgrad_alltaps_kernel at W = 8 / 16, its row-ring form
    # conv3x3_wgrad_rowring_kernel at W = 32 / 64) or the per-tap fallback
    kname = "conv3x3_wgrad_alltaps_kernel" if W in (8, 16, 32, 64) else "conv3x3_wgrad_kernel"
    with _timed((kname, B, H, W, Cin, Cout), 2.0 * B * H * W * 9 * Cin * Cout):
        call("tag_conv3x3_wgrad", ptr(x), prologue, ptr(scale), ptr(shift), ptr(dy), ptr(dw), B, H, W, Cin, Cout,
             ptr(ws))
    return dw


def conv3x3_c1(x, w, col_scale=None, col_shift=None):
    return conv3x3_c1_stats(x, w, col_scale, col_shift, want_stats=False)[0]


def conv3x3_c1_stats(x, w, col_scale=None, col_shift=None, want_stats=True, out_dtype=F32):
    """(y, partials) of the Cin = 1 convolution; partials = (P, buffer) when the kernel wrote the BatchNorm statistics of
    y itself (W == 64, Cout == 64), else None.  out_dtype bf16: y stored as bf16 (statistics from the fp32 values)."""
    B, H, W = x.shape
    Cout = w.shape[0]
    y = _empty(B, H, W, Cout, like=x, dtype=out_dtype)
    if out_dtype == BF16:
        P = query("tag_conv3x3_c1_stats_rows", B, H, W, Cout)
        if P <= 0:
            raise RuntimeError("bf16 activations: the Cin = 1 convolution is implemented for 64 mel bins x 64 channels")
        part = (P, _empty(P * (3 * Cout + 1), like=x)) if want_stats else None
        call("tag_conv3x3_c1_forward_stats_bf16", ptr(x), ptr(col_scale), ptr(col_shift), ptr(w), ptr(y),
             ptr(part[1]) if part else None, B, H, W, Cout)
        return y, part
    P = query("tag_conv3x3_c1_stats_rows", B, H, W, Cout) if (want_stats and cfg.FUSE_BN_STATS) else 0
    if P > 0:
        part = (P, _empty(P * (3 * Cout + 1), like=x))
        call("tag_conv3x3_c1_forward_stats", ptr(x), ptr(col_scale), ptr(col_shift), ptr(w), ptr(y), ptr(part[1]), B, H, W,
             Cout)
        return y, part
    call("tag_conv3x3_c1_forward", ptr(x), ptr(col_scale), ptr(col_shift), ptr(w), ptr(y), B, H, W, Cout)
    return y, None


def conv3x3_c1_wgrad(x, dy, col_scale=None, col_shift=None, out=None):
    B, H, W = x.shape
    Cout = dy.shape[3]
    dw = out if out is not None else _empty(Cout, 1, 3, 3, like=x)
    ws = _ws(query("tag_conv3x3_c1_wgrad_ws_bytes", B, H, W, Cout), x)
    call("tag_conv3x3_c1_wgrad", ptr(x), ptr(col_scale), ptr(col_shift), ptr(dy), ptr(dw), B, H, W, Cout, ptr(ws))
    return dw


C1_BWD_FUSED_SHAPE = (64, 64)            # (mel bins, channels) the one-pass Cin = 1 backward is written for


def conv3x3_c1_backward(x, dy, w, col_scale=None, col_shift=None, out=None, bn_bwd=None):
    """(dw, dx) of the Cin = 1 convolution; one fused pass over dy when the shape allows (W == 64, Cout == 64).
    bn_bwd = (yref, st, gamma, dgamma, dbeta): `dy` is da = dL/d relu(bn(yref)) and the BatchNorm + ReLU backward is applied
    while it is loaded (tag_conv3x3_c1_backward_bnrelu; fused shape only)."""
    B, H, W = x.shape
    Cout = dy.shape[3]
    if (W, Cout) == C1_BWD_FUSED_SHAPE:
        dw = out if out is not None else _empty(Cout, 1, 3, 3, like=x)
        dx = _empty(B, H, W, like=x)
        ws = _ws(query("tag_conv3x3_c1_backward_ws_bytes", B, H, W, Cout), x)
        if bn_bwd is not None:
            yref, st, gamma, dg, db = bn_bwd
            if yref.dtype != dy.dtype or yref.shape != dy.shape:
                raise RuntimeError("conv3x3_c1_backward: yref and da must agree in dtype and shape")
            call("tag_conv3x3_c1_backward_bnrelu" + _sfx(dy), ptr(x), ptr(col_scale), ptr(col_shift), ptr(dy), ptr(yref),
                 ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.invstd), ptr(gamma), ptr(dg), ptr(db), int(st.train),
                 ptr(w), ptr(dw), ptr(dx), B, H, W, Cout, ptr(ws))
            return dw, dx
        call("tag_conv3x3_c1_backward" + _sfx(dy), ptr(x), ptr(col_scale), ptr(col_shift), ptr(dy), ptr(w), ptr(dw), ptr(dx),
             B, H, W, Cout, ptr(ws))
        return dw, dx
    if bn_bwd is not None:
        raise RuntimeError("conv3x3_c1_backward: bn_bwd needs the fused 64 x 64 shape")
    if dy.dtype == BF16:
        raise RuntimeError("bf16 activations: the Cin = 1 backward is implemented for 64 mel bins x 64 channels")
    return conv3x3_c1_wgrad(x, dy, col_scale, col_shift), conv3x3_c1_dgrad(dy, w)


def conv3x3_c1_dgrad(dy, w):
    B, H, W, Cout = dy.shape
    dx = _empty(B, H, W, like=dy)
    call("tag_conv3x3_c1_dgrad", ptr(dy), ptr(w), ptr(dx), B, H, W, Cout)
    return dx


def bnact_pool(y, st: Optional[BNStat], ph, pw, act=1, pool=0, drop_p=0.0, seed=0):
    B, H, W, C = y.shape
    out = _empty(B, H // ph, W // pw, C, like=y, dtype=y.dtype)
    call("tag_bnact_pool_forward" + _sfx(y), ptr(y), ptr(st.scale) if st else None, ptr(st.shift) if st else None, ptr(out), B,
         H, W, C, ph, pw, act, pool, float(drop_p), seed)
    return out


def bnrelu_pool_backward(y, st: BNStat, gamma, dout, ph, pw, drop_p=0.0, seed=0, dg_out=None, db_out=None, pool=0,
                         partials=None):
    """partials = (P, buffer) from conv3x3_dgrad_poolsums: the sums were taken by the conv that produced dout; only the apply
    pass runs here."""
    B, H, W, C = y.shape
    if dout.dtype != y.dtype:
        raise RuntimeError("bnrelu_pool_backward: y and dout must share their storage type")
    dy = _empty(B, H, W, C, like=y, dtype=y.dtype)
    dg, db = _dg_db(dg_out, db_out, C, y)
    if partials is not None:
        P, part = partials
        ws = _ws(query("tag_bn_grad_from_partials_ws_bytes", P, C), y)
        call("tag_bn_grad_from_partials", ptr(part), P, C, ptr(dg), ptr(db), ptr(ws))
        call("tag_bnrelu_pool_backward_apply" + _sfx(y), ptr(y), ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.invstd),
             ptr(gamma), ptr(dout), ptr(dy), ptr(dg), ptr(db), B, H, W, C, ph, pw, int(pool), float(drop_p), seed, int(st.train))
        return dy, dg, db
    ws = _ws(query("tag_bn_backward_ws_bytes", B * H * W, C), y)
    call("tag_bnrelu_pool_backward" + _sfx(y), ptr(y), ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.invstd), ptr(gamma),
         ptr(dout), ptr(dy), ptr(dg), ptr(db), B, H, W, C, ph, pw, int(pool), float(drop_p), seed, int(st.train), ptr(ws))
    return dy, dg, db


def bnrelu_backward(y, st: BNStat, gamma, da, inplace=True, dg_out=None, db_out=None):
    C = y.shape[-1]
    rows = y.numel() // C
    dy = da if inplace else torch.empty_like(da)
    dg, db = _dg_db(dg_out, db_out, C, y)
    ws = _ws(query("tag_bn_backward_ws_bytes", rows, C), y)
    if da.dtype != y.dtype:
        raise RuntimeError("bnrelu_backward: y and da must share their storage type")
    call("tag_bnrelu_backward" + _sfx(y), ptr(y), ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.invstd), ptr(gamma),
         ptr(da), ptr(dy), ptr(dg), ptr(db), rows, C, int(st.train), ptr(ws))
    return dy, dg, db


def bn_param_grad(x2d, dy2d, st: BNStat, dg_out=None, db_out=None):
    rows, C = x2d.shape
    dg, db = _dg_db(dg_out, db_out, C, x2d)
    ws = _ws(query("tag_bn_backward_ws_bytes", rows, C), x2d)
    call("tag_bn_param_grad", ptr(x2d), ptr(dy2d), rows, C, ptr(st.mean), ptr(st.invstd), ptr(dg), ptr(db), ptr(ws))
    return dg, db


def _stripe_counts(stripes, n_time, B):
    if stripes is None:
        return 0, 0
    if (not stripes.is_cuda or not stripes.is_contiguous() or stripes.dtype != torch.int32 or stripes.dim() != 3
            or stripes.shape[0] != B or stripes.shape[2] != 2):
        raise RuntimeError(f"augment: stripes must be a contiguous device int32 (B={B}, n_time + n_freq, 2) table, got "
                           f"{stripes.dtype} {tuple(stripes.shape)} on {stripes.device}")
    if not 0 <= n_time <= stripes.shape[1]:
        raise RuntimeError(f"augment: n_time {n_time} outside the table's {stripes.shape[1]} rows")
    return n_time, stripes.shape[1] - n_time


def augment_forward(lm, scale=None, shift=None, stripes=None, n_time=0, lam=None):
    """SpecAugment + mixup of the bn0 output (csrc/augment.hip): lm (B,F,NM) -> x0 (B or B/2, F, NM), the bn0 affine (scale,
    shift) applied as the Cin = 1 convolutions apply it, then the stripes' zeros (stripes: int32 (B, n_time + n_freq, 2)
    [bgn, width], the first n_time rows along frames), then do_mixup with lam (B,) when given."""
    lm = _chk(lm, "lm")
    B, Fr, NM = lm.shape
    nt, nf = _stripe_counts(stripes, n_time, B)
    lam = None if lam is None else _chk(lam, "mixup_lambda")
    if lam is not None and (lam.numel() != B or B % 2):
        raise RuntimeError(f"augment: mixup needs an even batch and fp32 lambda of length B={B}, got {tuple(lam.shape)}")
    x0 = _empty(B // 2 if lam is not None else B, Fr, NM, like=lm)
    call("tag_augment_forward", ptr(lm), ptr(scale), ptr(shift), ptr(stripes), nt, nf, ptr(lam), ptr(x0), B, Fr, NM)
    return x0


def augment_backward(dx0, B, stripes=None, n_time=0, lam=None):
    """Gradient of augment_forward with respect to its masked input: dbn0 (B,F,NM) = mask[b] * lam[b] * dx0[b/2] (dx0[b]
    without lam)."""
    dx0 = _chk(dx0, "grad")
    _, Fr, NM = dx0.shape
    nt, nf = _stripe_counts(stripes, n_time, B)
    lam = None if lam is None else _chk(lam, "mixup_lambda")
    if dx0.shape[0] != (B // 2 if lam is not None else B):
        raise RuntimeError(f"augment_backward: dx0 has {dx0.shape[0]} clips for B={B}")
    dbn0 = _empty(B, Fr, NM, like=dx0)
    call("tag_augment_backward", ptr(dx0), ptr(stripes), nt, nf, ptr(lam), ptr(dbn0), B, Fr, NM)
    return dbn0


def dropout_mask(seed, shape, p, device, pooled=False):
    """The keep mask (0/1 bytes) a kernel draws for `seed`; pooled=True: the generator of the pooled activations' dropout
    (one hash per 4 elements; bnact_pool / bnrelu_pool_backward), else the per-element one (mean_w, dropout, attention)."""
    n = int(math.prod(shape))
    m = torch.empty(n, device=device, dtype=torch.uint8)
    call("tag_dropout_mask_pooled" if pooled else "tag_dropout_mask", seed, n, float(p), ptr(m))
    return m.view(*shape)


def gemm(A, B, M, N, K, transA=False, transB=False, lda=None, ldb=None, out=None, ldc=None, bias=None, act=0,
         accumulate=False):
    """Row-major C(M,N) = act(op(A) op(B) + bias) [+ C].  A/B may be strided views (lda/ldb).

    Split-K (a workspace) is offered to the library only for transA products -- the weight-gradient shape, whose reduction
    runs over the batch rows.  A product with A stored (M,K) has the batch in M: without K slices every output row is one
    fixed-order sum over k whatever M is, so forward passes are BATCH-INVARIANT (a clip scores bit-identically alone, in a
    64-clip pass or in a ragged remainder; tools/diag_batch_invariance.py, test_grounding_model_30s_full_pass_b67)."""
    lda = lda if lda is not None else (M if transA else K)
    ldb = ldb if ldb is not None else (K if transB else N)
    if out is None:
        out = _empty(M, N, like=A)
    ldc = ldc if ldc is not None else N
    nws = query("tag_gemm_ws_bytes", M, N, K) if transA else 0
    ws = _ws(nws, A) if nws else None
    call("tag_gemm_bf16" if gemm_bf16() else "tag_gemm", ptr(A), lda, int(transA), ptr(B), ldb, int(transB), ptr(out), ldc, M,
         N, K, ptr(bias), act, int(accumulate), ptr(ws))
    return out


def colsum(x, M, N, ld=None, out=None):
    out = out if out is not None else _empty(N, like=x)
    ws = _ws(query("tag_colsum_ws_bytes", M, N), x)
    call("tag_colsum", ptr(x), ld if ld is not None else N, M, N, ptr(out), ptr(ws))
    return out


def relu_backward(y, dy):
    call("tag_relu_backward", ptr(y), ptr(dy), ptr(dy), y.numel())
    return dy


def segments(frame_sim, thresholds, window_size, n_connect):
    """P1 on the device.  Returns (regions (B,NT,maxK,2) int64, counts (B,NT) int32)."""
    frame_sim = _chk(frame_sim, "frame_sim")
    B, T = frame_sim.shape
    th = torch.as_tensor(thresholds, dtype=torch.float64).to(frame_sim.device)
    NT = th.numel()
    maxk = (T + 1) // 2
    regions = torch.zeros(B, NT, maxk, 2, device=frame_sim.device, dtype=torch.int64)
    counts = torch.zeros(B, NT, device=frame_sim.device, dtype=torch.int32)
    call("tag_segments", ptr(frame_sim), T, B, T, ptr(th), NT, int(window_size), int(n_connect), ptr(regions),
         ptr(counts), maxk)
    return regions, counts


def align_dot(audio, text, l2norm=False, scaled=False):
    """align.DotProduct forward (models/align.py:14-31): (B,T,D),(B,N,D) -> (B,B,T,N); F.normalize of both operands first
    when l2norm (row kernels), then the MFMA GEMM with the [/sqrt D ->] sigmoid -> clamp -> (B,B,T,N) scatter epilogue."""
    audio, text = _chk(audio, "audio"), _chk(text, "text")
    _check_pair_batch("align_dot", audio, text)         # models/align.py:20-21 asserts a_bs == t_bs, a_dim == t_dim
    B, T, D = audio.shape
    N = text.shape[1]
    if l2norm:
        audio, text = _l2norm_rows(audio, B * T, D), _l2norm_rows(text, B * N, D)
    out = _empty(B, B, T, N, like=audio)
    call("tag_align_dot_forward", ptr(audio), ptr(text), ptr(out), 0, int(scaled), B, T, N, D, None)
    return out


def align_expnegl2(audio, text):
    """align.ExpNegL2 forward (models/align.py:34-64): (B,T,D),(B,N,D) -> (B,B,T,N) = exp(-||an - tn||) over the F.normalize'd
    rows (a quotient row pass), the distances as sums of squared differences in the tiled VALU kernel of align.hip.  Stays on
    the device (the reference writes into a CPU torch.zeros)."""
    audio, text = _chk(audio, "audio"), _chk(text, "text")
    _check_pair_batch("align_expnegl2", audio, text)    # models/align.py:39-40 asserts a_bs == t_bs, a_dim == t_dim
    B, T, D = audio.shape
    N = text.shape[1]
    an, tn = _unit_rows(audio, B * T, D), _unit_rows(text, B * N, D)
    out = _empty(B, B, T, N, like=audio)
    call("tag_align_expnegl2_forward", ptr(an), ptr(tn), ptr(out), B, T, N, D)
    return out


# ------------------------------------------------------------------------------------------------
# bidirectional GRU (row A4): input projection GEMM + persistent recurrence, and its backward
# ------------------------------------------------------------------------------------------------

#: persistent scratch of the GRU kernels per (device, B, H, pass): recurrent-weight transpose, exchange granules and a
#: STICKY error word (last 256 bytes; zeroed once here, raised by a persistent kernel whose bounded spin ran out and never
#: cleared by the library) -> check_async_errors()
_gru_scratch = {}


_GRU_SCRATCH_MAX = 8        # (B, H, pass) combinations kept per process; ragged epochs vary T, which the scratch ignores


def _gru_ws(B, T, Hh, like, which):
    """Scratch of one persistent GRU launch.  tag_gru_ws_bytes does not depend on T, so the cache key does not either (a
    ragged epoch pads every batch to its own longest clip); the least recently used entry is dropped beyond
    _GRU_SCRATCH_MAX.  Kernels run in stream order, so equal-shape GRUs may share one scratch."""
    key = (like.device.type, like.device.index, B, Hh, which)
    ws = _gru_scratch.pop(key, None)
    if ws is None:
        nbytes = query("tag_gru_ws_bytes", B, T, Hh)
        ws = torch.zeros((nbytes + 7) // 8, device=like.device, dtype=torch.float64)
        ws._tag_err_index = (nbytes - 256) // 4          # int32 index of the sticky error word
        while len(_gru_scratch) >= _GRU_SCRATCH_MAX:
            old_key = next(iter(_gru_scratch))
            _check_gru_word(old_key, _gru_scratch.pop(old_key))      # an evicted scratch must not take a raised flag with it
    _gru_scratch[key] = ws                                # (re-)inserted last = most recently used
    return ws


def _check_gru_word(key, ws):
    word = ws.view(torch.int32)[ws._tag_err_index: ws._tag_err_index + 1]
    err = word.cpu()
    if query("tag_gru_timed_out", err.data_ptr()):
        word.zero_()
        was_fast = query("tag_gru_disable_xcd_fast")      # later launches publish write-through (correct under every placement)
        raise RuntimeError(f"persistent GRU kernel timed out waiting for a neighbouring workgroup (B,H,pass = {key[2:]}): "
                           "its workgroups were not co-resident or an L2-resident exchange granule was read stale; outputs of "
                           "that step are NaN and the optimiser skipped it"
                           + ("; the same-XCD L2 publishing is now OFF for this process" if was_fast else ""))


def check_async_errors():
    """Host-side check of the sticky device error words (synchronises): raises RuntimeError when a persistent GRU kernel
    timed out waiting for its neighbours (its outputs were poisoned with NaN and the Adam kernel skipped the step) or an
    embedding lookup saw a token id outside the table.  Called by StrongRunner whenever it hands a loss VALUE to the host."""
    for key, ws in list(_gru_scratch.items()):
        _check_gru_word(key, ws)
    for dev, flag in _embed_err.items():
        if int(flag.cpu().item()) != 0:
            flag.zero_()
            raise IndexError("embedding lookup: token id out of range (nn.Embedding would raise; models/text_encoder.py:39)")


_embed_err = {}


def _embed_flag(like):
    key = (like.device.type, like.device.index)
    if key not in _embed_err:
        _embed_err[key] = torch.zeros(1, device=like.device, dtype=torch.int32)
    return _embed_err[key]


def _adjacent_view(a, b, shape):
    """The view over ``a`` and ``b`` as ONE tensor when b lies right behind a in the same storage, else None."""
    if (a is not None and b is not None and a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype
            and a.device == b.device and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.storage_offset() == a.storage_offset() + a.numel()):
        return torch.empty(0, device=a.device, dtype=a.dtype).set_(a.untyped_storage(), a.storage_offset(), tuple(shape))
    return None


def _joined(a, b, shape):
    """``torch.cat / stack([a, b])`` as a VIEW when b lies right behind a in the same storage (runner.FlatParams lays the
    two directions of an nn.GRU out that way), else a copy: no concatenation kernels per step on the flat-parameter path."""
    v = _adjacent_view(a, b, shape)
    return v if v is not None else torch.cat([a.reshape(-1), b.reshape(-1)]).view(*shape)


def bump_bn_counters(owner, bns):
    """``num_batches_tracked += 1`` of the BatchNorm modules ``bns`` (all in train mode) as ONE kernel: the nine 0-dim
    int64 buffers are re-homed (once per device move) as views of one flat tensor kept on ``owner``; state_dict keys,
    load_state_dict and the rank-0 buffer broadcast see the same buffers as before."""
    flat = getattr(owner, "_tag_nbt_flat", None)
    ok = (flat is not None and flat.numel() == len(bns) and flat.device == bns[0].num_batches_tracked.device
          and all(m._buffers["num_batches_tracked"].data_ptr() == flat.data_ptr() + 8 * i for i, m in enumerate(bns)))
    if not ok:
        flat = torch.stack([m.num_batches_tracked.detach().to(torch.long) for m in bns])
        for i, m in enumerate(bns):
            m._buffers["num_batches_tracked"] = flat[i]
        owner._tag_nbt_flat = flat
    flat += 1


def max_clips_per_pass(frames: int) -> int:
    """Largest batch the kernels take in one launch.  Round 4: the conv kernels add a 64-bit per-image base to 32-bit offsets
    INSIDE the image, so what is left is the 31-bit PIXEL index of the BatchNorm / pool passes over the largest tensor, the
    first block's (B, frames, 64 mel) pixels -- 33 520 clips of 10 s (rounds 1-3: 32-bit byte offsets over the whole batch, 261
    clips of 10 s in fp32).  Memory is the practical limit: ~75 MB of saved activations per 10 s clip in fp32."""
    return max(1, (2 ** 31 - 1) // (int(frames) * 64))


def check_pass_size(B: int, frames: int):
    """Loud and early instead of TAG_EINVAL from the first kernel: a batch beyond the 31-bit pixel index must be split by the
    CALLER (train-mode BatchNorm statistics are per forward pass, so the split is not invisible; the inference wrapper
    models/hf_modeling_grounding.py splits into passes of 64 for memory -- eval-mode BatchNorm makes its passes independent)."""
    lim = max_clips_per_pass(frames)
    if B > lim:
        raise RuntimeError(f"batch of {B} clips x {frames} frames exceeds the kernels' 31-bit pixel index: at most {lim} clips of "
                           "this length per forward pass. Split the batch (gradient accumulation over sub-batches; note that "
                           "train-mode BatchNorm statistics are then per sub-batch, as they would be with a smaller batch in the "
                           "reference)")


def gru_bidir_forward(x2d, rnn, B, T, need_grad):
    """x2d (B*T, I); rnn = [w_ih, w_hh, b_ih, b_hh] x (forward, reverse).  Returns y (B,T,2H) and the saved state."""
    Hh = rnn[1].shape[1]
    M = B * T
    I = rnn[0].shape[1]
    w_ih = _joined(rnn[0], rnn[4], (6 * Hh, I))            # (2*3H, I)
    b_ih = _joined(rnn[2], rnn[6], (6 * Hh,))
    w_hh = _joined(rnn[1], rnn[5], (2, 3 * Hh, Hh))
    b_hh = _joined(rnn[3], rnn[7], (2, 3 * Hh))
    gi = gemm(x2d, w_ih, M, 6 * Hh, x2d.shape[1], transB=True, bias=b_ih)
    y = _empty(B, T, 2 * Hh, like=x2d)
    gates = _empty(B, T, 2, 4 * Hh, like=x2d) if need_grad else None
    wsr = _gru_ws(B, T, Hh, x2d, "fwd")
    call("tag_gru_forward", ptr(gi), ptr(w_hh), ptr(b_hh), ptr(y), ptr(gates), ptr(wsr), B, T, Hh)
    return y, (dict(gates=gates, y=y, w_ih=w_ih, w_hh=w_hh, Hh=Hh) if need_grad else None)


def gru_bidir_backward(dy, x2d, sv, outs=None, side=None):
    """Returns (dx2d, [8 parameter gradients in nn.GRU order]).  outs: optional 8 destination tensors (flat-gradient
    views); a gradient whose destination is given is written there directly -- the bias gradients too when the two
    directions' sinks are adjacent (runner.FlatParams lays them out that way): one column sum fills both.
    side: a _SideWgrad; when EVERY gradient has its destination, the parameter-gradient work (2 column sums + 4 GEMMs, all
    off the dx chain) runs on its side stream beside the memory-bound passes that follow on the main stream."""
    Hh, y, gates = sv["Hh"], sv["y"], sv["gates"]
    B, T, _ = y.shape
    M = B * T
    dgi = _empty(B, T, 2, 3 * Hh, like=y)
    dgh = _empty(B, T, 2, 3 * Hh, like=y)
    hprev = _empty(B, T, 2, Hh, like=y)
    scratch = _gru_ws(B, T, Hh, y, "bwd")
    call("tag_gru_backward", ptr(dy), ptr(y), ptr(gates), ptr(sv["w_hh"]), ptr(dgi), ptr(dgh), ptr(hprev),
         ptr(scratch), B, T, Hh)
    I = x2d.shape[1]
    outs = list(outs) if outs is not None else [None] * 8
    g = [None] * 8
    bih_sink = _adjacent_view(outs[2], outs[6], (6 * Hh,))
    bhh_sink = _adjacent_view(outs[3], outs[7], (6 * Hh,))
    all_direct = bih_sink is not None and bhh_sink is not None and all(o is not None for o in outs)

    def param_grads():
        db_ih = colsum(dgi, M, 6 * Hh, out=bih_sink)
        db_hh = colsum(dgh, M, 6 * Hh, out=bhh_sink)
        for d in range(2):
            ai = dgi.view(M, 6 * Hh)[:, d * 3 * Hh:]
            a = dgh.view(M, 6 * Hh)[:, d * 3 * Hh:]
            hb = hprev.view(M, 2 * Hh)[:, d * Hh:]
            g[4 * d + 0] = gemm(ai, x2d, 3 * Hh, I, M, transA=True, lda=6 * Hh, out=outs[4 * d + 0])
            g[4 * d + 1] = gemm(a, hb, 3 * Hh, Hh, M, transA=True, lda=6 * Hh, ldb=2 * Hh, out=outs[4 * d + 1])
            g[4 * d + 2] = outs[4 * d + 2] if bih_sink is not None else db_ih[d * 3 * Hh:(d + 1) * 3 * Hh]
            g[4 * d + 3] = outs[4 * d + 3] if bhh_sink is not None else db_hh[d * 3 * Hh:(d + 1) * 3 * Hh]
    if side is not None and all_direct:
        side.run(param_grads, (dgi, dgh, hprev, x2d))
    else:
        param_grads()
    dx = gemm(dgi, sv["w_ih"], M, I, 6 * Hh)
    return dx, g


# ------------------------------------------------------------------------------------------------
# text GRU (row T3): per layer one input-projection GEMM + ONE row-local recurrence launch (csrc/text_gru.hip), and its backward
# ------------------------------------------------------------------------------------------------

def _text_gru_layer_params(params, l, dirs):
    """[w_ih, w_hh, b_ih, b_hh] of layer l with the directions joined: (dirs*3H, I), (dirs, 3H, H), (dirs*3H,), (dirs, 3H)."""
    pl = params[4 * dirs * l: 4 * dirs * (l + 1)]
    Hh, I = pl[1].shape[1], pl[0].shape[1]
    if dirs == 1:
        return [pl[0].contiguous(), pl[1].contiguous().view(1, 3 * Hh, Hh), pl[2].contiguous(), pl[3].contiguous().view(1, 3 * Hh)]
    return [_joined(pl[0], pl[4], (6 * Hh, I)), _joined(pl[1], pl[5], (2, 3 * Hh, Hh)), _joined(pl[2], pl[6], (6 * Hh,)),
            _joined(pl[3], pl[7], (2, 3 * Hh))]


def text_gru_dropout_seed(seed, l):
    """Seed of the dropout behind layer l of a stacked text GRU (one operator seed, one mask per layer)."""
    return (int(seed) + l) % (2 ** 62)


def text_gru_recurrence(gi, w_hh, b_hh, text_len, need_grad):
    """ONE launch of tag_text_gru_forward: gi (R, L, dirs, 3H), w_hh (dirs, 3H, H), b_hh (dirs, 3H), text_len (R) int64 or
    None -> y (R, L, dirs*H), gates (R, L, dirs, 4H) or None, seq_mean (R, dirs*H) or None (text_len is None)."""
    gi = _chk(gi, "gi")
    R, L, dirs, H3 = gi.shape
    Hh = H3 // 3
    if text_len is not None and (not text_len.is_cuda or text_len.dtype != torch.long):
        raise RuntimeError("text_gru: text_len must be an int64 tensor on the device (no CPU fallback)")
    y = _empty(R, L, dirs * Hh, like=gi)
    gates = _empty(R, L, dirs, 4 * Hh, like=gi) if need_grad else None
    seq = _empty(R, dirs * Hh, like=gi) if text_len is not None else None
    call("tag_text_gru_forward", ptr(gi), ptr(_chk(w_hh, "w_hh")), ptr(_chk(b_hh, "b_hh")), ptr(text_len), ptr(y), ptr(gates),
         ptr(seq), R, L, Hh, dirs)
    return y, gates, seq


def text_gru_recurrence_backward(dy, dseq, text_len, y, gates, w_hh):
    """ONE launch of tag_text_gru_backward: dy (R, L, dirs*H) or None, dseq (R, dirs*H) or None -> dgi, dgh (R, L, dirs, 3H) and
    hprev (R, L, dirs, H)."""
    R, L, dirs, H4 = gates.shape
    Hh = H4 // 4
    dy = _chk(dy, "grad") if dy is not None else None
    dseq = _chk(dseq, "grad") if dseq is not None else None
    dgi = _empty(R, L, dirs, 3 * Hh, like=y)
    dgh = _empty(R, L, dirs, 3 * Hh, like=y)
    hprev = _empty(R, L, dirs, Hh, like=y)
    call("tag_text_gru_backward", ptr(dy), ptr(dseq), ptr(text_len), ptr(y), ptr(gates), ptr(w_hh), ptr(dgi), ptr(dgh),
         ptr(hprev), R, L, Hh, dirs)
    return dgi, dgh, hprev


def text_gru_dropout(x2d, p, seed, backward):
    """Inter-layer dropout of the stacked text GRU on (M, D) rows: keep mask = tag_dropout_mask(seed) over the flat index,
    kept values scaled by 1 / (1 - p) (the W = 1 case of the mean-over-W + dropout kernels); the backward applies the same mask."""
    M, D = x2d.shape
    out = _empty(M, D, like=x2d)
    call("tag_mean_w_backward" if backward else "tag_mean_w_forward", ptr(_chk(x2d, "x")), M, 1, D, float(p), seed, ptr(out))
    return out


def text_gru_forward(x, text_len, params, dirs, layers, need_grad, drop_p=0.0, seed=0):
    """nn.GRU(batch_first=True) over ALL L padded positions + mean_with_lens (models/text_encoder.py:119-123).
    x (R, L, E) embedded tokens; text_len (R) int64 on the device; params = nn.GRU's flat weights, per layer and direction
    [w_ih, w_hh, b_ih, b_hh].  drop_p > 0: dropout on the output of every layer but the last (the counter-based keep mask
    tag_dropout_mask materialises, seed text_gru_dropout_seed(seed, l), index = flat index of (R, L, dirs*H)).
    -> token_emb (R, L, dirs*H), seq_emb (R, dirs*H), saved state per layer (None unless need_grad)."""
    x = _chk(x, "x")
    R, L, _ = x.shape
    Hh = params[1].shape[1]
    M, D = R * L, dirs * Hh
    inp = x.view(M, -1)
    saved, y, seq = [], None, None
    for l in range(layers):
        w_ih, w_hh, b_ih, b_hh = _text_gru_layer_params(params, l, dirs)
        last = l == layers - 1
        gi = gemm(inp, w_ih, M, 3 * D, inp.shape[1], transB=True, bias=b_ih)
        y, gates, seq = text_gru_recurrence(gi.view(R, L, dirs, 3 * Hh), w_hh, b_hh, text_len if last else None, need_grad)
        if need_grad:
            saved.append(dict(x=inp, y=y, gates=gates, w_ih=w_ih, w_hh=w_hh))
        if not last:
            inp = y.view(M, D)
            if drop_p > 0.0:
                inp = text_gru_dropout(inp, drop_p, text_gru_dropout_seed(seed, l), backward=False)
    return y, seq, (saved if need_grad else None)


def text_gru_backward(dtok, dseq, text_len, saved, dirs, drop_p=0.0, seed=0, outs=None, need=None, need_dx=True):
    """-> (dx (R, L, E) or None, parameter gradients in nn.GRU's flat order).  dtok (R, L, dirs*H) / dseq (R, dirs*H): either
    may be None.  outs: optional destination per parameter (flat-gradient views), written directly; need: per parameter,
    False skips its GEMM / column sum (requires_grad = False: freeze_text_encoder) and leaves None."""
    layers = len(saved)
    Hh = saved[0]["w_hh"].shape[2]
    R, L, D = saved[0]["y"].shape
    M = R * L
    n = 4 * dirs * layers
    outs = list(outs) if outs is not None else [None] * n
    need = list(need) if need is not None else [True] * n
    g = [None] * n
    dy, dsq, dx = dtok, dseq, None
    for l in range(layers - 1, -1, -1):
        sv = saved[l]
        x2d = sv["x"]
        I = x2d.shape[1]
        dgi, dgh, hprev = text_gru_recurrence_backward(dy, dsq, text_len, sv["y"], sv["gates"], sv["w_hh"])
        base = 4 * dirs * l
        o = outs[base: base + 4 * dirs]
        nd = need[base: base + 4 * dirs]
        for which, src in ((2, dgi), (3, dgh)):             # bias gradients: ONE column sum over all directions when possible
            idx = [4 * d + which for d in range(dirs)]
            if not any(nd[i] for i in idx):
                continue
            sink = o[idx[0]] if dirs == 1 else _adjacent_view(o[idx[0]], o[idx[1]], (6 * Hh,))
            tot = colsum(src, M, 3 * D, out=sink if all(nd[i] for i in idx) else None)
            for d, i in enumerate(idx):
                if nd[i]:
                    part = tot[d * 3 * Hh:(d + 1) * 3 * Hh]
                    if o[i] is not None and part.data_ptr() != o[i].data_ptr():
                        o[i].copy_(part)
                    g[base + i] = o[i] if o[i] is not None else part
        for d in range(dirs):
            if nd[4 * d]:
                g[base + 4 * d] = gemm(dgi.view(M, 3 * D)[:, d * 3 * Hh:], x2d, 3 * Hh, I, M, transA=True, lda=3 * D, out=o[4 * d])
            if nd[4 * d + 1]:
                g[base + 4 * d + 1] = gemm(dgh.view(M, 3 * D)[:, d * 3 * Hh:], hprev.view(M, D)[:, d * Hh:], 3 * Hh, Hh, M,
                                           transA=True, lda=3 * D, ldb=D, out=o[4 * d + 1])
        if l > 0 or need_dx:
            dx = gemm(dgi, sv["w_ih"], M, I, 3 * D)
        if l > 0:
            if drop_p > 0.0:
                dx = text_gru_dropout(dx, drop_p, text_gru_dropout_seed(seed, l - 1), backward=True)
            dy, dsq = dx.view(R, L, I), None
    return (dx.view(R, L, -1) if need_dx else None), g


# ------------------------------------------------------------------------------------------------
# text self-attention (row T4): cls + positions + dropout, in-projection GEMM, ONE row-local core launch (csrc/text_attn.hip),
# out-projection GEMM, and its backward
# ------------------------------------------------------------------------------------------------
TEXT_SELFATTN_MAX_S = 64


def text_selfattn_dropout_seeds(seed):
    """(seed of the dropout behind the positions, seed of the dropout on the attention weights) from ONE operator seed."""
    return int(seed) % (2 ** 62), (int(seed) + 1) % (2 ** 62)


def text_selfattn_check(E, heads, S=None):
    """The domain of tag_text_selfattn_*, raised before any launch with the limit named."""
    if heads < 1 or E % heads != 0:
        raise ValueError(f"text_selfattn: embed_dim {E} is not divisible by num_heads {heads}")
    dh = E // heads
    if E > 1024 or not (dh in (16, 32) or dh % 64 == 0):
        raise NotImplementedError(f"text_selfattn: head_dim {dh} (embed_dim {E} / {heads} heads) has no HIP kernel: head_dim must be 16, "
                                  "32 or a multiple of 64 and embed_dim <= 1024; there is no eager fallback")
    if S is not None and not 2 <= S <= TEXT_SELFATTN_MAX_S:
        raise ValueError(f"text_selfattn: {S} positions (cls + {S - 1} tokens); the kernel serves 2 ... {TEXT_SELFATTN_MAX_S} "
                         f"positions, that is 1 ... {TEXT_SELFATTN_MAX_S - 1} tokens")


def _klen_chk(klen, R):
    if not klen.is_cuda or klen.dtype != torch.long or klen.numel() != R:
        raise RuntimeError("text_selfattn: klen must be an int64 tensor of R entries on the device (no CPU fallback)")
    return klen.contiguous()


def text_selfattn_core(qkv, klen, heads, need_attn=True, drop_p=0.0, seed=0):
    """ONE launch of tag_text_selfattn_forward: qkv (R, S, 3E) packed [q|k|v] (read in place, any 4-byte aligned view), klen (R)
    int64 valid keys -> ctx (R, S, E), attn (R, H, S, S) = the weights before dropout, or None."""
    qkv = _chk(qkv, "qkv")
    R, S, E3 = qkv.shape
    E = E3 // 3
    text_selfattn_check(E, heads, S)
    klen = _klen_chk(klen, R)
    ctx = _empty(R, S, E, like=qkv)
    attn = _empty(R, heads, S, S, like=qkv) if need_attn else None
    call("tag_text_selfattn_forward", ptr(qkv), ptr(klen), ptr(ctx), ptr(attn), R, S, E, heads, float(drop_p), int(seed))
    return ctx, attn


def text_selfattn_core_backward(qkv, attn, dctx, klen, heads, drop_p=0.0, seed=0):
    """ONE launch of tag_text_selfattn_backward -> dqkv (R, S, 3E), packed like qkv."""
    qkv, attn, dctx = _chk(qkv, "qkv"), _chk(attn, "attn"), _chk(dctx, "grad")
    R, S, E3 = qkv.shape
    E = E3 // 3
    text_selfattn_check(E, heads, S)
    klen = _klen_chk(klen, R)
    dqkv = _empty(R, S, E3, like=qkv)
    call("tag_text_selfattn_backward", ptr(qkv), ptr(attn), ptr(dctx), ptr(klen), ptr(dqkv), R, S, E, heads, float(drop_p), int(seed))
    return dqkv


def text_cls_pe_forward(tok, cls, pe, drop_p=0.0, seed=0):
    """x (R, L+1, E) = dropout([cls ; tok] + pe[:L+1]); tok (R, L, E), cls (E) (any shape of E entries), pe (>= L+1, E)."""
    tok = _chk(tok, "tok")
    R, L, E = tok.shape
    cls, pe = _chk(cls, "cls_token").view(-1), _chk(pe, "pe").view(-1, E)
    if cls.numel() != E or pe.shape[0] < L + 1:
        raise ValueError(f"text_cls_pe: cls has {cls.numel()} entries for embed_dim {E}, the position table {pe.shape[0]} rows for "
                         f"{L + 1} positions")
    x = _empty(R, L + 1, E, like=tok)
    call("tag_text_cls_pe_forward", ptr(tok), ptr(cls), ptr(pe), ptr(x), R, L, E, float(drop_p), int(seed))
    return x


def text_cls_pe_backward(dx, drop_p=0.0, seed=0, need_dtok=True, need_dcls=True, dcls_out=None):
    """dx (R, L+1, E) -> dtok (R, L, E), dcls (E): the masked cls rows summed by tag_colsum (fixed order, no atomics)."""
    dx = _chk(dx, "grad")
    R, S, E = dx.shape
    if not (need_dtok or need_dcls):
        return None, None
    dtok = _empty(R, S - 1, E, like=dx) if need_dtok else None
    rows = _empty(R, E, like=dx) if need_dcls else None
    call("tag_text_cls_pe_backward", ptr(dx), ptr(dtok), ptr(rows), R, S - 1, E, float(drop_p), int(seed))
    dcls = colsum(rows, R, E, out=dcls_out.view(-1) if dcls_out is not None else None) if need_dcls else None
    return dtok, dcls


def text_selfattn_forward(tok, text_len, pe, cls, w_in, b_in, w_out, b_out, heads, need_grad, drop_p=0.0, seed=0):
    """SelfAttention.forward behind the embedding (models/text_encoder.py:263-268): tok (R, L, E) embedded tokens, text_len (R)
    int64 on the device (0 ... L, clamped), pe (>= L+1, E), cls (E), nn.MultiheadAttention's in_proj (3E, E) / (3E) and out_proj
    (E, E) / (E).  drop_p > 0 (train): the SAME p on the positions and on the attention weights, keep masks of
    text_selfattn_dropout_seeds(seed).  -> out (R, L+1, E) (row 0 = seq_emb, the rest = token_emb), saved state or None."""
    tok = _chk(tok, "tok")
    R, L, E = tok.shape
    text_selfattn_check(E, heads, L + 1)
    s_pe, s_attn = text_selfattn_dropout_seeds(seed)
    M = R * (L + 1)
    klen = text_len.clamp(0, L) + 1
    x = text_cls_pe_forward(tok, cls, pe, drop_p, s_pe)
    w_in, w_out = _chk(w_in, "in_proj_weight"), _chk(w_out, "out_proj.weight")
    qkv = gemm(x.view(M, E), w_in, M, 3 * E, E, transB=True, bias=_chk(b_in, "in_proj_bias"))
    ctx, attn = text_selfattn_core(qkv.view(R, L + 1, 3 * E), klen, heads, need_grad, drop_p, s_attn)
    out = gemm(ctx.view(M, E), w_out, M, E, E, transB=True, bias=_chk(b_out, "out_proj.bias"))
    saved = dict(x=x, qkv=qkv, attn=attn, ctx=ctx, klen=klen, w_in=w_in, w_out=w_out) if need_grad else None
    return out.view(R, L + 1, E), saved


def text_selfattn_backward(dout, saved, heads, drop_p=0.0, seed=0, outs=None, need=None, need_dtok=True):
    """-> (dtok (R, L, E) or None, [dcls, dw_in, db_in, dw_out, db_out]).  outs: optional destination per parameter (flat-gradient
    views), written directly; need: per parameter, False skips its GEMM / column sum (a frozen parameter) and leaves None."""
    dout = _chk(dout, "grad")
    R, S, E = dout.shape
    M = R * S
    outs = list(outs) if outs is not None else [None] * 5
    need = list(need) if need is not None else [True] * 5
    s_pe, s_attn = text_selfattn_dropout_seeds(seed)
    g = [None] * 5
    d2 = dout.view(M, E)
    if need[3]:
        g[3] = gemm(d2, saved["ctx"].view(M, E), E, E, M, transA=True, lda=E, out=outs[3])
    if need[4]:
        g[4] = colsum(d2, M, E, out=outs[4])
    if not (need[0] or need[1] or need[2] or need_dtok):
        return None, g
    dctx = gemm(d2, saved["w_out"], M, E, E)
    dqkv = text_selfattn_core_backward(saved["qkv"].view(R, S, 3 * E), saved["attn"], dctx.view(R, S, E), saved["klen"], heads,
                                       drop_p, s_attn).view(M, 3 * E)
    if need[1]:
        g[1] = gemm(dqkv, saved["x"].view(M, E), 3 * E, E, M, transA=True, lda=3 * E, out=outs[1])
    if need[2]:
        g[2] = colsum(dqkv, M, 3 * E, out=outs[2])
    dtok = None
    if need[0] or need_dtok:
        dx = gemm(dqkv, saved["w_in"], M, E, 3 * E)
        dtok, g[0] = text_cls_pe_backward(dx.view(R, S, E), drop_p, s_pe, need_dtok, need[0], dcls_out=outs[0])
    return dtok, g


# ------------------------------------------------------------------------------------------------
# text intra-attention (row T5): per layer ONE row-local core launch (csrc/text_intra.hip), the three gate products of the shared
# ConvGRUCell as tag_gemm calls over the two K halves of [message ; x], two element-wise launches; and its backward
# ------------------------------------------------------------------------------------------------
TEXT_INTRA_MAX_L = 64
TEXT_INTRA_MAX_E = 1024


def text_intra_dropout_seeds(seed, layers):
    """[(seed_a, seed_b)] per layer -- the 2 x num_layers masks behind the positions -- from ONE operator seed."""
    return [((int(seed) + 2 * l) % (2 ** 62), (int(seed) + 2 * l + 1) % (2 ** 62)) for l in range(layers)]


def text_intra_check(E, L=None):
    """The domain of tag_text_intra_*, raised before any launch with the limit named."""
    if E < 2 or E % 2:
        raise ValueError(f"text_intra: embed_dim {E} is odd (or below 2); the sin/cos position table is defined for even embed_dim only")
    if E > TEXT_INTRA_MAX_E:
        raise ValueError(f"text_intra: embed_dim {E}; the kernel serves embed_dim <= {TEXT_INTRA_MAX_E} and there is no eager fallback")
    if L is not None and not 1 <= L <= TEXT_INTRA_MAX_L:
        raise ValueError(f"text_intra: {L} tokens per phrase; the kernel serves 1 ... {TEXT_INTRA_MAX_L} tokens and there is no "
                         "eager fallback")


def _text_len_chk(text_len, R):
    if not text_len.is_cuda or text_len.dtype != torch.long or text_len.numel() != R:
        raise RuntimeError("text_intra: text_len must be an int64 tensor of R entries on the device (no CPU fallback)")
    return text_len.contiguous()


def _pe_rows(pe, L, E):
    pe = _chk(pe, "pe").view(-1, E)
    if pe.shape[0] < L:
        raise ValueError(f"text_intra: the position table has {pe.shape[0]} rows for {L} positions")
    return pe


def text_intra_core(x, pe, text_len, need_attn=True, drop_p=0.0, seeds=(0, 0)):
    """ONE launch of tag_text_intra_forward: x (R, L, E), pe (>= L, E), text_len (R) int64 -> message (R, L, E), attn (R, L, L) =
    the softmax output with the dead cells included, or None."""
    x = _chk(x, "x")
    R, L, E = x.shape
    text_intra_check(E, L)
    pe, text_len = _pe_rows(pe, L, E), _text_len_chk(text_len, R)
    msg = _empty(R, L, E, like=x)
    attn = _empty(R, L, L, like=x) if need_attn else None
    call("tag_text_intra_forward", ptr(x), ptr(pe), ptr(text_len), ptr(msg), ptr(attn), R, L, E, float(drop_p), int(seeds[0]),
         int(seeds[1]))
    return msg, attn


def text_intra_core_backward(dmsg, x, pe, attn, text_len, drop_p=0.0, seeds=(0, 0), out=None):
    """ONE launch of tag_text_intra_backward -> dx (R, L, E); out: a (R, L, E) tensor the result is ADDED to."""
    dmsg, x, attn = _chk(dmsg, "grad"), _chk(x, "x"), _chk(attn, "attn")
    R, L, E = x.shape
    text_intra_check(E, L)
    pe, text_len = _pe_rows(pe, L, E), _text_len_chk(text_len, R)
    dx = out if out is not None else _empty(R, L, E, like=x)
    call("tag_text_intra_backward", ptr(dmsg), ptr(x), ptr(pe), ptr(attn), ptr(text_len), ptr(dx), int(out is not None), R, L, E,
         float(drop_p), int(seeds[0]), int(seeds[1]))
    return dx


def convgru_gates_forward(u, r, x):
    """u, r (M, E) pre-activations -> sigmoid in place; -> xr = x * r."""
    M, E = u.shape
    xr = _empty(M, E, like=u)
    call("tag_convgru_gates_forward", ptr(_chk(u, "u")), ptr(_chk(r, "r")), ptr(_chk(x, "x")), ptr(xr), M, E)
    return xr


def convgru_update_forward(o, u, x, R, L, text_len=None):
    """o (R*L, E) pre-activation -> tanh in place; -> xnew = x (1 - u) + o u and, with text_len, its mean over the valid
    positions (R, E)."""
    E = o.shape[-1]
    xnew = _empty(R * L, E, like=o)
    seq = _empty(R, E, like=o) if text_len is not None else None
    call("tag_convgru_update_forward", ptr(_chk(o, "o")), ptr(_chk(u, "u")), ptr(_chk(x, "x")), ptr(xnew), ptr(text_len), ptr(seq),
         R, L, E)
    return xnew, seq


def convgru_update_backward(dnew, dseq, text_len, x, u, o, R, L):
    """-> do_pre, du_pre and the direct term dx = g (1 - u), each (R*L, E); g = dnew + the share of dseq (either may be None)."""
    E = o.shape[-1]
    dnew = _chk(dnew, "grad") if dnew is not None else None
    dseq = _chk(dseq, "grad") if dseq is not None else None
    do_pre, du_pre, dx = (_empty(R * L, E, like=o) for _ in range(3))
    call("tag_convgru_update_backward", ptr(dnew), ptr(dseq), ptr(text_len), ptr(_chk(x, "x")), ptr(_chk(u, "u")), ptr(_chk(o, "o")),
         ptr(do_pre), ptr(du_pre), ptr(dx), R, L, E)
    return do_pre, du_pre, dx


def convgru_gates_backward(dxr, x, r, dx):
    """dxr (M, E) -> dr_pre = dxr x r (1 - r); dx += dxr r (in place)."""
    M, E = dxr.shape
    dr_pre = _empty(M, E, like=dxr)
    call("tag_convgru_gates_backward", ptr(_chk(dxr, "grad")), ptr(_chk(x, "x")), ptr(_chk(r, "r")), ptr(dr_pre), ptr(dx), M, E)
    return dr_pre


def _gate_product(msg, h, w, bias, M, E):
    """[msg ; h] @ w^T + bias, w (E, 2E), as two K halves into one output: the concatenation is never materialised."""
    out = gemm(msg, w, M, E, E, transB=True, ldb=2 * E, bias=bias)
    return gemm(h, w[:, E:], M, E, E, transB=True, ldb=2 * E, out=out, accumulate=True)


def text_intra_forward(x, text_len, pe, w_r, b_r, w_u, b_u, w_o, b_o, layers, need_grad, drop_p=0.0, seed=0):
    """IntraAttention.forward behind the embedding (models/text_encoder.py:213-237): x (R, L, E) embedded tokens, text_len (R)
    int64 on the device, pe (>= L, E), the ConvGRUCell's reset / update / out gates (E, 2E) / (E), applied ``layers`` times.
    drop_p > 0 (train): two independent dropouts behind the positions per layer, keep masks of
    text_intra_dropout_seeds(seed, layers).  -> token_emb (R, L, E), seq_emb (R, E), saved state per layer or None."""
    x = _chk(x, "x")
    R, L, E = x.shape
    text_intra_check(E, L)
    if layers < 1:
        raise ValueError("text_intra: num_layers must be >= 1 (IntraAttention serves num_layers = 0 without this operator)")
    M = R * L
    w_r, w_u, w_o = _chk(w_r, "reset_gate.weight"), _chk(w_u, "update_gate.weight"), _chk(w_o, "out_gate.weight")
    b_r, b_u, b_o = _chk(b_r, "reset_gate.bias"), _chk(b_u, "update_gate.bias"), _chk(b_o, "out_gate.bias")
    seeds = text_intra_dropout_seeds(seed, layers)
    saved, seq = [], None
    h = x.view(M, E)
    for l in range(layers):
        msg, attn = text_intra_core(h.view(R, L, E), pe, text_len, need_grad, drop_p, seeds[l])
        msg = msg.view(M, E)
        u = _gate_product(msg, h, w_u, b_u, M, E)
        r = _gate_product(msg, h, w_r, b_r, M, E)
        xr = convgru_gates_forward(u, r, h)
        o = _gate_product(msg, xr, w_o, b_o, M, E)
        hnew, seq = convgru_update_forward(o, u, h, R, L, text_len if l == layers - 1 else None)
        if need_grad:
            saved.append(dict(x=h, msg=msg, attn=attn, u=u, r=r, o=o, xr=xr))
        h = hnew
    return h.view(R, L, E), seq, (saved if need_grad else None)


def text_intra_backward(dtok, dseq, text_len, pe, saved, w_r, w_u, w_o, drop_p=0.0, seed=0, outs=None, need=None, need_dx=True):
    """-> (dx (R, L, E) or None, [dw_r, db_r, dw_u, db_u, dw_o, db_o]).  dtok (R, L, E) / dseq (R, E): either may be None.  The
    cell is shared by the layers: every gate's gradient is accumulated over them (tag_gemm accumulate into ONE buffer per gate,
    the bias column sums added).  outs: optional destination per parameter (flat-gradient views), written directly; need: per
    parameter, False skips its GEMMs / column sums (a frozen parameter) and leaves None."""
    layers = len(saved)
    M, E = saved[0]["x"].shape
    L = saved[0]["attn"].shape[1]
    R = M // L
    outs = list(outs) if outs is not None else [None] * 6
    need = list(need) if need is not None else [True] * 6
    seeds = text_intra_dropout_seeds(seed, layers)
    w_r, w_u, w_o = _chk(w_r, "reset_gate.weight"), _chk(w_u, "update_gate.weight"), _chk(w_o, "out_gate.weight")
    g = [None] * 6

    def weight_grad(i, dpre, msg, h):
        if not need[i]:
            return
        first = g[i] is None
        if first:
            g[i] = outs[i] if outs[i] is not None else _empty(E, 2 * E, like=dpre)
        gemm(dpre, msg, E, E, M, transA=True, lda=E, out=g[i], ldc=2 * E, accumulate=not first)
        gemm(dpre, h, E, E, M, transA=True, lda=E, out=g[i][:, E:], ldc=2 * E, accumulate=not first)

    def bias_grad(i, dpre):
        if not need[i]:
            return
        if g[i] is None:
            g[i] = colsum(dpre, M, E, out=outs[i])
        else:
            g[i].add_(colsum(dpre, M, E))

    dnew, dsq, dx = (dtok.reshape(M, E) if dtok is not None else None), dseq, None
    for l in range(layers - 1, -1, -1):
        sv = saved[l]
        h, msg = sv["x"], sv["msg"]
        do_pre, du_pre, dx = convgru_update_backward(dnew, dsq, text_len, h, sv["u"], sv["o"], R, L)
        dxr = gemm(do_pre, w_o[:, E:], M, E, E, ldb=2 * E)
        dr_pre = convgru_gates_backward(dxr, h, sv["r"], dx)
        weight_grad(4, do_pre, msg, sv["xr"])
        bias_grad(5, do_pre)
        weight_grad(2, du_pre, msg, h)
        bias_grad(3, du_pre)
        weight_grad(0, dr_pre, msg, h)
        bias_grad(1, dr_pre)
        if l == 0 and not need_dx:
            dx = None
            break
        dmsg = gemm(do_pre, w_o, M, E, E, ldb=2 * E)
        gemm(du_pre, w_u, M, E, E, ldb=2 * E, out=dmsg, accumulate=True)
        gemm(dr_pre, w_r, M, E, E, ldb=2 * E, out=dmsg, accumulate=True)
        gemm(du_pre, w_u[:, E:], M, E, E, ldb=2 * E, out=dx, accumulate=True)
        gemm(dr_pre, w_r[:, E:], M, E, E, ldb=2 * E, out=dx, accumulate=True)
        text_intra_core_backward(dmsg.view(R, L, E), h.view(R, L, E), pe, sv["attn"], text_len, drop_p, seeds[l], out=dx.view(R, L, E))
        dnew, dsq = dx, None
    return (dx.view(R, L, E) if dx is not None else None), g


# ------------------------------------------------------------------------------------------------
# LAION-CLAP text tower for training (row T6): the RoBERTa embedding block, per layer one packed q|k|v GEMM + the row-local
# attention core of T4 + out-projection + residual LayerNorm + GELU feed-forward + residual LayerNorm, the tanh pooler and the
# two-layer projection; row kernels of csrc/text_clap.hip, and its backward
# ------------------------------------------------------------------------------------------------
TEXT_CLAP_MAX_L = 64
TEXT_CLAP_HEAD = ("embeddings.word_embeddings.weight", "embeddings.token_type_embeddings.weight",
                  "embeddings.position_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias")
TEXT_CLAP_LAYER = ("attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight",
                   "attention.self.key.bias", "attention.self.value.weight", "attention.self.value.bias",
                   "attention.output.dense.weight", "attention.output.dense.bias", "attention.output.LayerNorm.weight",
                   "attention.output.LayerNorm.bias", "intermediate.dense.weight", "intermediate.dense.bias", "output.dense.weight",
                   "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias")
TEXT_CLAP_TAIL = ("model.pooler.dense.weight", "model.pooler.dense.bias", "projection.linear1.weight", "projection.linear1.bias",
                  "projection.linear2.weight", "projection.linear2.bias")
#: what the forward keeps per layer for the backward, in the order the operator returns it
TEXT_CLAP_SAVED_LAYER = ("x", "qkv", "attn", "ctx", "xhat1", "rstd1", "h1", "u", "f", "xhat2", "rstd2")
TEXT_CLAP_SAVED_HEAD = ("pos_ids", "klen", "xhat0", "rstd0", "buf", "t1", "seq_raw")


def text_clap_param_names(layers):
    """State-dict names of LaionClapEncoder's parameters in the order the operator takes them: 5 of the embedding block, 16 per
    layer, the pooler and the two projection layers."""
    return (["model." + n for n in TEXT_CLAP_HEAD]
            + [f"model.encoder.layer.{l}.{n}" for l in range(layers) for n in TEXT_CLAP_LAYER] + list(TEXT_CLAP_TAIL))


def text_clap_layers(n_params):
    layers, rest = divmod(n_params - len(TEXT_CLAP_HEAD) - len(TEXT_CLAP_TAIL), len(TEXT_CLAP_LAYER))
    if layers < 1 or rest:
        raise ValueError(f"text_clap: {n_params} parameters are not 5 + 16 per layer (>= 1 layer) + 6")
    return layers


def text_clap_dropout_seeds(seed, layers):
    """(seed behind the embedding LayerNorm, [(attention weights, behind attention.output.dense, behind output.dense)] per layer)
    -- Hugging Face's four dropout sites -- from ONE operator seed: seed, then seed + 1 + 3 l + {0, 1, 2}, modulo 2^62."""
    s = int(seed)
    return s % (2 ** 62), [tuple((s + 1 + 3 * l + k) % (2 ** 62) for k in range(3)) for l in range(layers)]


def text_clap_check(D, heads, L=None):
    """The domain of the tower's kernels, raised before any launch with the limit named."""
    text_selfattn_check(D, heads)
    if L is not None and not 2 <= L <= TEXT_CLAP_MAX_L:
        raise ValueError(f"text_clap: {L} tokens per phrase; the attention kernel serves 2 ... {TEXT_CLAP_MAX_L} tokens and there is "
                         "no eager fallback")


def text_clap_resln_forward(x, res, gamma, beta, eps, need_state=True, out=None):
    """y = LayerNorm(x + res) gamma + beta over the rows of x (M, D), res (M, D) or None -> y, xhat (M, D), rstd (M) (None unless
    need_state).  out: a (M, D) destination for y."""
    x = _chk(x, "x")
    M, D = x.shape
    res = _chk(res, "res") if res is not None else None
    y = out if out is not None else _empty(M, D, like=x)
    xhat = _empty(M, D, like=x) if need_state else None
    rstd = _empty(M, like=x) if need_state else None
    call("tag_text_clap_resln_forward", ptr(x), ptr(res), ptr(_chk(gamma, "gamma")), ptr(_chk(beta, "beta")), float(eps), ptr(y),
         ptr(xhat), ptr(rstd), M, D)
    return y, xhat, rstd


def text_clap_resln_backward(dy, xhat, rstd, gamma, need_dgamma=True, need_dbeta=True, dgamma_out=None, dbeta_out=None):
    """-> ds (M, D) (the gradient of x AND of res), dgamma, dbeta (D) (None when not needed; written into *_out when given)."""
    dy, xhat = _chk(dy, "grad"), _chk(xhat, "xhat")
    M, D = xhat.shape
    ds = _empty(M, D, like=dy)
    dg = (dgamma_out if dgamma_out is not None else _empty(D, like=dy)) if need_dgamma else None
    db = (dbeta_out if dbeta_out is not None else _empty(D, like=dy)) if need_dbeta else None
    ws = _ws(query("tag_text_clap_resln_backward_ws_bytes", M, D), dy) if (need_dgamma or need_dbeta) else None
    call("tag_text_clap_resln_backward", ptr(dy), ptr(xhat), ptr(_chk(rstd, "rstd")), ptr(_chk(gamma, "gamma")), ptr(ds), ptr(dg),
         ptr(db), M, D, ptr(ws))
    return ds, dg, db


def _clap_ids_chk(ids, what):
    if not ids.is_cuda or ids.dtype != torch.long:
        raise RuntimeError(f"text_clap: {what} must be an int64 tensor on the device (no CPU fallback)")
    return ids.contiguous()


def text_clap_embed_forward(ids, word, type0, pos, gamma, beta, eps, pad_id, need_state=True):
    """ClapTextEmbeddings: ids (B, L) int64 -> h (B*L, D) = LayerNorm(word[ids] + type0 + pos[position ids]), the position ids
    (B*L) int64, xhat (B*L, D), rstd (B*L) (the last three None unless need_state)."""
    ids = _clap_ids_chk(ids, "input_ids")
    B, L = ids.shape
    word, pos = _chk(word, "word_embeddings"), _chk(pos, "position_embeddings")
    V, D = word.shape
    M = B * L
    h = _empty(M, D, like=word)
    pos_ids = torch.empty(M, device=ids.device, dtype=torch.long) if need_state else None
    xhat = _empty(M, D, like=word) if need_state else None
    rstd = _empty(M, like=word) if need_state else None
    call("tag_embed_check_ids", ptr(ids), M, V, ptr(_embed_flag(word)))       # nn.Embedding raises; see check_async_errors
    call("tag_text_clap_embed_forward", ptr(ids), ptr(word), ptr(_chk(type0, "token_type_embeddings")), ptr(pos),
         ptr(_chk(gamma, "gamma")), ptr(_chk(beta, "beta")), float(eps), ptr(h), ptr(pos_ids), ptr(xhat), ptr(rstd), B, L, D, V,
         pos.shape[0], int(pad_id))
    return h, pos_ids, xhat, rstd


def text_clap_embed_backward(dh, xhat, rstd, gamma, ids, pos_ids, V, P, pad_id, need=None, outs=None):
    """dh (B*L, D) -> [dword (V, D), dtype0 (1, D), dpos (P, D), dgamma (D), dbeta (D)] (None where need[i] is False).  outs:
    optional destination per gradient; the two table destinations must be ZEROED (the flat-gradient rows after zero_grad): the
    gather accumulates.  Row pad_id of dword and dpos receives exactly zero."""
    dh = _chk(dh, "grad")
    ids, pos_ids = _clap_ids_chk(ids, "input_ids"), _clap_ids_chk(pos_ids, "position ids")
    B, L = ids.shape
    D = dh.shape[-1]
    need = list(need) if need is not None else [True] * 5
    outs = list(outs) if outs is not None else [None] * 5
    if not any(need):
        return [None] * 5
    shapes = ((V, D), (1, D), (P, D), (D,), (D,))
    g = [None] * 5
    for i in range(5):
        if need[i]:
            g[i] = outs[i] if outs[i] is not None else (torch.zeros if i in (0, 2) else torch.empty)(
                shapes[i], device=dh.device, dtype=F32)
    ws = _ws(query("tag_text_clap_embed_backward_ws_bytes", B, L, D), dh)
    call("tag_text_clap_embed_backward", ptr(dh), ptr(_chk(xhat, "xhat")), ptr(_chk(rstd, "rstd")), ptr(_chk(gamma, "gamma")),
         ptr(ids), ptr(pos_ids), ptr(g[0]), ptr(g[2]), ptr(g[1]), ptr(g[3]), ptr(g[4]), B, L, D, V, P, int(pad_id), ptr(ws))
    return g


def text_clap_gelu_forward(u):
    f = torch.empty_like(_chk(u, "u"))
    call("tag_text_clap_gelu_forward", ptr(u), ptr(f), u.numel())
    return f


def text_clap_gelu_backward(u, df):
    """du = df (Phi(u) + u phi(u)) on the saved pre-activation u."""
    du = torch.empty_like(_chk(u, "u"))
    call("tag_text_clap_gelu_backward", ptr(u), ptr(_chk(df, "grad")), ptr(du), u.numel())
    return du


def text_clap_tanh_backward(y, dy):
    """dx = dy (1 - y^2); y, dy any contiguous views of the same size."""
    if not (y.is_contiguous() and dy.is_contiguous()):
        raise RuntimeError("text_clap_tanh_backward: contiguous tensors expected")
    dx = torch.empty_like(_chk(y, "y"))
    call("tag_text_clap_tanh_backward", ptr(y), ptr(_chk(dy, "grad")), ptr(dx), y.numel())
    return dx


def text_clap_l2norm_backward(x, du):
    """Gradient of F.normalize over the rows of x (R, P)."""
    x, du = _chk(x, "x"), _chk(du, "grad")
    dx = torch.empty_like(x)
    call("tag_l2norm_rows_backward", ptr(x), ptr(du), ptr(dx), x.shape[0], x.shape[1])
    return dx


def _clap_dropout(x2d, p, seed, backward=False):
    return text_gru_dropout(x2d, p, seed, backward) if p > 0.0 else x2d


def _text_stack_forward(h, klen, params, layers, R, L, heads, eps, need_grad, p_hidden, p_attn, s_layers, last_out=None):
    """The post-LayerNorm encoder layers shared by the CLAP and the BERT tower: per layer the packed q|k|v GEMM, the attention
    core, the out-projection, residual LayerNorm, GELU feed-forward and the second residual LayerNorm.  h (R*L, D) behind the
    embedding block; params[5 + 16 l ...] the layer's 16 parameters; last_out: a (R*L, D) destination of the last layer's rows.
    -> the last hidden state (R*L, D), what the backward reads per layer ([] unless need_grad)."""
    M, D = h.shape
    saved = []
    for l in range(layers):
        b = 5 + 16 * l
        qw, qb, kw, kb, vw, vb, aow, aob, g1, b1, iw, ib, ow, ob, g2, b2 = params[b:b + 16]
        s_attn, s_ao, s_out = s_layers[l]
        I = iw.shape[0]
        wqkv, bqkv = torch.cat((qw, kw, vw), 0), torch.cat((qb, kb, vb), 0)
        qkv = gemm(h, wqkv, M, 3 * D, D, transB=True, bias=bqkv)
        ctx, attn = text_selfattn_core(qkv.view(R, L, 3 * D), klen, heads, need_grad, p_attn, s_attn)
        ctx = ctx.view(M, D)
        a = _clap_dropout(gemm(ctx, aow, M, D, D, transB=True, bias=aob), p_hidden, s_ao)
        h1, xhat1, rstd1 = text_clap_resln_forward(a, h, g1, b1, eps, need_grad)
        u = gemm(h1, iw, M, I, D, transB=True, bias=ib)      # no fused activation: the backward reads the pre-activation
        f = text_clap_gelu_forward(u)
        f2 = _clap_dropout(gemm(f, ow, M, D, I, transB=True, bias=ob), p_hidden, s_out)
        hn, xhat2, rstd2 = text_clap_resln_forward(f2, h1, g2, b2, eps, need_grad, out=last_out if l == layers - 1 else None)
        if need_grad:
            saved.append(dict(x=h, qkv=qkv, attn=attn, ctx=ctx, xhat1=xhat1, rstd1=rstd1, h1=h1, u=u, f=f, xhat2=xhat2, rstd2=rstd2,
                              wqkv=wqkv))
        h = hn
    return h, saved


def _text_stack_backward(dh, saved_layers, klen, params, layers, R, L, heads, p_hidden, p_attn, s_layers, need, outs, g):
    """Backward of _text_stack_forward: dh (R*L, D) on the last hidden state -> the gradient behind the embedding block, or None
    when the walk stopped because nothing below needs a gradient.  Fills g[5 + 16 l ...] where need says so (outs: destinations)."""
    M, D = dh.shape

    def below(i):                                   # does anything at an index < i need a gradient?
        return any(need[:i])

    for l in range(layers - 1, -1, -1):
        b = 5 + 16 * l
        sv = saved_layers[l]
        _, _, _, _, _, _, aow, _, g1, _, iw, _, ow, _, g2, _ = params[b:b + 16]
        s_attn, s_ao, s_out = s_layers[l]
        I = iw.shape[0]
        ds2, g[b + 14], g[b + 15] = text_clap_resln_backward(dh, sv["xhat2"], sv["rstd2"], g2, need[b + 14], need[b + 15],
                                                             outs[b + 14], outs[b + 15])
        df2 = _clap_dropout(ds2, p_hidden, s_out, backward=True)
        if need[b + 12]:
            g[b + 12] = gemm(df2, sv["f"], D, I, M, transA=True, lda=D, out=outs[b + 12])
        if need[b + 13]:
            g[b + 13] = colsum(df2, M, D, out=outs[b + 13])
        if not below(b + 12):
            return None
        du = text_clap_gelu_backward(sv["u"], gemm(df2, ow, M, I, D))
        if need[b + 10]:
            g[b + 10] = gemm(du, sv["h1"], I, D, M, transA=True, lda=I, out=outs[b + 10])
        if need[b + 11]:
            g[b + 11] = colsum(du, M, I, out=outs[b + 11])
        if not below(b + 10):
            return None
        dh1 = gemm(du, iw, M, D, I, out=ds2, accumulate=True)                           # + the residual branch (df2 is spent)
        ds1, g[b + 8], g[b + 9] = text_clap_resln_backward(dh1, sv["xhat1"], sv["rstd1"], g1, need[b + 8], need[b + 9],
                                                           outs[b + 8], outs[b + 9])
        if not below(b + 8):
            return None
        da = _clap_dropout(ds1, p_hidden, s_ao, backward=True)
        if need[b + 6]:
            g[b + 6] = gemm(da, sv["ctx"], D, D, M, transA=True, lda=D, out=outs[b + 6])
        if need[b + 7]:
            g[b + 7] = colsum(da, M, D, out=outs[b + 7])
        if not below(b + 6):
            return None
        dctx = gemm(da, aow, M, D, D)
        dqkv = text_selfattn_core_backward(sv["qkv"].view(R, L, 3 * D), sv["attn"], dctx.view(R, L, D), klen, heads,
                                           p_attn, s_attn).view(M, 3 * D)
        for j in range(3):
            if need[b + 2 * j]:
                g[b + 2 * j] = gemm(dqkv[:, j * D:], sv["x"], D, D, M, transA=True, lda=3 * D, out=outs[b + 2 * j])
            if need[b + 2 * j + 1]:
                g[b + 2 * j + 1] = colsum(dqkv[:, j * D:], M, D, ld=3 * D, out=outs[b + 2 * j + 1])
        if not below(b):
            return None
        dh = gemm(dqkv, sv["wqkv"], M, D, 3 * D, out=ds1, accumulate=True)              # + the residual branch (da is spent)
    return dh


def text_clap_forward(ids, mask, params, heads, eps, pad_id, need_grad, p_hidden=0.0, p_attn=0.0, seed=0):
    """LaionClapEncoder.forward (models/text_encoder.py:320-327) over Hugging Face's ClapTextModel + ClapProjectionLayer:
    ids, mask (R, L) int64 on the device, mask a right-padded prefix (only its row sums are read: klen = mask.sum(-1), a row
    without a valid key attends position 0 -- the clamp of the attention core); params in the order of text_clap_param_names.
    p_hidden / p_attn > 0 (train): Hugging Face's dropouts behind the embedding LayerNorm, on the attention weights, behind
    attention.output.dense and behind output.dense, keep masks of text_clap_dropout_seeds(seed, layers) over the flat index of
    (R*L, D) / (R, H, L, L).  -> token_emb (R, L, P), seq_emb (R, P) L2-normalised, saved state or None."""
    ids, mask = _clap_ids_chk(ids, "input_ids"), _clap_ids_chk(mask, "attention_mask")
    R, L = ids.shape
    layers = text_clap_layers(len(params))
    params = [_chk(p, "parameter") for p in params]
    word, type0, pos, g0, b0 = params[:5]
    D = word.shape[1]
    text_clap_check(D, heads, L)
    if pos.shape[0] <= L + pad_id:
        raise ValueError(f"text_clap: the position table has {pos.shape[0]} rows; {L} tokens need {L + pad_id + 1}")
    M = R * L
    klen = mask.sum(-1)
    s_emb, s_layers = text_clap_dropout_seeds(seed, layers)
    h, pos_ids, xhat0, rstd0 = text_clap_embed_forward(ids, word, type0, pos, g0, b0, eps, pad_id, need_grad)
    h = _clap_dropout(h, p_hidden, s_emb)
    buf = h.new_empty(M + R, D)                       # the last layer's rows, then the pooled rows: ONE projection over both
    h, saved = _text_stack_forward(h, klen, params, layers, R, L, heads, eps, need_grad, p_hidden, p_attn, s_layers, buf[:M])
    pw, pb, w1, c1, w2, c2 = params[-6:]
    P = w1.shape[0]
    gemm(buf, pw, R, D, D, transB=True, lda=L * D, bias=pb, act=4, out=buf[M:])         # tanh(dense(h[:, 0]))
    t1 = gemm(buf, w1, M + R, P, D, transB=True, bias=c1, act=1)
    t2 = gemm(t1, w2, M + R, P, P, transB=True, bias=c2)
    seq_raw = t2[M:]
    seq = _l2norm_rows(seq_raw, R, P)
    state = dict(pos_ids=pos_ids, klen=klen, xhat0=xhat0, rstd0=rstd0, buf=buf, t1=t1, seq_raw=seq_raw, layers=saved) \
        if need_grad else None
    return t2[:M].view(R, L, P), seq, state


def text_clap_backward(dtok, dseq, ids, saved, params, heads, pad_id, p_hidden=0.0, p_attn=0.0, seed=0, outs=None, need=None):
    """-> one gradient per parameter (text_clap_param_names order).  dtok (R, L, P) / dseq (R, P): either may be None.  outs:
    optional destination per parameter (flat-gradient views), written directly -- the two embedding tables' must be zeroed, the
    gather accumulates; need: per parameter, False skips its GEMM / column sum (a frozen parameter) and leaves None.  The walk
    stops below the lowest parameter that needs a gradient.  The q / k / v weights are used packed; their gradients go to the
    three parameters separately."""
    n = len(params)
    layers = text_clap_layers(n)
    params = [_chk(p, "parameter") for p in params]
    outs = list(outs) if outs is not None else [None] * n
    need = list(need) if need is not None else [True] * n
    g = [None] * n
    if not any(need):
        return g
    R, L = ids.shape
    M = R * L
    D = params[0].shape[1]
    pw, _, w1, _, w2, _ = params[-6:]
    P = w1.shape[0]
    buf, t1 = saved["buf"], saved["t1"]
    s_emb, s_layers = text_clap_dropout_seeds(seed, layers)

    def below(i):                                   # does anything at an index < i need a gradient?
        return any(need[:i])

    dt2 = buf.new_zeros(M + R, P) if (dtok is None or dseq is None) else buf.new_empty(M + R, P)
    if dtok is not None:
        dt2[:M].copy_(_chk(dtok, "grad").view(M, P))
    if dseq is not None:
        dt2[M:].copy_(text_clap_l2norm_backward(saved["seq_raw"], dseq))
    if need[n - 2]:
        g[n - 2] = gemm(dt2, t1, P, P, M + R, transA=True, lda=P, out=outs[n - 2])
    if need[n - 1]:
        g[n - 1] = colsum(dt2, M + R, P, out=outs[n - 1])
    if not below(n - 2):
        return g
    dt1 = relu_backward(t1, gemm(dt2, w2, M + R, P, P))
    if need[n - 4]:
        g[n - 4] = gemm(dt1, buf, P, D, M + R, transA=True, lda=P, out=outs[n - 4])
    if need[n - 3]:
        g[n - 3] = colsum(dt1, M + R, P, out=outs[n - 3])
    if not below(n - 4):
        return g
    dbuf = gemm(dt1, w1, M + R, D, P)
    dpre = text_clap_tanh_backward(buf[M:], dbuf[M:])
    if need[n - 6]:
        g[n - 6] = gemm(dpre, buf, D, D, R, transA=True, lda=D, ldb=L * D, out=outs[n - 6])
    if need[n - 5]:
        g[n - 5] = colsum(dpre, R, D, out=outs[n - 5])
    if not below(n - 6):
        return g
    gemm(dpre, pw, R, D, D, out=dbuf, ldc=L * D, accumulate=True)                       # into the rows h[:, 0]
    dh = dbuf[:M]
    dh = _text_stack_backward(dh, saved["layers"], saved["klen"], params, layers, R, L, heads, p_hidden, p_attn, s_layers, need, outs, g)
    if dh is None:
        return g
    dh0 = _clap_dropout(dh, p_hidden, s_emb, backward=True)
    g[:5] = text_clap_embed_backward(dh0, saved["xhat0"], saved["rstd0"], params[3], ids, saved["pos_ids"], params[0].shape[0],
                                     params[2].shape[0], pad_id, need[:5], outs[:5])
    return g


# ------------------------------------------------------------------------------------------------
# BERT for training (row T7; models/text_encoder.py:271-308 Bert / SentenceBert over Hugging Face's BertModel): BertEmbeddings
# (token types, absolute positions) and the sentence poolings of csrc/text_bert.hip around the encoder stack of the CLAP tower
# ------------------------------------------------------------------------------------------------
TEXT_BERT_POOLER = ("model.pooler.dense.weight", "model.pooler.dense.bias")
TEXT_BERT_SAVED_HEAD = ("klen", "xhat0", "rstd0", "raw")
TEXT_BERT_POOL_MODES = {"cls": 0, "mean": 1}
TEXT_BERT_NORMS = {"none": 0, "normalize": 1, "retrieval": 2}
TEXT_BERT_MAX_TYPES = 16


def text_bert_param_names(layers, pooler=True):
    """State-dict names of Bert's / SentenceBert's parameters in the order the operator takes them: 5 of the embedding block, 16
    per layer, then (pooler) BertPooler's two -- held for checkpoint compatibility, they take no part in the arithmetic."""
    return (["model." + n for n in TEXT_CLAP_HEAD]
            + [f"model.encoder.layer.{l}.{n}" for l in range(layers) for n in TEXT_CLAP_LAYER]
            + (list(TEXT_BERT_POOLER) if pooler else []))


def text_bert_layers(n_params):
    """-> (layers, pooler parameters present) from the number of parameters."""
    rest = n_params - len(TEXT_CLAP_HEAD)
    layers, tail = divmod(rest, len(TEXT_CLAP_LAYER))
    if layers < 1 or tail not in (0, 2):
        raise ValueError(f"text_bert: {n_params} parameters are not 5 + 16 per layer (>= 1 layer) (+ 2 of the pooler)")
    return layers, tail == 2


def text_bert_check(D, heads, L=None, P=None, T=None, pool_mode=None, norm=None, need_grad=False):
    """The domain of the BERT path, raised before any launch with the limit named: the tower's limits (text_clap_check), L within
    the position table, at most 16 token types, a known pooling / normalisation, and no backward through normalisation 2."""
    try:
        text_selfattn_check(D, heads)
    except NotImplementedError as e:                # one exception type for every limit of this path
        raise ValueError(str(e)) from None
    if L is not None and not 2 <= L <= TEXT_CLAP_MAX_L:
        raise ValueError(f"text_bert: {L} tokens per phrase; the attention kernel serves 2 ... {TEXT_CLAP_MAX_L} tokens and there is "
                         "no eager fallback")
    if L is not None and P is not None and L > P:
        raise ValueError(f"text_bert: {L} tokens per phrase but max_position_embeddings is {P}")
    if T is not None and not 1 <= T <= TEXT_BERT_MAX_TYPES:
        raise ValueError(f"text_bert: type_vocab_size {T}; the token-type gradient serves 1 ... {TEXT_BERT_MAX_TYPES} types")
    if pool_mode is not None and pool_mode not in (0, 1):
        raise ValueError(f"text_bert: pooling mode {pool_mode!r}; 0 ([CLS]) and 1 (masked mean) exist")
    if norm is not None and norm not in (0, 1, 2):
        raise ValueError(f"text_bert: normalisation {norm!r}; 0 (none), 1 (F.normalize) and 2 (x / (|x| + 1e-7), clipped) exist")
    if norm == 2 and need_grad:
        raise ValueError("text_bert: normalisation 2 (the retrieval model's) is forward-only")


def text_bert_embed_forward(ids, type_ids, word, type_tab, pos, gamma, beta, eps, need_state=True):
    """BertEmbeddings: ids, type_ids (B, L) int64 (type_ids None = all zeros) -> h (B*L, D) = LayerNorm(word[ids] + type[type_ids]
    + pos[column]), xhat (B*L, D), rstd (B*L) (None unless need_state)."""
    ids = _clap_ids_chk(ids, "input_ids")
    type_ids = _clap_ids_chk(type_ids, "token_type_ids") if type_ids is not None else None
    B, L = ids.shape
    word, type_tab, pos = _chk(word, "word_embeddings"), _chk(type_tab, "token_type_embeddings"), _chk(pos, "position_embeddings")
    V, D = word.shape
    T, P = type_tab.shape[0], pos.shape[0]
    if L > P:
        raise ValueError(f"text_bert: {L} tokens per phrase but the position table has {P} rows")
    if type_ids is not None and tuple(type_ids.shape) != (B, L):
        raise ValueError(f"text_bert: token_type_ids {tuple(type_ids.shape)} and input_ids {(B, L)} differ in shape")
    M = B * L
    h = _empty(M, D, like=word)
    xhat = _empty(M, D, like=word) if need_state else None
    rstd = _empty(M, like=word) if need_state else None
    call("tag_embed_check_ids", ptr(ids), M, V, ptr(_embed_flag(word)))       # nn.Embedding raises; see check_async_errors
    if type_ids is not None:
        call("tag_embed_check_ids", ptr(type_ids), M, T, ptr(_embed_flag(word)))
    call("tag_text_bert_embed_forward", ptr(ids), ptr(type_ids), ptr(word), ptr(type_tab), ptr(pos), ptr(_chk(gamma, "gamma")),
         ptr(_chk(beta, "beta")), float(eps), ptr(h), ptr(xhat), ptr(rstd), B, L, D, V, T, P)
    return h, xhat, rstd


def text_bert_embed_backward(dh, xhat, rstd, gamma, ids, type_ids, V, T, P, pad_id, need=None, outs=None):
    """dh (B*L, D) -> [dword (V, D), dtype (T, D), dpos (P, D), dgamma (D), dbeta (D)] (None where need[i] is False).  outs:
    optional destination per gradient; the table destinations must be ZEROED (the flat-gradient rows after zero_grad): dword is
    accumulated by the gather and only the first L rows of dpos are written.  Row pad_id of dword receives exactly zero (pad_id
    None / negative: no padding index); padded positions DO contribute to dtype and dpos, as in Hugging Face."""
    dh = _chk(dh, "grad")
    ids = _clap_ids_chk(ids, "input_ids")
    type_ids = _clap_ids_chk(type_ids, "token_type_ids") if type_ids is not None else None
    B, L = ids.shape
    D = dh.shape[-1]
    need = list(need) if need is not None else [True] * 5
    outs = list(outs) if outs is not None else [None] * 5
    if not any(need):
        return [None] * 5
    shapes = ((V, D), (T, D), (P, D), (D,), (D,))
    g = [None] * 5
    for i in range(5):
        if need[i]:
            g[i] = outs[i] if outs[i] is not None else (torch.zeros if i in (0, 2) else torch.empty)(
                shapes[i], device=dh.device, dtype=F32)
    ws = _ws(query("tag_text_bert_embed_backward_ws_bytes", B, L, D, T), dh)
    call("tag_text_bert_embed_backward", ptr(dh), ptr(_chk(xhat, "xhat")), ptr(_chk(rstd, "rstd")), ptr(_chk(gamma, "gamma")),
         ptr(ids), ptr(type_ids), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(g[4]), B, L, D, V, T, P,
         -1 if pad_id is None else int(pad_id), ptr(ws))
    return g


def text_bert_pool_forward(h, klen, mode, norm, need_raw=False):
    """h (R, L, D), klen (R) int64 -> seq (R, D), raw (R, D) or None: the sentence pooling (0 [CLS], 1 masked mean over the first
    klen rows) and normalisation (0 none, 1 F.normalize, 2 x / (|x| + 1e-7) clipped to +-1e3) in one pass."""
    h = _chk(h, "h")
    R, L, D = h.shape
    if mode not in (0, 1) or norm not in (0, 1, 2):
        raise ValueError(f"text_bert: pooling mode {mode!r} / normalisation {norm!r}")
    if klen is None and mode == 1:
        raise ValueError("text_bert: the masked mean needs klen")
    klen = _klen_chk(klen, R) if klen is not None else None
    out = _empty(R, D, like=h)
    raw = _empty(R, D, like=h) if need_raw else None
    call("tag_text_bert_pool_forward", ptr(h), ptr(klen), int(mode), int(norm), ptr(raw), ptr(out), R, L, D)
    return out, raw


def text_bert_pool_backward(dseq, dtok, raw, klen, mode, norm, shape):
    """-> dh (R, L, D) = dtok (or zero) + the pooling's gradient of dseq (R, D) (or nothing) on row 0 / the first klen rows,
    through the F.normalize backward when norm is 1 (raw: the forward's pooled rows)."""
    R, L, D = shape
    if norm not in (0, 1):
        raise ValueError("text_bert: normalisation 2 (the retrieval model's) is forward-only")
    if mode not in (0, 1):
        raise ValueError(f"text_bert: pooling mode {mode!r}")
    if dseq is None and dtok is None:
        raise ValueError("text_bert_pool_backward: neither dseq nor dtok")
    like = dseq if dseq is not None else dtok
    dseq = _chk(dseq, "grad") if dseq is not None else None
    dtok = _chk(dtok, "grad") if dtok is not None else None
    if klen is None and mode == 1:
        raise ValueError("text_bert: the masked mean needs klen")
    klen = _klen_chk(klen, R) if klen is not None else None
    dh = _empty(R, L, D, like=like)
    call("tag_text_bert_pool_backward", ptr(dseq), ptr(dtok), ptr(_chk(raw, "raw")) if norm == 1 else None, ptr(klen), int(mode),
         int(norm), ptr(dh), R, L, D)
    return dh


def text_bert_forward(ids, type_ids, mask, params, heads, eps, pad_id, pool_mode, norm, need_grad, p_hidden=0.0, p_attn=0.0,
                      seed=0):
    """Bert.forward / SentenceBert.forward (models/text_encoder.py:281-308) over Hugging Face's BertModel: ids, mask (R, L) int64 on
    the device, type_ids the same or None (all zeros), mask a right-padded prefix (only its row sums are read, as in
    text_clap_forward); params in the order of text_bert_param_names (with or without the pooler's two, which are not read).
    pool_mode 0 [CLS] / 1 masked mean, norm 0 none / 1 F.normalize / 2 the retrieval model's (forward-only).  Dropout sites and
    seeds are text_clap_dropout_seeds'.  -> token_emb (R, L, D) the last hidden state, seq_emb (R, D), saved state or None."""
    ids, mask = _clap_ids_chk(ids, "input_ids"), _clap_ids_chk(mask, "attention_mask")
    R, L = ids.shape
    layers, _ = text_bert_layers(len(params))
    params = [_chk(p, "parameter") for p in params]
    word, type_tab, pos, g0, b0 = params[:5]
    D = word.shape[1]
    text_bert_check(D, heads, L, pos.shape[0], type_tab.shape[0], pool_mode, norm, need_grad)
    klen = mask.sum(-1)
    s_emb, s_layers = text_clap_dropout_seeds(seed, layers)
    h, xhat0, rstd0 = text_bert_embed_forward(ids, type_ids, word, type_tab, pos, g0, b0, eps, need_grad)
    h = _clap_dropout(h, p_hidden, s_emb)
    h, saved = _text_stack_forward(h, klen, params, layers, R, L, heads, eps, need_grad, p_hidden, p_attn, s_layers)
    tok = h.view(R, L, D)
    seq, raw = text_bert_pool_forward(tok, klen, pool_mode, norm, need_grad and norm == 1)
    state = None
    if need_grad:
        state = dict(klen=klen, xhat0=xhat0, rstd0=rstd0, raw=raw if raw is not None else seq, layers=saved)
    return tok, seq, state


def text_bert_backward(dtok, dseq, ids, type_ids, saved, params, heads, pad_id, pool_mode, norm, p_hidden=0.0, p_attn=0.0, seed=0,
                       outs=None, need=None):
    """-> one gradient per parameter (text_bert_param_names order; the pooler's stay None).  dtok (R, L, D) / dseq (R, D): either
    may be None.  outs / need: as in text_clap_backward -- destinations written directly (the embedding tables' must be zeroed) and
    per-parameter switches; the walk stops below the lowest parameter that needs a gradient."""
    n = len(params)
    layers, pooler = text_bert_layers(n)
    params = [_chk(p, "parameter") for p in params]
    outs = list(outs) if outs is not None else [None] * n
    need = list(need) if need is not None else [True] * n
    if pooler:
        need[-2:] = [False, False]                  # BertPooler takes no part in the arithmetic
    g = [None] * n
    if not any(need) or (dtok is None and dseq is None):
        return g
    R, L = ids.shape
    D = params[0].shape[1]
    M = R * L
    s_emb, s_layers = text_clap_dropout_seeds(seed, layers)
    if dseq is None:
        dh = _chk(dtok, "grad").view(M, D)
    else:
        dh = text_bert_pool_backward(dseq, dtok, saved["raw"], saved["klen"], pool_mode, norm, (R, L, D)).view(M, D)
    dh = _text_stack_backward(dh, saved["layers"], saved["klen"], params, layers, R, L, heads, p_hidden, p_attn, s_layers, need, outs, g)
    if dh is None:
        return g
    dh0 = _clap_dropout(dh, p_hidden, s_emb, backward=True)
    g[:5] = text_bert_embed_backward(dh0, saved["xhat0"], saved["rstd0"], params[3], ids, type_ids, params[0].shape[0],
                                     params[1].shape[0], params[2].shape[0], pad_id, need[:5], outs[:5])
    return g


# ------------------------------------------------------------------------------------------------
# One conv3x3 -> BatchNorm -> ReLU (-> pool) stage as a standalone operator: what SURVEY.md section 8(b) lists as
# ``conv3x3_bn_relu[_pool]`` and what ConvBlock.forward (models/panns.py:46-62) is made of.  The fused Cnn8Rnn node (functions.py)
# never materialises relu(bn(y)); this stage does (its output IS that tensor, pooled), so that it composes like an nn.Module.
# ------------------------------------------------------------------------------------------------
POOL_TYPES = {"avg+max": 0, "avg": 2, "max": 3}
POOL_SIZES = {(1, 1), (1, 2), (2, 1), (2, 2)}      # (time, mel) windows instantiated for forward AND backward in bn_pool.hip


def conv_bn_relu_pool_forward(x, w, gamma, beta, running_mean, running_var, training, momentum, eps, ph, pw, pool):
    """x channels-last (B,H,W,Cin) fp32; w (Cout,Cin,3,3).  -> (out (B,H/ph,W/pw,Cout), y raw conv output, BNStat).
    running statistics are updated in place when training (nn.BatchNorm2d semantics)."""
    x = _chk(x, "x")
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    if (ph, pw) not in POOL_SIZES:
        raise RuntimeError(f"conv3x3_bn_relu_pool: pool_size {(ph, pw)} has no kernel instance (built: {sorted(POOL_SIZES)})")
    if Cin == 1:
        y, part = conv3x3_c1_stats(x.view(B, H, W), w, want_stats=training)
    elif Cin % 32 == 0:
        wf, _ = pack_conv_weight(w, want_dgrad=False, W=W)
        y, part = conv3x3_stats(x, wf, Cout, want_stats=training)
    else:
        raise RuntimeError(f"conv3x3_bn_relu_pool: in_channels must be 1 or a multiple of 32, got {Cin}")
    st = bn_stats(y.view(-1, Cout), gamma, beta, running_mean, running_var, training, eps, momentum, partials=part)
    out = bnact_pool(y, st, ph, pw, act=1, pool=pool)
    return out, y, st


def conv_bn_relu_pool_backward(dout, x, w, y, st: BNStat, gamma, ph, pw, pool, need_dx=True):
    """-> (dx or None, dw, dgamma, dbeta): BatchNorm/ReLU/pool backward (two passes over y), weight gradient and input
    gradient of the stage above."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    dy, dg, db = bnrelu_pool_backward(y, st, gamma, _chk(dout, "grad_output"), ph, pw, pool=pool)
    if Cin == 1:
        dw = conv3x3_c1_wgrad(x.view(B, H, W), dy)
        dx = conv3x3_c1_dgrad(dy, w).view(B, H, W, 1) if need_dx else None
    else:
        dw = conv3x3_wgrad(x, dy)
        dx = None
        if need_dx:
            _, wd = pack_conv_weight(w, want_dgrad=True, W=W)
            dx = conv3x3(dy, wd, Cin)
    return dx, dw, dg, db


# ------------------------------------------------------------------------------------------------
# launches of CrnnEncoder (row A1') and of the text / match / loss heads
# ------------------------------------------------------------------------------------------------

def bn_act_backward(x, pre_op, st: BNStat, gamma, du, dg_out=None, db_out=None):
    C = x.shape[-1]
    rows = x.numel() // C
    dx = torch.empty_like(x)
    dg, db = _dg_db(dg_out, db_out, C, x)
    ws = _ws(query("tag_bn_backward_ws_bytes", rows, C), x)
    call("tag_bn_act_backward", ptr(x), pre_op, ptr(st.mean), ptr(st.invstd), ptr(gamma), ptr(du), ptr(dx), ptr(dg),
         ptr(db), rows, C, int(st.train), ptr(ws))
    return dx, dg, db


def lppool_leaky_backward(y, dout, ph, pw, drop_p=0.0, seed=0):
    B, H, W, C = y.shape
    dy = torch.empty_like(y)
    call("tag_lppool_leaky_backward", ptr(y), ptr(dout), ptr(dy), B, H, W, C, ph, pw, float(drop_p), seed)
    return dy


def embed_mean_forward(table, text, text_len, want_tokens=True):
    """nn.Embedding gather + mean over the valid tokens (rows T1/T2): -> (seq_emb (B,D), token_emb (B,L,D) or None)."""
    tab = _chk(table, "embedding table")
    if not text.is_cuda:
        raise RuntimeError("embed_mean: token ids must live on the device (no CPU fallback)")
    B, L = text.shape
    V, D = tab.shape
    seq = _empty(B, D, like=tab)
    tok = _empty(B, L, D, like=tab) if want_tokens else None
    call("tag_embed_check_ids", ptr(text), B * L, V, ptr(_embed_flag(tab)))     # nn.Embedding raises; see check_async_errors
    call("tag_embed_mean_forward", ptr(text), ptr(text_len), ptr(tab), ptr(tok), ptr(seq), B, L, D, V)
    return seq, tok


def embed_mean_backward_into(dtab, dseq, dtok, text, text_len):
    """Adds the seq_emb / token_emb gradients into ``dtab`` (V,D) -- a zeroed tensor or the zeroed flat-gradient rows of the
    table.  Deterministic (fixed-order per-row sums, no atomics)."""
    B, L = text.shape
    V, D = dtab.shape
    if dseq is not None:
        call("tag_embed_mean_backward", ptr(_chk(dseq, "grad")), ptr(text), ptr(text_len), ptr(dtab), B, L, D, V)
    if dtok is not None:
        call("tag_embed_tokens_backward", ptr(_chk(dtok, "grad")), ptr(text), ptr(dtab), B, L, D, V)
    return dtab


def _check_pair_batch(what, a, t):
    """Heads that pair audio clip b with text row b: the batches must agree (the reference's broadcast / assert fails otherwise;
    mixup halves the audio batch of a BiEncoder).  Raised before any launch: the kernels take B from the audio side."""
    if a.dim() != 3 or t.dim() < 2 or t.shape[0] != a.shape[0] or t.shape[-1] != a.shape[2]:
        raise RuntimeError(f"{what}: audio {tuple(a.shape)} and text {tuple(t.shape)} must agree in batch and embedding size "
                           f"(audio clip b is scored against text row b; mixup halves the audio batch)")


def match_forward(audio, text, kind, l2norm, scale):
    """match.DotProduct (kind 0) / match.ExpNegL2 (kind 1), text_level='seq' (models/match.py:16-33,43-60): (B,T,D),(B,D) -> (B,T)."""
    a, t = _chk(audio, "audio_emb"), _chk(text, "text_emb")
    _check_pair_batch("frame_match", a, t)
    if t.dim() != 2:
        raise RuntimeError(f"frame_match: text_emb must be (B, D), got {tuple(t.shape)}")
    B, T, D = a.shape
    sim = _empty(B, T, like=a)
    call("tag_match_forward", ptr(a), ptr(t), ptr(sim), int(kind), int(l2norm), int(scale), B, T, D)
    return sim


def match_backward(audio, text, sim, dsim, kind, l2norm, scale):
    a, t = _chk(audio, "audio_emb"), _chk(text, "text_emb")
    _check_pair_batch("frame_match_backward", a, t)
    if t.dim() != 2:
        raise RuntimeError(f"frame_match_backward: text_emb must be (B, D), got {tuple(t.shape)}")
    B, T, D = a.shape
    da, dt = torch.empty_like(a), torch.empty_like(t)
    call("tag_match_backward", ptr(a), ptr(t), ptr(sim), ptr(_chk(dsim, "grad")), ptr(da), ptr(dt), int(kind), int(l2norm),
         int(scale), B, T, D)
    return da, dt


def frame_bce_forward(sim, label, length, Tt):
    """FrameBceLoss (losses.py:12-24) on (frame_sim[:, :Tt], label[:, :Tt], clamp(length, 1, Tt)) -> 0-dim loss."""
    s, lab = _chk(sim, "frame_sim"), _chk(label, "label")
    loss = _empty(1, like=s)
    call("tag_frame_bce_forward", ptr(s), s.shape[1], ptr(lab), lab.shape[1], ptr(length), s.shape[0], int(Tt), ptr(loss))
    return loss.view(())


def frame_bce_backward(sim, label, length, Tt, dloss):
    s, lab = _chk(sim, "frame_sim"), _chk(label, "label")
    ds = torch.empty_like(s)
    call("tag_frame_bce_backward", ptr(s), s.shape[1], ptr(lab), lab.shape[1], ptr(length), s.shape[0], int(Tt),
         ptr(_chk(dloss.reshape(1), "grad")), ptr(ds))
    return ds


# ---- AudioTagging head (csrc/tagging.hip): (B, T, C) passes with the classes innermost ----
def class_pool_forward(prob, length, mode):
    """*_with_lens pooling of prob (B,T,C) over the frames < length[b] -> clip (B,C), aux (B,C) (what the backward needs)."""
    p = _chk(prob, "frame_sim")
    B, T, C = p.shape
    clip, aux = _empty(B, C, like=p), _empty(B, C, like=p)
    call("tag_class_pool_forward", ptr(p), ptr(length), ptr(clip), ptr(aux), B, T, C, int(mode))
    return clip, aux


def tagging_head_dlogit(prob, dprob, dclip, clip, aux, length, mode, out=None):
    """dlogit (B,T,C) = (dprob + dclip * d clip / d prob) * prob (1 - prob); dprob / dclip may be None; out may be dprob."""
    p = _chk(prob, "frame_sim")
    B, T, C = p.shape
    dp = _chk(dprob, "grad") if dprob is not None else None
    dc = _chk(dclip, "grad") if dclip is not None else None
    out = out if out is not None else torch.empty_like(p)
    call("tag_tagging_head_backward", ptr(p), ptr(dp), ptr(dc), ptr(clip), ptr(aux), ptr(length), ptr(out), B, T, C, int(mode),
         T)
    return out


def _frames_per_clip(t, name):
    """(B,Tt,C) fp32 device tensor, possibly a view truncated in time -> (tensor, frames per clip of its buffer); anything
    else strided is made contiguous."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the MI355X (cuda) device, got {t.device}; "
                           "the HIP path has no CPU fallback")
    if t.dtype != F32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    B, Tt, C = t.shape
    s0, s1, s2 = t.stride()
    if (C == 1 or s2 == 1) and (Tt == 1 or s1 == C) and (B == 1 or (s0 % C == 0 and s0 >= Tt * C)):
        return t, (s0 // C if B > 1 else Tt)
    return t.contiguous(), Tt


def _masked_bce_args(prob, label, length, cls_mask):
    p, ld_p = _frames_per_clip(prob, "frame_sim")
    y, ld_y = _frames_per_clip(label, "strong_label")
    if y.shape != p.shape:
        raise RuntimeError(f"frame_sim {tuple(p.shape)} and strong_label {tuple(y.shape)} must be aligned first "
                           "(ClassMappingRunner.forward does it)")
    B, Tt, C = p.shape
    m = _chk(cls_mask, "strong_label_mask") if cls_mask is not None else None
    if m is not None and tuple(m.shape) != (B, C):
        raise RuntimeError(f"strong_label_mask: expected {(B, C)}, got {tuple(m.shape)}")
    ws = _ws(query("tag_masked_frame_bce_ws_bytes", B, Tt, C), p)
    return p, ld_p, y, ld_y, m, B, Tt, C, ws


def masked_frame_bce_forward(prob, label, length, cls_mask=None):
    """MaskedFrameBceLoss (losses.py:157-170) on prob / label (B,Tt,C), clamp(length, 1, Tt), cls_mask (B,C) -> 0-dim loss."""
    p, ld_p, y, ld_y, m, B, Tt, C, ws = _masked_bce_args(prob, label, length, cls_mask)
    loss = _empty(1, like=p)
    call("tag_masked_frame_bce_forward", ptr(p), ld_p, ptr(y), ld_y, ptr(length), ptr(m), B, Tt, C, ptr(loss), ptr(ws))
    return loss.view(())


def masked_frame_bce_backward(prob, label, length, cls_mask, dloss):
    p, ld_p, y, ld_y, m, B, Tt, C, ws = _masked_bce_args(prob, label, length, cls_mask)
    dp = _empty(B, Tt, C, like=p)
    call("tag_masked_frame_bce_backward", ptr(p), ld_p, ptr(y), ld_y, ptr(length), ptr(m), B, Tt, C,
         ptr(_chk(dloss.reshape(1), "grad")), ptr(dp), ptr(ws))
    return dp


def _l2norm_rows(x, rows, D):
    y = torch.empty_like(x)
    call("tag_l2norm_rows_forward", ptr(x), ptr(y), rows, D)
    return y


def align_dot_backward(audio, text, out, dout, l2norm, scaled):
    """Gradient of align.DotProduct (models/align.py:14-31): d score from (out, dout), then two MFMA GEMMs against the
    (re-normalised when l2norm) operands and the backward of F.normalize."""
    a, t = _chk(audio, "audio"), _chk(text, "text")
    _check_pair_batch("align_dot_backward", a, t)
    B, T, D = a.shape
    N = t.shape[1]
    an, tn = (_l2norm_rows(a, B * T, D), _l2norm_rows(t, B * N, D)) if l2norm else (a, t)
    ds = _empty(B * T, B * N, like=a)
    call("tag_align_dot_dscore", ptr(out), ptr(_chk(dout, "grad")), ptr(ds), int(scaled), B, T, N, D)
    da = gemm(ds, tn.view(B * N, D), B * T, D, B * N)                       # (B*T, D)
    dt = gemm(ds, an.view(B * T, D), B * N, D, B * T, transA=True, lda=B * N)   # (B*N, D)
    if l2norm:
        da2, dt2 = torch.empty_like(da), torch.empty_like(dt)
        call("tag_l2norm_rows_backward", ptr(a), ptr(da), ptr(da2), B * T, D)
        call("tag_l2norm_rows_backward", ptr(t), ptr(dt), ptr(dt2), B * N, D)
        da, dt = da2, dt2
    return da.view(B, T, D), dt.view(B, N, D)


def _unit_rows(x, rows, D):
    """F.normalize as a quotient (align.hip): x / max(||x||, 1e-12)."""
    y = torch.empty_like(x)
    call("tag_align_expnegl2_normalize", ptr(x), ptr(y), rows, D)
    return y


def align_expnegl2_backward(audio, text, dout):
    """Gradient of align.ExpNegL2: the distances recomputed from the re-normalised rows, g = -dout * out / dist per pair (0 at
    dist == 0), the pair sums of g (an - tn) for both operands (no atomics), then the backward of F.normalize."""
    a, t = _chk(audio, "audio"), _chk(text, "text")
    _check_pair_batch("align_expnegl2_backward", a, t)
    B, T, D = a.shape
    N = t.shape[1]
    an, tn = _unit_rows(a, B * T, D), _unit_rows(t, B * N, D)
    ws = _ws(query("tag_align_expnegl2_ws_bytes", B, T, N, D), a)
    dan, dtn = torch.empty_like(a), torch.empty_like(t)
    call("tag_align_expnegl2_backward", ptr(an), ptr(tn), ptr(_chk(dout, "grad")), ptr(dan), ptr(dtn), B, T, N, D, ptr(ws))
    da, dt = torch.empty_like(a), torch.empty_like(t)
    call("tag_align_expnegl2_normalize_backward", ptr(a), ptr(an), ptr(dan), ptr(da), B * T, D)
    call("tag_align_expnegl2_normalize_backward", ptr(t), ptr(tn), ptr(dtn), ptr(dt), B * N, D)
    return da, dt


# ------------------------------------------------------------------------------------------------
# per-clip bias passes and heads of the early-fusion CrossCnn8_Rnn (models/audio_text_model.py:571-840), fp32
# ------------------------------------------------------------------------------------------------

def _clip_ws(B, C, like):
    return _ws(query("tag_clip_reduce_ws_bytes", B, C), like), torch.empty(B, 2, C, device=like.device, dtype=torch.float64)


def bias_bnrelu_forward(y, st: BNStat, bias):
    """relu(bn(y) + bias[b, c]) of a channels-last y (B,H,W,C); bias (B, C)."""
    B, H, W, C = y.shape
    out = torch.empty_like(y)
    call("tag_bias_bnrelu_forward", ptr(y), ptr(st.scale), ptr(st.shift), ptr(bias), ptr(out), B, H * W, C)
    return out


def bias_bnrelu_pool(y, st: BNStat, bias, ph, pw, pool=0, drop_p=0.0, seed=0):
    """dropout(pool(relu(bn(y) + bias[b, c]))): bnact_pool (act 1) with the per-clip bias."""
    B, H, W, C = y.shape
    out = _empty(B, H // ph, W // pw, C, like=y)
    call("tag_bias_bnrelu_pool_forward", ptr(y), ptr(st.scale), ptr(st.shift), ptr(bias), ptr(out), B, H, W, C, ph, pw,
         int(pool), float(drop_p), seed)
    return out


def bias_bnrelu_pool_backward(y, st: BNStat, gamma, bias, dout, ph, pw, pool=0, drop_p=0.0, seed=0, dg_out=None, db_out=None):
    """-> (dy, dgamma, dbeta, clip): clip (B, 2, C) fp64 = [sum dz | sum dz*xhat] of each clip (dz: gradient at bn(y) + bias)."""
    B, H, W, C = y.shape
    dy = torch.empty_like(y)
    dg, db = _dg_db(dg_out, db_out, C, y)
    ws, clip = _clip_ws(B, C, y)
    call("tag_bias_bnrelu_pool_backward", ptr(y), ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.invstd), ptr(gamma),
         ptr(bias), ptr(dout), ptr(dy), ptr(dg), ptr(db), ptr(clip), B, H, W, C, ph, pw, int(pool), float(drop_p), seed,
         int(st.train), ptr(ws))
    return dy, dg, db, clip


def bias_bnrelu_backward(y, st: BNStat, gamma, bias, da, prev=None, want_dt=True, dg_out=None, db_out=None):
    """Backward of bias_bnrelu_forward given da.  -> (dy, dgamma, dbeta, dt): dt (B, C) = this site's per-clip sum of dz plus
    prev's (the clip sums bias_bnrelu_pool_backward returned for the block's other site), or None."""
    B, H, W, C = y.shape
    dy = torch.empty_like(y)
    dg, db = _dg_db(dg_out, db_out, C, y)
    dt = _empty(B, C, like=y) if want_dt else None
    ws, clip = _clip_ws(B, C, y)
    call("tag_bias_bnrelu_backward", ptr(y), ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.invstd), ptr(gamma), ptr(bias),
         ptr(da), ptr(dy), ptr(dg), ptr(db), ptr(clip), ptr(prev), ptr(dt), B, H * W, C, int(st.train), ptr(ws))
    return dy, dg, db, dt


def rowgroup_bias_relu(x, bias, T, out=None):
    """relu(x + bias[row // T]) over x (B*T, N); bias (B, N).  out may be x."""
    M, N = x.shape
    out = out if out is not None else torch.empty_like(x)
    call("tag_rowgroup_bias_relu", ptr(x), ptr(bias), ptr(out), M // T, T, N)
    return out


def rowgroup_colsum(x, T, dtotal=None):
    """x (B*T, N) -> (per-group column sums (B, N), their total (N))."""
    M, N = x.shape
    B = M // T
    dgroup = _empty(B, N, like=x)
    dtotal = dtotal if dtotal is not None else _empty(N, like=x)
    ws, clip = _clip_ws(B, N, x)
    call("tag_rowgroup_colsum", ptr(x), B, T, N, ptr(dgroup), ptr(dtotal), ptr(clip), ptr(ws))
    return dgroup, dtotal


def frame_head_forward(y, rb, w, b0, T):
    """prob = clamp(sigmoid((y + rb[row // T]) . w + b0), 1e-7, 1) of y (B*T, N) -> (prob (B*T,), sig (B*T,))."""
    M, N = y.shape
    sig, prob = _empty(M, like=y), _empty(M, like=y)
    call("tag_frame_head_forward", ptr(y), ptr(rb), ptr(w), ptr(b0), ptr(sig), ptr(prob), M // T, T, N)
    return prob, sig


def frame_head_backward(y, rb, w, sig, dprob, T, dw_out=None, db_out=None):
    """-> (dy (B*T, N), dw (N), db0 (1), drb (B, N))."""
    M, N = y.shape
    B = M // T
    dy, drb = torch.empty_like(y), _empty(B, N, like=y)
    dw = dw_out if dw_out is not None else _empty(N, like=y)
    dsum = _empty(N, like=y)
    ws, clip = _clip_ws(B, N, y)
    call("tag_frame_head_backward", ptr(y), ptr(rb), ptr(w), ptr(sig), ptr(dprob), ptr(dy), ptr(dw), ptr(dsum), ptr(drb),
         ptr(clip), B, T, N, ptr(ws))
    db0 = dsum[:1]
    if db_out is not None:
        db_out.copy_(db0)
        db0 = db_out
    return dy, dw, db0, drb


# ------------------------------------------------------------------------------------------------
# biased convs of the early-fusion CrossCDur (models/audio_text_model.py:461-568): the text is added to the RAW conv output,
# leaky(conv(bn(x)) + t[b, c]), so the bias lives in the conv kernels' epilogue (fp32, direct kernels only)
# ------------------------------------------------------------------------------------------------

def _check_clip_bias(bias, B, Cout):
    if bias.dim() != 2 or bias.shape[0] != B or bias.shape[1] != Cout:
        raise RuntimeError(f"per-clip bias of shape {tuple(bias.shape)}, expected ({B}, {Cout})")


def conv3x3_bias(x, wpack, Cout, prologue, scale, shift, bias):
    """y = conv(prologue(x)) + bias[b, cout] of a channels-last x (B,H,W,Cin); wpack: the fp32 forward pack of pack_conv_weight.
    A shape without an instance raises (TAG_EINVAL of tag_conv3x3_forward_bias)."""
    B, H, W, Cin = x.shape
    _check_clip_bias(bias, B, Cout)
    if wpack.dtype != F32 or x.dtype != F32:
        raise RuntimeError("conv3x3_bias: fp32 activations and the fp32 weight pack only")
    y = _empty(B, H, W, Cout, like=x)
    with _timed(("conv3x3_halo_kernel", B, H, W, Cin, Cout), 2.0 * B * H * W * 9 * Cin * Cout):
        call("tag_conv3x3_forward_bias", ptr(x), ptr(wpack), prologue, ptr(scale), ptr(shift), ptr(bias), ptr(y), B, H, W, Cin,
             Cout)
    return y


def conv3x3_c1_bias(x, w, col_scale, col_shift, bias):
    """y = conv(affine(x)) + bias[b, cout] of the Cin = 1 convolution: x (B,H,W), w (Cout,1,3,3) -> (B,H,W,Cout)."""
    B, H, W = x.shape
    Cout = w.shape[0]
    _check_clip_bias(bias, B, Cout)
    y = _empty(B, H, W, Cout, like=x)
    call("tag_conv3x3_c1_forward_bias", ptr(x), ptr(col_scale), ptr(col_shift), ptr(w), ptr(bias), ptr(y), B, H, W, Cout)
    return y


def lppool_leaky_backward_clip(y, dout, ph, pw, drop_p=0.0, seed=0):
    """lppool_leaky_backward that also returns dt (B, C), the per-clip sums of dy, from the same pass."""
    B, H, W, C = y.shape
    dy, dt = torch.empty_like(y), _empty(B, C, like=y)
    ws, clip = _clip_ws(B, C, y)
    call("tag_lppool_leaky_backward_clip", ptr(y), ptr(dout), ptr(dy), ptr(dt), ptr(clip), B, H, W, C, ph, pw, float(drop_p), seed,
         ptr(ws))
    return dy, dt


def bn_act_backward_clip(x, pre_op, st: BNStat, gamma, du, dg_out=None, db_out=None):
    """bn_act_backward of a channels-last x (B,H,W,C) that also returns dt (B, C), the per-clip sums of dx, from its apply pass."""
    B, C = x.shape[0], x.shape[-1]
    rows = x.numel() // C
    dx, dt = torch.empty_like(x), _empty(B, C, like=x)
    dg, db = _dg_db(dg_out, db_out, C, x)
    ws = _ws(query("tag_bn_backward_ws_bytes", rows, C), x)
    wsc, clip = _clip_ws(B, C, x)
    call("tag_bn_act_backward_clip", ptr(x), pre_op, ptr(st.mean), ptr(st.invstd), ptr(gamma), ptr(du), ptr(dx), ptr(dg), ptr(db),
         ptr(dt), ptr(clip), B, rows // B, C, int(st.train), ptr(ws), ptr(wsc))
    return dx, dg, db, dt


def leaky_forward(z):
    """leaky_relu(z, 0.1) of a contiguous fp32 tensor (numel % 4 == 0)."""
    out = torch.empty_like(z)
    call("tag_leaky_forward", ptr(z), ptr(out), z.numel())
    return out


def leaky_backward(z, dout):
    dz = torch.empty_like(z)
    call("tag_leaky_backward", ptr(z), ptr(dout), ptr(dz), z.numel())
    return dz


# ------------------------------------------------------------------------------------------------
# optimiser step on flat buffers (O1)
# ------------------------------------------------------------------------------------------------

def grad_sumsq(flat_grad):
    out = torch.empty(1, device=flat_grad.device, dtype=torch.float64)
    ws = _ws(query("tag_sumsq_ws_bytes", flat_grad.numel()), flat_grad)
    call("tag_sumsq", ptr(flat_grad), flat_grad.numel(), ptr(out), ptr(ws))
    return out


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    call("tag_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, step, ptr(gnorm_sq),
         float(max_norm), float(grad_scale))


# ------------------------------------------------------------------------------------------------ contrastive objectives
TRIPLET_MODES = {"max": 0, "weighted": 1, "random": 2}


def _square(sim, name="sim"):
    x = _chk(sim, name)                                  # sim.T arrives strided: the kernels read rows
    if x.ndim != 2 or x.shape[0] != x.shape[1] or x.shape[0] < 1:
        raise RuntimeError(f"{name}: expected a square (n,n) matrix with n >= 1, got {tuple(x.shape)}")
    return x, x.shape[0]


def _contrastive_ws(n, like):
    return _ws(query("tag_contrastive_ws_bytes", n), like)


def _dloss(dloss):
    return _chk(dloss.reshape(1), "grad")


def infonce_forward(sim, tau):
    """InfoNceLoss (losses.py:267-281) on sim (n,n) -> (0-dim loss, workspace holding the row / column log-sum-exp)."""
    x, n = _square(sim)
    loss, ws = _empty(1, like=x), _contrastive_ws(n, x)
    call("tag_infonce_forward", ptr(x), n, float(tau), ptr(loss), ptr(ws))
    return loss.view(()), ws


def infonce_backward(sim, tau, dloss, ws=None):
    """d loss / d sim.  ws: what infonce_forward returned for the SAME sim; None runs that forward again to refill it."""
    x, n = _square(sim)
    if ws is None:
        ws = infonce_forward(x, tau)[1]
    dx = torch.empty_like(x)
    call("tag_infonce_backward", ptr(x), n, float(tau), ptr(_dloss(dloss)), ptr(dx), ptr(ws))
    return dx


def _triplet_indices(mode, n, s_index, a_index, like):
    if mode != TRIPLET_MODES["random"]:
        return None, None
    out = []
    for name, t in (("s_index", s_index), ("a_index", a_index)):
        if t is None or not t.is_cuda or t.dtype != torch.int32 or tuple(t.shape) != (n,):
            raise RuntimeError(f"{name}: the random triplet needs a device int32 vector of {n} draws, got "
                               f"{None if t is None else (t.device, t.dtype, tuple(t.shape))}; there is no CPU fallback")
        out.append(t.contiguous())
    return out


def triplet_forward(sim, mode, margin, s_index=None, a_index=None):
    """Max / Weighted / RandomTripletLoss (losses.py:285-417; mode: TRIPLET_MODES value) on sim (n,n) -> (0-dim loss,
    workspace holding the row / column argmax, -1 where inactive)."""
    x, n = _square(sim)
    if mode not in TRIPLET_MODES.values():
        raise RuntimeError(f"triplet mode {mode!r}: expected one of {TRIPLET_MODES}")
    s, a = _triplet_indices(mode, n, s_index, a_index, x)
    loss, ws = _empty(1, like=x), _contrastive_ws(n, x)
    call("tag_triplet_forward", ptr(x), n, int(mode), float(margin), ptr(s), ptr(a), ptr(loss), ptr(ws))
    return loss.view(()), ws


def triplet_backward(sim, mode, margin, s_index, a_index, dloss, ws=None):
    x, n = _square(sim)
    s, a = _triplet_indices(mode, n, s_index, a_index, x)
    if ws is None:                                         # (the random mode keeps nothing: its workspace is never read)
        ws = triplet_forward(x, mode, margin, s, a)[1] if mode != TRIPLET_MODES["random"] else _contrastive_ws(n, x)
    dx = torch.empty_like(x)
    call("tag_triplet_backward", ptr(x), n, int(mode), float(margin), ptr(s), ptr(a), ptr(_dloss(dloss)), ptr(dx), ptr(ws))
    return dx


def _clip_pair(clip_sim, label):
    c, y = _chk(clip_sim, "clip_sim"), _chk(label, "label")
    if c.ndim != 2 or c.shape != y.shape or c.numel() < 1:
        raise RuntimeError(f"clip_sim {tuple(c.shape)} and label {tuple(y.shape)}: expected the same (B,N), B, N >= 1")
    return c, y, c.shape[0], c.shape[1]


def milnce_forward(clip_sim, label, tau):
    """MilNceLoss (losses.py:46-56) on clip_sim / label (B,N) -> (0-dim loss, workspace holding both log-sum-exp per row)."""
    c, y, B, N = _clip_pair(clip_sim, label)
    loss, ws = _empty(1, like=c), _contrastive_ws(B, c)
    call("tag_milnce_forward", ptr(c), ptr(y), B, N, float(tau), ptr(loss), ptr(ws))
    return loss.view(()), ws


def milnce_backward(clip_sim, label, tau, dloss, ws=None):
    c, y, B, N = _clip_pair(clip_sim, label)
    if ws is None:
        ws = milnce_forward(c, y, tau)[1]
    dc = torch.empty_like(c)
    call("tag_milnce_backward", ptr(c), ptr(y), B, N, float(tau), ptr(_dloss(dloss)), ptr(dc), ptr(ws))
    return dc


# ------------------------------------------------------------------------------------------------ clip-level BCE objectives
CLIP_BCE_MODES = {"focal": 0, "freq_weight": 1, "symmetric": 2, "origin_symmetric": 3, "prior_adjusted": 4}
_CLIP_BCE_AUX = (CLIP_BCE_MODES["freq_weight"], CLIP_BCE_MODES["prior_adjusted"])
CLIP_BCE_ONE_LAUNCH_MAX = 4096        # = ONE_LAUNCH_MAX of csrc/clip_bce.hip: the largest M whose forward is one launch


def _clip_bce_args(clip_sim, label, aux, mode, consts):
    """Shapes, dtypes, mode and constants first (they need no device), then the device of every tensor."""
    if mode not in CLIP_BCE_MODES.values():
        raise RuntimeError(f"clip_bce mode {mode!r}: expected one of {CLIP_BCE_MODES}")
    if any(math.isnan(float(c)) for c in consts):
        raise RuntimeError(f"clip_bce: a constant is NaN: {tuple(consts)}")
    if clip_sim.ndim != 2 or clip_sim.numel() < 1:
        raise RuntimeError(f"clip_sim: expected a (B,N) matrix with B, N >= 1, got {tuple(clip_sim.shape)}")
    if mode in _CLIP_BCE_AUX and aux is None:
        raise RuntimeError(f"clip_bce mode {mode}: needs aux (the weight / prior) of clip_sim's shape {tuple(clip_sim.shape)}")
    for name, t in (("label", label), ("aux", aux)):
        if t is not None and t.shape != clip_sim.shape:
            raise RuntimeError(f"{name} {tuple(t.shape)}: expected clip_sim's shape {tuple(clip_sim.shape)}")
    for name, t in (("clip_sim", clip_sim), ("label", label), ("aux", aux)):
        if t is not None and t.dtype != F32:
            raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    c, y = _chk(clip_sim, "clip_sim"), _chk(label, "label")      # (a strided clip_sim view is made contiguous)
    a = _chk(aux, "aux") if aux is not None and mode in _CLIP_BCE_AUX else None
    for name, t in (("label", y), ("aux", a)):
        if t is not None and t.device != c.device:
            raise RuntimeError(f"{name} on {t.device}, clip_sim on {c.device}: expected one device")
    return c, y, a


def clip_bce_forward(clip_sim, label, aux, mode, c0, c1, c2):
    """The clip-level BCE variants (losses.py:59-143 in the reference; mode: CLIP_BCE_MODES value, the constants as
    include/tag_hip.h lists them) on clip_sim / label / aux (B,N) -> 0-dim loss."""
    c, y, a = _clip_bce_args(clip_sim, label, aux, mode, (c0, c1, c2))
    M = c.numel()
    loss, ws = _empty(1, like=c), _ws(query("tag_clip_bce_ws_bytes", M), c)
    call("tag_clip_bce_forward", ptr(c), ptr(y), ptr(a), M, int(mode), float(c0), float(c1), float(c2), ptr(loss), ptr(ws))
    return loss.view(())


def clip_bce_backward(clip_sim, label, aux, mode, c0, c1, c2, dloss):
    """d loss / d clip_sim (B,N), contiguous; label and aux get no gradient."""
    c, y, a = _clip_bce_args(clip_sim, label, aux, mode, (c0, c1, c2))
    dc = torch.empty_like(c)
    call("tag_clip_bce_backward", ptr(c), ptr(y), ptr(a), c.numel(), int(mode), float(c0), float(c1), float(c2),
         ptr(_dloss(dloss)), ptr(dc))
    return dc


# ------------------------------------------------------------------------------------------------
# thresholded similarity count (utils/data/calc_phrase_sim_count.py in the reference), phrase_sim.hip
# ------------------------------------------------------------------------------------------------

def _phrase_sim_rows(t, name):
    """(rows, D) fp32 on the device with unit column stride; a row-strided view of a wider buffer is passed as it is."""
    if not t.is_cuda:
        _chk(t, name)
    if t.dtype != F32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise RuntimeError(f"{name}: expected a float32 matrix (rows >= 1, D >= 1), got {t.dtype} {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def phrase_sim_count(q, bank, weight=None, threshold=0.5, normalize=True):
    """out[i] = sum_j weight[j] * [q[i] . bank[j] >= threshold] as int64 (M,), q (M, D) against bank (N, D); weight (N) int64
    or None for all ones.  normalize: both operands through x / max(||x||, 1e-12) first (sklearn's cosine_similarity, the
    all-zero row staying zero); ``q is bank`` normalises once.  No (M, N) scores exist on the device."""
    same = q is bank
    qr = _phrase_sim_rows(q, "q")
    br = qr if same else _phrase_sim_rows(bank, "bank")
    if br.device != qr.device or br.shape[1] != qr.shape[1]:
        raise RuntimeError(f"bank {tuple(br.shape)} on {br.device}: expected q's device {qr.device} and D = {qr.shape[1]}")
    (M, D), N = qr.shape, br.shape[0]
    if normalize:
        qr = _unit_rows(qr.contiguous(), M, D)
        br = qr if same else _unit_rows(br.contiguous(), N, D)
    w = None
    if weight is not None:
        if not weight.is_cuda:
            _chk(weight, "weight")
        if weight.dtype != torch.int64 or weight.shape != (N,) or weight.device != qr.device:
            raise RuntimeError(f"weight: expected int64 ({N},) on {qr.device}, got {weight.dtype} {tuple(weight.shape)} on "
                               f"{weight.device}")
        w = weight.contiguous()
    out = torch.empty(M, device=qr.device, dtype=torch.int64)
    ws = _ws(query("tag_phrase_sim_count_ws_bytes", M, N, D), qr)
    call("tag_phrase_sim_count", ptr(qr), qr.stride(0), ptr(br), br.stride(0), ptr(w), float(threshold), ptr(out), M, N, D,
         ptr(ws))
    return out


# ------------------------------------------------------------------------------------------------
# device k-means (python_scripts/clustering/kmeans_emb.py in the reference runs sklearn on the host), kmeans.hip
# ------------------------------------------------------------------------------------------------

def _kmeans_vec(t, name, dtype, n, like):
    if not t.is_cuda:
        _chk(t, name)
    if t.dtype != dtype or t.shape != (n,) or t.device != like.device:
        raise RuntimeError(f"{name}: expected {dtype} ({n},) on {like.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.contiguous()


def _kmeans_pair(x, centers):
    xr, cr = _phrase_sim_rows(x, "x"), _phrase_sim_rows(centers, "centers")
    if cr.device != xr.device or cr.shape[1] != xr.shape[1]:
        raise RuntimeError(f"centers {tuple(cr.shape)} on {cr.device}: expected x's device {xr.device} and D = {xr.shape[1]}")
    return xr, cr


def kmeans_assign(x, centers):
    """(label int32 (N,), dist2 fp32 (N,)): label[i] = argmin_k (||c_k||^2 - 2 x_i . c_k) on the exact-fp32 MFMA, ties to the lowest
    k; dist2[i] = sum_d (x_id - c_label,d)^2 from the differences.  x (N, D), centers (K, D), row-strided views are passed as they
    are.  No (N, K) scores exist on the device."""
    xr, cr = _kmeans_pair(x, centers)
    (N, D), K = xr.shape, cr.shape[0]
    label = torch.empty(N, device=xr.device, dtype=torch.int32)
    dist2 = torch.empty(N, device=xr.device, dtype=F32)
    ws = _ws(query("tag_kmeans_assign_ws_bytes", N, K, D), xr)
    call("tag_kmeans_assign", ptr(xr), xr.stride(0), ptr(cr), cr.stride(0), ptr(label), ptr(dist2), N, K, D, ptr(ws))
    return label, dist2


def kmeans_update(x, label, centers, check_labels=True):
    """(sums fp64 (K, D), count int64 (K,)); ``centers`` (K, D) is updated IN PLACE: row k = sums[k] / count[k] where count[k] > 0,
    untouched otherwise.  label (N,) int32 in [0, K) (check_labels: one torch min / max with a host read).  The same bits on
    every run."""
    xr = _phrase_sim_rows(x, "x")
    if not centers.is_cuda:
        _chk(centers, "centers")
    (N, D) = xr.shape
    if (centers.dtype != F32 or centers.dim() != 2 or centers.shape[0] < 1 or centers.shape[1] != D or centers.stride(1) != 1
            or centers.stride(0) < D or centers.device != xr.device):
        raise RuntimeError(f"centers: expected a float32 (K >= 1, {D}) matrix with unit column stride on {xr.device} (it is written "
                           f"in place), got {centers.dtype} {tuple(centers.shape)} strides {tuple(centers.stride())} on "
                           f"{centers.device}")
    K = centers.shape[0]
    lab = _kmeans_vec(label, "label", torch.int32, N, xr)
    if check_labels:
        lo, hi = (int(v) for v in torch.stack((lab.min(), lab.max())).tolist())
        if lo < 0 or hi >= K:
            raise RuntimeError(f"label: values must lie in [0, {K}), got min {lo}, max {hi}")
    sums = torch.empty(K, D, device=xr.device, dtype=torch.float64)
    count = torch.empty(K, device=xr.device, dtype=torch.int64)
    ws = _ws(query("tag_kmeans_update_ws_bytes", N, K, D), xr)
    call("tag_kmeans_update", ptr(xr), xr.stride(0), ptr(lab), ptr(sums), ptr(count), ptr(centers), centers.stride(0), N, K, D,
         ptr(ws))
    return sums, count


def kmeans_seed_step(x, pick, closest, first=False):
    """closest[i] = min(closest[i], ||x_i - x_p||^2) in place, p = pick (one int64 ON THE DEVICE: no host round trip in the
    k-means++ loop); first: write the distance without the min.  Returns closest."""
    xr = _phrase_sim_rows(x, "x")
    N, D = xr.shape
    if not pick.is_cuda:
        _chk(pick, "pick")
    if pick.dtype != torch.int64 or pick.numel() != 1 or pick.device != xr.device:
        raise RuntimeError(f"pick: expected one int64 on {xr.device}, got {pick.dtype} {tuple(pick.shape)} on {pick.device}")
    if not closest.is_cuda:
        _chk(closest, "closest")
    if closest.dtype != F32 or closest.shape != (N,) or not closest.is_contiguous() or closest.device != xr.device:
        raise RuntimeError(f"closest: expected contiguous float32 ({N},) on {xr.device} (it is written in place), got "
                           f"{closest.dtype} {tuple(closest.shape)} on {closest.device}")
    call("tag_kmeans_seed_step", ptr(xr), xr.stride(0), ptr(pick), ptr(closest), int(bool(first)), N, D)
    return closest


# ------------------------------------------------------------------------------------------------
# device DBSCAN (python_scripts/clustering/dbscan_emb.py in the reference runs sklearn on an N x N float matrix), dbscan.hip
# ------------------------------------------------------------------------------------------------

def dbscan_words(N):
    """32-bit words per row of the adjacency bit matrix of N rows: 4 * ceil(N / 128)."""
    W = query("tag_dbscan_words", int(N))
    if W < 1:
        raise RuntimeError(f"dbscan: N = {N} rows: expected 1 <= N <= {2**31 - 129}")
    return W


def _dbscan_ints(t, name, shape, like, what=""):
    if not t.is_cuda:
        _chk(t, name)
    if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or (like is not None and t.device != like.device):
        on = f" on {like.device}" if like is not None else ""
        raise RuntimeError(f"{name}: expected contiguous int32 {shape}{on}{what}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def _dbscan_graph_args(adj, core_bits):
    if not adj.is_cuda:
        _chk(adj, "adj")
    if adj.dim() != 2 or adj.shape[0] < 1:
        raise RuntimeError(f"adj: expected the int32 (N, W) bit matrix of dbscan_graph, got {adj.dtype} {tuple(adj.shape)}")
    N = adj.shape[0]
    W = dbscan_words(N)
    _dbscan_ints(adj, "adj", (N, W), None, " (W = 4 * ceil(N / 128))")
    _dbscan_ints(core_bits, "core_bits", (W,), adj)
    return N, W


def dbscan_graph(x, eps=0.5, normalize=True):
    """(adj int32 (N, W), degree int32 (N,)): bit j % 32 of adj[i, j // 32] = [x_i . x_j >= 1 - eps] on the exact-fp32 MFMA, W =
    4 * ceil(N / 128), bits at columns >= N are 0; degree = the row popcounts.  normalize: rows through x / max(||x||, 1e-12)
    first, so that the products are cosines and the test is sklearn's 1 - cos <= eps (an all-zero row stays zero: no neighbour,
    not even itself).  x (N, D); a row-strided view is passed as it is.  adj is the only device memory that scales with N^2."""
    eps = float(eps)
    if not 0.0 < eps <= 2.0:
        raise ValueError(f"eps: expected a cosine distance in (0, 2], got {eps}")
    xr = _phrase_sim_rows(x, "x")
    N, D = xr.shape
    W = dbscan_words(N)
    if normalize:
        xr = _unit_rows(xr.contiguous(), N, D)
    adj = torch.empty(N, W, device=xr.device, dtype=torch.int32)
    degree = torch.empty(N, device=xr.device, dtype=torch.int32)
    call("tag_dbscan_graph", ptr(xr), xr.stride(0), 1.0 - eps, ptr(adj), ptr(degree), N, D)
    return adj, degree


def dbscan_core(degree, min_samples):
    """core_bits int32 (W,): bit i % 32 of word i // 32 = [degree[i] >= min_samples]."""
    if not degree.is_cuda:
        _chk(degree, "degree")
    if degree.dim() != 1 or degree.shape[0] < 1:
        raise RuntimeError(f"degree: expected int32 (N >= 1,), got {degree.dtype} {tuple(degree.shape)}")
    N = degree.shape[0]
    _dbscan_ints(degree, "degree", (N,), None)
    core_bits = torch.empty(dbscan_words(N), device=degree.device, dtype=torch.int32)
    call("tag_dbscan_core", ptr(degree), int(min_samples), ptr(core_bits), N)
    return core_bits


def dbscan_hook(adj, core_bits, f_in, f_out, changed, check=True):
    """One FastSV pass on the parent array: f_out (written in place) from f_in, both int32 (N,) and distinct; ``changed`` (one
    int32 on the device) becomes 1 if f_out differs from f_in, else 0.  Every value of f_in must be a row index (check: one torch
    min / max with a host read).  Returns f_out."""
    N, _ = _dbscan_graph_args(adj, core_bits)
    _dbscan_ints(f_in, "f_in", (N,), adj)
    _dbscan_ints(f_out, "f_out", (N,), adj, " (it is written in place)")
    _dbscan_ints(changed, "changed", (1,), adj, " (it is written in place)")
    if f_in.data_ptr() == f_out.data_ptr():
        raise RuntimeError("f_out: expected a buffer other than f_in (a pass reads f_in only)")
    if check:
        lo, hi = (int(v) for v in torch.stack((f_in.min(), f_in.max())).tolist())
        if lo < 0 or hi >= N:
            raise RuntimeError(f"f_in: values must lie in [0, {N}), got min {lo}, max {hi}")
    call("tag_dbscan_hook", ptr(adj), ptr(core_bits), ptr(f_in), ptr(f_out), ptr(changed), N)
    return f_out


def dbscan_roots(adj, core_bits, f):
    """root int32 (N,): f[i] for a core row; for any other row the smallest f[j] over its core neighbours j, or -1 (noise)."""
    N, _ = _dbscan_graph_args(adj, core_bits)
    _dbscan_ints(f, "f", (N,), adj)
    root = torch.empty(N, device=adj.device, dtype=torch.int32)
    call("tag_dbscan_roots", ptr(adj), ptr(core_bits), ptr(f), ptr(root), N)
    return root


# ------------------------------------------------------------------------------------------------
# device average-linkage clustering (python_scripts/clustering/agc_emb.py in the reference runs sklearn on an N x N float
# matrix), agc.hip
# ------------------------------------------------------------------------------------------------

def _agc_buf(t, name, dtype, shape, like, what=""):
    if not t.is_cuda:
        _chk(t, name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or (like is not None and t.device != like.device):
        on = f" on {like.device}" if like is not None else ""
        raise RuntimeError(f"{name}: expected contiguous {dtype} {tuple(shape)}{on}{what}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def agc_nearest(means):
    """(nn int32 (M,), dist fp32 (M,)): nn[i] = the j != i with the largest means[i] . means[j] on the exact-fp32 MFMA, ties to the
    lowest j; dist[i] = 1 - that product.  means (M, D); a row-strided view is passed as it is.  The scores are bit-symmetric
    (score(i, j) == score(j, i)).  M = 1 gives nn = -1, dist = +inf.  No (M, M) scores exist on the device."""
    mr = _phrase_sim_rows(means, "means")
    M, D = mr.shape
    nn = torch.empty(M, device=mr.device, dtype=torch.int32)
    dist = torch.empty(M, device=mr.device, dtype=F32)
    ws = _ws(query("tag_agc_nearest_ws_bytes", M, D), mr)
    call("tag_agc_nearest", ptr(mr), mr.stride(0), ptr(nn), ptr(dist), M, D, ptr(ws))
    return nn, dist


def agc_merge(nn, dist, sums, sizes, ids, sums_out, sizes_out, ids_out, means_out, log_dist, log_ids, counts, log_off, next_id):
    """One round's bookkeeping on the first M = nn.shape[0] rows: row a is the left half of a pair when nn[nn[a]] == a and
    a < nn[a].  The survivors go to the front of the ``*_out`` buffers in their relative order, the merged clusters follow in
    ascending a with sum_a + sum_b (fp64), size_a + size_b (int64) and node id ``next_id + rank`` (int32); ``means_out`` rows
    (fp32, row-strided or not) = sum / size for every output row; pair r writes ``log_dist[log_off + r] = dist[a]`` and
    ``log_ids[log_off + r] = (id_a, id_b, next_id + r)``.  ``counts`` (2 int32 on the device) = (pairs, new M).  The buffers hold
    at least M rows and are written in place; the ``*_out`` buffers differ from the inputs.  Returns counts (no host read)."""
    if not nn.is_cuda:
        _chk(nn, "nn")
    if nn.dim() != 1 or nn.shape[0] < 1:
        raise RuntimeError(f"nn: expected int32 (M >= 1,), got {nn.dtype} {tuple(nn.shape)}")
    M = nn.shape[0]
    _agc_buf(nn, "nn", torch.int32, (M,), None)
    _agc_buf(dist, "dist", F32, (M,), nn)
    for t, name in ((sums, "sums"), (sums_out, "sums_out")):
        if not t.is_cuda:
            _chk(t, name)
        if (t.dtype != torch.float64 or t.dim() != 2 or t.shape[0] < M or t.shape[1] < 1 or not t.is_contiguous()
                or t.device != nn.device):
            raise RuntimeError(f"{name}: expected contiguous float64 (rows >= {M}, D >= 1) on {nn.device}, got {t.dtype} "
                               f"{tuple(t.shape)} on {t.device}")
    D = sums.shape[1]
    if sums_out.shape[1] != D:
        raise RuntimeError(f"sums_out: expected D = {D}, got {tuple(sums_out.shape)}")
    for t, name, dtype in ((sizes, "sizes", torch.int64), (sizes_out, "sizes_out", torch.int64), (ids, "ids", torch.int32),
                           (ids_out, "ids_out", torch.int32)):
        if not t.is_cuda:
            _chk(t, name)
        if t.dtype != dtype or t.dim() != 1 or t.shape[0] < M or not t.is_contiguous() or t.device != nn.device:
            raise RuntimeError(f"{name}: expected contiguous {dtype} (rows >= {M},) on {nn.device}, got {t.dtype} {tuple(t.shape)} on "
                               f"{t.device}")
    if not means_out.is_cuda:
        _chk(means_out, "means_out")
    if (means_out.dtype != F32 or means_out.dim() != 2 or means_out.shape[0] < M or means_out.shape[1] != D
            or means_out.stride(1) != 1 or means_out.stride(0) < D or means_out.device != nn.device):
        raise RuntimeError(f"means_out: expected a float32 (rows >= {M}, {D}) matrix with unit column stride on {nn.device} (it is "
                           f"written in place), got {means_out.dtype} {tuple(means_out.shape)} strides {tuple(means_out.stride())} on "
                           f"{means_out.device}")
    if sums.data_ptr() == sums_out.data_ptr() or sizes.data_ptr() == sizes_out.data_ptr() or ids.data_ptr() == ids_out.data_ptr():
        raise RuntimeError("sums_out, sizes_out, ids_out: expected buffers other than the inputs (rows move)")
    if not log_dist.is_cuda:
        _chk(log_dist, "log_dist")
    if log_dist.dim() != 1:
        raise RuntimeError(f"log_dist: expected float32 (rows,), got {log_dist.dtype} {tuple(log_dist.shape)}")
    rows = log_dist.shape[0]
    _agc_buf(log_dist, "log_dist", F32, (rows,), nn, " (it is written in place)")
    _agc_buf(log_ids, "log_ids", torch.int32, (rows, 3), nn, " (it is written in place)")
    _agc_buf(counts, "counts", torch.int32, (2,), nn, " (it is written in place)")
    log_off, next_id = int(log_off), int(next_id)
    if log_off < 0 or next_id < 0 or log_off + M // 2 > rows:
        raise RuntimeError(f"log_off = {log_off}, next_id = {next_id}: expected both >= 0 and room for {M // 2} pairs in a log of "
                           f"{rows} rows")
    ws = _ws(query("tag_agc_merge_ws_bytes", M, D), nn)
    call("tag_agc_merge", ptr(nn), ptr(dist), ptr(sums), ptr(sizes), ptr(ids), ptr(sums_out), ptr(sizes_out), ptr(ids_out),
         ptr(means_out), means_out.stride(0), ptr(log_dist), ptr(log_ids), rows, log_off, next_id, ptr(counts), M, D, ptr(ws))
    return counts


# ------------------------------------------------------------------------------------------------
# device spectral clustering (python_scripts/clustering/spectral_emb.py in the reference runs sklearn on an N x N fp64 matrix),
# spectral.hip
# ------------------------------------------------------------------------------------------------

#: rows per slice of spectral_gram's fp32 partial sums (= TAG_SPECTRAL_CHAIN of include/tag_hip.h, tag_spectral_chain()): the
#: length that bounds an fp32 chain whatever N is
SPECTRAL_CHAIN = 256


def _spectral_vec(t, name, n, like):
    if not t.is_cuda:
        _chk(t, name)
    if t.dtype != F32 or tuple(t.shape) != (n,) or t.device != like.device:
        raise RuntimeError(f"{name}: expected float32 ({n},) on {like.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.contiguous()


def spectral_gram(P, Q, w=None):
    """out (p, q) fp64 = sum_i w_i P[i, a] Q[i, b] over the N rows of P (N, p) and Q (N, q); w (N,) fp32 or None for ones.  Rows are
    cut into slices of SPECTRAL_CHAIN rows: inside a slice the products are fp32 on the exact-fp32 MFMA, the slices are added in
    fp64, so |err| <= SPECTRAL_CHAIN 2^-24 sum_i |w_i P_ia Q_ib| for every N.  ``P is Q`` computes the tiles on or above the
    diagonal only and returns a bit-symmetric matrix.  Row-strided views are passed as they are.  The same bits on every run."""
    same = P is Q
    pr = _phrase_sim_rows(P, "P")
    qr = pr if same else _phrase_sim_rows(Q, "Q")
    if qr.device != pr.device or qr.shape[0] != pr.shape[0]:
        raise RuntimeError(f"Q {tuple(qr.shape)} on {qr.device}: expected P's device {pr.device} and N = {pr.shape[0]} rows")
    (N, p), q = pr.shape, qr.shape[1]
    wv = None if w is None else _spectral_vec(w, "w", N, pr)
    nws = query("tag_spectral_gram_ws_bytes", N, p, q)
    if nws == 0:
        raise RuntimeError(f"spectral_gram: N = {N}, p = {p}, q = {q}: expected N <= {2**31 - 1 - SPECTRAL_CHAIN}, p and q <= 32768")
    out = torch.empty(p, q, device=pr.device, dtype=torch.float64)
    ws = _ws(nws, pr)
    call("tag_spectral_gram", ptr(pr), pr.stride(0), ptr(qr), qr.stride(0), ptr(wv), ptr(out), q, N, p, q, ptr(ws))
    return out


def spectral_rows(u, t):
    """(Y fp32 (N, D + 1), s fp32 (N,), e fp32 (N,)) of the normalised cosine affinity (u_i . u_j + 1) / 2 over unit rows u (N, D),
    t (D,) fp64 = the column sums of u.  Per row in fp64: deg = (u_i . t + N) / 2 - a_ii, a_ii = (u_i . u_i + 1) / 2 (the degree
    without the diagonal), s = deg^-1/2, e = a_ii / deg, Y[i] = s_i / sqrt 2 * [u_i, 1].  Y has 16-byte aligned rows: a (N, D + 1)
    view of a buffer whose row stride is a multiple of 4.  A row with deg <= 0 is reported as s[i] == 0 (e and Y's row zero)."""
    ur = _phrase_sim_rows(u, "u")
    N, D = ur.shape
    if not t.is_cuda:
        _chk(t, "t")
    if t.dtype != torch.float64 or tuple(t.shape) != (D,) or t.device != ur.device:
        raise RuntimeError(f"t: expected float64 ({D},) on {ur.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    Y = torch.empty(N, (D + 4) // 4 * 4, device=ur.device, dtype=F32)[:, :D + 1]
    s = torch.empty(N, device=ur.device, dtype=F32)
    e = torch.empty(N, device=ur.device, dtype=F32)
    call("tag_spectral_rows", ptr(ur), ur.stride(0), ptr(t.contiguous()), ptr(Y), Y.stride(0), ptr(s), ptr(e), N, D)
    return Y, s, e


def spectral_apply(Y, T, e, X, out=None):
    """out (N, b) fp32 = Y @ T - e[:, None] * X: the operator M = Y Y^T - diag(e) applied to a block X once T = Y^T X is known.
    Y (N, Dp), T (Dp, b), e (N,), X (N, b); one MFMA launch with the row epilogue fused, |err| <= (Dp + 2) 2^-24 (|Y||T| + |e X|).
    Row-strided views are passed as they are; ``out`` (given or new) may be X."""
    yr, tr, xr = _phrase_sim_rows(Y, "Y"), _phrase_sim_rows(T, "T"), _phrase_sim_rows(X, "X")
    (N, Dp), b = yr.shape, tr.shape[1]
    if tr.shape[0] != Dp or tuple(xr.shape) != (N, b) or tr.device != yr.device or xr.device != yr.device:
        raise RuntimeError(f"spectral_apply: Y {tuple(yr.shape)} needs T ({Dp}, b) and X ({N}, b) on {yr.device}, got T "
                           f"{tuple(tr.shape)} on {tr.device}, X {tuple(xr.shape)} on {xr.device}")
    ev = _spectral_vec(e, "e", N, yr)
    if out is None:
        out = torch.empty(N, b, device=yr.device, dtype=F32)
    elif (not out.is_cuda or out.dtype != F32 or tuple(out.shape) != (N, b) or out.stride(1) != 1 or out.stride(0) < b
          or out.device != yr.device):
        raise RuntimeError(f"out: expected a float32 ({N}, {b}) matrix with unit column stride on {yr.device} (it is written in "
                           f"place), got {out.dtype} {tuple(out.shape)} strides {tuple(out.stride())} on {out.device}")
    call("tag_spectral_apply", ptr(yr), yr.stride(0), ptr(tr), tr.stride(0), ptr(ev), ptr(xr), xr.stride(0), ptr(out),
         out.stride(0), N, Dp, b)
    return out


# ------------------------------------------------------------------------------------------------
# operating-point counts of the grounding evaluation (utils/grounding_eval.py on the host), grounding_eval.hip
# ------------------------------------------------------------------------------------------------

def _grounding_tensor(t, name, dtype, shape, like, what):
    """A device tensor as it is, a host tensor or array copied over (the ground truth comes from the dataset, on the host)."""
    t = torch.as_tensor(t)
    if t.dtype != dtype or tuple(t.shape) != shape:
        raise RuntimeError(f"{name}: expected {dtype} {shape}{what}, got {t.dtype} {tuple(t.shape)}")
    return t.to(like.device).contiguous()


def grounding_counts(regions, counts, gt, gt_count, time_resolution, dtc=0.5, gtc=0.5, out=None, check=True):
    """``segments``' outputs + the clips' ground truths -> (B, NT, 4) int32 ``{tp_preds, tp_refs, psds_tp, psds_fp}`` per (clip,
    threshold): the integers utils.grounding_eval.evaluate_detections and psds_operating_point add up for that clip as one file,
    exactly (fp64, numpy's order of additions; grounding_eval.hip).  regions (B,NT,maxK,2) int64 and counts (B,NT) int32 on the
    device; gt (B,Gmax,2) float64 [onset, offset] seconds and gt_count (B,) int32 rows in use, on the device or on the host
    (utils.device_eval.ground_truth_arrays), Gmax <= 128 (0: no clip has a ground truth).  Every entry of ``out`` (given or
    new) is written.  check: refuse gt_count outside [0, Gmax] and counts outside [0, maxK] (ONE host read); the kernel clamps
    them either way."""
    if not regions.is_cuda:
        _chk(regions, "regions")
    if regions.dtype != torch.int64 or regions.dim() != 4 or regions.shape[3] != 2 or not regions.is_contiguous():
        raise RuntimeError(f"regions: expected the contiguous int64 (B,NT,maxK,2) of ops.segments, got {regions.dtype} "
                           f"{tuple(regions.shape)}")
    B, NT, maxk, _ = regions.shape
    counts = _grounding_tensor(counts, "counts", torch.int32, (B, NT), regions, " (ops.segments)")
    gt = torch.as_tensor(gt)
    if gt.dim() != 3 or gt.shape[2] != 2:
        raise RuntimeError(f"gt: expected float64 ({B},Gmax,2), got {gt.dtype} {tuple(gt.shape)}")
    max_gt = gt.shape[1]
    if B < 1 or NT < 1:
        raise RuntimeError(f"grounding_counts: expected B, NT >= 1, got {B}, {NT}")
    gt_count = torch.as_tensor(gt_count)
    if gt_count.dtype != torch.int32 or tuple(gt_count.shape) != (B,):
        raise RuntimeError(f"gt_count: expected {torch.int32} ({B},), got {gt_count.dtype} {tuple(gt_count.shape)}")
    if check:
        ends = [counts.min(), counts.max()] + ([gt_count.min(), gt_count.max()] if gt_count.is_cuda else [])
        lo_c, hi_c, *g_ends = torch.stack(ends).tolist()
        lo_g, hi_g = g_ends or (int(gt_count.min()), int(gt_count.max()))
        if lo_g < 0 or hi_g > max_gt or lo_c < 0 or hi_c > maxk:
            raise RuntimeError(f"grounding_counts: gt_count must lie in [0, {max_gt}] and counts in [0, {maxk}], got "
                               f"[{lo_g}, {hi_g}] and [{lo_c}, {hi_c}]")
    gt = _grounding_tensor(gt, "gt", torch.float64, (B, max_gt, 2), regions, "")
    gt_count = gt_count.to(regions.device).contiguous()
    if out is None:
        out = torch.empty(B, NT, 4, device=regions.device, dtype=torch.int32)
    elif not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != (B, NT, 4) or not out.is_contiguous():
        raise RuntimeError(f"out: expected contiguous int32 ({B},{NT},4) on the device, got {out.dtype} {tuple(out.shape)}")
    call("tag_grounding_counts", ptr(regions), ptr(counts), maxk, ptr(gt) if max_gt else None, ptr(gt_count), max_gt, B, NT,
         float(time_resolution), float(dtc), float(gtc), ptr(out))
    return out


# ------------------------------------------------------------------------------------------------
# the sed_eval protocol (utils/sed_metrics.py on the host) and the double threshold in front of it, sed_eval.hip
# ------------------------------------------------------------------------------------------------

#: the most segments of one (clip, operating point) pair tag_sed_counts rolls (= TAG_SED_MAX_SEGMENTS of include/tag_hip.h)
SED_MAX_SEGMENTS = 16384


def segments_double(frame_sim, high, low, n_connect=1):
    """The double threshold of utils/sed_utils.py:145-198 (``_double_threshold(..., return_arr=False)``) on the device: runs of
    ``x > low[i]`` that hold a frame with ``x > high[i]``, then ``connect_`` with gap <= n_connect.  high, low: length-NT
    vectors, one operating point per entry, high[i] >= low[i] (ValueError otherwise, for vectors on the host; vectors already on
    the device are not read back).  Both are rounded to float32 and compared
    in float32, as numpy compares a float32 array with a Python float -- ``segments`` compares in float64.  Returns ``segments``'
    (regions (B,NT,maxK,2) int64, counts (B,NT) int32)."""
    frame_sim = _chk(frame_sim, "frame_sim")
    B, T = frame_sim.shape
    hi = torch.as_tensor(high, dtype=torch.float64).reshape(-1)
    lo = torch.as_tensor(low, dtype=torch.float64).reshape(-1)
    NT = hi.numel()
    if NT < 1 or lo.numel() != NT:
        raise ValueError(f"segments_double: high and low must be vectors of one length >= 1, got {hi.numel()} and {lo.numel()}")
    # (host vectors are checked; device vectors are taken as they are -- SedEvaluator checked its pairs once -- so that the
    #  call reads nothing back: with high < low the kernel keeps the runs of x > low that hold a frame above high, no more)
    if not (hi.is_cuda or lo.is_cuda) and not bool((hi >= lo).all()):
        raise ValueError("segments_double: every high threshold must be >= its low threshold (a NaN is neither), got high "
                         f"{hi.tolist()}, low {lo.tolist()}")
    hi, lo = hi.to(frame_sim.device), lo.to(frame_sim.device)
    maxk = (T + 1) // 2
    regions = torch.zeros(B, NT, maxk, 2, device=frame_sim.device, dtype=torch.int64)
    counts = torch.zeros(B, NT, device=frame_sim.device, dtype=torch.int32)
    call("tag_segments_double", ptr(frame_sim), T, B, T, ptr(hi), ptr(lo), NT, int(n_connect), ptr(regions), ptr(counts), maxk)
    return regions, counts


def sed_counts(regions, counts, gt, gt_count, time_resolution, t_collar=0.2, percentage_of_length=0.2, segment_resolution=1.0,
               out=None, check=True):
    """``segments`` / ``segments_double`` outputs + the clips' ground truths -> (B, NT, 5) int32 ``{ev_tp, seg_tp, seg_fp, seg_fn,
    seg_n}`` per (clip, operating point): the integers utils.sed_metrics.event_based_counts (maximum matching inside the
    collars) and segment_based_counts (event rolls at ``segment_resolution``) give for that clip as one file, exactly
    (sed_eval.hip).  Arguments as for ``grounding_counts``; the regions in use must ascend and be disjoint, ground-truth times
    must be >= 0.  A pair may span at most SED_MAX_SEGMENTS segments.  Every entry of ``out`` (given or new) is written.
    check: refuse gt_count outside [0, Gmax], counts outside [0, maxK] and a pair above the segment limit (ONE host read);
    without it the kernel clamps the counts and writes -1 into all five entries of a pair above the limit."""
    if not regions.is_cuda:
        _chk(regions, "regions")
    if regions.dtype != torch.int64 or regions.dim() != 4 or regions.shape[3] != 2 or not regions.is_contiguous():
        raise RuntimeError(f"regions: expected the contiguous int64 (B,NT,maxK,2) of ops.segments, got {regions.dtype} "
                           f"{tuple(regions.shape)}")
    B, NT, maxk, _ = regions.shape
    counts = _grounding_tensor(counts, "counts", torch.int32, (B, NT), regions, " (ops.segments)")
    gt = torch.as_tensor(gt)
    if gt.dim() != 3 or gt.shape[2] != 2:
        raise RuntimeError(f"gt: expected float64 ({B},Gmax,2), got {gt.dtype} {tuple(gt.shape)}")
    max_gt = gt.shape[1]
    if B < 1 or NT < 1:
        raise RuntimeError(f"sed_counts: expected B, NT >= 1, got {B}, {NT}")
    gt_count = torch.as_tensor(gt_count)
    if gt_count.dtype != torch.int32 or tuple(gt_count.shape) != (B,):
        raise RuntimeError(f"gt_count: expected {torch.int32} ({B},), got {gt_count.dtype} {tuple(gt_count.shape)}")
    time_resolution, segment_resolution = float(time_resolution), float(segment_resolution)
    gt = _grounding_tensor(gt, "gt", torch.float64, (B, max_gt, 2), regions, "")
    gt_count = gt_count.to(regions.device).contiguous()
    if check and max_gt <= 128 and maxk >= 1:                   # (the sizes the library refuses it names itself)
        # the largest offsets in use, in one read with the ends of the counts (every integer here is exact in fp64)
        used = torch.arange(maxk, device=regions.device) < counts[..., None]
        last_frame = torch.where(used, regions[..., 1], 0).max()
        gt_used = torch.arange(max_gt, device=regions.device) < gt_count[:, None]
        zero = torch.zeros((), device=regions.device, dtype=torch.float64)
        last_gt = torch.where(gt_used, gt[..., 1], zero).max() if max_gt else zero
        ends = [counts.min(), counts.max(), gt_count.min(), gt_count.max(), last_frame, last_gt]
        lo_c, hi_c, lo_g, hi_g, last_frame, last_gt = torch.stack([e.double() for e in ends]).tolist()
        if lo_g < 0 or hi_g > max_gt or lo_c < 0 or hi_c > maxk:
            raise RuntimeError(f"sed_counts: gt_count must lie in [0, {max_gt}] and counts in [0, {maxk}], got "
                               f"[{int(lo_g)}, {int(hi_g)}] and [{int(lo_c)}, {int(hi_c)}]")
        if not math.isfinite(last_gt):
            raise RuntimeError(f"gt: an offset in use is not finite ({last_gt})")
        if segment_resolution > 0 and time_resolution > 0:
            n_seg = max(math.ceil(last_frame * time_resolution / segment_resolution), math.ceil(last_gt / segment_resolution))
            if not n_seg <= SED_MAX_SEGMENTS:
                raise RuntimeError(f"sed_counts: segment_resolution = {segment_resolution} cuts the longest pair into {n_seg} "
                                   f"segments; at most {SED_MAX_SEGMENTS} are taken")
    if out is None:
        out = torch.empty(B, NT, 5, device=regions.device, dtype=torch.int32)
    elif not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != (B, NT, 5) or not out.is_contiguous():
        raise RuntimeError(f"out: expected contiguous int32 ({B},{NT},5) on the device, got {out.dtype} {tuple(out.shape)}")
    call("tag_sed_counts", ptr(regions), ptr(counts), maxk, ptr(gt) if max_gt else None, ptr(gt_count), max_gt, B, NT,
         time_resolution, float(t_collar), float(percentage_of_length), segment_resolution, ptr(out))
    return out


# ------------------------------------------------------------------------------------------------
# score-based PSDS: the counts of every threshold the scores define (utils/psds_scores.py on the host), psds_scores.hip
# ------------------------------------------------------------------------------------------------

#: the most frames per pair tag_psds_score_deltas takes (= TAG_PSDS_SCORES_MAX_T of include/tag_hip.h)
PSDS_SCORES_MAX_T = 1024


def psds_score_deltas(frame_sim, gt, gt_count, time_resolution, dtc=0.5, gtc=0.5, check=True):
    """Frame scores + the pairs' ground truths -> ``(values (B,T) fp32, deltas (B,T,2) int32, base (B,2) int32, n_values (B,)
    int32)``: per pair the ascending distinct non-NaN scores v_1 .. v_m (then +inf; -0.0 is +0.0), the differences
    c_{j+1} - c_j of the PSDS counts c_k = (psds_tp, psds_fp) of the regimes ``score > v_k`` (then 0), c_0 (v_0 = -inf) and m --
    the integers utils.psds_scores.pair_regimes gives, exactly (psds_scores.hip).  ``n_values`` is authoritative: a genuine +inf
    score is a value.  frame_sim (B, T) float32 on the device, T <= PSDS_SCORES_MAX_T; a view with unit inner stride and a row
    stride >= T is taken as it is.  gt (B,Gmax,2) float64 seconds and gt_count (B,) int32, on the device or on the host
    (utils.device_eval.ground_truth_arrays), Gmax <= 128.  Every entry of the four outputs is written; one launch.
    check: refuse gt_count outside [0, Gmax] (ONE host read for a device tensor); the kernel clamps it either way."""
    if not frame_sim.is_cuda:
        _chk(frame_sim, "frame_sim")
    if frame_sim.dtype != F32 or frame_sim.dim() != 2 or frame_sim.shape[0] < 1 or frame_sim.shape[1] < 1:
        raise RuntimeError(f"frame_sim: expected a float32 (B >= 1, T >= 1) matrix, got {frame_sim.dtype} {tuple(frame_sim.shape)}")
    B, T = frame_sim.shape
    if frame_sim.stride(1) != 1 or (B > 1 and frame_sim.stride(0) < T):
        frame_sim = frame_sim.contiguous()
    ld = frame_sim.stride(0) if B > 1 else T
    gt = torch.as_tensor(gt)
    if gt.dim() != 3 or gt.shape[2] != 2:
        raise RuntimeError(f"gt: expected float64 ({B},Gmax,2), got {gt.dtype} {tuple(gt.shape)}")
    max_gt = gt.shape[1]
    gt_count = torch.as_tensor(gt_count)
    if gt_count.dtype != torch.int32 or tuple(gt_count.shape) != (B,):
        raise RuntimeError(f"gt_count: expected {torch.int32} ({B},), got {gt_count.dtype} {tuple(gt_count.shape)}")
    if check:
        lo_g, hi_g = torch.stack([gt_count.min(), gt_count.max()]).tolist()
        if lo_g < 0 or hi_g > max_gt:
            raise RuntimeError(f"psds_score_deltas: gt_count must lie in [0, {max_gt}], got [{lo_g}, {hi_g}]")
    gt = _grounding_tensor(gt, "gt", torch.float64, (B, max_gt, 2), frame_sim, "")
    gt_count = gt_count.to(frame_sim.device).contiguous()
    values = torch.empty(B, T, device=frame_sim.device, dtype=F32)
    deltas = torch.empty(B, T, 2, device=frame_sim.device, dtype=torch.int32)
    base = torch.empty(B, 2, device=frame_sim.device, dtype=torch.int32)
    n_values = torch.empty(B, device=frame_sim.device, dtype=torch.int32)
    call("tag_psds_score_deltas", ptr(frame_sim), ld, B, T, ptr(gt) if max_gt else None, ptr(gt_count), max_gt,
         float(time_resolution), float(dtc), float(gtc), ptr(values), ptr(deltas), ptr(base), ptr(n_values))
    return values, deltas, base, n_values


# ------------------------------------------------------------------------------------------------
# phrase-to-label cosine map of the ASMapping datasets (sklearn's cosine_similarity per item on the host in the reference),
# label_map.hip
# ------------------------------------------------------------------------------------------------

#: the largest k of tag_label_map_topk (= TAG_LABEL_MAP_MAX_TOPK of include/tag_hip.h)
LABEL_MAP_MAX_TOPK = 32

LabelMapResult = collections.namedtuple("LabelMapResult", "best best_sim min_sim win_best win_count win_bits sim idx")


def label_map(x, e, th0, th1, topk=1, want_sim=False):
    """The cosine map of phrases x (N, D) onto labels e (C, D), one march on the exact-fp32 MFMA: s = x_i . e_c / (||x_i|| ||e_c||)
    in fp32 (a zero row's norm taken as 1), the WINDOW of a row = the labels with th0 <= s <= th1 and s != 0, th0 / th1 compared as
    float32.  -> LabelMapResult of device tensors:

    best (N,) int32 argmax_c s (ties to the lowest c), best_sim (N,) fp32, min_sim (N,) fp32; win_best (N,) int32 the argmax over
    the window or -1, win_count (N,) int32, win_bits (N, ceil(C / 32)) int32 (bit c % 32 of word c // 32; bits past C are 0);
    sim (N, C) fp32 when want_sim, else None (no (N, C) array exists unless topk >= 2 needs one); idx (N, min(topk, C)) int32,
    the window members in descending s padded with -1, when topk >= 2, else None (win_best is the topk == 1 answer, win_bits the
    topk <= 0 one).  Row-strided views of x and e are passed as they are.  The same bits on every run."""
    xr, er = _phrase_sim_rows(x, "x"), _phrase_sim_rows(e, "e")
    if er.device != xr.device or er.shape[1] != xr.shape[1]:
        raise RuntimeError(f"e {tuple(er.shape)} on {er.device}: expected x's device {xr.device} and D = {xr.shape[1]}")
    (N, D), C = xr.shape, er.shape[0]
    th0, th1, topk = float(th0), float(th1), int(topk)
    if math.isnan(th0) or math.isnan(th1):
        raise ValueError(f"label_map: thresholds must be numbers, got {th0}, {th1}")
    k = min(topk, C)
    if k > LABEL_MAP_MAX_TOPK:
        raise ValueError(f"label_map: topk = {topk} over {C} labels exceeds {LABEL_MAP_MAX_TOPK}; topk <= 0 gives the whole window")
    nws = query("tag_label_map_ws_bytes", N, C, D)
    if nws == 0:
        raise RuntimeError(f"label_map: N = {N}, C = {C}, D = {D}: expected N and C <= {2**31 - 129}")
    dev = xr.device
    best, win_best, win_count = (torch.empty(N, device=dev, dtype=torch.int32) for _ in range(3))
    best_sim, min_sim = torch.empty(N, device=dev, dtype=F32), torch.empty(N, device=dev, dtype=F32)
    win_bits = torch.empty(N, (C + 31) // 32, device=dev, dtype=torch.int32)
    sim = torch.empty(N, C, device=dev, dtype=F32) if (want_sim or k >= 2) else None
    ws = _ws(nws, xr)
    call("tag_label_map", ptr(xr), xr.stride(0), ptr(er), er.stride(0), th0, th1, ptr(best), ptr(best_sim), ptr(min_sim),
         ptr(win_best), ptr(win_count), ptr(win_bits), ptr(sim), C, N, C, D, ptr(ws))
    idx = None
    if k >= 2:
        idx = torch.empty(N, k, device=dev, dtype=torch.int32)
        call("tag_label_map_topk", ptr(sim), C, th0, th1, ptr(idx), N, C, k)
    return LabelMapResult(best, best_sim, min_sim, win_best, win_count, win_bits, sim if want_sim else None, idx)


# ------------------------------------------------------------------------------------------------
# BERTScore phrase-to-label map (bert_score.score on every (phrase, label) pair in the reference's prepare_phrase_bertscore.py),
# bertscore.hip
# ------------------------------------------------------------------------------------------------

#: the item slots of tag_bertscore_map (include/tag_hip.h) and the longest item
BERTSCORE_SLOTS = (8, 16, 32)
BERTSCORE_MAX_LEN = 32

BertScoreMapResult = collections.namedtuple("BertScoreMapResult", "best best_f best_p best_r scores")


def bertscore_slot(L):
    """The smallest accepted slot that holds items of L tokens."""
    for s in BERTSCORE_SLOTS:
        if L <= s:
            return s
    raise ValueError(f"bertscore_map: items of {L} tokens exceed the largest slot {BERTSCORE_MAX_LEN}")


def bertscore_default_weights(lens, L):
    """bert_score's weights with idf=False: 1 for every token below the length, 0 for the first and the last token of an item
    (its [CLS] and [SEP]); (rows, L) fp32 on the device of lens.  An item of one or two tokens has no weight left."""
    pos = torch.arange(L, device=lens.device)[None, :]
    n = lens.to(torch.int64)[:, None]
    return ((pos >= 1) & (pos < n - 1)).to(F32)


def _bertscore_check(x, x_len, x_w, name):
    """The checks of one operand that need no device -> (lengths tensor, the longest length)."""
    if not torch.is_tensor(x) or x.dtype != F32 or x.dim() != 3 or min(x.shape) < 1:
        raise RuntimeError(f"{name}: expected a float32 (items >= 1, L >= 1, D >= 1) tensor, got "
                           f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    rows, L, D = x.shape
    if x_len is None:
        if L > BERTSCORE_MAX_LEN:
            raise ValueError(f"{name}: L = {L} tokens per item exceed the limit {BERTSCORE_MAX_LEN}; pass {name}_len")
        x_len = torch.full((rows,), L, device=x.device, dtype=torch.int32)
    if not torch.is_tensor(x_len) or x_len.device != x.device or x_len.dtype not in (torch.int32, torch.int64) \
            or tuple(x_len.shape) != (rows,):
        raise RuntimeError(f"{name}_len: expected an int32 / int64 ({rows},) tensor on {x.device}, got "
                           f"{getattr(x_len, 'dtype', type(x_len))} {tuple(getattr(x_len, 'shape', ()))} on "
                           f"{getattr(x_len, 'device', 'the host')}")
    if x_w is not None and (not torch.is_tensor(x_w) or x_w.device != x.device or x_w.dtype != F32
                            or tuple(x_w.shape) != (rows, L)):
        raise RuntimeError(f"{name}_w: expected a float32 ({rows}, {L}) tensor on {x.device}, got "
                           f"{getattr(x_w, 'dtype', type(x_w))} {tuple(getattr(x_w, 'shape', ()))} on "
                           f"{getattr(x_w, 'device', 'the host')}")
    if x.device.type == "meta":
        return x_len, min(L, BERTSCORE_MAX_LEN)
    lo, hi = torch.stack([x_len.min(), x_len.max()]).tolist()          # (one read of the device per operand)
    if lo < 1 or hi > min(L, BERTSCORE_MAX_LEN):
        raise ValueError(f"{name}_len: lengths must lie in [1, {min(L, BERTSCORE_MAX_LEN)}] (L = {L}, the limit is "
                         f"{BERTSCORE_MAX_LEN} tokens per item), got [{lo}, {hi}]")
    return x_len, hi


def _bertscore_operand(x, x_len, x_w, longest, normalize):
    """-> (tokens (rows, slot, D) fp32 with unit column stride, lengths int32 (rows,), weights fp32 (rows, slot), slot)"""
    rows, L, D = x.shape
    slot = bertscore_slot(longest)
    keep = min(L, slot)                                   # (columns past the longest item hold nothing that is used)
    if x_w is None:
        w = bertscore_default_weights(x_len, slot)
    else:
        w = torch.zeros(rows, slot, device=x.device, dtype=F32)
        w[:, :keep] = x_w[:, :keep]
    if L == slot and not normalize and x.stride(2) == 1 and x.stride(1) >= D and x.stride(0) == slot * x.stride(1):
        tok = x                                           # slot-sized unit rows: passed as they are, any 4-byte aligned base
    else:
        tok = torch.zeros(rows, slot, D, device=x.device, dtype=F32)
        tok[:, :keep] = x[:, :keep]
        if normalize:
            tok = _unit_rows(tok.view(rows * slot, D), rows * slot, D).view(rows, slot, D)
    return tok, x_len.to(torch.int32).contiguous(), w.contiguous(), slot


def bertscore_map(a, a_len, a_w, b, b_len, b_w, want_scores=False, normalize=True):
    """BERTScore of every phrase against every label by greedy token matching, one march on the exact-fp32 MFMA (bertscore.hip):
    a (N, La, D) phrase tokens with lengths a_len (N,) and weights a_w (N, La), b (C, Lb, D), b_len (C,), b_w (C, Lb) the labels;
    any La, Lb, every length in 1 .. 32 (and <= La, Lb).  With s_ij = a[n,i] . b[c,j] over the tokens below the lengths:
    P = sum_i a_w max_j s_ij / sum_i a_w, R = sum_j b_w max_i s_ij / sum_j b_w, F = 2 P R / (P + R); a zero weight sum gives 0, and
    so does P + R == 0.  A padded position enters no maximum and no sum.  -> BertScoreMapResult of device tensors:

    best (N,) int32 argmax_c F (ties to the lowest c), best_f, best_p, best_r (N,) fp32 the values there, scores (3, N, C) fp32
    = P, R, F of every pair when want_scores, else None (no score array of any kind exists then).

    a_len / b_len None: every item is full; a_w / b_w None: bert_score's idf=False weights (bertscore_default_weights: 0 for the
    first and last token of an item, 1 between).  normalize: the token vectors through x / max(||x||, 1e-12) first (bert_score's
    order: normalise, then multiply); with normalize=False a (items, slot, D) tensor or row-strided view whose L is an accepted
    slot (8, 16, 32) is passed to the kernel as it is.  Items are padded to the smallest slot that holds the longest one.
    The same bits on every run; there is no CPU fallback."""
    a_len, a_hi = _bertscore_check(a, a_len, a_w, "a")
    b_len, b_hi = _bertscore_check(b, b_len, b_w, "b")
    if b.device != a.device or b.shape[2] != a.shape[2]:
        raise RuntimeError(f"b {tuple(b.shape)} on {b.device}: expected a's device {a.device} and D = {a.shape[2]}")
    if not a.is_cuda:
        raise RuntimeError(f"a, b: expected tensors on the MI355X (cuda) device, got {a.device}; the HIP path has no CPU fallback")
    at, al, aw, sa = _bertscore_operand(a, a_len, a_w, a_hi, normalize)
    bt, bl, bw, sb = _bertscore_operand(b, b_len, b_w, b_hi, normalize)
    N, C, D = at.shape[0], bt.shape[0], at.shape[2]
    nws = query("tag_bertscore_map_ws_bytes", N, C, D, sa, sb)
    if nws == 0:
        raise RuntimeError(f"bertscore_map: N = {N} x slot {sa}, C = {C} x slot {sb}: expected at most {2**31 - 129} token rows")
    dev = at.device
    best = torch.empty(N, device=dev, dtype=torch.int32)
    best_f, best_p, best_r = (torch.empty(N, device=dev, dtype=F32) for _ in range(3))
    scores = torch.empty(3, N, C, device=dev, dtype=F32) if want_scores else None
    ws = _ws(nws, at)
    call("tag_bertscore_map", ptr(at), at.stride(1), ptr(al), ptr(aw), ptr(bt), bt.stride(1), ptr(bl), ptr(bw), sa, sb, N, C, D,
         ptr(best), ptr(best_f), ptr(best_p), ptr(best_r), ptr(scores), ptr(ws))
    return BertScoreMapResult(best, best_f, best_p, best_r, scores)
