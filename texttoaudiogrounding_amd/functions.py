"""torch.autograd nodes of the hot path: forward() / backward() of each node are sequences of dispatch.py launches; parameter
gradients are delivered through engine.py's direct-gradient sinks.  The four whole-encoder nodes state each launch plan once:

* Cnn8 family -- Cnn8RnnFunction and the early-fusion CrossCnn8RnnFunction share the set-up, the stem (logmel, bn0, augment, the
  Cin = 1 conv), the tail (mean over W, fc1) and the per-block epilogue (_cnn8_*); their block middles are different algorithms
  (fused BatchNorm / pool epilogues against per-clip bias passes) and stay apart.  ConvTextBlockFunction runs
  CrossCnn8RnnFunction's text-block forward (_text_block_forward).
* CDur family -- CrnnFunction and the early-fusion CrossCDurFunction are thin callers of _cdur_forward / _cdur_backward, which
  walk the five-block table CDUR_POOLS without or with the text biases; CDurTextBlockFunction shares their kernel choice
  (_cdur_conv) and the scalar-bn0 backward (_scalar_bn_backward).

Then the weight-gradient side-stream helper, the text / match / loss heads and the cross-encoder nodes.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import settings as cfg
from .lib import call, ptr, query
from .engine import (F32, TagFunction, _chk, _deliver, _empty, _flush, _ready, _side_stream, _sinks, _ws, new_seed,
                     side_stream_enabled)
from .dispatch import (BF16, BNStat, C1_BWD_FUSED_SHAPE, _sfx, _wino_u, act_bf16, augment_backward, augment_forward,
                       bn_act_backward, bn_param_grad,
                       bn_stats, bnact_pool, bnrelu_pool_backward, check_pass_size, colsum, conv3x3,
                       conv3x3_bnrelu_pool_eval, conv3x3_c1, conv3x3_c1_backward, conv3x3_c1_dgrad, conv3x3_c1_stats,
                       conv3x3_c1_wgrad, conv3x3_dgrad_bnrelu_backward, conv3x3_dgrad_poolsums, conv3x3_stats,
                       conv3x3_wgrad, embed_mean_backward_into, embed_mean_forward, eval_pool_fusable, gemm,
                       gru_bidir_backward, gru_bidir_forward, logmel, lppool_leaky_backward, pack_conv_weight,
                       pool_sums_fusable, relu_backward)
from .dispatch import (bias_bnrelu_backward, bias_bnrelu_forward, bias_bnrelu_pool, bias_bnrelu_pool_backward,
                       bn_act_backward_clip, conv3x3_bias, conv3x3_c1_bias, frame_head_backward, frame_head_forward, gemm_bf16, leaky_backward,
                       leaky_forward, lppool_leaky_backward_clip, rowgroup_bias_relu, rowgroup_colsum)
from .dispatch import class_pool_forward, tagging_head_dlogit
from .dispatch import text_gru_backward, text_gru_forward
from .dispatch import text_selfattn_backward, text_selfattn_forward
from .dispatch import text_bert_backward, text_bert_forward
from .dispatch import text_clap_backward, text_clap_forward
from .dispatch import text_intra_backward, text_intra_forward
from . import engine

# ------------------------------------------------------------------------------------------------
# Cnn8Rnn and the early-fusion CrossCnn8_Rnn: the whole audio encoder as one autograd node (rows F1-F3, A1-A4 forward + backward)
# ------------------------------------------------------------------------------------------------

CNN8_POOLS = [(2, 2), (2, 2), (1, 2), (1, 2)]


class _SideWgrad:
    """Runs conv3x3_wgrad calls on the side stream; join() makes the main stream wait for all of them.

    Lifetime of the tensors the side stream reads or writes: they are allocated on the MAIN stream, and the caching allocator
    would hand their memory to the main stream's next allocation the moment Python drops them.  They are therefore kept alive in
    ``self.keep`` until join() has made the main stream wait for the side stream -- from then on a release on the main stream is
    ordered after every side-stream access.  (Round 4 used ``Tensor.record_stream`` instead.  That defers the reuse of a block
    until the HOST sees the side stream's event complete; a host that enqueues K unsynchronised steps runs far ahead of the
    GPU, sees none complete and takes NEW memory for every step (measured: 53-75 GB of reserve for 3-6 GB of tensors after 30-60
    steps -- 100-150 GB on a fast box --, 22-26 ms of host time per step inside hipMalloc), and in every second of a row of
    `bench.py --conv-math x3 --steps 30` processes ONE such hipMalloc blocked for 0.7-2.6 s (the driver still reclaiming the
    previous process's reserve): kernels at their normal durations, the main thread asleep (docs/experiments_r05.md).)"""

    def __init__(self, device):
        self.on = side_stream_enabled()
        self.main = torch.cuda.current_stream(device)
        self.side = _side_stream(device) if self.on else None
        self.pending = []
        self.keep = []

    def wgrad(self, x, dy, prologue=0, scale=None, shift=None, out=None):
        if not self.on:
            return conv3x3_wgrad(x, dy, prologue, scale, shift, out=out)
        dw = out if out is not None else _empty(dy.shape[3], x.shape[3], 3, 3, like=x)
        self.pending.append((x, dy, prologue, scale, shift, dw))
        if not cfg.WGRAD_LAG:
            self.release()
        return dw

    def run(self, fn, tensors=()):
        """``fn()`` on the side stream, ordered after everything enqueued on the main stream so far (inline when the side
        stream is off).  ``tensors``: main-stream allocations fn reads (kept alive until join())."""
        if not self.on:
            fn()
            return
        self.release()
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side):
            fn()
        self._hold(tensors)

    def release(self):
        """Launch the queued wgrads on the side stream, ordered after everything enqueued on the main stream so far."""
        if not self.pending:
            return
        self.side.wait_stream(self.main)                 # x, dy (and the BN constants) are ready
        with torch.cuda.stream(self.side):
            for x, dy, prologue, scale, shift, dw in self.pending:
                conv3x3_wgrad(x, dy, prologue, scale, shift, out=dw)
        for item in self.pending:
            self._hold(item)
        self.pending = []

    def _hold(self, tensors):
        for t in tensors:
            if isinstance(t, torch.Tensor):
                if cfg.SIDE_RECORD_STREAM:
                    t.record_stream(self.side)
                else:
                    self.keep.append(t)

    def join(self):
        if self.on:
            self.release()
            self.main.wait_stream(self.side)
            self.keep = []                               # released on the main stream, ordered after the wait


def _cnn8_begin(waveform, mod, params):
    """What both Cnn8 nodes do before their first launch: input checks, detached parameters (bn0.w, bn0.b, 4 x (conv1.w,
    bn1.w, bn1.b, conv2.w, bn2.w, bn2.b), fc1.w, fc1.b, 8 GRU tensors, ...), dropout probabilities and the five seeds."""
    wave = _chk(waveform, "waveform")
    check_pass_size(wave.shape[0], wave.shape[1] // mod.hop_length + 1)
    training = mod.training
    p = [_chk(t.detach(), "parameter") for t in params]
    drop = mod.dropout_p if training else (0.0, 0.0)
    seeds = [new_seed() for _ in range(5)] if training and (drop[0] > 0 or drop[1] > 0) else [0] * 5
    return wave, p, training and not mod.freeze_bn, drop, seeds


def _cnn8_stem_forward(wave, mod, p, bn_train, aug, out_dtype=F32):
    """logmel -> bn0 statistics -> [augment] -> conv_block1.conv1.  ``aug`` (ctx.augment): bn0 is then applied by augment_forward
    into x0 (B or B/2 clips) instead of inside the Cin = 1 convolution; bn0's statistics stay over all B clips.
    -> (lm, st0, x0, y1, part1)."""
    lm = logmel(wave, mod.n_fft, mod.win_length, mod.hop_length, mod.window, mod.mel_fb)   # (B,F,64)
    B, Fr, NM = lm.shape
    st0 = bn_stats(lm.view(B * Fr, NM), p[0], p[1], mod.bn0.running_mean, mod.bn0.running_var, bn_train, mod.bn0.eps,
                   mod.bn0.momentum)
    if aug is None:
        x0 = None
        y1, part1 = conv3x3_c1_stats(lm, p[2], st0.scale, st0.shift, want_stats=bn_train, out_dtype=out_dtype)
    else:
        x0 = augment_forward(lm, st0.scale, st0.shift, *aug)                                 # (B',F,64), bn0 applied
        y1, part1 = conv3x3_c1_stats(x0, p[2], None, None, want_stats=bn_train, out_dtype=out_dtype)
    return lm, st0, x0, y1, part1


def _cnn8_tail_forward(x, fc_w, fc_b, drop_p, seed, act):
    """Mean over W (with its dropout) and fc1: x (B,T',W',C) -> xm (B*T', C), fc = act(xm fc_w^T + fc_b)."""
    Bx, Tp, Wp, C = x.shape
    xm = _empty(Bx * Tp, C, like=x)
    call("tag_mean_w_forward" + _sfx(x), ptr(x), Bx * Tp, Wp, C, float(drop_p), seed, ptr(xm))
    return xm, gemm(xm, fc_w, Bx * Tp, fc_w.shape[0], C, transB=True, bias=fc_b, act=act)


def _cnn8_tail_backward(dfc, fc_w, x_last, drop_p, seed):
    """fc1's input gradient and the backward of the mean over W: -> dx, shaped like the last block's output x_last."""
    M = dfc.shape[0]
    dxm = gemm(dfc, fc_w, M, fc_w.shape[1], fc_w.shape[0])
    Bx, Tp, Wp, C = x_last.shape
    dx = torch.empty_like(x_last)
    call("tag_mean_w_backward" + _sfx(dx), ptr(dxm), Bx * Tp, Wp, C, float(drop_p), seed, ptr(dx))
    return dx


def _cnn8_stem_backward(sv, dy1, grads, sk, bn_bwd=None):
    """Backward of conv_block1.conv1 [and augment] and bn0's parameter gradients; delivers parameters 2, 0 and 1.
    bn_bwd: see conv3x3_c1_backward (the deferred BatchNorm + ReLU backward of bn1)."""
    lm, st0, x0 = sv["lm"], sv["st0"], sv["x0"]
    if x0 is None:
        dw0, dbn0 = conv3x3_c1_backward(lm, dy1, sv["p"][2], st0.scale, st0.shift, out=sk[2], bn_bwd=bn_bwd)   # dbn0: (B,F,64)
    else:
        dw0, dx0 = conv3x3_c1_backward(x0, dy1, sv["p"][2], None, None, out=sk[2], bn_bwd=bn_bwd)
        dbn0 = augment_backward(dx0, lm.shape[0], *sv["aug"])
        del dx0
    _deliver(grads, sk, 2, dw0)
    Bq, Fr, NM = lm.shape
    dg0, db0 = bn_param_grad(lm.view(Bq * Fr, NM), dbn0.view(Bq * Fr, NM), st0, dg_out=sk[0], db_out=sk[1])
    _deliver(grads, sk, 0, dg0)
    _deliver(grads, sk, 1, db0)


def _cnn8_block_done(sw, prm, i):
    """End of block i's backward: every gradient kernel of the block is enqueued before its parameters are announced."""
    sw.release()
    if prm is not None:
        o = 2 + 6 * i
        _ready(prm[o:o + 6] + ((prm[0], prm[1]) if i == 0 else ()))
        _flush()


class Cnn8RnnFunction(TagFunction):
    """params order: bn0.w, bn0.b, 4 x (conv1.w, bn1.w, bn1.b, conv2.w, bn2.w, bn2.b), fc1.w, fc1.b,
    rnn (w_ih, w_hh, b_ih, b_hh) x (fwd, reverse).

    ``ctx.augment`` (set by tag::cnn8rnn_encoder, absent otherwise): (stripes, n_time, lam) -- SpecAugment's stripe table and /
    or mixup's lambda applied to the bn0 output (models/audio_encoder.py:192-200).  Then bn0 is applied by augment_forward into
    x0 (B or B/2 clips) instead of inside the Cin = 1 convolution, and every later stage takes its batch from the tensor it reads;
    bn0's statistics stay over all B clips."""

    @staticmethod
    def forward(ctx, waveform, mod, *params):
        wave, p, bn_train, drop, seeds = _cnn8_begin(waveform, mod, params)
        need_grad = any(ctx.needs_input_grad[2:])
        aug = getattr(ctx, "augment", None)
        lm, st0, x0, y1, part1 = _cnn8_stem_forward(wave, mod, p, bn_train, aug, out_dtype=BF16 if act_bf16() else F32)
        x = wd1 = None
        acts = []
        for i in range(4):
            c1w, g1, b1, c2w, g2, b2 = p[2 + 6 * i: 8 + 6 * i]
            blk = getattr(mod, f"conv_block{i + 1}")
            if i > 0:
                wf1, wd1 = pack_conv_weight(c1w, want_dgrad=need_grad, W=x.shape[2])
                y1, part1 = conv3x3_stats(x, wf1, c1w.shape[0], want_stats=bn_train,
                                          inference=not need_grad and not bn_train and drop[0] == 0.0)
            Bx, H, W, C = y1.shape
            s1 = bn_stats(y1.view(-1, C), g1, b1, blk.bn1.running_mean, blk.bn1.running_var, bn_train, blk.bn1.eps,
                          blk.bn1.momentum, partials=part1)
            wf2, wd2 = pack_conv_weight(c2w, want_dgrad=need_grad, W=y1.shape[2])
            ph, pw = CNN8_POOLS[i]
            if not need_grad and not bn_train and drop[0] == 0.0 and eval_pool_fusable(y1, wf2, ph, pw):
                # inference (models/hf_modeling_grounding.py; evaluation between epochs): bn2's affine is known before the conv
                # runs, so conv2 pools its own output tile -- y2, the block's largest tensor, is never written or read back
                s2 = bn_stats(g2.view(1, C), g2, b2, blk.bn2.running_mean, blk.bn2.running_var, False, blk.bn2.eps, blk.bn2.momentum)
                x = conv3x3_bnrelu_pool_eval(y1, wf2, C, s2, ph, pw, prologue=1, scale=s1.scale, shift=s1.shift)
                continue
            y2, part2 = conv3x3_stats(y1, wf2, C, prologue=1, scale=s1.scale, shift=s1.shift, want_stats=bn_train)
            s2 = bn_stats(y2.view(-1, C), g2, b2, blk.bn2.running_mean, blk.bn2.running_var, bn_train, blk.bn2.eps,
                          blk.bn2.momentum, partials=part2)
            xo = bnact_pool(y2, s2, ph, pw, act=1, pool=0, drop_p=drop[0], seed=seeds[i])
            if need_grad:                      # inference: intermediates die here (30 s clips x 64 are GBs per layer)
                acts.append((x, y1, s1, y2, s2, wd1, wd2))
            x = xo
        xm, fc = _cnn8_tail_forward(x, p[26], p[27], drop[1], seeds[4], act=1)
        y, gsave = gru_bidir_forward(fc, p[28:36], x.shape[0], x.shape[1], need_grad)
        if need_grad:
            ctx.saved = dict(lm=lm, st0=st0, aug=aug, x0=x0, acts=acts, x_last=x, xm=xm, fc=fc, gsave=gsave, p=p, drop=drop,
                             seeds=seeds, sinks=_sinks(params), params=params if cfg.DIRECT_GRADS else None)
        mod._last_dropout = dict(p=drop, seeds=seeds)
        return y

    @staticmethod
    def backward(ctx, dy):
        sv = ctx.saved
        ctx.saved = None
        p = sv["p"]
        drop, seeds = sv["drop"], sv["seeds"]
        dy = _chk(dy, "grad_output")
        grads: List[Optional[torch.Tensor]] = [None] * len(p)
        sk, prm = sv["sinks"], sv["params"]
        fc = sv["fc"]
        sw = _SideWgrad(dy.device)
        dfc, ggru = gru_bidir_backward(dy, fc, sv["gsave"], outs=sk[28:36], side=sw if cfg.SIDE_PARAM_GRADS >= 1 else None)
        for k in range(8):
            _deliver(grads, sk, 28 + k, ggru[k])
        M = fc.shape[0]
        dfc = relu_backward(fc, dfc)
        xm = sv["xm"]
        fc_w = p[26]
        if cfg.SIDE_PARAM_GRADS >= 2 and sk[26] is not None and sk[27] is not None:
            # fc1's parameter gradients are off the dx chain too: beside the passes below, on the side stream
            sw.run(lambda: (gemm(dfc, xm, fc_w.shape[0], fc_w.shape[1], M, transA=True, lda=fc_w.shape[0], out=sk[26]),
                            colsum(dfc, M, fc_w.shape[0], out=sk[27])), (dfc, xm))
            _deliver(grads, sk, 26, sk[26])
            _deliver(grads, sk, 27, sk[27])
        else:
            _deliver(grads, sk, 26, gemm(dfc, xm, fc_w.shape[0], fc_w.shape[1], M, transA=True, lda=fc_w.shape[0], out=sk[26]))
            _deliver(grads, sk, 27, colsum(dfc, M, fc_w.shape[0], out=sk[27]))
        if prm is not None:
            # the persistent GRU backward is enqueued: from here on a bucket's all-reduce may run beside the kernels of
            # this stream (never beside the spinning GRU workgroups: the collective is ordered after them)
            _ready(prm[26:36])
            _flush()
        if not any(ctx.needs_input_grad[2:28]):
            # Cnn8Rnn(freeze_cnn=True) (models/audio_encoder.py:164-168: everything but the GRU frozen): no parameter below the
            # GRU takes a gradient and the waveform never does -- the conv stack's backward (97 % of the step) is not run
            sw.join()
            return (None, None, *grads)
        dx = _cnn8_tail_backward(dfc, fc_w, sv["x_last"], drop[1], seeds[4])
        # ---- conv blocks, last to first ----
        poolpart = None                            # sums of block i's pool backward, taken by block i+1's dgrad conv
        for i in range(3, -1, -1):
            x_in, y1, s1, y2, s2, wd1, wd2 = sv["acts"][i]
            c1w, g1, b1, c2w, g2, b2 = p[2 + 6 * i: 8 + 6 * i]
            o = 2 + 6 * i
            ph, pw = CNN8_POOLS[i]
            C = y2.shape[3]
            dy2, dg2, db2 = bnrelu_pool_backward(y2, s2, g2, dx, ph, pw, drop[0], seeds[i], dg_out=sk[o + 4], db_out=sk[o + 5],
                                                 partials=poolpart)
            poolpart = None
            _deliver(grads, sk, o + 4, dg2)
            _deliver(grads, sk, o + 5, db2)
            del dx
            _deliver(grads, sk, o + 3, sw.wgrad(y1, dy2, prologue=1, scale=s1.scale, shift=s1.shift, out=sk[o + 3]))
            # block 1: its first conv has ONE consumer of dy1 (the Cin = 1 backward), which applies bn1's backward itself
            defer = i == 0 and cfg.FUSE_C1_BN_BWD and (y1.shape[2], y1.shape[3]) == C1_BWD_FUSED_SHAPE
            res = conv3x3_dgrad_bnrelu_backward(dy2, wd2, y1, s1, g1, dg_out=sk[o + 1], db_out=sk[o + 2],
                                                after_conv=sw.release, defer_apply=defer)
            dy1, dg1, db1 = res[:3]
            applied = res[3] if defer else True
            del dy2
            _deliver(grads, sk, o + 1, dg1)
            _deliver(grads, sk, o + 2, db1)
            if i > 0:
                _deliver(grads, sk, o, sw.wgrad(x_in, dy1, out=sk[o]))
                below = sv["acts"][i - 1]          # (x, y1, s1, y2, s2, ...) of the block whose pooled output x_in is
                if pool_sums_fusable(dy1, wd1, below[3], *CNN8_POOLS[i - 1]):
                    # (direct halo-tile kernel or, for the deep layers, the Winograd form: both carry the sums in their epilogue)
                    dx, poolpart = conv3x3_dgrad_poolsums(dy1, wd1, below[3], below[4], *CNN8_POOLS[i - 1], drop[0], seeds[i - 1])
                elif _wino_u(wd1, dy1, x_in.shape[3], count=False) is not None:
                    dx = conv3x3(dy1, wd1, x_in.shape[3], training_launch=True)
                else:
                    dx = conv3x3(dy1, wd1, x_in.shape[3])
                sw.release()
            else:
                _cnn8_stem_backward(sv, dy1, grads, sk, bn_bwd=None if applied else (y1, s1, g1, dg1, db1))
            del dy1
            sv["acts"][i] = None
            _cnn8_block_done(sw, prm, i)
        sw.join()
        return (None, None, *grads)


def _check_fp32_only(model):
    if cfg.CONV_MATH != "fp32" or act_bf16() or gemm_bf16():
        raise RuntimeError(f"{model} supports fp32 arithmetic only (CONV_MATH 'fp32', fp32 activations and GEMMs); got "
                           f"CONV_MATH {cfg.CONV_MATH!r}, ACT_DTYPE {cfg.ACT_DTYPE!r}, GEMM_MATH {cfg.GEMM_MATH!r}")


def check_cross_precision():
    """CrossCnn8_Rnn runs in fp32 only: its per-clip bias passes have no bf16 or split-fp32 (x3) form."""
    _check_fp32_only("CrossCnn8_Rnn")


def _text_block_forward(y1, part1, prm, bns, train, t, ph, pw, pool=0, drop_p=0.0, seed=0, want_dgrad=True):
    """A ConvTextBlock behind its first convolution (raw output y1 with the statistics partials the conv wrote):
    pool(relu(bn2(conv2(relu(bn1(y1) + t))) + t)) [with dropout] -> (out, (s1, a1, y2, s2, wd2)).  prm = (conv1.w, bn1.w, bn1.b,
    conv2.w, bn2.w, bn2.b), bns = (bn1, bn2) (their running statistics are updated where ``train`` says so)."""
    _, g1, b1, c2w, g2, b2 = prm
    (bn1, bn2), (train1, train2) = bns, train
    C = y1.shape[3]
    s1 = bn_stats(y1.view(-1, C), g1, b1, bn1.running_mean, bn1.running_var, train1, bn1.eps, bn1.momentum, partials=part1)
    a1 = bias_bnrelu_forward(y1, s1, t)                              # relu(bn1(conv1(x)) + t), written out
    wf2, wd2 = pack_conv_weight(c2w, want_dgrad=want_dgrad, W=a1.shape[2])
    y2, part2 = conv3x3_stats(a1, wf2, C, want_stats=train2)
    s2 = bn_stats(y2.view(-1, C), g2, b2, bn2.running_mean, bn2.running_var, train2, bn2.eps, bn2.momentum, partials=part2)
    return bias_bnrelu_pool(y2, s2, t, ph, pw, pool=pool, drop_p=drop_p, seed=seed), (s1, a1, y2, s2, wd2)


class CrossCnn8RnnFunction(TagFunction):
    """The early-fusion CrossCnn8_Rnn (models/audio_text_model.py:677-840) below its text encoder, as one autograd node:
    waveform (B,S) -> frame_sim (B, T', 1).  t1..t4 = conv_block{i}.fc_text(e) (B, C_i), u = fc1_text(e), r = rnn_text(e)
    (B, 512): differentiable inputs, so autograd sums their six gradients into the text embedding.

    params order: bn0.w, bn0.b, 4 x (conv1.w, bn1.w, bn1.b, conv2.w, bn2.w, bn2.b), fc1.w, fc1.b, rnn (w_ih, w_hh, b_ih, b_hh)
    x (fwd, reverse), fc_output.w, fc_output.b.  The stem, the tail and the conv / BatchNorm-statistics / GRU / GEMM launches
    are Cnn8RnnFunction's; the text bias enters through the per-clip bias passes (dispatch.bias_*), so the conv kernels' fused
    BatchNorm epilogues (which assume a per-channel shift) are not used.  ``ctx.augment``: (stripes, n_time, None) as in
    Cnn8RnnFunction."""

    @staticmethod
    def forward(ctx, waveform, mod, t1, t2, t3, t4, u, r, *params):
        check_cross_precision()
        wave, p, bn_train, drop, seeds = _cnn8_begin(waveform, mod, params)
        texts = [_chk(t.detach(), "text bias") for t in (t1, t2, t3, t4)]
        u_, r_ = _chk(u.detach(), "fc1_text"), _chk(r.detach(), "rnn_text")
        need_grad = any(ctx.needs_input_grad[2:])
        aug = getattr(ctx, "augment", None)
        B = wave.shape[0]
        for i, t in enumerate(texts + [u_, r_]):
            if t.dim() != 2 or t.shape[0] != B:
                raise RuntimeError(f"CrossCnn8_Rnn: text bias {i} has shape {tuple(t.shape)}, expected ({B}, channels)")
        for i, t in enumerate(texts):
            if t.shape[1] != p[2 + 6 * i].shape[0]:
                raise RuntimeError(f"CrossCnn8_Rnn: conv_block{i + 1} text bias has {t.shape[1]} channels, expected "
                                   f"{p[2 + 6 * i].shape[0]}")
        lm, st0, x0, y1, part1 = _cnn8_stem_forward(wave, mod, p, bn_train, aug)
        x = wd1 = None
        acts = []
        for i in range(4):
            prm = p[2 + 6 * i: 8 + 6 * i]
            blk = getattr(mod, f"conv_block{i + 1}")
            if i > 0:
                wf1, wd1 = pack_conv_weight(prm[0], want_dgrad=need_grad, W=x.shape[2])
                y1, part1 = conv3x3_stats(x, wf1, prm[0].shape[0], want_stats=bn_train)
            xo, (s1, a1, y2, s2, wd2) = _text_block_forward(y1, part1, prm, (blk.bn1, blk.bn2), (bn_train, bn_train), texts[i],
                                                            *CNN8_POOLS[i], drop_p=drop[0], seed=seeds[i], want_dgrad=need_grad)
            if need_grad:
                acts.append((x, y1, s1, a1, y2, s2, wd1, wd2))
            del a1
            x = xo
        Bx, Tp = x.shape[0], x.shape[1]
        xm, fc = _cnn8_tail_forward(x, p[26], p[27], drop[1], seeds[4], act=0)
        h = rowgroup_bias_relu(fc, u_, Tp, out=fc)                       # relu(fc1(x) + fc1_text(e)), in place
        y, gsave = gru_bidir_forward(h, p[28:36], Bx, Tp, need_grad)
        y2d = y.reshape(Bx * Tp, -1)
        prob, sig = frame_head_forward(y2d, r_, p[36].reshape(-1), p[37], Tp)
        if need_grad:
            ctx.saved = dict(lm=lm, st0=st0, aug=aug, x0=x0, acts=acts, x_last=x, xm=xm, h=h, gsave=gsave, y=y2d, sig=sig,
                             texts=texts, u=u_, r=r_, p=p, drop=drop, seeds=seeds, sinks=_sinks(params),
                             params=params if cfg.DIRECT_GRADS else None)
        mod._last_dropout = dict(p=drop, seeds=seeds)
        return prob.view(Bx, Tp, 1)

    @staticmethod
    def backward(ctx, dprob):
        sv = ctx.saved
        ctx.saved = None
        p = sv["p"]
        drop, seeds = sv["drop"], sv["seeds"]
        dprob = _chk(dprob, "grad_output")
        grads: List[Optional[torch.Tensor]] = [None] * len(p)
        sk, prm = sv["sinks"], sv["params"]
        y, h = sv["y"], sv["h"]
        M = y.shape[0]
        Tp = sv["x_last"].shape[1]
        wo = p[36]
        dyh, dwo, dbo, dr = frame_head_backward(y, sv["r"], wo.reshape(-1), sv["sig"], dprob.reshape(-1), Tp)
        _deliver(grads, sk, 36, dwo.view_as(wo))
        _deliver(grads, sk, 37, dbo)
        sw = _SideWgrad(dprob.device)
        dh, ggru = gru_bidir_backward(dyh.view(M // Tp, Tp, -1), h, sv["gsave"], outs=sk[28:36],
                                      side=sw if cfg.SIDE_PARAM_GRADS >= 1 else None)
        for k in range(8):
            _deliver(grads, sk, 28 + k, ggru[k])
        dfc = relu_backward(h, dh)
        du, dfc_b = rowgroup_colsum(dfc, Tp, dtotal=sk[27])
        _deliver(grads, sk, 27, dfc_b)
        xm = sv["xm"]
        fc_w = p[26]
        _deliver(grads, sk, 26, gemm(dfc, xm, fc_w.shape[0], fc_w.shape[1], M, transA=True, lda=fc_w.shape[0], out=sk[26]))
        if prm is not None:
            _ready(list(prm[26:38]))
            _flush()
        dtexts = [None] * 4
        du = du if ctx.needs_input_grad[6] else None
        dr = dr if ctx.needs_input_grad[7] else None
        if not any(ctx.needs_input_grad[2:6]) and not any(ctx.needs_input_grad[8:34]):
            # freeze_cnn (models/audio_text_model.py:703-707): nothing below the GRU takes a gradient, the text encoder
            # included -- the conv stack's backward is not run
            sw.join()
            return (None, None, *dtexts, du, dr, *grads)
        dx = _cnn8_tail_backward(dfc, fc_w, sv["x_last"], drop[1], seeds[4])
        texts = sv["texts"]
        for i in range(3, -1, -1):
            x_in, y1, s1, a1, y2, s2, wd1, wd2 = sv["acts"][i]
            g1, g2 = p[3 + 6 * i], p[6 + 6 * i]
            o = 2 + 6 * i
            ph, pw = CNN8_POOLS[i]
            t = texts[i]
            dy2, dg2, db2, clip2 = bias_bnrelu_pool_backward(y2, s2, g2, t, dx, ph, pw, pool=0, drop_p=drop[0], seed=seeds[i],
                                                             dg_out=sk[o + 4], db_out=sk[o + 5])
            _deliver(grads, sk, o + 4, dg2)
            _deliver(grads, sk, o + 5, db2)
            del dx
            _deliver(grads, sk, o + 3, sw.wgrad(a1, dy2, out=sk[o + 3]))
            da1 = conv3x3(dy2, wd2, y1.shape[3])                       # plain conv2 dgrad
            sw.release()
            del dy2
            dy1, dg1, db1, dtexts[i] = bias_bnrelu_backward(y1, s1, g1, t, da1, prev=clip2, dg_out=sk[o + 1], db_out=sk[o + 2])
            del da1, clip2
            _deliver(grads, sk, o + 1, dg1)
            _deliver(grads, sk, o + 2, db1)
            if i > 0:
                _deliver(grads, sk, o, sw.wgrad(x_in, dy1, out=sk[o]))
                dx = conv3x3(dy1, wd1, x_in.shape[3])
                sw.release()
            else:
                _cnn8_stem_backward(sv, dy1, grads, sk)
            del dy1
            sv["acts"][i] = None
            _cnn8_block_done(sw, prm, i)
        sw.join()
        return (None, None, *dtexts, du, dr, *grads)


class ConvTextBlockFunction(TagFunction):
    """ConvTextBlock.forward on its own (models/audio_text_model.py:614-636): channels-last x (B,H,W,Cin), t = fc_text(text)
    (B, C) -> dropout-free pool(relu(bn2(conv2(relu(bn1(conv1(x)) + t))) + t)) (B, H/ph, W/pw, C); the forward passes are
    CrossCnn8RnnFunction's (_text_block_forward).  ``bns`` = (bn1, bn2): their running statistics are updated in train mode."""

    @staticmethod
    def forward(ctx, x, t, bns, ph, pw, pool, c1w, g1, b1, c2w, g2, b2):
        check_cross_precision()
        x, t_ = _chk(x, "x"), _chk(t.detach(), "text bias")
        prm = [_chk(v.detach(), "parameter") for v in (c1w, g1, b1, c2w, g2, b2)]
        c1w = prm[0]
        train = (bns[0].training, bns[1].training)
        B, H, W, Cin = x.shape
        C = c1w.shape[0]
        if t_.shape != (B, C):
            raise RuntimeError(f"ConvTextBlock: text bias of shape {tuple(t_.shape)}, expected {(B, C)}")
        if Cin == 1:
            y1, part1 = conv3x3_c1_stats(x.view(B, H, W), c1w, want_stats=train[0])
            wd1 = None
        elif Cin % 32 == 0:
            wf1, wd1 = pack_conv_weight(c1w, want_dgrad=True, W=W)
            y1, part1 = conv3x3_stats(x, wf1, C, want_stats=train[0])
        else:
            raise RuntimeError(f"ConvTextBlock: in_channels must be 1 or a multiple of 32, got {Cin}")
        out, (s1, a1, y2, s2, wd2) = _text_block_forward(y1, part1, prm, bns, train, t_, ph, pw, pool=pool)
        ctx.saved = (x, t_, y1, s1, a1, y2, s2, wd1, wd2, c1w, prm[1], prm[4], ph, pw, pool)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, t_, y1, s1, a1, y2, s2, wd1, wd2, c1w, g1, g2, ph, pw, pool = ctx.saved
        ctx.saved = None
        B, H, W, Cin = x.shape
        C = y1.shape[3]
        dy2, dg2, db2, clip2 = bias_bnrelu_pool_backward(y2, s2, g2, t_, _chk(dout, "grad"), ph, pw, pool=pool)
        dc2 = conv3x3_wgrad(a1, dy2)
        da1 = conv3x3(dy2, wd2, C)
        dy1, dg1, db1, dt = bias_bnrelu_backward(y1, s1, g1, t_, da1, prev=clip2)
        if Cin == 1:
            dc1 = conv3x3_c1_wgrad(x.view(B, H, W), dy1)
            dx = conv3x3_c1_dgrad(dy1, c1w).view(B, H, W, 1)
        else:
            dc1 = conv3x3_wgrad(x, dy1)
            dx = conv3x3(dy1, wd1, Cin)
        return dx, dt, None, None, None, None, dc1, dg1, db1, dc2, dg2, db2


class SpecAugmentFunction(TagFunction):
    """models.augmentation.SpecAugmentation.forward on a (B, C, T, F) tensor: the stripes of clip b zero frames / mel bins of every
    channel of that clip (torchlibrosa augmentation.py DropStripes); the gradient is the incoming one with the same zeros."""

    @staticmethod
    def forward(ctx, x, stripes, n_time):
        x = _chk(x, "input")
        B, C, T, Fq = x.shape
        st = stripes.repeat_interleave(C, 0) if C > 1 else stripes          # one table row block per (clip, channel) image
        ctx.stripes, ctx.n_time = st, n_time
        return augment_forward(x.view(B * C, T, Fq), None, None, st, n_time).view(B, C, T, Fq)

    @staticmethod
    def backward(ctx, dy):
        B, C, T, Fq = dy.shape
        dx = augment_backward(_chk(dy, "grad").view(B * C, T, Fq), B * C, ctx.stripes, ctx.n_time)
        return dx.view(B, C, T, Fq), None, None


# ------------------------------------------------------------------------------------------------
# CrnnEncoder (row A1') and the early-fusion CrossCDur: cdur_block = BN -> conv3x3 -> LeakyReLU(0.1), LPPool2d(4),
# Dropout(0.3), BiGRU(128) -- one forward body and one backward body, without and with the per-clip text biases
# ------------------------------------------------------------------------------------------------
#: the five-block plan: the LPPool2d(4) window behind block i (dropout behind the last), or None -- the next block then reads
#: the raw conv output.  A block behind a pool takes its BatchNorm statistics over its input as it is (pre_op 0) and folds the
#: BatchNorm into its conv's operand load as prologue 3; a block behind a conv takes them over leaky(input) (pre_op 1) and folds
#: LeakyReLU + BatchNorm as prologue 2.  Block 0 is the Cin = 1 conv behind the scalar BatchNorm2d(1).  Block i's parameters
#: are p[3 * i: 3 * i + 3] = (bn.w, bn.b, conv.w); its channel count is its conv weight's.
CDUR_POOLS = [(2, 4), None, (2, 4), None, (1, 4)]
CRNN_POOLS = [w for w in CDUR_POOLS if w is not None]


def check_cross_cdur_precision():
    """CrossCDur runs in fp32 only: the biased conv epilogues exist for the fp32 direct kernels alone."""
    _check_fp32_only("CrossCDur")


def _cdur_conv(x, w, cout, prologue, scale, shift, t):
    """The kernel that writes a block's output z = conv(bn(x)) [+ t[b, c]].  x (B,H,W): the Cin = 1 conv (w its weight, scale /
    shift per column); else w is the forward pack.  Without t, conv3x3 dispatches on CONV_MATH as everywhere."""
    if x.dim() == 3:
        return conv3x3_c1(x, w, scale, shift) if t is None else conv3x3_c1_bias(x, w, scale, shift, t)
    if t is None:
        return conv3x3(x, w, cout, prologue=prologue, scale=scale, shift=shift)
    return conv3x3_bias(x, w, cout, prologue, scale, shift, t)


def _cdur_pool_backward(z, g, pool, drop_p, seed, want_dt):
    """(dz, dt) of a block's raw output z from g, the gradient of its pooled output; dt = the per-clip sums of dz from the same
    pass when wanted (the *_clip kernel), else None."""
    if want_dt:
        return lppool_leaky_backward_clip(z, g, *pool, drop_p, seed)
    return lppool_leaky_backward(z, g, *pool, drop_p, seed), None


def _cdur_bn_backward(z, st, gamma, g, dg_out, db_out, want_dt):
    """(dz, dgamma, dbeta, dt) of a raw output z that feeds the next block's BatchNorm (st, gamma) through LeakyReLU; g is the
    gradient of that BatchNorm's output, dt as in _cdur_pool_backward."""
    if want_dt:
        return bn_act_backward_clip(z, 1, st, gamma, g, dg_out=dg_out, db_out=db_out)
    return (*bn_act_backward(z, 1, st, gamma, g, dg_out=dg_out, db_out=db_out), None)


def _scalar_bn_backward(x2d, dz, w, st):
    """(dgamma, dbeta), each (1,), of a BatchNorm2d(1) in front of a Cin = 1 conv: x2d (rows, W) its input, dz the gradient of
    the conv's output."""
    rows, W = x2d.shape
    du0 = conv3x3_c1_dgrad(dz, w)                                              # (B,H,W) grad wrt the BatchNorm output
    stc = BNStat()
    stc.mean, stc.invstd = st.mean.expand(W).contiguous(), st.invstd.expand(W).contiguous()
    dgc, dbc = bn_param_grad(x2d, du0.view(rows, W), stc)
    return dgc.sum().view(1), dbc.sum().view(1)                                # W columns share one channel


def _cdur_forward(ctx, waveform, mod, params, texts=None, r=None):
    """CrnnFunction.forward (texts None) / CrossCDurFunction.forward (texts: t1..t5, r the frame head's text term).
    Layer plan (channels-last): lm -> [bn0 scalar | conv 1->32] -> LP(2,4) -> [bn | conv 32->128] -> [leaky,bn | conv]
    -> LP(2,4) -> [bn | conv] -> [leaky,bn | conv] -> LP(1,4)+dropout -> GRU [-> frame head]: CDUR_POOLS."""
    wave = _chk(waveform, "waveform")
    check_pass_size(wave.shape[0], wave.shape[1] // mod.hop_length + 1)
    training = mod.training
    p = [_chk(t.detach(), "parameter") for t in params]
    rnn = p[15:23]
    if texts is not None:
        texts = [_chk(t.detach(), "text bias") for t in texts]
        r = _chk(r.detach(), "fc_text")
    bns = mod._bn_modules()
    drop = mod.dropout_p if training else 0.0
    seed = new_seed() if training and drop > 0 else 0
    drops = [(0.0, 0)] * (len(CDUR_POOLS) - 1) + [(drop, seed)]   # (probability, seed) behind block i's pool: the last one only

    lm = logmel(wave, mod.n_fft, mod.win_length, mod.hop_length, mod.window, mod.mel_fb)   # (B,F,64)
    B, Fr, NM = lm.shape
    if texts is not None:
        for i, t in enumerate(texts + [r]):
            C = 2 * rnn[1].shape[1] if i == 5 else p[3 * i + 2].shape[0]
            if t.dim() != 2 or t.shape[0] != B or t.shape[1] != C:
                raise RuntimeError(f"CrossCDur: text bias {i + 1} has shape {tuple(t.shape)}, expected ({B}, {C})")
    x, after_pool = lm, True
    st, xs, zs, wd = [], [], [], []
    for i, pool in enumerate(CDUR_POOLS):
        g, b, cw = p[3 * i: 3 * i + 3]
        bn = bns[i]
        s = bn_stats(x.view(-1, 1 if i == 0 else x.shape[3]), g, b, bn.running_mean, bn.running_var, training, bn.eps,
                     bn.momentum, 0 if after_pool else 1)
        t = texts[i] if texts is not None else None
        if i == 0:                                                 # BatchNorm2d(1): one scalar affine, spread over the columns
            cs, ct = s.scale.expand(NM).contiguous(), s.shift.expand(NM).contiguous()
            z = _cdur_conv(lm, cw, cw.shape[0], 0, cs, ct, t)      # (B,F,64,32)
        else:
            wf, wdi = pack_conv_weight(cw, W=x.shape[2])
            wd.append(wdi)
            z = _cdur_conv(x, wf, cw.shape[0], 3 if after_pool else 2, s.scale, s.shift, t)
        st.append(s)
        xs.append(x)
        zs.append(z)
        after_pool = pool is not None
        if after_pool:                                             # leaky + LPPool; the dropout behind the last one
            x = bnact_pool(z, None, *pool, act=2, pool=1, drop_p=drops[i][0], seed=drops[i][1])
        else:
            x = z
    Bx, Tp = x.shape[0], x.shape[1]                                # x: (B,T',1,128)
    x2d = x.view(Bx * Tp, -1)
    need_grad = any(ctx.needs_input_grad[2:])
    y, gsave = gru_bidir_forward(x2d, rnn, Bx, Tp, need_grad)
    if texts is not None:
        y2d = y.reshape(Bx * Tp, -1)
        prob, sig = frame_head_forward(y2d, r, p[23].reshape(-1), p[24], Tp)
        y = prob.view(Bx, Tp)
    if need_grad:
        ctx.saved = dict(cs=cs, ct=ct, st=st, xs=xs, zs=zs, wd=wd, x2d=x2d, gsave=gsave, p=p, drops=drops,
                         sinks=_sinks(params), params=params if cfg.DIRECT_GRADS else None, n_texts=0)
        if texts is not None:
            ctx.saved.update(y=y2d, sig=sig, r=r, Tp=Tp, n_texts=len(texts) + 1)
    mod._last_dropout = dict(p=drop, seeds=[seed])
    return y


def _cdur_backward(ctx, dy):
    """CrnnFunction.backward / CrossCDurFunction.backward -> (None, None, [dt1..dt5, dr,] *parameter gradients).  A frozen
    parameter's gradient kernels are not launched (a conv weight: its weight-gradient conv; bn0: the Cin = 1 input gradient and
    the column reduction); dt_i = per-clip sums of dz_i, emitted by the pass that writes dz_i (dispatch.*_backward_clip; 2 % of
    the step faster than a rowgroup_colsum pass over each dz, docs/experiments_cross_cdur.md)."""
    sv = ctx.saved
    ctx.saved = None
    p, st, xs, zs, wd, nt = sv["p"], sv["st"], sv["xs"], sv["zs"], sv["wd"], sv["n_texts"]
    need = ctx.needs_input_grad
    need_t, need_p = (need[2:2 + nt] if nt else (False,) * 5), need[2 + nt:]
    grads: List[Optional[torch.Tensor]] = [None] * len(p)
    dts: List[Optional[torch.Tensor]] = [None] * 5
    # every gradient is written straight into its flat-gradient view when the parameter has one (sk[k]; None = returned to
    # autograd): the 23 per-parameter copies of the former form were 0.11 ms of a 5.3 ms step (tools/step_timeline.py)
    sk = sv["sinks"]
    dy = _chk(dy, "grad_output")
    dr = None
    if nt:
        y2d, Tp, wo = sv["y"], sv["Tp"], p[23]
        dy, dwo, dbo, dr = frame_head_backward(y2d, sv["r"], wo.reshape(-1), sv["sig"], dy.reshape(-1), Tp)
        grads[23], grads[24] = dwo.view_as(wo), dbo
        dy = dy.view(y2d.shape[0] // Tp, Tp, -1)
    dx2d, grads[15:23] = gru_bidir_backward(dy, sv["x2d"], sv["gsave"], outs=sk[15:23])
    g = dx2d.view(zs[4].shape[0], -1, 1, zs[4].shape[3])          # gradient of the last pooled output (B,T',1,128)
    du = None
    for i in range(4, -1, -1):
        k = 3 * i                                                  # parameters k, k + 1, k + 2: bn.w, bn.b, conv.w of block i
        x, z, pool = xs[i], zs[i], CDUR_POOLS[i]
        if pool is not None:
            dz, dts[i] = _cdur_pool_backward(z, g, pool, *sv["drops"][i], need_t[i])
        else:                                                      # g is already dz: the BatchNorm of block i + 1 gave it
            dz = g
        del g
        if i == 0:
            break
        after_pool = CDUR_POOLS[i - 1] is not None
        if need_p[k + 2]:                                          # a frozen conv weight: its weight-gradient conv is not launched
            grads[k + 2] = conv3x3_wgrad(x, dz, prologue=3 if after_pool else 2, scale=st[i].scale, shift=st[i].shift,
                                         out=sk[k + 2])
        du = conv3x3(dz, wd[i - 1], x.shape[3])
        del dz
        if after_pool:
            g, grads[k], grads[k + 1] = bn_act_backward(x, 0, st[i], p[k], du, dg_out=sk[k], db_out=sk[k + 1])
        else:                                                      # x is z_{i-1}: bn_i's backward gives dz_{i-1} (and dt_{i-1})
            g, grads[k], grads[k + 1], dts[i - 1] = _cdur_bn_backward(x, st[i], p[k], du, sk[k], sk[k + 1], need_t[i - 1])
    del du
    lm = xs[0]
    if need_p[2]:
        grads[2] = conv3x3_c1_wgrad(lm, dz, sv["cs"], sv["ct"], out=sk[2])
    if need_p[0] or need_p[1]:
        grads[0], grads[1] = _scalar_bn_backward(lm.view(-1, lm.shape[2]), dz, p[2], st[0])
    for k in range(len(grads)):
        if not need_p[k]:
            grads[k] = None
        elif grads[k] is not None:
            _deliver(grads, sk, k, grads[k])
    _ready(sv["params"])
    if nt:
        return (None, None, *dts, dr if need_t[5] else None, *grads)
    return (None, None, *grads)


class CrnnFunction(TagFunction):
    """params order: 5 x (bn.w, bn.b, conv.w) for cnn.{0,2,3,5,6}, then gru (w_ih, w_hh, b_ih, b_hh) x (fwd, reverse).
    The bodies are _cdur_forward / _cdur_backward without texts; conv3x3 dispatches on CONV_MATH (x3, bf16 GEMMs)."""

    @staticmethod
    def forward(ctx, waveform, mod, *params):
        return _cdur_forward(ctx, waveform, mod, params)

    @staticmethod
    def backward(ctx, dy):
        return _cdur_backward(ctx, dy)


class CrossCDurFunction(TagFunction):
    """The early-fusion CrossCDur (models/audio_text_model.py:482-568) below its text encoder, as one autograd node: waveform
    (B,S) -> frame_sim (B, T').  t1..t5 = block{i}.fc_text(e) (B, C_i), r = fc_text(e) (B, 256): differentiable inputs, so
    autograd sums their six gradients into the text embedding.

    params order: 5 x (bn.w, bn.b, conv.w) for block1..5, gru (w_ih, w_hh, b_ih, b_hh) x (fwd, reverse), fc_output.w,
    fc_output.b.  CrnnFunction's layer plan with z_i = conv_i(bn_i(.)) + t_i[b, c] written by the biased conv kernels
    (dispatch.conv3x3_c1_bias / conv3x3_bias) where CrnnFunction writes y_i: the forward has no extra pass over the activations.
    The statistics of bn_{i+1} are taken over leaky(z_i), bias included."""

    @staticmethod
    def forward(ctx, waveform, mod, t1, t2, t3, t4, t5, r, *params):
        check_cross_cdur_precision()
        return _cdur_forward(ctx, waveform, mod, params, (t1, t2, t3, t4, t5), r)

    @staticmethod
    def backward(ctx, dy):
        return _cdur_backward(ctx, dy)


def _clip_sums(dz):
    """dt[b, c] = sum over (h, w) of a channels-last gradient dz (B,H,W,C): the gradient of a per-clip bias added to z."""
    B, H, W, C = dz.shape
    return rowgroup_colsum(dz.view(B * H * W, C), H * W)[0]


class CDurTextBlockFunction(TagFunction):
    """CDurTextBlock.forward on its own (models/audio_text_model.py:473-479): channels-last x (B,H,W,Cin), t = fc_text(text)
    (B, Cout) -> leaky(conv(bn(x)) + t) (B,H,W,Cout); the launches of CrossCDurFunction's blocks plus a LeakyReLU pass.  ``bn``:
    its running statistics are updated in train mode.  Cin = 1: no gradient for x (BatchNorm2d(1)'s input gradient has no kernel;
    the block's input there is the spectrogram)."""

    @staticmethod
    def forward(ctx, x, t, bn, g, b, cw):
        check_cross_cdur_precision()
        x, t_ = _chk(x, "x"), _chk(t.detach(), "text bias")
        g, b, cw = (_chk(v.detach(), "parameter") for v in (g, b, cw))
        B, H, W, Cin = x.shape
        Cout = cw.shape[0]
        if Cin == 1 and ctx.needs_input_grad[0]:
            raise RuntimeError("CDurTextBlock: the input gradient of the Cin = 1 block has no kernel")
        st = bn_stats(x.view(-1, Cin), g, b, bn.running_mean, bn.running_var, bn.training, bn.eps, bn.momentum)
        if Cin == 1:
            cs, ct = st.scale.expand(W).contiguous(), st.shift.expand(W).contiguous()
            z = _cdur_conv(x.view(B, H, W), cw, Cout, 0, cs, ct, t_)
            wd = None
        else:
            cs = ct = None
            wf, wd = pack_conv_weight(cw, W=W)
            z = _cdur_conv(x, wf, Cout, 3, st.scale, st.shift, t_)
        ctx.saved = (x, z, st, cs, ct, wd, g, cw)
        return leaky_forward(z)

    @staticmethod
    def backward(ctx, dout):
        x, z, st, cs, ct, wd, g, cw = ctx.saved
        ctx.saved = None
        B, H, W, Cin = x.shape
        dz = leaky_backward(z, _chk(dout, "grad"))
        dt = _clip_sums(dz)
        if Cin == 1:
            dcw = conv3x3_c1_wgrad(x.view(B, H, W), dz, cs, ct)
            dg, db = _scalar_bn_backward(x.view(B * H, W), dz, cw, st)
            return None, dt, None, dg, db, dcw
        dcw = conv3x3_wgrad(x, dz, prologue=3, scale=st.scale, shift=st.shift)
        du = conv3x3(dz, wd, Cin)
        dx, dg, db = bn_act_backward(x, 0, st, g, du)
        return dx, dt, None, dg, db, dcw


# ------------------------------------------------------------------------------------------------
# small heads
# ------------------------------------------------------------------------------------------------

class LinearFunction(TagFunction):
    """nn.Linear on the MFMA GEMM (audio_proj / text_proj, models/audio_text_model.py:45-46,78-87)."""

    @staticmethod
    def forward(ctx, x, w, b):
        x2 = _chk(x, "x").view(-1, x.shape[-1])
        w_, b_ = _chk(w.detach(), "weight"), (_chk(b.detach(), "bias") if b is not None else None)
        M, K = x2.shape
        N = w_.shape[0]
        y = gemm(x2, w_, M, N, K, transB=True, bias=b_)
        ctx.save_for_backward(x2, w_)
        ctx.has_bias = b is not None
        ctx.xshape = x.shape
        ctx.sinks = _sinks([x, w, b])
        ctx.params = [w, b] if cfg.DIRECT_GRADS else None
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        M, K = x2.shape
        N = w.shape[0]
        dy2 = _chk(dy, "grad").view(M, N)
        dx = gemm(dy2, w, M, K, N).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        sk = ctx.sinks
        g = [dx, None, None]
        _deliver(g, sk, 1, gemm(dy2, x2, N, K, M, transA=True, lda=N, out=sk[1]))
        if ctx.has_bias:
            _deliver(g, sk, 2, colsum(dy2, M, N, out=sk[2]))
        _ready(ctx.params)
        return tuple(g)


# Each head's forward / backward arithmetic lives in ONE plain function below.  texttoaudiogrounding_amd/torch_ops.py
# registers them as PyTorch operators (torch.ops.tag.embed_mean / frame_match / align_dot / frame_bce + *_backward, with
# autograd formulas) and the reference-shaped modules (models/match.py, models/align.py, losses.py, models/text_encoder.py)
# call THOSE operators; the only autograd.Function kept here is EmbedMeanFunction, the direct-gradient variant that scatters
# straight into the flat-gradient rows of the table (an operator may not mutate hidden state).

class EmbedMeanFunction(TagFunction):
    """embed_mean with direct gradients (StrongRunner): the table gradient is scattered straight into the (zeroed)
    flat-gradient rows; same kernels as torch.ops.tag.embed_mean."""

    @staticmethod
    def forward(ctx, table, text, text_len, want_tokens):
        seq, tok = embed_mean_forward(table.detach(), text, text_len, want_tokens)
        ctx.save_for_backward(text, text_len)
        ctx.vd = tuple(table.shape)
        ctx.sinks = _sinks([table])
        ctx.table = table
        ctx.set_materialize_grads(False)
        return seq, tok

    @staticmethod
    def backward(ctx, dseq, dtok):
        text, text_len = ctx.saved_tensors
        sink = ctx.sinks[0]
        direct = sink is not None
        dtab = sink if direct else torch.zeros(*ctx.vd, device=text.device, dtype=F32)
        embed_mean_backward_into(dtab, dseq, dtok, text, text_len)
        if direct:
            _ready([ctx.table])
            return None, None, None, None
        return dtab, None, None, None


class TextGruFunction(TagFunction):
    """torch.ops.tag.text_gru with direct gradients (StrongRunner): the recurrence of RnnEncoder (models/text_encoder.py:119-123)
    whose parameter gradients go straight into their flat-gradient views; a parameter with requires_grad = False
    (freeze_text_encoder) costs no GEMM and its flat-gradient rows are not touched.  Same kernels as the operator."""

    @staticmethod
    def forward(ctx, x, text_len, dirs, layers, drop_p, seed, *params):
        need = engine._RECORDING and any(ctx.needs_input_grad)
        tok, seq, saved = text_gru_forward(x, text_len, [p.detach() for p in params], dirs, layers, need, drop_p, seed)
        ctx.tg = (saved, text_len, dirs, drop_p, seed)
        ctx.sinks = _sinks(list(params))
        ctx.params = list(params) if cfg.DIRECT_GRADS else None
        ctx.set_materialize_grads(False)
        return tok, seq

    @staticmethod
    def backward(ctx, dtok, dseq):
        saved, text_len, dirs, drop_p, seed = ctx.tg
        sk, need = ctx.sinks, list(ctx.needs_input_grad[6:])
        n = len(need)
        if (dtok is None and dseq is None) or saved is None:
            return (None,) * (6 + n)
        dx, g = text_gru_backward(dtok, dseq, text_len, saved, dirs, drop_p, seed, outs=[sk[i] for i in range(n)], need=need,
                                  need_dx=ctx.needs_input_grad[0])
        grads = [None] * n
        for i in range(n):
            if need[i]:
                _deliver(grads, sk, i, g[i])
        _ready(ctx.params)
        return (dx, None, None, None, None, None, *grads)


class TextSelfAttnFunction(TagFunction):
    """torch.ops.tag.text_selfattn with direct gradients (StrongRunner): SelfAttention behind its embedding
    (models/text_encoder.py:263-268) whose parameter gradients (cls_token, in_proj, out_proj) go straight into their
    flat-gradient views; a parameter with requires_grad = False costs no GEMM / column sum and its flat-gradient rows are not
    touched.  Same kernels as the operator."""

    @staticmethod
    def forward(ctx, tok, text_len, pe, heads, drop_p, seed, *params):
        need = engine._RECORDING and any(ctx.needs_input_grad)
        cls, w_in, b_in, w_out, b_out = [p.detach() for p in params]
        out, saved = text_selfattn_forward(tok, text_len, pe, cls, w_in, b_in, w_out, b_out, heads, need, drop_p, seed)
        ctx.sa = (saved, heads, drop_p, seed)
        ctx.shapes = [tuple(p.shape) for p in params]
        ctx.sinks = _sinks(list(params))
        ctx.params = list(params) if cfg.DIRECT_GRADS else None
        return out

    @staticmethod
    def backward(ctx, dout):
        saved, heads, drop_p, seed = ctx.sa
        sk, need = ctx.sinks, list(ctx.needs_input_grad[6:])
        if saved is None:
            return (None,) * 11
        dtok, g = text_selfattn_backward(dout, saved, heads, drop_p, seed, outs=[sk[i] for i in range(5)], need=need,
                                         need_dtok=ctx.needs_input_grad[0])
        grads = [None] * 5
        for i in range(5):
            if need[i]:
                _deliver(grads, sk, i, g[i] if sk[i] is not None else g[i].view(ctx.shapes[i]))
        _ready(ctx.params)
        return (dtok, None, None, None, None, None, *grads)


class TextIntraFunction(TagFunction):
    """torch.ops.tag.text_intra with direct gradients (StrongRunner): IntraAttention behind its embedding
    (models/text_encoder.py:213-237) whose gate gradients, accumulated over the layers that share the cell, go straight into
    their flat-gradient views; a parameter with requires_grad = False costs no GEMM / column sum and its flat-gradient rows
    are not touched.  Same kernels as the operator."""

    @staticmethod
    def forward(ctx, x, text_len, pe, layers, drop_p, seed, *params):
        need = engine._RECORDING and any(ctx.needs_input_grad)
        tok, seq, saved = text_intra_forward(x, text_len, pe, *[p.detach() for p in params], layers, need, drop_p, seed)
        ctx.ti = (saved, text_len, pe, drop_p, seed)
        ctx.weights = [params[i].detach() for i in (0, 2, 4)]
        ctx.sinks = _sinks(list(params))
        ctx.params = list(params) if cfg.DIRECT_GRADS else None
        ctx.set_materialize_grads(False)
        return tok, seq

    @staticmethod
    def backward(ctx, dtok, dseq):
        saved, text_len, pe, drop_p, seed = ctx.ti
        sk, need = ctx.sinks, list(ctx.needs_input_grad[6:])
        if (dtok is None and dseq is None) or saved is None:
            return (None,) * 12
        dx, g = text_intra_backward(dtok, dseq, text_len, pe, saved, *ctx.weights, drop_p, seed, outs=[sk[i] for i in range(6)],
                                    need=need, need_dx=ctx.needs_input_grad[0])
        grads = [None] * 6
        for i in range(6):
            if need[i]:
                _deliver(grads, sk, i, g[i])
        _ready(ctx.params)
        return (dx, None, None, None, None, None, *grads)


class TextClapFunction(TagFunction):
    """torch.ops.tag.text_clap with direct gradients (StrongRunner / WeakPhraseRunner): LaionClapEncoder
    (models/text_encoder.py:311-327) whose parameter gradients go straight into their flat-gradient views -- the two embedding
    tables' rows are accumulated into the zeroed flat buffer, like EmbedMeanFunction's; a parameter with requires_grad = False
    costs no GEMM / column sum, its flat-gradient rows are not touched and the walk stops below the lowest trainable parameter.
    With nothing to differentiate (a frozen tower, eval, no_grad) nothing is saved.  Same kernels as the operator."""

    N_ARGS = 8                                          # arguments in front of the parameters

    @staticmethod
    def forward(ctx, input_ids, attention_mask, heads, eps, pad_id, p_hidden, p_attn, seed, *params):
        need = engine._RECORDING and any(ctx.needs_input_grad)
        tok, seq, saved = text_clap_forward(input_ids, attention_mask, [p.detach() for p in params], heads, eps, pad_id, need,
                                            p_hidden, p_attn, seed)
        ctx.tc = (saved, input_ids, heads, pad_id, p_hidden, p_attn, seed)
        ctx.weights = [p.detach() for p in params] if need else None
        ctx.shapes = [tuple(p.shape) for p in params]
        ctx.sinks = _sinks(list(params))
        ctx.params = list(params) if cfg.DIRECT_GRADS else None
        ctx.set_materialize_grads(False)
        return tok, seq

    @staticmethod
    def backward(ctx, dtok, dseq):
        saved, input_ids, heads, pad_id, p_hidden, p_attn, seed = ctx.tc
        k = TextClapFunction.N_ARGS
        sk, need = ctx.sinks, list(ctx.needs_input_grad[k:])
        n = len(need)
        if (dtok is None and dseq is None) or saved is None:
            return (None,) * (k + n)
        g = text_clap_backward(dtok, dseq, input_ids, saved, ctx.weights, heads, pad_id, p_hidden, p_attn, seed,
                               outs=[sk[i] for i in range(n)], need=need)
        grads = [None] * n
        for i in range(n):
            if need[i]:
                _deliver(grads, sk, i, g[i] if sk[i] is not None else g[i].view(ctx.shapes[i]))
        _ready(ctx.params)
        return (*([None] * k), *grads)


class TextBertFunction(TagFunction):
    """torch.ops.tag.text_bert with direct gradients (StrongRunner / WeakPhraseRunner): Bert / SentenceBert
    (models/text_encoder.py:271-308) whose parameter gradients go straight into their flat-gradient views -- the embedding tables'
    rows into the zeroed flat buffer, like TextClapFunction's; a parameter with requires_grad = False costs no GEMM / column sum
    and the walk stops below the lowest trainable parameter.  The pooler's two parameters (when passed) receive no gradient and
    their flat-gradient rows are not touched.  Same kernels as the operator."""

    N_ARGS = 11                                         # arguments in front of the parameters

    @staticmethod
    def forward(ctx, input_ids, token_type_ids, attention_mask, heads, eps, pad_id, pool_mode, norm, p_hidden, p_attn, seed, *params):
        need = engine._RECORDING and any(ctx.needs_input_grad)
        tok, seq, saved = text_bert_forward(input_ids, token_type_ids, attention_mask, [p.detach() for p in params], heads, eps,
                                            pad_id, pool_mode, norm, need, p_hidden, p_attn, seed)
        ctx.tb = (saved, input_ids, token_type_ids, heads, pad_id, pool_mode, norm, p_hidden, p_attn, seed)
        ctx.weights = [p.detach() for p in params] if need else None
        ctx.shapes = [tuple(p.shape) for p in params]
        ctx.sinks = _sinks(list(params))
        ctx.params = list(params) if cfg.DIRECT_GRADS else None
        ctx.set_materialize_grads(False)
        return tok, seq

    @staticmethod
    def backward(ctx, dtok, dseq):
        saved, input_ids, type_ids, heads, pad_id, pool_mode, norm, p_hidden, p_attn, seed = ctx.tb
        k = TextBertFunction.N_ARGS
        sk, need = ctx.sinks, list(ctx.needs_input_grad[k:])
        n = len(need)
        if (dtok is None and dseq is None) or saved is None:
            return (None,) * (k + n)
        g = text_bert_backward(dtok, dseq, input_ids, type_ids, saved, ctx.weights, heads, pad_id, pool_mode, norm, p_hidden, p_attn,
                               seed, outs=[sk[i] for i in range(n)], need=need)
        grads = [None] * n
        for i in range(n):
            if need[i] and g[i] is not None:
                _deliver(grads, sk, i, g[i] if sk[i] is not None else g[i].view(ctx.shapes[i]))
        _ready(ctx.params)
        return (*([None] * k), *grads)


class Seq2SeqAttentionFunction(TagFunction):
    """Seq2SeqAttention.forward (models/cross_encoder.py:11-42): additive attention of every query row over the key/value
    rows, ``score[b,q,k] = v . tanh(W [query_q ; kv_k] + b)``, the two -1e10 mask fills, softmax over k, ``out = attn @ kv``.
    The reference materialises the (B, Lq*Lk, Dq+Dkv) concatenation; here ``W = [Wq | Wk]`` is applied as two MFMA GEMMs and
    cross.hip does the rest.  query (B,Lq,Dq), kv (B,Lk,Dkv) -> (B,Lq,Dkv).  params: h2attn.weight (Da, Dq+Dkv),
    h2attn.bias (Da), v (Da)."""

    @staticmethod
    def forward(ctx, query, kv, query_len, kv_len, w_h, b_h, v):
        a, t = _chk(query, "query"), _chk(kv, "kv")
        B, T, D = a.shape
        L, Dk = t.shape[1], t.shape[2]
        Da = w_h.shape[0]
        ctx.sinks = _sinks([w_h, b_h, v])
        ctx.params = [w_h, b_h, v] if cfg.DIRECT_GRADS else None
        w_h, b_h, v = (_chk(x.detach(), "parameter") for x in (w_h, b_h, v))
        if w_h.shape[1] != D + Dk or b_h.shape != (Da,) or v.shape != (Da,):
            raise RuntimeError("Seq2SeqAttention: inconsistent dimensions")
        dev = a.device
        ql = torch.as_tensor(query_len).long().to(dev).contiguous()
        kl = torch.as_tensor(kv_len).long().to(dev).contiguous()
        aq = gemm(a, w_h, B * T, Da, D, transB=True, ldb=D + Dk)
        ak = gemm(t, w_h[:, D:], B * L, Da, Dk, transB=True, ldb=D + Dk, bias=b_h)
        attn = _empty(B, T, L, like=a)
        cx = _empty(B, T, Dk, like=a)
        call("tag_addattn_forward", ptr(aq), ptr(ak), ptr(v), ptr(t), ptr(ql), ptr(kl), ptr(attn), ptr(cx), B, T, L, Da, Dk)
        ctx.save_for_backward(a, t, aq, ak, attn, ql, kl, w_h, v)
        return cx

    @staticmethod
    def backward(ctx, dcx):
        a, t, aq, ak, attn, ql, kl, w_h, v = ctx.saved_tensors
        B, T, D = a.shape
        L, Dk = t.shape[1], t.shape[2]
        Da, M = w_h.shape[0], B * T
        dcx = _chk(dcx, "grad")
        daq, dak = _empty(B, T, Da, like=a), _empty(B, L, Da, like=a)
        dkv, dv = _empty(B, L, Dk, like=a), _empty(Da, like=a)
        ws = _ws(query("tag_addattn_backward_ws_bytes", B, T, L, Da, Dk), a)
        call("tag_addattn_backward", ptr(aq), ptr(ak), ptr(v), ptr(t), ptr(attn), ptr(dcx), ptr(ql), ptr(kl), ptr(daq),
             ptr(dak), ptr(dkv), ptr(dv), B, T, L, Da, Dk, ptr(ws))
        dw_h = _empty(Da, D + Dk, like=a)
        gemm(daq, a, Da, D, M, transA=True, lda=Da, out=dw_h, ldc=D + Dk)
        gemm(dak, t, Da, Dk, B * L, transA=True, lda=Da, out=dw_h[:, D:], ldc=D + Dk)
        db_h = colsum(dak, B * L, Da)
        da = gemm(daq, w_h, M, D, Da, ldb=D + Dk).view(B, T, D)
        gemm(dak, w_h[:, D:], B * L, Dk, Da, ldb=D + Dk, out=dkv, accumulate=True)
        g = [dw_h, db_h, dv]
        for k in range(3):
            _deliver(g, ctx.sinks, k, g[k])
        _ready(ctx.params)
        return (da, dkv, None, None, *g)


class CrossGatingFunction(TagFunction):
    """CrossGating.forward (models/cross_encoder.py:45-57): ``s_out = s * sigmoid(fc_u(u))``, ``u_out = u * sigmoid(fc_s(s))``
    -- two MFMA GEMMs with the sigmoid epilogue + tag_mul / tag_gate_backward.  u, s (..., D) -> (u_out, s_out)."""

    @staticmethod
    def forward(ctx, u, s, w_u, b_u, w_s, b_s):
        a, cx = _chk(u, "u"), _chk(s, "s")
        D = a.shape[-1]
        if cx.shape != a.shape or w_u.shape != (D, D) or w_s.shape != (D, D):
            raise RuntimeError("CrossGating: inconsistent dimensions")
        ctx.sinks = _sinks([w_u, b_u, w_s, b_s])
        ctx.params = [w_u, b_u, w_s, b_s] if cfg.DIRECT_GRADS else None
        w_u, b_u, w_s, b_s = (_chk(x.detach(), "parameter") for x in (w_u, b_u, w_s, b_s))
        M = a.numel() // D
        g_u = gemm(a, w_u, M, D, D, transB=True, bias=b_u, act=5)
        g_s = gemm(cx, w_s, M, D, D, transB=True, bias=b_s, act=5)
        u_out, s_out = torch.empty_like(a), torch.empty_like(cx)
        call("tag_mul", ptr(a), ptr(g_s), ptr(u_out), a.numel())
        call("tag_mul", ptr(cx), ptr(g_u), ptr(s_out), cx.numel())
        ctx.save_for_backward(a, cx, g_u, g_s, w_u, w_s)
        return u_out, s_out

    @staticmethod
    def backward(ctx, du_out, ds_out):
        a, cx, g_u, g_s, w_u, w_s = ctx.saved_tensors
        D = a.shape[-1]
        M = a.numel() // D
        du_out, ds_out = _chk(du_out, "grad"), _chk(ds_out, "grad")
        da, dz_s = torch.empty_like(a), torch.empty_like(a)
        call("tag_gate_backward", ptr(du_out), ptr(a), ptr(g_s), ptr(da), 0, ptr(dz_s), a.numel())       # u_out = u * g_s
        dcx, dz_u = torch.empty_like(cx), torch.empty_like(cx)
        call("tag_gate_backward", ptr(ds_out), ptr(cx), ptr(g_u), ptr(dcx), 0, ptr(dz_u), cx.numel())    # s_out = s * g_u
        dw_s = gemm(dz_s, cx, D, D, M, transA=True, lda=D)
        db_s = colsum(dz_s, M, D)
        gemm(dz_s, w_s, M, D, D, out=dcx, accumulate=True)
        dw_u = gemm(dz_u, a, D, D, M, transA=True, lda=D)
        db_u = colsum(dz_u, M, D)
        gemm(dz_u, w_u, M, D, D, out=da, accumulate=True)
        g = [dw_u, db_u, dw_s, db_s]
        for k in range(4):
            _deliver(g, ctx.sinks, k, g[k])
        _ready(ctx.params)
        return (da, dcx, *g)


def cross_pairs_served(L, D):
    """Whether csrc/cross_pairs.hip serves L tokens per phrase at width D (a host-side question: no launch, no device)."""
    return query("tag_crosspairs_ws_bytes", 1, 1, 1, int(L), int(D)) > 0


class CrossPairsFunction(TagFunction):
    """The tail of AudioTextCrossAlignByPhrase (models/audio_text_model.py:1033-1063 in the reference) as ONE node:
    CrossAttentionGating + match.DotProduct(text_level="token") of every clip against every phrase of the batch.
    a (B,T,D) with alen (B); w (P,L,D) with wlen (P); pnum (B) phrases per clip (host integers, sum P) ->
    sim_matrix (B,B,T,N), N = max(pnum), zero where n >= pnum[j].  The reference expands each clip to (P,T,D) and runs the
    cross-encoder on P*T rows, B times; here four GEMMs project the B*T frames and the P*L tokens once (fc_s is applied to the
    tokens: the attention weights sum to 1) and csrc/cross_pairs.hip does the rest per (clip, phrase, frame) row.
    params: h2attn.weight (D,2D), h2attn.bias, v, fc_u.weight, fc_u.bias, fc_s.weight, fc_s.bias."""

    @staticmethod
    def forward(ctx, a, alen, w, wlen, pnum, w_h, b_h, v, w_u, b_u, w_s, b_s, scale):
        a_, t_ = _chk(a, "audio_emb"), _chk(w, "token_emb")
        B, T, D = a_.shape
        P, L = t_.shape[0], t_.shape[1]
        params = [w_h, b_h, v, w_u, b_u, w_s, b_s]
        ctx.sinks = _sinks(params)
        ctx.params = params if cfg.DIRECT_GRADS else None
        w_h, b_h, v, w_u, b_u, w_s, b_s = (_chk(x.detach(), "parameter") for x in params)
        if (t_.shape[2] != D or w_h.shape != (D, 2 * D) or b_h.shape != (D,) or v.shape != (D,) or w_u.shape != (D, D)
                or w_s.shape != (D, D) or b_u.shape != (D,) or b_s.shape != (D,)):
            raise RuntimeError("CrossPairs: inconsistent dimensions")
        pn = torch.as_tensor(pnum).detach().to("cpu", torch.int64).contiguous()
        if pn.shape != (B,) or int(pn.sum()) != P or int(pn.min()) < 0:
            raise RuntimeError(f"CrossPairs: {pn.tolist()} phrases per clip for {B} clips and {P} phrases")
        N = int(pn.max())
        dev = a_.device
        al = torch.as_tensor(alen).long().to(dev).contiguous()
        wl = torch.as_tensor(wlen).long().to(dev).contiguous()
        if al.shape != (B,) or wl.shape != (P,):
            raise RuntimeError("CrossPairs: one length per clip and per phrase is needed")
        aq = gemm(a_, w_h, B * T, D, D, transB=True, ldb=2 * D)
        ak = gemm(t_, w_h[:, D:], P * L, D, D, transB=True, ldb=2 * D, bias=b_h)
        gu = gemm(a_, w_u, B * T, D, D, transB=True, bias=b_u, act=5)
        ws = gemm(t_, w_s, P * L, D, D, transB=True)
        sim = _empty(B, B, N, T, like=a_)
        alpha, dyfac, simp = _empty(B, P, T, L, like=a_), _empty(B, P, T, like=a_), _empty(B, P, T, like=a_)
        call("tag_crosspairs_forward", ptr(a_), ptr(aq), ptr(gu), ptr(t_), ptr(ak), ptr(ws), ptr(v), ptr(b_s), ptr(al), ptr(wl),
             pn.data_ptr(), ptr(sim), ptr(alpha), ptr(dyfac), ptr(simp), B, T, P, L, D, N, int(bool(scale)))
        ctx.save_for_backward(a_, t_, aq, ak, gu, ws, alpha, dyfac, al, wl, w_h, v, w_u, w_s, b_s)
        ctx.pn, ctx.N = pn, N
        return sim.transpose(2, 3)                       # (B,B,T,N), as align.py returns its matrices

    @staticmethod
    def backward(ctx, dsim):
        a, t, aq, ak, gu, ws, alpha, dyfac, al, wl, w_h, v, w_u, w_s, b_s = ctx.saved_tensors
        B, T, D = a.shape
        P, L = t.shape[0], t.shape[1]
        M, ML, N = B * T, P * L, ctx.N
        dsim = _chk(dsim.transpose(2, 3), "grad")        # (B,B,N,T), contiguous
        daq, da, dgu = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
        dak, dt, dws = torch.empty_like(t), torch.empty_like(t), torch.empty_like(t)
        dv, db_s = _empty(D, like=a), _empty(D, like=a)
        wsp = _ws(query("tag_crosspairs_backward_ws_bytes", B, T, P, L, D), a)
        call("tag_crosspairs_backward", ptr(a), ptr(aq), ptr(gu), ptr(t), ptr(ak), ptr(ws), ptr(v), ptr(b_s), ptr(al), ptr(wl),
             ctx.pn.data_ptr(), ptr(alpha), ptr(dyfac), ptr(dsim), ptr(daq), ptr(da), ptr(dgu), ptr(dak), ptr(dt), ptr(dws),
             ptr(dv), ptr(db_s), B, T, P, L, D, N, ptr(wsp))
        # h2attn = [Wq | Wk]: aq = a Wq^T, ak = t Wk^T + b_h
        dw_h = _empty(D, 2 * D, like=a)
        gemm(daq, a, D, D, M, transA=True, lda=D, out=dw_h, ldc=2 * D)
        gemm(dak, t, D, D, ML, transA=True, lda=D, out=dw_h[:, D:], ldc=2 * D)
        db_h = colsum(dak, ML, D)
        gemm(daq, w_h, M, D, D, ldb=2 * D, out=da, accumulate=True)
        gemm(dak, w_h[:, D:], ML, D, D, ldb=2 * D, out=dt, accumulate=True)
        # gu = sigmoid(a Wu^T + b_u): dz_u = dgu * gu * (1 - gu), in place
        dz_u = dgu
        call("tag_sigmoid_backward", ptr(dgu), ptr(gu), ptr(dz_u), dgu.numel())
        dw_u = gemm(dz_u, a, D, D, M, transA=True, lda=D)
        db_u = colsum(dz_u, M, D)
        gemm(dz_u, w_u, M, D, D, out=da, accumulate=True)
        # ws = t Ws^T
        dw_s = gemm(dws, t, D, D, ML, transA=True, lda=D)
        gemm(dws, w_s, ML, D, D, out=dt, accumulate=True)
        g = [dw_h, db_h, dv, dw_u, db_u, dw_s, db_s]
        for k in range(7):
            _deliver(g, ctx.sinks, k, g[k])
        _ready(ctx.params)
        return (da, None, dt, None, None, *g, None)


class CrossAttentionHeadFunction(TagFunction):
    """match.CrossAttention (models/match.py:63-88): nn.MultiheadAttention(E, H, p, batch_first, kdim = vdim = kvdim) of every
    audio frame over the phrase tokens, ``audio + dropout(out)``, LayerNorm, Linear(E,1), sigmoid -> (B,T).
    params = (wq (E,E), wk (E,Dk), wv (E,Dk), in_proj_bias (3E), out_proj.weight, out_proj.bias, norm.weight, norm.bias,
    linear.weight (1,E), linear.bias (1)); wq/wk/wv may be row blocks of one in_proj_weight (kvdim = E)."""

    @staticmethod
    def forward(ctx, audio, token, text_len, num_heads, drop_p, training, *params):
        a, t = _chk(audio, "audio_emb"), _chk(token, "token_emb")
        B, T, E = a.shape
        L, Dk = t.shape[1], t.shape[2]
        sinks = _sinks(params)
        wq, wk, wv, b_in, wo, bo, g, be, wl, bl = (_chk(x.detach(), "parameter") for x in params)
        if wq.shape != (E, E) or wk.shape != (E, Dk) or wv.shape != (E, Dk) or wo.shape != (E, E) or E % num_heads:
            raise RuntimeError("CrossAttention: inconsistent dimensions")
        kl = torch.as_tensor(text_len).long().to(a.device).contiguous()
        M, ML = B * T, B * L
        p = float(drop_p) if training else 0.0
        seeds = [new_seed(), new_seed()] if p > 0 else [0, 0]
        q = gemm(a, wq, M, E, E, transB=True, bias=b_in[:E])
        k = gemm(t, wk, ML, E, Dk, transB=True, bias=b_in[E:2 * E])
        v = gemm(t, wv, ML, E, Dk, transB=True, bias=b_in[2 * E:])
        attn = _empty(B, T, num_heads, L, like=a)
        cx = _empty(B, T, E, like=a)
        call("tag_mha_cross_forward", ptr(q), ptr(k), ptr(v), ptr(kl), ptr(attn), ptr(cx), B, T, L, E, num_heads, p, seeds[0])
        r = gemm(cx, wo, M, E, E, transB=True, bias=bo)
        sim = _empty(B, T, like=a)
        mu, rstd = _empty(M, like=a), _empty(M, like=a)
        call("tag_resln_head_forward", ptr(a), ptr(r), ptr(g), ptr(be), ptr(wl), ptr(bl), ptr(sim), ptr(mu), ptr(rstd), M, E,
             1e-5, p, seeds[1])
        ctx.save_for_backward(a, t, q, k, v, attn, cx, r, sim, mu, rstd, kl, wq, wk, wv, wo, g, be, wl)
        ctx.cfg = (num_heads, p, seeds)
        ctx.sinks = sinks
        ctx.params = list(params) if cfg.DIRECT_GRADS else None
        return sim

    @staticmethod
    def backward(ctx, dsim):
        a, t, q, k, v, attn, cx, r, sim, mu, rstd, kl, wq, wk, wv, wo, g, be, wl = ctx.saved_tensors
        H, p, seeds = ctx.cfg
        B, T, E = a.shape
        L, Dk = t.shape[1], t.shape[2]
        M, ML = B * T, B * L
        dsim = _chk(dsim, "grad")
        da, dr = torch.empty_like(a), torch.empty_like(a)
        gw, gg, gb = _empty(M, E, like=a), _empty(M, E, like=a), _empty(M, E, like=a)
        ds = _empty(M, like=a)
        call("tag_resln_head_backward", ptr(a), ptr(r), ptr(g), ptr(be), ptr(wl), ptr(mu), ptr(rstd), ptr(sim), ptr(dsim),
             ptr(da), ptr(dr), ptr(gw), ptr(gg), ptr(gb), ptr(ds), M, E, p, seeds[1])
        d_wl = colsum(gw, M, E).view(1, E)
        d_g, d_be = colsum(gg, M, E), colsum(gb, M, E)
        d_bl = colsum(ds, M, 1)
        # out_proj
        d_wo = gemm(dr, cx, E, E, M, transA=True, lda=E)
        d_bo = colsum(dr, M, E)
        dcx = gemm(dr, wo, M, E, E)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = _ws(query("tag_mha_cross_backward_ws_bytes", B, T, L, E), a)
        call("tag_mha_cross_backward", ptr(q), ptr(k), ptr(v), ptr(attn), ptr(dcx), ptr(kl), ptr(dq), ptr(dk), ptr(dv), B, T, L,
             E, H, p, seeds[0], ptr(ws))
        d_wq = gemm(dq, a, E, E, M, transA=True, lda=E)
        d_wk = gemm(dk, t, E, Dk, ML, transA=True, lda=E)
        d_wv = gemm(dv, t, E, Dk, ML, transA=True, lda=E)
        d_bin = torch.cat([colsum(dq, M, E), colsum(dk, ML, E), colsum(dv, ML, E)])
        gemm(dq, wq, M, E, E, out=da, accumulate=True)                     # d audio: residual branch + query projection
        dt = gemm(dk, wk, ML, Dk, E)
        gemm(dv, wv, ML, Dk, E, out=dt, accumulate=True)
        grads = [d_wq, d_wk, d_wv, d_bin, d_wo, d_bo, d_g, d_be, d_wl, d_bl]
        for i in range(len(grads)):
            _deliver(grads, ctx.sinks, i, grads[i])
        _ready(ctx.params)
        return (da, dt.view(B, L, Dk), None, None, None, None, *grads)


class RowDotFunction(TagFunction):
    """match.DotProduct with text_level='token' after a cross-encoder: one text vector per frame (models/match.py:43-60)."""

    @staticmethod
    def forward(ctx, audio, text, scale):
        a, t = _chk(audio, "audio_emb"), _chk(text, "token_emb")
        B, T, D = a.shape
        sim = _empty(B, T, like=a)
        call("tag_rowdot_sigmoid_forward", ptr(a), ptr(t), ptr(sim), B * T, D, int(scale))
        ctx.save_for_backward(a, t)
        ctx.scale = int(scale)
        return sim

    @staticmethod
    def backward(ctx, dsim):
        a, t = ctx.saved_tensors
        B, T, D = a.shape
        da, dt = torch.empty_like(a), torch.empty_like(t)
        call("tag_rowdot_sigmoid_backward", ptr(a), ptr(t), ptr(_chk(dsim, "grad")), ptr(da), ptr(dt), B * T, D, ctx.scale)
        return da, dt, None


class RowPairFunction(TagFunction):
    """Either head with text_level='token' in general (models/match.py:16-33, 43-60): text (B,T,D) holds one vector per frame.
    kind 0 = DotProduct, 1 = ExpNegL2; optional F.normalize of both operands."""

    @staticmethod
    def forward(ctx, audio, text, kind, l2norm, scale):
        a, t = _chk(audio, "audio_emb"), _chk(text, "token_emb")
        B, T, D = a.shape
        sim = _empty(B, T, like=a)
        call("tag_rowpair_forward", ptr(a), ptr(t), ptr(sim), B * T, D, int(kind), int(bool(l2norm)), int(bool(scale)))
        ctx.save_for_backward(a, t)
        ctx.cfg = (int(kind), int(bool(l2norm)), int(bool(scale)))
        return sim

    @staticmethod
    def backward(ctx, dsim):
        a, t = ctx.saved_tensors
        B, T, D = a.shape
        da, dt = torch.empty_like(a), torch.empty_like(t)
        call("tag_rowpair_backward", ptr(a), ptr(t), ptr(_chk(dsim, "grad")), ptr(da), ptr(dt), B * T, D, *ctx.cfg)
        return da, dt, None, None, None


class MatchGroupFunction(TagFunction):
    """DotProduct head of MultiTextBiEncoder (models/audio_text_model.py:150-190): N phrases per clip scored against the
    same audio embedding.  audio (B,T,D), text (B*N,D) -> sim (B*N,T)."""

    @staticmethod
    def forward(ctx, audio, text, N, scale):
        a, t = _chk(audio, "audio_emb"), _chk(text, "text_emb")
        B, T, D = a.shape
        if t.shape != (B * N, D):
            raise RuntimeError(f"text_emb must be (B*N, D) = ({B * N}, {D}), got {tuple(t.shape)}")
        sim = _empty(B * N, T, like=a)
        call("tag_match_group_forward", ptr(a), ptr(t), ptr(sim), int(scale), B, N, T, D)
        ctx.save_for_backward(a, t)
        ctx.cfg = (N, int(scale))
        return sim

    @staticmethod
    def backward(ctx, dsim):
        a, t = ctx.saved_tensors
        N, scale = ctx.cfg
        B, T, D = a.shape
        da, dt = torch.empty_like(a), torch.empty_like(t)
        call("tag_match_group_backward", ptr(a), ptr(t), ptr(_chk(dsim, "grad")), ptr(da), ptr(dt), scale, B, N, T, D)
        return da, dt, None, None


class LinearSoftmaxPoolFunction(TagFunction):
    """linear_softmax_with_lens (models/utils.py:75-76): rows (R,T) of frame probabilities -> (R,), row r uses
    length[r // group]."""

    @staticmethod
    def forward(ctx, fs, length, group):
        f = _chk(fs, "frame_sim")
        R, T = f.shape
        clip = _empty(R, like=f)
        call("tag_linear_softmax_pool_forward", ptr(f), ptr(length), ptr(clip), R, T, group)
        ctx.save_for_backward(f, length)
        ctx.group = group
        return clip

    @staticmethod
    def backward(ctx, dclip):
        f, length = ctx.saved_tensors
        R, T = f.shape
        dfs = torch.empty_like(f)
        call("tag_linear_softmax_pool_backward", ptr(f), ptr(length), ptr(_chk(dclip, "grad")), ptr(dfs), R, T, ctx.group)
        return dfs, None, None


class MeanMeanPoolFunction(TagFunction):
    """sim_pooling.AudioMeanTextMean (models/sim_pooling.py:6-22): (B,B,T,N) -> (B,B)."""

    @staticmethod
    def forward(ctx, sim, audio_len, text_len):
        s = _chk(sim, "sim")
        B, _, T, N = s.shape
        out = _empty(B, B, like=s)
        call("tag_meanmean_pool_forward", ptr(s), ptr(audio_len), ptr(text_len), ptr(out), B, T, N)
        ctx.save_for_backward(audio_len, text_len)
        ctx.shape = (B, T, N)
        return out

    @staticmethod
    def backward(ctx, dout):
        audio_len, text_len = ctx.saved_tensors
        B, T, N = ctx.shape
        dsim = torch.empty(B, B, T, N, device=dout.device, dtype=F32)
        call("tag_meanmean_pool_backward", ptr(_chk(dout, "grad")), ptr(audio_len), ptr(text_len), ptr(dsim), B, T, N)
        return dsim, None, None


class AttnPoolFunction(TagFunction):
    """AttentionPooling (models/text_encoder.py:46-58): softmax(fc(x)) over the valid tokens, weighted sum -> (B,D)."""

    @staticmethod
    def forward(ctx, x, lens, w, b):
        xs = _chk(x, "token_emb")
        B, L, D = xs.shape
        w_, b_ = _chk(w.detach(), "fc.weight").view(-1), _chk(b.detach(), "fc.bias")
        weight, out = _empty(B, L, like=xs), _empty(B, D, like=xs)
        call("tag_attnpool_forward", ptr(xs), ptr(lens), ptr(w_), ptr(b_), ptr(weight), ptr(out), B, L, D)
        ctx.save_for_backward(xs, w_, weight)
        ctx.sinks = _sinks([w, b])
        ctx.params = [w, b] if cfg.DIRECT_GRADS else None
        return out

    @staticmethod
    def backward(ctx, dout):
        xs, w_, weight = ctx.saved_tensors
        B, L, D = xs.shape
        dx, gw, gb = torch.empty_like(xs), _empty(B, D, like=xs), _empty(B, like=xs)
        call("tag_attnpool_backward", ptr(xs), ptr(w_), ptr(weight), ptr(_chk(dout, "grad")), ptr(dx), ptr(gw), ptr(gb), B, L, D)
        g = [colsum(gw, B, D).view(1, D), colsum(gb, B, 1)]
        for i in range(2):
            _deliver(g, ctx.sinks, i, g[i])
        _ready(ctx.params)
        return dx, None, g[0], g[1]


class UpsampleLinearFunction(TagFunction):
    """F.interpolate(x.unsqueeze(1), T * ratio, mode="linear", align_corners=False).squeeze(1) on (R,T) frame scores."""

    @staticmethod
    def forward(ctx, x, ratio):
        xs = _chk(x, "frame_sim")
        R, T = xs.shape
        out = _empty(R, T * ratio, like=xs)
        call("tag_upsample_linear_forward", ptr(xs), ptr(out), R, T, int(ratio))
        ctx.cfg = (R, T, int(ratio))
        return out

    @staticmethod
    def backward(ctx, dout):
        R, T, ratio = ctx.cfg
        dx = torch.empty(R, T, device=dout.device, dtype=F32)
        call("tag_upsample_linear_backward", ptr(_chk(dout, "grad")), ptr(dx), R, T, ratio)
        return dx, None


class GroupExpandFunction(TagFunction):
    """(B, ...) -> (B*N, ...): every clip's rows repeated for its N phrases (MultiTextBiEncoder with a cross-encoder,
    models/audio_text_model.py:165-168); backward sums the N copies in a fixed order."""

    @staticmethod
    def forward(ctx, x, n):
        xs = _chk(x, "audio_emb")
        B = xs.shape[0]
        R = xs.numel() // B
        out = _empty(B * n, *xs.shape[1:], like=xs)
        call("tag_group_expand_forward", ptr(xs), ptr(out), B, int(n), R)
        ctx.cfg = (xs.shape, int(n), R)
        return out

    @staticmethod
    def backward(ctx, dout):
        shape, n, R = ctx.cfg
        dx = torch.empty(shape, device=dout.device, dtype=F32)
        call("tag_group_expand_backward", ptr(_chk(dout, "grad")), ptr(dx), shape[0], n, R)
        return dx, None


class SimPoolFunction(TagFunction):
    """General similarity pooling (tag_sim_pool_*): sim (R,T,N) -> (R) or, with tmode = -1, (R,N).
    amode 0 mean / 1 max / 2 linear_softmax / 3 exp_softmax over the frames < alen[r // a_div];
    tmode 0 mean / 1 sum / 2 max / 3 mean+sum over the tokens < tlen[r % t_mod]."""

    @staticmethod
    def forward(ctx, sim, alen, tlen, a_div, t_mod, amode, tmode):
        s = _chk(sim, "sim")
        R, T, N = s.shape
        out = _empty(R, N, like=s) if tmode < 0 else _empty(R, like=s)
        call("tag_sim_pool_forward", ptr(s), ptr(alen), ptr(tlen), ptr(out), R, T, N, a_div, t_mod, amode, tmode)
        ctx.save_for_backward(s, alen, tlen if tlen is not None else alen)
        ctx.cfg = (a_div, t_mod, amode, tmode, tlen is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        s, alen, tlen = ctx.saved_tensors
        a_div, t_mod, amode, tmode, has_t = ctx.cfg
        R, T, N = s.shape
        dsim = torch.empty_like(s)
        call("tag_sim_pool_backward", ptr(s), ptr(alen), ptr(tlen) if has_t else None, ptr(_chk(dout, "grad")), ptr(dsim), R, T,
             N, a_div, t_mod, amode, tmode)
        return dsim, None, None, None, None, None, None


POOL_MODES = {"mean": 0, "max": 1, "linear_softmax": 2, "exp_softmax": 3}
TEXT_MODES = {"mean": 0, "sum": 1, "max": 2, "mean_sum": 3}


def check_tagging_precision(embedding):
    """The AudioTagging head's passes are fp32: it runs behind the encoder in every mode that hands over an fp32 embedding
    (the GEMMs follow GEMM_MATH like every other linear); anything else is refused before any launch."""
    if embedding.dtype != F32:
        raise RuntimeError(f"AudioTagging: the head takes an fp32 embedding, the encoder handed over {embedding.dtype} "
                           f"(CONV_MATH {cfg.CONV_MATH!r}, ACT_DTYPE {cfg.ACT_DTYPE!r}, GEMM_MATH {cfg.GEMM_MATH!r})")


def tagging_head_forward(embedding, weight, bias, length, mode):
    """AudioTagging.forward below the encoder (models/audio_text_model.py:441-453): sigmoid(fc_output(embedding)) and its
    pooling over the valid frames -> frame_sim (B,T,C), clip_sim (B,C), aux (B,C)."""
    x = _chk(embedding, "embedding")
    B, T, E = x.shape
    w, b = _chk(weight, "weight"), _chk(bias, "bias")
    C = w.shape[0]
    if tuple(w.shape) != (C, E) or tuple(b.shape) != (C,):
        raise RuntimeError(f"tagging head: weight {tuple(w.shape)} / bias {tuple(b.shape)} do not fit an embedding of {E}")
    prob = gemm(x.view(B * T, E), w, B * T, C, E, transB=True, bias=b, act=5).view(B, T, C)
    clip, aux = class_pool_forward(prob, length, mode)
    return prob, clip, aux


def tagging_head_backward(embedding, weight, prob, clip, aux, length, mode, dprob, dclip, need=(True, True, True),
                          outs=(None, None)):
    """-> (dembedding, dweight, dbias), None where ``need`` is off; outs: where dweight / dbias are written (or None)."""
    B, T, E = embedding.shape
    C = weight.shape[0]
    M = B * T
    dlogit = tagging_head_dlogit(prob, dprob, dclip, clip, aux, length, mode).view(M, C)
    x2 = embedding.view(M, E)
    dx = gemm(dlogit, weight, M, E, C).view(B, T, E) if need[0] else None
    dw = gemm(dlogit, x2, C, E, M, transA=True, lda=C, out=outs[0]) if need[1] else None
    db = colsum(dlogit, M, C, out=outs[1]) if need[2] else None
    return dx, dw, db


class TaggingHeadFunction(TagFunction):
    """The AudioTagging head as one node: embedding (B,T,E), fc_output.weight (C,E), fc_output.bias (C), length (B) int64,
    mode (POOL_MODES) -> frame_sim (B,T,C), clip_sim (B,C).  Saves prob, clip, aux; parameter gradients go through the
    direct-gradient sinks like LinearFunction's."""

    @staticmethod
    def forward(ctx, embedding, weight, bias, length, mode):
        x = _chk(embedding, "embedding")
        w_, b_ = _chk(weight.detach(), "weight"), _chk(bias.detach(), "bias")
        prob, clip, aux = tagging_head_forward(x, w_, b_, length, mode)
        ctx.save_for_backward(x, w_, prob, clip, aux, length)
        ctx.mode = mode
        ctx.set_materialize_grads(False)          # an unused output arrives as None, not as a 34 MB zero fill
        ctx.sinks = _sinks([embedding, weight, bias])
        ctx.params = [weight, bias] if cfg.DIRECT_GRADS else None
        return prob, clip

    @staticmethod
    def backward(ctx, dprob, dclip):
        x, w, prob, clip, aux, length = ctx.saved_tensors
        sk = ctx.sinks
        need = tuple(ctx.needs_input_grad[:3])
        dx, dw, db = tagging_head_backward(x, w, prob, clip, aux, length, ctx.mode, dprob, dclip, need,
                                           (sk[1] if need[1] else None, sk[2] if need[2] else None))
        g = [dx, None, None, None, None]
        if need[1]:
            _deliver(g, sk, 1, dw)
        if need[2]:
            _deliver(g, sk, 2, db)
        _ready(ctx.params)
        return tuple(g)


class MaxMarginFunction(TagFunction):
    """MaxMarginRankingLoss (losses.py:226-264) on an (n,n) similarity matrix; fix_norm drops the diagonal pairs."""

    @staticmethod
    def forward(ctx, x, margin, lamda1, fix_norm=True):
        xs = _chk(x, "sim")
        n = xs.shape[0]
        loss = _empty(1, like=xs)
        call("tag_maxmargin_forward", ptr(xs), n, float(margin), float(lamda1), int(bool(fix_norm)), ptr(loss))
        ctx.save_for_backward(xs)
        ctx.cfg = (float(margin), float(lamda1), int(bool(fix_norm)))
        return loss.view(())

    @staticmethod
    def backward(ctx, dloss):
        (xs,) = ctx.saved_tensors
        dx = torch.empty_like(xs)
        call("tag_maxmargin_backward", ptr(xs), xs.shape[0], ctx.cfg[0], ctx.cfg[1], ctx.cfg[2],
             ptr(_chk(dloss.reshape(1), "grad")), ptr(dx))
        return dx, None, None, None
