/*
 * tag_hip.h -- C ABI of libtag_hip.so: the MI355X (gfx950) hot path of text-to-audio grounding.
 *
 * The reference (wsntxxn/TextToAudioGrounding) is pure Python/PyTorch: it has no FFI of its own.
 * The replaceable seam is the nn.Module contract of SURVEY.md section 8(b); every entry point below
 * names the reference call site whose arithmetic it replaces (paths relative to the reference
 * root).  The Python host side (texttoaudiogrounding_amd/) binds these with ctypes and mirrors the
 * reference's module names and forward() signatures; INTEGRATION.md shows the stub a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter comment says "host";
 *   - all floating tensors are contiguous fp32 unless a stride is given; indices are int64;
 *   - image tensors are channels-last: (B, H=time, W=freq, C);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are async;
 *   - return value: 0 on success, otherwise a negative TAG_E* code or a positive hipError_t;
 *     tag_last_error() returns a static, thread-local message for the last failure;
 *   - no call allocates device memory: scratch is passed in by the caller (`ws`), with the size
 *     given by the matching *_ws_bytes() query.
 */
#ifndef TAG_HIP_H
#define TAG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAG_ABI_VERSION 3   /* bump whenever an EXISTING entry point changes its arguments / data layout (lib.py checks it FIRST);
                               entry points that are only added do not bump it: a library without them fails lib.load() on its
                               build id and on the symbol lookup */
#define TAG_EINVAL (-1) /* bad argument (shape not supported, null pointer, ...) */
#define TAG_ELAUNCH (-2)

int tag_abi_version(void);
/* sha256 (hex) over the kernel sources the library was compiled from, as lib.csrc_sha256() forms it: the BINARY attests its
 * sources, so a stale libtag_hip.so beside edited sources is refused by lib.load() and a PMC profile is only quoted by
 * bench.py for the binary that actually ran (the reference has no native code: nothing is replaced) */
const char* tag_build_id(void);
const char* tag_last_error(void);
/* Developer switch for A/B timing by tools/ and tests/ (csrc/tag_lib.hip lists the names: "halo_bn256", "gru_coop", ...): set before
 * the first launch that reads it.  The launchers read no environment; texttoaudiogrounding_amd/lib.py forwards the TAG_* variables
 * of the tool scripts here at load time.  Nothing of the reference is replaced.  TAG_EINVAL for an unknown name. */
int tag_set_option(const char* name, int value);
/* Measurement aid of bench.py (csrc/probe.hip; nothing of the reference is replaced): `workgroups` x 4 waves of register-resident
 * MFMA work for `iters` iterations.  kind 0: bf16 32x32x16 on RANDOM operands (what a real kernel's toggling costs: the part's
 * power limit), 1: bf16 constant operands (datasheet conditions), 2 / 3: the same for the exact-fp32 32x32x2.  clocks: 3 x u64,
 * device; [0] shader clocks and [1] 100 MHz reference ticks workgroup 0 ran for.  tag_mfma_probe_flop: the FLOP of such a launch. */
int tag_mfma_probe(int kind, int iters, int workgroups, unsigned seed, void* clocks, void* stream);
double tag_mfma_probe_flop(int kind, int iters, int workgroups);
/* the VALU member of the probe family (tools/hybrid_probe.py): `workgroups` x 4 waves of v_pk_fma_f32 on register operands,
 * iters x 32 instructions x 256 FLOP per wave; clocks as above */
int tag_valu_probe(int iters, int workgroups, unsigned seed, void* clocks, void* stream);
/* number of CUs of the current device (used by the host to size split-K workspaces) */
int tag_device_cu_count(void);

/* ---------------------------------------------------------------------------------------------
 * F1 + F2: torchaudio MelSpectrogram(power=2, center=True, reflect) + AmplitudeToDB(power)
 * models/audio_encoder.py:113-124,183-184 (Cnn8Rnn) and :29-37,68-69 (CrnnEncoder).
 * wave (B,S) -> out (B, F=S/hop+1, n_mels) in dB, time-major (= the (B,1,F,n_mels) image the CNN reads).
 * window: (win_length) hann; fb: (n_fft/2+1, n_mels).  n_fft in {1024, 2048}; n_mels <= 64.
 * power_out (nullable): (B,F,n_mels) mel power before the dB step (parity is checked in the power domain).
 * ------------------------------------------------------------------------------------------- */
int tag_logmel_forward(const float* wave, int B, int S, int n_fft, int win_length, int hop,
                       const float* window, const float* fb, int n_mels, float* out_db,
                       float* power_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Input side of F1: waveform packs hold float16 samples (utils/data/pack_waveform.py:46-52); the reference's loaders widen
 * them to float32 on the host (datasets/single_phrase_dataset.py:44-45) and zero-pad the batch to its longest clip
 * (utils/train_util.py:211-216 via datasets/collate_function.py:24-28).  Device form: packed_f16 = the B ragged clips
 * back to back (what crosses PCIe), offsets (B+1) int64 sample offsets, out (B,S) float32 zero-padded (clips longer than S
 * are cut), len_out (B) int64 = clip lengths (nullable).  Exact: every float16 is a float32.
 * ------------------------------------------------------------------------------------------- */
int tag_waveform_f16_to_f32_padded(const void* packed_f16, const long* offsets, int B, int S, float* out,
                                   long* len_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * F3 / A1: BatchNorm2d statistics over a channels-last tensor x (rows, C)  (nn.BatchNorm2d, train)
 * models/audio_encoder.py:133,188-190 (bn0 over the mel axis) and models/panns.py:35-36,49-50.
 * Produces batch mean / invstd (biased var, eps) and the fused affine  scale = gamma*invstd,
 * shift = beta - mean*scale; updates running_mean/var (momentum, unbiased var) when non-null.
 * pre_op: 0 = stats of x; 1 = stats of leaky_relu(x, 0.1) (CrnnEncoder cdur_block chain).
 * ------------------------------------------------------------------------------------------- */
size_t tag_bn_stats_ws_bytes(long rows, int C);
int tag_bn_stats(const float* x, long rows, int C, int pre_op, const float* gamma, const float* beta,
                 float eps, float momentum, float* running_mean, float* running_var, float* mean,
                 float* invstd, float* scale, float* shift, void* ws, void* stream);
/* the same outputs from the partial statistics a conv kernel wrote in its epilogue (P rows; layout: see
 * tag_conv3x3_forward).  A row's pivot is any value near its pixels (the tile mean rounded to fp32 in conv.hip / conv_x3.hip,
 * the first output of the row in conv_wino.hip, conv_wino_fused.hip and the Cin = 1 conv); the rows are merged in fp64 (Chan et al.) about the pivot of
 * ROW 0, whatever its count, so row 0 must not be empty.  Every conv epilogue keeps that: its row 0 belongs to the first tile, strip or M group of clip 0, which starts at
 * pixel (0, 0) of that clip and so holds at least one pixel (conv.hip, conv_x3.hip, conv_rows.hip: h0 = 0 < H; conv_wino.hip,
 * conv_wino_fused.hip: tile 0, output (0, 0)).  Rows with count 0 occur only further down (tile halves past H, padding rows
 * of a tile block); they are skipped and their contents are never read.  ws: tag_bn_stats_from_partials_ws_bytes(P, C) bytes. */
size_t tag_bn_stats_from_partials_ws_bytes(int P, int C);
int tag_bn_stats_from_partials(const float* partials, int P, int C, const float* gamma, const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, float* mean,
                               float* invstd, float* scale, float* shift, void* ws, void* stream);
/* eval mode: scale/shift from running statistics */
int tag_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, int C, float* scale, float* shift,
                       void* stream);
/* y = x*scale[c] + shift[c] over (rows, C) (bn0 apply) */
int tag_affine_forward(const float* x, long rows, int C, const float* scale, const float* shift,
                       float* y, void* stream);
/* dgamma[c] = sum dy*xhat, dbeta[c] = sum dy  for a plain affine BN (bn0): xhat=(x-mean)*invstd */
int tag_bn_param_grad(const float* x, const float* dy, long rows, int C, const float* mean,
                      const float* invstd, float* dgamma, float* dbeta, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training-time augmentation of the bn0 output (csrc/augment.hip): SpecAugment = torchlibrosa's
 * SpecAugmentation / DropStripes (augmentation.py; time dropper first, then frequency), applied at
 * models/audio_encoder.py:126-131,192-195, and mixup = utils/train_util.py:73-88 do_mixup, applied at
 * models/audio_encoder.py:197-200.
 *   lm (B, F, NM) log-mel in dB (frames x mel bins); scale / shift (NM): the bn0 affine, applied as
 *   fmaf(lm, scale[m], shift[m]) exactly as the Cin = 1 convolutions apply it on load (both null: plain copy);
 *   stripes (B, n_time + n_freq, 2) int32 [bgn, width]: rows 0..n_time-1 zero frames [bgn, bgn+width), the rest zero
 *   mel bins (null when n_time = n_freq = 0; the values are compared, never used as addresses);
 *   lam (B) fp32 or null: x0[k] = x[2k]*lam[2k] + x[2k+1]*lam[2k+1] (two products, one add), B even.
 *   x0 (B' = B, or B/2 with lam, F, NM).  NM % 4 == 0, n_time, n_freq <= 8.
 * backward: dbn0 (B, F, NM) = mask[b] * lam[b] * dx0[b/2]  (dx0[b] without lam); masked elements exactly 0.
 */
int tag_augment_forward(const float* lm, const float* scale, const float* shift, const int* stripes, int n_time,
                        int n_freq, const float* lam, float* x0, int B, int F, int NM, void* stream);
int tag_augment_backward(const float* dx0, const int* stripes, int n_time, int n_freq, const float* lam, float* dbn0,
                         int B, int F, int NM, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1: 3x3 convolution, stride 1, pad 1, no bias (models/panns.py:25-33,49-50), channels-last,
 * implicit GEMM on the fp32 MFMA (v_mfma_f32_32x32x2_f32).
 *   wpack: (9, Cin, Cout) produced by tag_pack_conv_weight.
 *   prologue applied to x on load (padding stays zero):
 *     0 none | 1 relu(x*in_scale[c]+in_shift[c]) | 2 leaky(x,.1)*in_scale+in_shift | 3 x*in_scale+in_shift
 * Requires Cin % 32 == 0 (use tag_conv3x3_c1_* for Cin == 1).
 * The same entry computes dgrad when given the flipped/transposed pack (wdgrad) and dy as x.
 * ------------------------------------------------------------------------------------------- */
int tag_pack_conv_weight(const float* w /*(Cout,Cin,3,3)*/, float* wfwd /*(9,Cin,Cout)*/,
                         float* wdgrad /*(9,Cout,Cin), nullable*/, int Cin, int Cout, void* stream);
/* stats (nullable): when given, the kernel also writes BatchNorm partial statistics of y in its epilogue --
 * tag_conv3x3_stats_rows(B,H,W,Cout) rows of (3*Cout) floats {tile pivot mu, sum(y-mu), sum((y-mu)^2)} followed
 * by one pixel count per row, i.e. rows*(3*Cout+1) floats; tag_bn_stats_from_partials turns them into
 * the batch statistics (saves the separate pass over y).  rows == 0: not available for this shape. */
int tag_conv3x3_stats_rows(int B, int H, int W, int Cout);
int tag_conv3x3_forward(const float* x, const float* wpack, int prologue, const float* in_scale,
                        const float* in_shift, float* y, float* stats, int B, int H, int W, int Cin, int Cout,
                        void* stream);

/* Alternative arithmetic for the same convolution (forward and dgrad): every fp32 operand is split exactly into
 * three bf16 terms and the products run on the bf16 MFMA (v_mfma_f32_32x32x16_bf16) with fp32 accumulation --
 * 6 of the 9 partial products by default (error of the dropped terms <= 2^-23 per product), TAG_X3_PRODUCTS=9
 * for all of them, =1 for plain bf16.  Opt-in; tag_conv3x3_forward above stays the exact-fp32 default.
 *   wfwd / wdgrad: tag_conv3x3_x3_pack_bytes(Cin, Cout) bytes each (pre-split, MFMA-fragment order).
 * Argument rules of tag_conv3x3_forward_x3 and tag_conv3x3_forward_x3_bf16 (anything else returns -1 before any launch, outputs
 * untouched): B, H > 0; W in {8,16,32,64}; Cin % 32 == 0 and Cin <= 512 (the prologue table of one workgroup: 2 x 512 floats);
 * Cout % 64 == 0 (tiles of 128 couts where Cout % 128 == 0, else of 64); prologue 0..3, with in_scale AND in_shift unless 0;
 * B H W < 2^31 and H W Cin sizeof(element) < 2^32 (32-bit byte offsets inside one image).  The data gradient is the same entry
 * on the wdgrad pack with Cin and Cout exchanged, so it needs Cout % 32 == 0, Cout <= 512 and Cin % 64 == 0.
 * tag_pack_conv_weight_x3: Cin % 32 == 0, Cout % 32 == 0, both packs non-NULL.  Pack layout: 16-byte fragment pieces at
 * (((tap * K/16 + kk) * N/32 + nb) * 3 + plane) * 64 + lane, lane holding k = kk*16 + 8*(lane>>5) + 0..7 of n = nb*32 + (lane&31);
 * forward K = Cin, N = Cout; dgrad K = Cout, N = Cin, tap 8 - tap.  Planes hi / mid / lo by truncation (hi + mid + lo == w
 * exactly); products == 1: hi rounded to nearest even, mid = lo = 0. */
size_t tag_conv3x3_x3_pack_bytes(int Cin, int Cout);
/* products: partial products per fp32 multiply -- 6 (default), 9 (all), 1 (plain bf16: operands rounded to nearest
 * bf16, one product; BASELINE configs[2] arithmetic), 0 = process default (TAG_X3_PRODUCTS, else 6).  A weight pack
 * made with products == 1 must only be used with products == 1 (its hi plane is rounded, not truncated). */
int tag_pack_conv_weight_x3(const float* w /*(Cout,Cin,3,3)*/, void* wfwd, void* wdgrad, int Cin, int Cout,
                            int products, void* stream);
int tag_conv3x3_x3_stats_rows(int B, int H, int W, int Cout);
/* the same for the bf16-storage entry points (tag_conv3x3_forward_x3_bf16 with this Cin / prologue; tag_conv3x3_dgrad_bnsums_bf16:
 * prologue 0).  The shapes (W, Cin, Cout) = (64, 64, 64) and (32, 64, multiple of 128) with H >= 2 and prologue 0 | 1 run on
 * the row-streaming kernel (csrc/conv_rows.hip: weights stationary in registers, input rows by LDS-DMA into a ring) whose
 * statistics accumulate over a whole strip of rows: B * strips * 2 * (2 | 1) partial rows, strips = min(ceil(CUs / (B * n-tiles)),
 * H / 16), at least 1; every other shape writes one row per tile M-group of the tile kernel: B * ceil(H / (128 / W)) * (1 where
 * Cout % 128 == 0, else 2).  (ABI 2: Cin and prologue were added.) */
int tag_conv3x3_x3_bf16_stats_rows(int B, int H, int W, int Cin, int Cout, int prologue);
/* 0: keep every bf16-storage layer on the tile kernel (A/B timing, tools/conv_rows_bench.py); returns the previous setting.
 * The environment variable TAG_CONV_ROWS=0 is the process-wide form. */
int tag_conv_rows_enable(int on);
/* the same switch for the bf16-storage weight gradient: 1 (default) = the layers without a producer prologue run on
 * csrc/conv_wgrad_dma.hip (operands by LDS-DMA), 2 = the prologue-1 layers too, 0 = every layer on the register-staged kernel
 * of conv_x3.hip; returns the previous setting.  Environment TAG_WGRAD_DMA is the process-wide form. */
int tag_wgrad_dma_enable(int on);
int tag_conv3x3_forward_x3(const float* x, const void* wpack, int prologue, const float* in_scale,
                           const float* in_shift, float* y, float* stats, int B, int H, int W, int Cin, int Cout,
                           int products, void* stream);
/* wgrad with the same arithmetic (K = pixels; operands fetched with the transposing LDS read ds_read_b64_tr_b16).
 * Requires B, H > 0, W in {8,16,32,64}, Cin % 64 == 0, Cout % 64 == 0 (no upper limit on either), prologue 0..3 with both tables
 * unless 0, B H W < 2^31, H W Cin sizeof(element) < 2^32 and H W Cout sizeof(element) < 2^32; the same rules hold for
 * tag_conv3x3_wgrad_x3_bf16.  ws: tag_conv3x3_wgrad_x3_ws_bytes (non-NULL) = splits * 9 * Cin * Cout floats for the larger of the
 * two split counts (32-pixel chunks: fp32 tensors; 64-pixel chunks: bf16 tensors); a launch writes its own split count of
 * partials and leaves the rest untouched.  The result is bit-identical from run to run. */
size_t tag_conv3x3_wgrad_x3_ws_bytes(int B, int H, int W, int Cin, int Cout);
int tag_conv3x3_wgrad_x3(const float* x, int prologue, const float* in_scale, const float* in_shift,
                         const float* dy, float* dw /*(Cout,Cin,3,3)*/, int B, int H, int W, int Cin, int Cout,
                         int products, void* ws, void* stream);
/* dw (Cout,Cin,3,3) = sum over pixels of prologue(x)[shifted] * dy ; ws from *_ws_bytes */
/* dgrad convolution fused with the REDUCTION half of the BatchNorm+ReLU backward its result flows into
 * (models/panns.py:49-50 backward: relu_(bn(conv(x)))).  da = conv(dy, wpack_dgrad) is written as by
 * tag_conv3x3_forward; in the epilogue every 64-pixel wave tile also reads yref (the raw conv output the forward
 * pass saved = the BatchNorm input at the same pixels/channels) and writes the partial sums over the tile of
 *   g = da * [yref*bn_scale + bn_shift > 0]    and    g * (yref - bn_mean) * bn_invstd
 * to bnpart [P][2][Cout] (P = tag_conv3x3_stats_rows(B,H,W,Cout) > 0: halo-tile shapes only).  The MFMA-bound conv
 * hides that read; the separate two-tensor reduction pass of tag_bnrelu_backward disappears.
 * tag_bn_grad_from_partials folds the rows (fp64, fixed order) into dgamma / dbeta; tag_bnrelu_backward_apply is the
 * apply half: dy = gamma*invstd*(g - dbeta/N - xhat*dgamma/N) (bn_train) or gamma*invstd*g. */
int tag_conv3x3_dgrad_bnsums(const float* dy, const float* wpack, float* da, const float* yref,
                             const float* bn_scale, const float* bn_shift, const float* bn_mean,
                             const float* bn_invstd, float* bnpart, int B, int H, int W, int Cin, int Cout,
                             void* stream);
/* Winograd F(2x2,3x3) form of the same convolution, all fp32: the A1 ConvBlock convs of models/panns.py:29-38,49-50 with 2.25 x
 * fewer MFMA FLOP than tag_conv3x3_forward.  Drop-in for tag_conv3x3_forward(stats) / tag_conv3x3_dgrad_bnsums / _dgrad_poolsums /
 * _forward_bnrelu_pool_eval / tag_conv3x3_wgrad.  Error vs an fp64 convolution: at or below the direct fp32 kernel's.
 *   Cout % 64 == 0 with Cin % 8 == 0 (of the shapes tag_conv3x3_wino_ok serves: Cin = 32 too, besides the multiples of 64; every
 *   Cnn8Rnn layer but the Cin = 1 conv): ONE kernel per launch (round 6, csrc/conv_wino_fused.hip) -- the input transform B^T d B (producer BatchNorm+ReLU prologue and zero padding applied on load) is
 *   formed on the way into LDS, the 16 products (tiles x Cin).(Cin x Cout) run on the exact-fp32 MFMA into 16 accumulator sets that
 *   stay in registers, the output transform A^T m A and the epilogue (BatchNorm statistics rows [K | r | q][Cout] + counts for
 *   tag_bn_stats_from_partials / rows [sum g | sum g*xhat][Cout] for tag_bn_grad_from_partials / pooled inference output) work from
 *   a parked output tile.  No workspace (ws is ignored, tag_conv3x3_wino_ws_bytes = 64); one partial row per 64-tile block
 *   (tiles in (b, tile row, tile column) order, 2 x 2 outputs each), its pivot the output at pixel (0, 0) of the block's first tile.
 *   Exactly Cout = 32 (Cin = 32, 64, 128, 256, 512 or 1024): round 5's plane form (csrc/conv_wino.hip): input transform -> 16
 *   batched products -> output transform through planes in ws, 16 T (Cin + Cout) floats, T = B ceil(H/2) ceil(W/2) tiles; partial
 *   rows: 32 per 256 tiles (row 32 g + s: tiles 256 g + 32 it + s, it = 0..7; pivot = the output at pixel (0, 0) of the first of
 *   them; a row without tiles is written as zeros with count 0).
 *   Served shapes (tag_conv3x3_wino_ok): both counts multiples of 64 up to 1024, or both of 32, 64, 128, 256, 512, 1024.
 *   ufwd / udgrad (16 * Cin * Cout floats each): G g G^T of the filter / of the tap-flipped, channel-swapped filter -- an OPAQUE
 *   pack of tag_pack_conv_weight_wino (fused form: per (64-cout block, 8-channel K chunk) the kernel's LDS image [xi][n 64][k 8];
 *   plane form: [16][Cin][Cout] / [16][Cout][Cin]); P = tag_conv3x3_wino_stats_rows; tag_conv3x3_wino_ok: 1 when the shape is served
 *   (every tensor below 2^31 bytes: a caller cuts larger inference batches, any cut gives the same rows). */
int tag_conv3x3_wino_ok(int B, int H, int W, int Cin, int Cout);
int tag_pack_conv_weight_wino(const float* w /*(Cout,Cin,3,3)*/, float* ufwd, float* udgrad, int Cin, int Cout, void* stream);
size_t tag_conv3x3_wino_ws_bytes(int B, int H, int W, int Cin, int Cout);
int tag_conv3x3_wino_stats_rows(int B, int H, int W, int Cout);
/* weight gradient in the Winograd domain: dw (Cout,Cin,3,3) = G^T [ sum over tiles (A dY A^T) (.) (B^T prologue(x) B) ] G -- the
 * adjoint of the forward form.  Fused form (ONLY when Cin and Cout are both multiples of 64): both transforms at staging, 64 ci x
 * 64 co x 16 xi accumulators per workgroup over one slice of the tile axis (one transform row x 128 ci x 128 co when both are
 * multiples of 128), ws = 2 S partial filters folded in a fixed order.  Every other served pair (Cin = 32 or Cout = 32, whatever
 * form the forward took): plane form, 16 x S batched products over K slices of kc rows, the planes padded with zero rows to
 * Tpad = S kc.  Drop-in for tag_conv3x3_wgrad on the shapes tag_conv3x3_wino_ok accepts. */
size_t tag_conv3x3_wino_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout);
/* v_saved (optional, plane-form weight gradient only): the transformed input the forward launch of the same convolution left
 * in its v_keep buffer -- the input transform is then not repeated (x may be NULL); allowed when
 * tag_conv3x3_wino_wgrad_can_reuse_v: 0 for the fused weight gradient, which has no planes, and 0 where the K slices need zero
 * rows (Tpad > T); otherwise the call is refused. */
int tag_conv3x3_wino_wgrad_can_reuse_v(int B, int H, int W, int Cin, int Cout);
int tag_conv3x3_wino_wgrad(const float* x, int prologue, const float* in_scale, const float* in_shift, const float* dy,
                           float* dw /*(Cout,Cin,3,3)*/, int B, int H, int W, int Cin, int Cout, void* ws, const float* v_saved,
                           void* stream);
/* v_keep (optional): 16 * T * Cin floats [16][T][Cin] that receive the transformed input B^T prologue(x) B -- kept by the caller
 * for tag_conv3x3_wino_wgrad(v_saved).  Plane form: instead of ws (which then needs the product planes only: 16 * T * Cout
 * floats).  The fused forward honours it too (Cin = 32 -> Cout % 64 == 0 is the pair whose weight gradient is plane form): the
 * input transform then runs as a side launch, y has the same bits. */
int tag_conv3x3_wino_forward(const float* x, const float* ufwd, int prologue, const float* in_scale, const float* in_shift,
                             float* y, float* stats, int B, int H, int W, int Cin, int Cout, void* ws, float* v_keep,
                             void* stream);
/* Winograd twin of tag_conv3x3_dgrad_poolsums (same arguments + ws): dx = conv(dy, udgrad) and, from the output transform, the
 * partial sums [sum dz | sum dz*xhat][Cout] of the BatchNorm+ReLU+pool(ph x 2)+dropout backward of the block below (yref unpooled
 * (B,Hf,Wf,Cout)); P = tag_conv3x3_wino_stats_rows rows for tag_bn_grad_from_partials. */
int tag_conv3x3_wino_dgrad_poolsums(const float* dy, const float* udgrad, float* dx, const float* yref, const float* bn_scale,
                                    const float* bn_shift, const float* bn_mean, const float* bn_invstd, float* bnpart, int B,
                                    int H, int W, int Cin, int Cout, int Hf, int Wf, int ph, int pw, int pool, float drop_p,
                                    uint64_t seed, void* ws, void* stream);
/* inference twin of tag_conv3x3_forward_bnrelu_pool_eval: the output transform pools its own 2 x 2 tile (one 2 x 2 window or two
 * 1 x 2 windows) after BatchNorm(eval) + ReLU; the raw conv output is never written. */
int tag_conv3x3_wino_forward_bnrelu_pool_eval(const float* x, const float* ufwd, int prologue, const float* in_scale,
                                              const float* in_shift, float* out, const float* bn_scale, const float* bn_shift,
                                              int B, int H, int W, int Cin, int Cout, int ph, int pw, int pool, void* ws,
                                              void* stream);
int tag_conv3x3_wino_dgrad_bnsums(const float* dy, const float* udgrad, float* da, const float* yref, const float* bn_scale,
                                  const float* bn_shift, const float* bn_mean, const float* bn_invstd, float* bnpart, int B,
                                  int H, int W, int Cin, int Cout, void* ws, void* stream);
size_t tag_bn_grad_from_partials_ws_bytes(int P, int C);
int tag_bn_grad_from_partials(const float* bnpart, int P, int C, float* dgamma, float* dbeta, void* ws, void* stream);
int tag_bnrelu_backward_apply(const float* y, const float* scale, const float* shift, const float* mean,
                              const float* invstd, const float* gamma, const float* da, float* dy,
                              const float* dgamma, const float* dbeta, long rows, int C, int bn_train, void* stream);
/* Weight gradient (Cout,Cin,3,3); Cin % 4 == 0, Cout % 4 == 0, W <= 64, any H >= 1 and B >= 1 -- images of a few pixels included:
 * where no all-taps form serves the width, a 32-pixel chunk of the per-tap kernel may hold pixels of three or more images (H W <
 * 32 + W) and wraps its row index by a true modulo.  The workspace holds tag_conv3x3_wgrad_ws_bytes / (36 Cin Cout) partial
 * gradients, each written whole, reduced in a fixed order: two calls give the same bits. */
size_t tag_conv3x3_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout);
int tag_conv3x3_wgrad(const float* x, int prologue, const float* in_scale, const float* in_shift,
                      const float* dy, float* dw, int B, int H, int W, int Cin, int Cout, void* ws,
                      void* stream);
/* Cin == 1 (conv_block1.conv1): x (B,H,W) with optional per-column affine x*col_scale[w]+col_shift[w]
 * (bn0 folded: the BatchNorm2d(64) over the mel axis; applied BEFORE the zero padding), w (Cout,1,3,3).
 * Every entry of the family wants B, H, W, Cout > 0 and Cout % 4 == 0 and both or neither of col_scale / col_shift; the weight
 * gradient and dgrad also want Cout / 4 to divide 64 (Cout 4, 8, 16, 32, 64, 128, 256).  Anything else is TAG_EINVAL with the
 * outputs untouched (Cout = 0 included: the checks come before any division by Cout / 4). */
int tag_conv3x3_c1_forward(const float* x, const float* col_scale, const float* col_shift,
                           const float* w, float* y, int B, int H, int W, int Cout, void* stream);
/* the same with the BatchNorm partial statistics of y written by the kernel (W == 64, Cout == 64: rows > 0):
 * stats = [P][3][Cout] rows (pivot, sum(y - pivot), sum((y - pivot)^2)) + [P] pixel counts -> tag_bn_stats_from_partials */
int tag_conv3x3_c1_stats_rows(int B, int H, int W, int Cout);
int tag_conv3x3_c1_forward_stats(const float* x, const float* col_scale, const float* col_shift, const float* w,
                                 float* y, float* stats, int B, int H, int W, int Cout, void* stream);
size_t tag_conv3x3_c1_wgrad_ws_bytes(int B, int H, int W, int Cout);
int tag_conv3x3_c1_wgrad(const float* x, const float* col_scale, const float* col_shift,
                         const float* dy, float* dw, int B, int H, int W, int Cout, void* ws,
                         void* stream);
int tag_conv3x3_c1_dgrad(const float* dy, const float* w, float* dx, int B, int H, int W, int Cout,
                         void* stream);
/* fused wgrad + dgrad of the Cin = 1 convolution: ONE pass over dy (W == 64, Cout == 64 only) */
size_t tag_conv3x3_c1_backward_ws_bytes(int B, int H, int W, int Cout);
int tag_conv3x3_c1_backward(const float* x, const float* col_scale, const float* col_shift, const float* dy,
                            const float* w /*(Cout,1,3,3)*/, float* dw /*(Cout,1,3,3)*/, float* dx /*(B,H,W)*/,
                            int B, int H, int W, int Cout, void* ws, void* stream);
/* The same pass fed the RAW dgrad output of block 1's second conv: `da` = dL/d relu(bn1(yref)), and the backward of that
 * BatchNorm + ReLU (models/panns.py:46-48, x = F.relu_(self.bn1(self.conv1(x)))) is applied as the values are loaded --
 * dy = gamma*invstd * (dz - dbeta/N - xhat * dgamma/N), dz = da where bn1(yref) > 0, N = B*H*W (bn_train = 0: the two
 * mean terms are dropped) -- instead of in a separate tag_bnrelu_backward_apply pass over the largest activation.
 * dgamma / dbeta are INPUTS here: sum(dz * xhat) / sum(dz), as tag_bn_grad_from_partials leaves them. */
int tag_conv3x3_c1_backward_bnrelu(const float* x, const float* col_scale, const float* col_shift, const float* da,
                                   const float* yref, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                                   const float* bn_invstd, const float* gamma, const float* dgamma, const float* dbeta,
                                   int bn_train, const float* w, float* dw, float* dx, int B, int H, int W, int Cout,
                                   void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1 + A2: relu(bn(y)) -> avg_pool + max_pool (kernel = stride = (ph,pw), floor) -> dropout
 * models/panns.py:49-58 with pool_type 'avg+max'; F.dropout models/audio_encoder.py:203-210.
 * y raw conv output (B,H,W,C); out (B,H/ph,W/pw,C).  Dropout keep-mask = counter-based hash of
 * (seed, flat output index); p = 0 disables.  act: 1 relu(bn) | 2 leaky(.1) without bn (scale=NULL),
 * pool: 0 avg+max | 1 LPPool(norm 4) | 2 avg | 3 max (the three pool_type values of ConvBlock.forward, models/panns.py:51-60).
 * ------------------------------------------------------------------------------------------- */
int tag_bnact_pool_forward(const float* y, const float* scale, const float* shift, float* out, int B,
                           int H, int W, int C, int ph, int pw, int act, int pool, float drop_p,
                           uint64_t seed, void* stream);
/* backward of the above + the BatchNorm backward, two passes:
 *   reduce: dgamma/dbeta (needs ws), apply: dy = invstd*gamma*(dz - dbeta/N - xhat*dgamma/N)
 * dout is the gradient wrt `out`.  */
size_t tag_bn_backward_ws_bytes(long rows, int C);
int tag_bnrelu_pool_backward(const float* y, const float* scale, const float* shift,
                             const float* mean, const float* invstd, const float* gamma,
                             const float* dout, float* dy, float* dgamma, float* dbeta, int B, int H,
                             int W, int C, int ph, int pw, int pool /* 0 avg+max | 2 avg | 3 max */, float drop_p,
                             uint64_t seed, int bn_train, void* ws, void* stream);
/* Pool backward without its own reduction pass (round 5; models/panns.py:46-62 backward).  The dgrad convolution of the NEXT block's first
 * conv produces dout = dL/d(pooled, dropped-out output) -- tag_conv3x3_dgrad_poolsums writes it as tag_conv3x3_forward would AND, from its
 * output tile (parked in LDS at the end of the kernel), the partial sums over the tile of dz and dz * xhat, where dz is the gradient at the
 * BatchNorm output of yref (B,Hf,Wf,Cout): dropout undone with the forward's counter-based mask, ReLU mask and first-maximum arg-max
 * recomputed from the ph x 2 window of yref.  bnpart [P][2][Cout], P = tag_conv3x3_stats_rows(B,H,W,Cout) (row 2t carries m-tile t,
 * row 2t + 1 is zero), H = Hf / ph, W = Wf / pw; windows ph x 2 with ph 1 or 2.  tag_bn_grad_from_partials folds the rows into
 * dgamma / dbeta; tag_bnrelu_pool_backward_apply is the apply pass of tag_bnrelu_pool_backward alone. */
int tag_conv3x3_dgrad_poolsums(const float* dy, const float* wpack, float* dx, const float* yref, const float* bn_scale,
                               const float* bn_shift, const float* bn_mean, const float* bn_invstd, float* bnpart, int B, int H,
                               int W, int Cin, int Cout, int Hf, int Wf, int ph, int pw, int pool, float drop_p, uint64_t seed,
                               void* stream);
/* Inference forward of one ConvBlock stage (models/panns.py:49-60 with BatchNorm in eval mode; models/hf_modeling_grounding.py:97-180
 * runs the encoder that way): out (B, H/ph, W/pw, Cout) = pool(relu(conv3x3(prologue(x)) * bn_scale + bn_shift)), window ph x 2 (ph 1 | 2,
 * floor), pool 0 avg+max | 2 avg | 3 max.  The raw conv output -- the largest tensor of the block -- is never written: the kernel
 * pools its own output tile.  Bit-identical to tag_conv3x3_forward followed by tag_bnact_pool_forward (act 1, no dropout).
 * Halo-tile shapes only (W 8/16/32/64), producer prologue 0 | 1. */
int tag_conv3x3_forward_bnrelu_pool_eval(const float* x, const float* wpack, int prologue, const float* in_scale,
                                         const float* in_shift, float* out, const float* bn_scale, const float* bn_shift, int B,
                                         int H, int W, int Cin, int Cout, int ph, int pw, int pool, void* stream);
/* bf16-storage twin (BASELINE configs[2] mode): the sums are taken from the bf16 values of dx the apply pass will read back; rows:
 * tag_conv3x3_dgrad_poolsums_bf16_rows = B * ceil(H / (128 / W)), one per workgroup m-tile (0 = shape not served: keep
 * tag_bnrelu_pool_backward_bf16).  Served: W in {8,16,32,64}, Cin % 32 == 0, Cin <= 512, Cout % 64 == 0 and NOT a shape of the
 * row-streaming kernel (tag_conv3x3_x3_bf16_stats_rows above) while that kernel is enabled; pw == 2, ph 1 | 2, H == Hf / ph,
 * W == Wf / 2, pool 0 | 2 | 3, 0 <= drop_p < 1, B Hf Wf < 2^31.  Anything else returns -1 with nothing written. */
int tag_conv3x3_dgrad_poolsums_bf16_rows(int B, int H, int W, int Cin, int Cout);
int tag_conv3x3_dgrad_poolsums_bf16(const void* dy, const void* wpack, void* dx, const void* yref, const float* bn_scale,
                                    const float* bn_shift, const float* bn_mean, const float* bn_invstd, float* bnpart, int B,
                                    int H, int W, int Cin, int Cout, int Hf, int Wf, int ph, int pw, int pool, float drop_p,
                                    uint64_t seed, void* stream);
int tag_bnrelu_pool_backward_apply(const float* y, const float* scale, const float* shift, const float* mean,
                                   const float* invstd, const float* gamma, const float* dout, float* dy, const float* dgamma,
                                   const float* dbeta, int B, int H, int W, int C, int ph, int pw, int pool, float drop_p,
                                   uint64_t seed, int bn_train, void* stream);
int tag_bnrelu_pool_backward_apply_bf16(const void* y, const float* scale, const float* shift, const float* mean,
                                        const float* invstd, const float* gamma, const void* dout, void* dy, const float* dgamma,
                                        const float* dbeta, int B, int H, int W, int C, int ph, int pw, int pool, float drop_p,
                                        uint64_t seed, int bn_train, void* stream);
/* same without pooling: upstream gradient da (rows,C) wrt relu(bn(y)); dy may alias da */
int tag_bnrelu_backward(const float* y, const float* scale, const float* shift, const float* mean,
                        const float* invstd, const float* gamma, const float* da, float* dy,
                        float* dgamma, float* dbeta, long rows, int C, int bn_train, void* ws,
                        void* stream);
/* CrnnEncoder (cdur_block, models/audio_encoder.py:16-22,39-49): BatchNorm in FRONT of the conv, applied to
 * v = pre(x), pre_op 0 identity | 1 leaky_relu(x, 0.1).  du = gradient wrt bn(v) (from the conv dgrad);
 * dx = gradient wrt x; dgamma/dbeta the BN parameter gradients.  gamma nullable (= 1). */
int tag_bn_act_backward(const float* x, int pre_op, const float* mean, const float* invstd,
                        const float* gamma, const float* du, float* dx, float* dgamma, float* dbeta,
                        long rows, int C, int bn_train, void* ws, void* stream);
/* backward of dropout(LPPool2d(4,(ph,pw))(leaky_relu(y,0.1))) (forward: tag_bnact_pool_forward act=2 pool=1) */
int tag_lppool_leaky_backward(const float* y, const float* dout, float* dy, int B, int H, int W, int C,
                              int ph, int pw, float drop_p, uint64_t seed, void* stream);
/* materialise the dropout keep-masks (0/1 bytes) the kernels use, for parity tests.  tag_dropout_mask: one splitmix64 per
 * element, 24-bit uniform (tag_mean_w_*, tag_dropout_*, the attention heads); tag_dropout_mask_pooled: the mask of the pooled
 * activations (tag_bnact_pool_forward, tag_bnrelu_pool_backward, tag_lppool_leaky_backward): one splitmix64 per 4 consecutive
 * elements, 16-bit uniform each (csrc/tag_common.h tag_keep4; F.dropout in models/audio_encoder.py:203-210 draws from
 * torch's Philox stream instead -- masks are replayed by seed, never compared with torch's) */
int tag_dropout_mask(uint64_t seed, long n, float p, uint8_t* mask, void* stream);
int tag_dropout_mask_pooled(uint64_t seed, long n, float p, uint8_t* mask, void* stream);

/* A3: mean over W then dropout: x (rows, W, C) -> (rows, C)   models/audio_encoder.py:212-215 */
int tag_mean_w_forward(const float* x, long rows, int W, int C, float drop_p, uint64_t seed, float* out,
                       void* stream);
int tag_mean_w_backward(const float* dout, long rows, int W, int C, float drop_p, uint64_t seed,
                        float* dx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense fp32 GEMM on the MFMA, row-major:  C = act(op(A) op(B) + bias) [+ C if accumulate]
 *   op(A): transA ? A^T : A, A stored (M,K) ld=lda or (K,M) when transA; same for B (K,N)/(N,K).
 * Serves nn.Linear fc1 / audio_proj / text_proj (models/audio_encoder.py:140,216;
 * models/audio_text_model.py:45-46,78-87), the GRU input projections and all their backward GEMMs.
 * act: 0 none, 1 relu, 3 gelu (erf form), 4 tanh, 5 sigmoid.  bias (N) nullable.
 * ------------------------------------------------------------------------------------------- */
/* ws (nullable): scratch of tag_gemm_ws_bytes(M,N,K) bytes enabling a deterministic split-K for problems whose
 * MxN tile count cannot fill the chip (weight gradients: K = B*T); 0 bytes = not needed. */
size_t tag_gemm_ws_bytes(int M, int N, int K);
int tag_gemm(const float* A, int lda, int transA, const float* B, int ldb, int transB, float* C,
             int ldc, int M, int N, int K, const float* bias, int act, int accumulate, void* ws,
             void* stream);
/* tag_gemm with both operands rounded to bf16 (nearest-even) on v_mfma_f32_32x32x16_bf16, fp32 accumulate and fp32 tensors:
 * what autocast does to nn.Linear / the GRU projections in BASELINE configs[2] (bf16).  Same arguments, same workspace. */
int tag_gemm_bf16(const float* A, int lda, int transA, const float* B, int ldb, int transB, float* C,
             int ldc, int M, int N, int K, const float* bias, int act, int accumulate, void* ws,
             void* stream);
/* out[n] = sum_m x[m, n] (bias gradients); x (M,N) ld; ws >= tag_colsum_ws_bytes */
size_t tag_colsum_ws_bytes(long M, int N);
int tag_colsum(const float* x, int ld, long M, int N, float* out, void* ws, void* stream);
/* dx = dy * (y > 0) elementwise (relu_ backward), dx may alias dy */
int tag_relu_backward(const float* y, const float* dy, float* dx, long n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A4: bidirectional GRU recurrence, PyTorch gate order (r,z,n), h0 = 0, ALL T steps
 * nn.GRU(512,256,bidirectional=True,batch_first=True) models/audio_encoder.py:141,217.
 *   gi   (B,T,2,3H): x W_ih^T + b_ih for both directions (a tag_gemm)
 *   w_hh (2,3H,H), b_hh (2,3H)
 *   y    (B,T,2H)   hidden states, forward direction in [:H], reverse in [H:]
 *   gates(B,T,2,4H) saved r,z,n and (W_hn h + b_hn) for the backward pass (nullable in inference)
 * backward: dy (B,T,2H) -> dgi (B,T,2,3H), dgh (B,T,2,3H); hprev (B,T,2,H) is also written
 * (h_{t-1} per direction) so that dW_hh = dgh^T hprev is a plain GEMM for the caller.
 * When the grid (H/16)*ceil(B/16)*2 fits the device (occupancy query x CUs) the whole sequence is ONE persistent
 * launch (weights in registers, state exchanged between workgroups through tagged 8-byte granules), issued with
 * hipLaunchCooperativeKernel so that co-residency of the spinning workgroups is guaranteed by the runtime; if the
 * grid does not fit or the cooperative launch is refused, one launch per step (same arithmetic).
 * ------------------------------------------------------------------------------------------- */
/* scratch for both directions of either pass: transposed weights + the exchange granules of the persistent
 * kernels + a STICKY error word (last 256 bytes): the CALLER zero-fills the scratch once when it allocates it; a
 * persistent kernel whose bounded spin ran out sets the word (and poisons its outputs with NaN, which makes
 * tag_adam_step skip the step); the library never clears it.  Copy the last 256 bytes to the host after a
 * synchronisation and pass them to tag_gru_timed_out. */
size_t tag_gru_ws_bytes(int B, int T, int H);
int tag_gru_forward(const float* gi, const float* w_hh, const float* b_hh, float* y, float* gates,
                    void* ws /* tag_gru_ws_bytes */, int B, int T, int H, void* stream);
int tag_gru_backward(const float* dy, const float* y, const float* gates, const float* w_hh,
                     float* dgi, float* dgh, float* hprev, void* scratch /* tag_gru_ws_bytes */, int B, int T,
                     int H, void* stream);
/* A HIP stream restricted to the compute units set in mask (bit i = CU i; `words` 32-bit words) -- hipExtStreamCreateWithCUMask.
 * The host side keeps the weight-gradient side stream off a share of the CUs with it (ops.py, TAG_WGRAD_CU_SKIP). */
int tag_stream_create_cu_mask(const unsigned* mask, int words, void** stream_out);
int tag_gru_timed_out(const void* host_copy_of_err_word);
/* After a timeout: make every later persistent GRU launch of this process publish its exchange granules write-through
 * (agent scope) instead of L2-resident on one XCD -- the fast form depends on gfx950 cache behaviour (SPX partition mode,
 * MTYPE_RW) beyond the HIP memory model; a stale granule can only show as a timeout.  Returns the previous setting. */
int tag_gru_disable_xcd_fast(void);
/* Debug query for tests and tools (host only, launches nothing): the recurrence form that the last successful tag_gru_forward
 * (backward = 0) / tag_gru_backward (backward != 0) of this process launched: 0 = none yet, 1 = one launch per step,
 * 2 = 16-row persistent, 3 = 4-row persistent.  Recorded after the launch succeeded: a refused cooperative launch that fell
 * back reports the fallback.
 * Hidden sizes (pinned by tests/test_gpu_gru_sweep.py): tag_gru_forward takes every H >= 16 with H % 16 == 0; tag_gru_backward
 * also needs (3 H) % 32 == 0, i.e. H % 32 == 0 -- H = 16, 48, 80, ... run forward (inference) and are REFUSED by backward with
 * TAG_EINVAL before anything is written, so a model of such a width cannot be trained. */
int tag_gru_last_form(int backward);

/* ---------------------------------------------------------------------------------------------
 * T3: row-local GRU recurrence of the text side, PyTorch gate order (r,z,n), h0 = 0, ALL L padded positions, one launch
 * per layer for every direction and step: RnnEncoder.forward, models/text_encoder.py:117-125
 * (``token_emb, h = self.rnn(x)`` :119 over the padded batch, ``mean_with_lens(token_emb, text_len)`` :123,
 * models/utils.py mean_with_lens).  Rows never interact: a workgroup owns 16 rows x all H units of one direction, h in
 * LDS, W_hh streamed from L2, exact fp32 MFMA; no cooperative launch, no flags, no atomics (two runs are bit-identical).
 * Any R >= 1, L >= 1, 1 <= H <= 512, dirs 1 | 2; anything else is TAG_EINVAL.
 *   gi       (R,L,dirs,3H): x W_ih^T + b_ih for all directions (a tag_gemm)
 *   w_hh     (dirs,3H,H), b_hh (dirs,3H)
 *   text_len (R) int64, nullable when seq_mean is
 *   y        (R,L,dirs*H) hidden states, direction d in [d*H, (d+1)*H)
 *   gates    (R,L,dirs,4H) nullable: r, z, n and h_{t-1} W_hn^T + b_hn, saved for the backward pass
 *   seq_mean (R,dirs*H) nullable: sum of y over t < min(text_len, L), divided by text_len (the last layer's seq_emb)
 * backward (reverse time order, same tiling):
 *   dy (R,L,dirs*H) nullable, dseq (R,dirs*H) nullable (not both): dL/dy, and dL/dseq_mean whose share dseq / text_len is
 *   added at the valid positions; y, gates: the forward's; outputs dgi, dgh (R,L,dirs,3H) and hprev (R,L,dirs,H) = h_{t-1},
 *   from which the caller forms dW_ih = dgi^T x, dW_hh = dgh^T hprev, the bias column sums and dx = dgi W_ih. */
int tag_text_gru_forward(const float* gi, const float* w_hh, const float* b_hh, const int64_t* text_len /* nullable */,
                         float* y, float* gates /* nullable */, float* seq_mean /* nullable */, int R, int L, int H, int dirs,
                         void* stream);
int tag_text_gru_backward(const float* dy /* nullable */, const float* dseq /* nullable */, const int64_t* text_len,
                          const float* y, const float* gates, const float* w_hh, float* dgi, float* dgh, float* hprev, int R,
                          int L, int H, int dirs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * T4: self-attention of the text side: SelfAttention.forward, models/text_encoder.py:261-268
 * (``cat(cls_token, x)`` :263, ``self.pe(x)`` :264 = + sinusoidal positions then dropout, ``self.mha(x, x, x, padding_mask)``
 * :267 with keys >= text_len + 1 masked).  The in- and out-projections are tag_gemm calls; tag_text_selfattn_* is the
 * scaled-dot-product core over the PACKED in-projection, tag_text_cls_pe_* builds the attention input.  Rows and heads
 * never interact: one wave owns a (row, head) pair, the S x S weights live in wave-private LDS, dq / dk / dv of the pair
 * are complete fixed-order sums; no partials, no workspace, no atomics (two runs are bit-identical).  Exact fp32 on the VALU.
 * R >= 1, 2 <= S <= 64, E <= 1024, head_dim = E/H in {16, 32} or a multiple of 64; anything else is TAG_EINVAL.
 *   qkv   (R,S,3E) [q|k|v] exactly as the in-projection GEMM leaves it; head h = channels [h*E/H, (h+1)*E/H) of each part
 *   klen  (R) int64 valid keys, 1 ... S (clamped into that range): keys >= klen get -inf before the softmax; queries are
 *         NOT masked (padded positions produce output, as in the reference); scale 1/sqrt(E/H)
 *   ctx   (R,S,E)
 *   attn  (R,H,S,S) nullable: the softmax weights BEFORE dropout (exactly 0 at keys >= klen), saved for the backward pass
 *   drop_p / seed: dropout on the weights, tag_keep(seed, flat index of (R,H,S,S)) -- what tag_dropout_mask materialises
 * backward: qkv, attn, dctx (R,S,E), klen -> dqkv (R,S,3E) packed the same way, every element written; the caller forms
 *   dW_in = dqkv^T x (one tag_gemm), db_in (one tag_colsum) and dx = dqkv W_in.
 * tag_text_cls_pe_forward:  x (R,L+1,E) = dropout([cls ; tok] + pe[:L+1]); tok (R,L,E), cls (E), pe (>= L+1 rows of E);
 *   keep mask = tag_keep(seed, flat index of (R,L+1,E)).
 * tag_text_cls_pe_backward: dx (R,L+1,E) through the same mask -> dtok (R,L,E) (nullable) and dcls_rows (R,E) (nullable),
 *   the gradient rows of the cls position, whose column sum (tag_colsum: fixed order, no atomics) is dcls (E).
 * ------------------------------------------------------------------------------------------- */
int tag_text_selfattn_forward(const float* qkv, const int64_t* klen, float* ctx, float* attn /* nullable */, int R, int S,
                              int E, int H, float drop_p, uint64_t seed, void* stream);
int tag_text_selfattn_backward(const float* qkv, const float* attn, const float* dctx, const int64_t* klen, float* dqkv,
                               int R, int S, int E, int H, float drop_p, uint64_t seed, void* stream);
int tag_text_cls_pe_forward(const float* tok, const float* cls, const float* pe, float* x, int R, int L, int E, float drop_p,
                            uint64_t seed, void* stream);
int tag_text_cls_pe_backward(const float* dx, float* dtok /* nullable */, float* dcls_rows /* nullable */, int R, int L,
                             int E, float drop_p, uint64_t seed, void* stream);

/* ---------------------------------------------------------------------------------------------
 * T5: intra-attention of the text side: IntraAttention.forward, models/text_encoder.py:206-237, with its ConvGRUCell
 * (:147-188).  Per layer: score = drop(x + pe) drop(x + pe)^T (two independent masks, UNSCALED), cells with query or key
 * >= text_len FILLED WITH 1e-10 (not -inf: they take part in the softmax), attn = softmax over all L cells,
 * message = attn @ x (x, not x + pe); then the cell on [message ; x].  The three gate products are tag_gemm calls.
 * Rows never interact: one workgroup owns a phrase, its L x L scores live in LDS, every output element is a complete
 * fixed-order sum; no partials, no workspace, no atomics (two runs are bit-identical).  Exact fp32 on the VALU.
 * R >= 1, 1 <= L <= 64, E even, 2 <= E <= 1024; anything else is TAG_EINVAL.  text_len (R) int64, clamped to [0, L].
 *   x (R,L,E), pe (>= L rows of E), message (R,L,E), attn (R,L,L) nullable: the softmax output, dead cells included
 *   drop_p / seed_a / seed_b: the two dropouts behind the positions, tag_keep(seed, flat index of (R,L,E)) scaled by
 *   1 / (1 - p) -- what tag_dropout_mask materialises; drop_p = 0 is the shared a == b path of eval mode
 * backward: dmessage (R,L,E), x, pe, attn, text_len -> dx (R,L,E) [+= when accumulate]: the attn-weighted path into x, the
 *   softmax backward, zero through dead cells, both dropout replays onto x.  pe is a buffer and has no gradient.
 * ConvGRUCell element-wise kernels (all tensors (M,E) = (R*L,E)):
 *   gates_forward:   u = sigmoid(u), r = sigmoid(r) in place, xr = x * r
 *   update_forward:  o = tanh(o) in place, xnew = x (1 - u) + o u; seq_mean (R,E) nullable: sum of xnew over
 *                    t < min(text_len, L) divided by text_len (0/0 for an empty phrase, like tag_embed_mean_forward)
 *   update_backward: g = dnew (nullable) + [t < text_len] dseq (nullable; at least one) / text_len ->
 *                    do_pre = g u (1 - o^2), du_pre = g (o - x) u (1 - u), dx = g (1 - u)
 *   gates_backward:  dxr (= do_pre W_o[:, E:]) -> dr_pre = dxr x r (1 - r), dx += dxr r
 * ------------------------------------------------------------------------------------------- */
int tag_text_intra_forward(const float* x, const float* pe, const int64_t* text_len, float* message, float* attn /* nullable */,
                           int R, int L, int E, float drop_p, uint64_t seed_a, uint64_t seed_b, void* stream);
int tag_text_intra_backward(const float* dmessage, const float* x, const float* pe, const float* attn, const int64_t* text_len,
                            float* dx, int accumulate, int R, int L, int E, float drop_p, uint64_t seed_a, uint64_t seed_b,
                            void* stream);
int tag_convgru_gates_forward(float* u, float* r, const float* x, float* xr, long M, int E, void* stream);
int tag_convgru_update_forward(float* o, const float* u, const float* x, float* xnew, const int64_t* text_len /* nullable */,
                               float* seq_mean /* nullable */, int R, int L, int E, void* stream);
int tag_convgru_update_backward(const float* dnew /* nullable */, const float* dseq /* nullable */, const int64_t* text_len,
                                const float* x, const float* u, const float* o, float* do_pre, float* du_pre, float* dx, int R,
                                int L, int E, void* stream);
int tag_convgru_gates_backward(const float* dxr, const float* x, const float* r, float* dr_pre, float* dx, long M, int E,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * T6: the TRAINING path of the LAION-CLAP text tower: LaionClapEncoder, models/text_encoder.py:311-327 = Hugging Face
 * ClapTextModel + ClapProjectionLayer (transformers models/clap/modeling_clap.py).  The dense layers are tag_gemm calls, the
 * attention core is tag_text_selfattn_*; text_clap.hip holds the row kernels in between with their backward.  fp32, one wave
 * per row, no atomics; sums over rows are per-wave partial rows (rows in a fixed stride) folded by tag_colsum and the table
 * gradients are a first-occurrence gather like tag_embed_tokens_backward's: two runs are bit-identical.  1 <= D <= 1024, rows >= 1;
 * anything else (and a null pointer that is not marked nullable) is TAG_EINVAL before any launch.  Rows need 4-byte alignment
 * only; 16-byte accesses are used when D % 4 == 0 and every base is 16-byte aligned (same bits).
 * resln_forward (ClapTextSelfOutput / ClapTextOutput: LayerNorm(dropout(dense(x)) + input)):
 *   y = LayerNorm(x + res) * gamma + beta, res nullable; xhat (rows,D) and rstd (rows), both or neither: the normalised row
 *   and 1 / sqrt(var + eps), what the backward reads (x-hat is never recovered by dividing by gamma).
 * resln_backward: dy, xhat, rstd, gamma -> ds (rows,D) = the gradient of x AND of res; dgamma, dbeta (D) nullable (a frozen
 *   LayerNorm); ws >= tag_text_clap_resln_backward_ws_bytes when either is asked for.
 * embed_forward (ClapTextEmbeddings): tag_roberta_embed_ln's arithmetic -- position id = cumsum(ids != pad) * (ids != pad)
 *   + pad, h = LayerNorm(word[ids] + type[0] + pos[position id]) -- and pos_ids (B*L) int64 (nullable), xhat, rstd as above.
 *   P rows in the position table, P > L + pad_id; an id outside [0,V) reads nothing (tag_embed_check_ids raises the flag).
 * embed_backward: dh (B*L,D) -> dword (V,D) and dpos (P,D), ACCUMULATED into caller-zeroed tables like
 *   tag_embed_tokens_backward (repeated ids summed in a fixed order, the first occurrence owns the table row); pad tokens are
 *   skipped, so row pad_id of both is not touched and stays exactly zero (nn.Embedding(padding_idx = pad_token_id) on both); dtype0 (D) = the column sum over ALL B*L rows; dgamma, dbeta.
 *   Every output is nullable (at least one is asked for).  ws >= tag_text_clap_embed_backward_ws_bytes.
 * gelu_forward (ClapTextIntermediate, ACT2FN["gelu"]): f = u Phi(u), Phi by erf; gelu_backward: du = df (Phi(u) + u phi(u)).
 * tanh_backward (ClapTextPooler): dx = dy (1 - y^2).  Any n >= 1; out must not alias an input.
 * ------------------------------------------------------------------------------------------- */
int tag_text_clap_resln_forward(const float* x, const float* res /* nullable */, const float* gamma, const float* beta, float eps,
                                float* y, float* xhat /* nullable */, float* rstd /* nullable */, long rows, int D, void* stream);
size_t tag_text_clap_resln_backward_ws_bytes(long rows, int D);
int tag_text_clap_resln_backward(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* ds,
                                 float* dgamma /* nullable */, float* dbeta /* nullable */, long rows, int D, void* ws,
                                 void* stream);
int tag_text_clap_embed_forward(const int64_t* ids, const float* word, const float* type0, const float* pos, const float* gamma,
                                const float* beta, float eps, float* h, int64_t* pos_ids /* nullable */, float* xhat /* nullable */,
                                float* rstd /* nullable */, int B, int L, int D, int V, int P, int pad_id, void* stream);
size_t tag_text_clap_embed_backward_ws_bytes(int B, int L, int D);
int tag_text_clap_embed_backward(const float* dh, const float* xhat, const float* rstd, const float* gamma, const int64_t* ids,
                                 const int64_t* pos_ids, float* dword, float* dpos, float* dtype0, float* dgamma, float* dbeta,
                                 int B, int L, int D, int V, int P, int pad_id, void* ws, void* stream);
int tag_text_clap_gelu_forward(const float* u, float* f, long n, void* stream);
int tag_text_clap_gelu_backward(const float* u, const float* df, float* du, long n, void* stream);
int tag_text_clap_tanh_backward(const float* y, const float* dy, float* dx, long n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * T7: BERT (models/text_encoder.py:271-308 Bert / SentenceBert over Hugging Face's BertModel): the encoder stack is the one of
 * T6; text_bert.hip holds BertEmbeddings and the sentence poolings, each with its backward.  Same conventions as T6: fp32, one
 * wave per row, 1 <= D <= 1024, no atomics, two runs bit-identical, TAG_EINVAL before any launch for anything else.
 * embed_forward: h[b,l] = LayerNorm(word[ids[b,l]] + type[type_ids[b,l]] + pos[l]) gamma + beta; the position of a token is its
 *   column l (pads included), L <= P.  T >= 1 (the backward serves T <= 16 only: a trainable model keeps to that).  type_ids
 *   nullable (all zeros); a type id outside [0,T) is clamped, a token id outside
 *   [0,V) reads nothing (tag_embed_check_ids raises the flag for either).  xhat (B*L,D), rstd (B*L): both or neither.
 * embed_backward: dh (B*L,D) -> dword (V,D) ACCUMULATED into a caller-zeroed table by the first-occurrence gather of T6 (tokens
 *   equal to pad_id skipped: row pad_id stays exactly zero; pad_id < 0: no padding index); dpos rows [0,L) WRITTEN with
 *   sum_b ds[b,l], rows >= L not touched; dtype (T,D) WRITTEN with the sums of the rows of each type id (T <= 16); dgamma, dbeta.
 *   Padded positions contribute to dpos and dtype.  Every output nullable (at least one asked for).
 * pool_forward: h (R,L,D), klen (R) int64 (read by mode 1 only, clamped to [0,L]).  mode 0: x = h[r,0]; mode 1: x =
 *   sum_{l<klen} h[r,l] / max(klen, 1e-9) (klen = 0: a zero row).  norm 0: out = x; 1: x / max(|x|, 1e-12); 2: x / (|x| + 1e-7)
 *   clipped to +-1e3 (forward only).  raw (R,D) nullable receives x.
 * pool_backward: dh (R,L,D) = dtok (nullable: zeros) + the pooling's gradient of dseq (nullable) on row 0 / the first klen rows,
 *   through the F.normalize backward for norm 1 (raw = the forward's x).  norm in {0, 1}.  dh must not alias an input.
 * ------------------------------------------------------------------------------------------- */
int tag_text_bert_embed_forward(const int64_t* ids, const int64_t* type_ids /* nullable */, const float* word, const float* type,
                                const float* pos, const float* gamma, const float* beta, float eps, float* h,
                                float* xhat /* nullable */, float* rstd /* nullable */, int B, int L, int D, int V, int T, int P,
                                void* stream);
size_t tag_text_bert_embed_backward_ws_bytes(int B, int L, int D, int T);
int tag_text_bert_embed_backward(const float* dh, const float* xhat, const float* rstd, const float* gamma, const int64_t* ids,
                                 const int64_t* type_ids /* nullable */, float* dword, float* dtype, float* dpos, float* dgamma,
                                 float* dbeta, int B, int L, int D, int V, int T, int P, int pad_id, void* ws, void* stream);
int tag_text_bert_pool_forward(const float* h, const int64_t* klen, int mode, int norm, float* raw /* nullable */, float* out,
                               long R, int L, int D, void* stream);
int tag_text_bert_pool_backward(const float* dseq /* nullable */, const float* dtok /* nullable */, const float* raw,
                                const int64_t* klen, int mode, int norm, float* dh, long R, int L, int D, void* stream);

/* ---------------------------------------------------------------------------------------------
 * T1 + T2: nn.Embedding gather + mean over valid tokens
 * models/text_encoder.py:39-43,79-88; models/utils.py:33-58.
 * text (B,L) int64, text_len (B) int64, table (V,D); token_emb (B,L,D) nullable; seq_emb (B,D).
 * backward accumulates into dtable (V,D), which the caller zero-fills; it is DETERMINISTIC (no atomics: the
 * first occurrence of a token id owns its table row and sums all occurrences in a fixed order).
 * nn.Embedding raises on ids outside [0,V): tag_embed_check_ids sets *err_flag (device int, sticky, caller-zeroed)
 * to 1 when any id is out of range -- the host reads it at its next synchronisation; the gather/scatter kernels
 * clamp (forward) or skip (backward) such ids so that nothing is read or written out of bounds.
 * ------------------------------------------------------------------------------------------- */
int tag_embed_check_ids(const int64_t* text, long n, int V, int* err_flag, void* stream);
int tag_embed_mean_forward(const int64_t* text, const int64_t* text_len, const float* table,
                           float* token_emb, float* seq_emb, int B, int L, int D, int V, void* stream);
int tag_embed_mean_backward(const float* dseq, const int64_t* text, const int64_t* text_len,
                            float* dtable, int B, int L, int D, int V, void* stream);

/* ---------------------------------------------------------------------------------------------
 * M1 / M2: frame x phrase heads, text_level 'seq'   models/match.py:16-33 (ExpNegL2), :43-60 (DotProduct)
 * kind 0: sigmoid(a.t [/sqrt(D)]).clamp(1e-7,1)   kind 1: exp(-||a - t||)   (l2norm: normalise both first)
 * audio (B,T,D), text (B,D) -> sim (B,T).  backward -> daudio (B,T,D), dtext (B,D).
 * ------------------------------------------------------------------------------------------- */
int tag_match_forward(const float* audio, const float* text, float* sim, int kind, int l2norm,
                      int scale, int B, int T, int D, void* stream);
int tag_match_backward(const float* audio, const float* text, const float* sim, const float* dsim,
                       float* daudio, float* dtext, int kind, int l2norm, int scale, int B, int T,
                       int D, void* stream);

/* M3: align.DotProduct models/align.py:14-31: audio (B,T,D), text (B,N,D) -> (B,B,T,N) */
int tag_align_dot_forward(const float* audio, const float* text, float* out, int l2norm, int scaled,
                          int B, int T, int N, int D, float* ws /* (B*T + B*N)*D floats when l2norm */,
                          void* stream);
/* backward pieces of M3 (composed by the host with two tag_gemm calls: daudio = ds x text, dtext = ds^T x audio):
 * ds (B*T, B*N) = dout * p(1-p) * [1/sqrt(D)] through the clamp; F.normalize forward / backward on rows */
int tag_align_dot_dscore(const float* out, const float* dout, float* ds, int scaled, int B, int T, int N,
                         int D, void* stream);
int tag_l2norm_rows_forward(const float* x, float* y, long rows, int D, void* stream);
int tag_l2norm_rows_backward(const float* x, const float* du, float* dx, long rows, int D, void* stream);

/* align.ExpNegL2 models/align.py:34-64 (align.hip): out[a][i][t][j] = exp(-||an[a,t,:] - tn[i,j,:]||), (B,B,T,N) as
 * tag_align_dot_forward.  an (B,T,D), tn (B,N,D) are the rows ALREADY normalised by tag_align_expnegl2_normalize
 * (y = x / max(||x||, 1e-12): a quotient, where tag_l2norm_rows_forward multiplies by the reciprocal -- exact unit rows at D = 1
 * and for rows that are multiples of each other).  The distance is the sum of squared differences (VALU tiles, no 2 - 2 cos).
 * The backward recomputes the distances, leaves g = -dout * out / dist (0 where dist == 0) for every pair in ws
 * (tag_align_expnegl2_ws_bytes: B*T*B*N floats, then the per-slice sums of a pass whose summed rows are cut over several
 * workgroups, folded in slice order) and writes dan = sum_pairs g (an - tn), dtn = -sum_pairs g (an - tn) -- gradients with
 * respect to the NORMALISED rows; the caller applies tag_align_expnegl2_normalize_backward (x the raw rows, u the unit rows:
 * dx = (du - u (u . du)) / ||x||).  Fixed summation order, no atomics.  Any B, T, N, D >= 1 with B*T <= 2^31 - 1,
 * B*N <= 65535 * 64 and D <= 65535 * 64; anything else is TAG_EINVAL before any launch, the limit named in tag_last_error. */
int tag_align_expnegl2_normalize(const float* x, float* y, long rows, int D, void* stream);
int tag_align_expnegl2_normalize_backward(const float* x, const float* u, const float* du, float* dx, long rows, int D,
                                          void* stream);
size_t tag_align_expnegl2_ws_bytes(int B, int T, int N, int D);
int tag_align_expnegl2_forward(const float* an, const float* tn, float* out, int B, int T, int N, int D, void* stream);
int tag_align_expnegl2_backward(const float* an, const float* tn, const float* dout, float* dan, float* dtn, int B, int T,
                                int N, int D, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * R1 + L1: FrameBceLoss losses.py:12-24 after the label alignment of run_strong.py:107-118.
 * sim (B, >=Tt) row stride ld_sim, label (B, >=Tt) row stride ld_label, length (B) int64 (unclamped:
 * clamped to [1,Tt] inside).  loss: 1 float.  backward: dsim (B,ld_sim) zero outside the mask.
 * ------------------------------------------------------------------------------------------- */
int tag_frame_bce_forward(const float* sim, int ld_sim, const float* label, int ld_label,
                          const int64_t* length, int B, int Tt, float* loss, void* stream);
int tag_frame_bce_backward(const float* sim, int ld_sim, const float* label, int ld_label,
                           const int64_t* length, int B, int Tt, const float* dloss, float* dsim,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * P1: post-processing utils/eval_util.py:18-116 driven as in run_strong.py:203-252:
 * binarize (strict >, float64 compare) -> median filter (window, scipy 'reflect') -> connect
 * clusters (gap <= n_connect) -> contiguous regions.  One (clip, threshold) pair per thread.
 * sim (B,T) ld; thresholds (NT) double; regions (B,NT,max_regions,2) int64 rows [onset, offset);
 * counts (B,NT) int32.
 * ------------------------------------------------------------------------------------------- */
int tag_segments(const float* sim, int ld, int B, int T, const double* thresholds, int NT, int window,
                 int n_connect, int64_t* regions, int32_t* counts, int max_regions, void* stream);

/* ---------------------------------------------------------------------------------------------
 * P1 with a double threshold (sed_eval.hip; utils/sed_utils.py:145-198 _double_threshold(..., return_arr=False)): the
 * contiguous runs of x > low[i] that hold a frame with x > high[i], THEN connect_ (gap <= n_connect) -- a run without a high
 * frame is dropped before the connection and does not bridge its neighbours.  One (clip, operating point) pair per thread.
 * sim (B,T) ld; high, low (NT) double, one operating point per entry, high[i] >= low[i] (the caller's duty: the wrapper
 * refuses other pairs); regions, counts, max_regions >= (T + 1) / 2 exactly as tag_segments writes them, so every consumer of
 * its outputs takes these unchanged.
 * COMPARISON PRECISION DIFFERS FROM tag_segments: the reference compares the float32 scores with a Python float here, which
 * numpy rounds to float32 (np.float32(0.3) > 0.3 is False), so both comparisons are fp32 against (float)high[i] and
 * (float)low[i]; tag_segments follows run_strong.py, whose np.float64 thresholds promote the scores, and compares in fp64.
 * TAG_EINVAL before any launch: a null pointer, B, T or NT < 1, ld < T, B * NT above 2^31 - 65, n_connect < 0, max_regions
 * below (T + 1) / 2.
 * ------------------------------------------------------------------------------------------- */
int tag_segments_double(const float* sim, int ld, int B, int T, const double* high, const double* low, int NT, int n_connect,
                        int64_t* regions, int32_t* counts, int max_regions, void* stream);

/* ---------------------------------------------------------------------------------------------
 * O1: clip_grad_norm_ + Adam on a flat fp32 buffer (run_strong.py:143-145; torch.optim.Adam).
 * tag_sumsq: out[0] (double) = sum g^2 (zero-filled by the call).  tag_adam_step reads the squared
 * norm from device memory: coef = min(1, max_norm / (sqrt(gnorm_sq) + 1e-6)); max_norm <= 0 disables.
 * grad_scale multiplies g first (1/world_size for DP averaging).  A non-finite squared norm makes tag_adam_step a
 * no-op (parameters and moments untouched): one poisoned step cannot destroy the optimiser state.
 * ------------------------------------------------------------------------------------------- */
size_t tag_sumsq_ws_bytes(long n);
int tag_sumsq(const float* g, long n, double* out, void* ws, void* stream);
int tag_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                  float beta2, float eps, int step, const double* gnorm_sq, float max_norm,
                  float grad_scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Inference path, text tower (next row of the scope table: models/hf_modeling_grounding.py:183-199 LaionClapEncoder =
 * Hugging Face ClapTextModel + ClapProjectionLayer, RoBERTa-style post-LayerNorm encoder), forward only.  Dense
 * layers are tag_gemm calls (bias + GELU / tanh / ReLU epilogues); these are the row kernels in between.
 * ------------------------------------------------------------------------------------------- */
/* out[b,l,:] = LayerNorm(word[ids] + type0 + pos[position_id]), position_id = cumsum(ids != pad)*(ids != pad) + pad */
int tag_roberta_embed_ln(const long* ids /*(B,L)*/, const float* word, const float* type0, const float* pos,
                         const float* gamma, const float* beta, float eps, float* out /*(B*L,D)*/, int B, int L,
                         int D, int pad_id, void* stream);
/* out = LayerNorm(x + res) * gamma + beta over rows of D (res nullable) */
int tag_add_layernorm(const float* x, const float* res, const float* gamma, const float* beta, float eps,
                      float* out, long rows, int D, void* stream);
/* softmax(q k^T / sqrt(dh) + key mask) v per (sequence, head); qkv (B*L, 3*heads*dh) = [q|k|v]; L <= 64;
 * dh in {16,32,64}; mask (B,L) int64 (0 = padded key; a key is valid wherever the mask is non-zero, holes included).
 * A sequence whose mask is all zero is a softmax over no key: every output of THAT sequence is NaN (0 * 1/0), the other
 * sequences of the batch are untouched. */
int tag_mha_small(const float* qkv, const long* mask, float* out /*(B*L, heads*dh)*/, int B, int L, int heads,
                  int dh, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BASELINE configs[3]: cross-encoder (models/cross_encoder.py:5-79) + token-level DotProduct (models/match.py:43-60).
 * Seq2SeqAttention's Linear over the concatenation [query ; kv] is applied as two tag_gemm calls
 * (aq = query Wq^T (B,T,Da), ak = kv Wk^T + b (B,L,Da)); these entries do the rest.  L <= 32 tokens.
 * ------------------------------------------------------------------------------------------- */
/* score = v . tanh(aq[b,q] + ak[b,k]); rows q >= qlen[b] and columns k >= klen[b] filled with -1e10; attn = softmax_k;
 * ctx = attn @ kv (B,T,Dk).  qlen[b] > T / klen[b] > L fill nothing.  A fully filled row (q >= qlen[b], or klen[b] = 0) is the
 * uniform 1/L over ALL L tokens, padding included (the reference's masked_fill, not -inf), and passes no score gradient.
 * Forward takes any Da, Dk > 0; backward holds a row in registers and refuses Da or Dk > 1024. */
int tag_addattn_forward(const float* aq, const float* ak, const float* v, const float* kv /*(B,L,Dk)*/,
                        const long* qlen, const long* klen, float* attn /*(B,T,L)*/, float* ctx, int B, int T, int L,
                        int Da, int Dk, void* stream);
size_t tag_addattn_backward_ws_bytes(int B, int T, int L, int Da, int Dk);
/* given dctx: daq (B,T,Da), dak (B,L,Da), dkv (B,L,Dk) (the attn @ kv term only), dv (Da); deterministic */
int tag_addattn_backward(const float* aq, const float* ak, const float* v, const float* kv, const float* attn,
                         const float* dctx, const long* qlen, const long* klen, float* daq, float* dak, float* dkv,
                         float* dv, int B, int T, int L, int Da, int Dk, void* ws, void* stream);
/* CrossGating pieces (models/cross_encoder.py:51-57): out = a * b; backward of out = x * g, g = sigmoid(z):
 * dx (+)= dout * g, dz = dout * x * g * (1 - g).  n % 4 == 0 */
int tag_mul(const float* a, const float* b, float* out, long n, void* stream);
int tag_gate_backward(const float* dout, const float* x, const float* g, float* dx, int accumulate, float* dz, long n,
                      void* stream);
/* DotProduct with text_level="token" after a cross-encoder: sim[r] = sigmoid(a[r].b[r] [/sqrt(D)]).clamp(1e-7, 1).
 * Same arithmetic in the same order as tag_rowpair_* with kind 0 and no l2norm: the two agree bit for bit. */
int tag_rowdot_sigmoid_forward(const float* a, const float* b, float* sim, long rows, int D, int scale, void* stream);
int tag_rowdot_sigmoid_backward(const float* a, const float* b, const float* dsim, float* da, float* db, long rows,
                                int D, int scale, void* stream);
/* Both heads with text_level="token" in general (models/match.py:16-33, 43-60): rows r = (clip, frame), one text vector per
 * frame.  kind 0 = DotProduct (sigmoid(u.w [/sqrt(D)]).clamp(1e-7,1)), kind 1 = ExpNegL2 (exp(-||u - w||)); l2norm:
 * u = a/max(||a||,1e-12), w likewise (F.normalize). */
int tag_rowpair_forward(const float* a, const float* b, float* sim, long rows, int D, int kind, int l2norm, int scale,
                        void* stream);
int tag_rowpair_backward(const float* a, const float* b, const float* dsim, float* da, float* db, long rows, int D,
                         int kind, int l2norm, int scale, void* stream);
/* dtable[text[b,l]] += dtok[b,l,:] (token_emb gradient of EmbeddingLayer, models/text_encoder.py:37-43) */
int tag_embed_tokens_backward(const float* dtok, const long* text, float* dtable, int B, int L, int D, int V,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * AudioTextCrossAlignByPhrase (models/audio_text_model.py:979-1073): the cross-encoder above and the token-level DotProduct
 * over ALL pairs (clip i, phrase p) of a batch.  a (B,T,D) audio with alen (B); w (P,L,D) tokens with wlen (P); pnum (B) phrases
 * per clip, a HOST array with entries >= 0 and sum P (clip j owns phrases off[j] .. off[j] + pnum[j] - 1, off = its exclusive
 * prefix sum); N >= max(pnum).  The caller projects with tag_gemm first: aq = a Wq^T, gu = sigmoid(a Wu^T + b_u) (B,T,D),
 * ak = w Wk^T + b_h, ws_tok = w Ws^T (P,L,D) -- fc_s(attn @ tok) = attn @ (tok Ws^T) + b_s because the weights sum to 1.  Per
 * row (i,p,t): the scores, mask fills, softmax over all L slots and the fully-filled-row convention of tag_addattn_*,
 * c = alpha @ w[p], z = alpha @ ws_tok[p] + b_s, u = a[i,t] * sigmoid(z), s = c * gu[i,t], then the arithmetic and clamp
 * gradient of tag_rowdot_sigmoid_*.  Nothing of B*P*T*D elements exists; every sum over pairs has one fixed order (no atomics),
 * so two calls agree bit for bit.
 * Limits (TAG_EINVAL with a tag_last_error message otherwise): L <= 32; D a multiple of 32, D <= 1024; pnum as above.
 * ------------------------------------------------------------------------------------------- */
/* bytes of everything a forward keeps for its backward (aq, gu, ak, ws_tok, alpha, dyfac), the forward's simp and the backward's
 * workspace; 0 with a tag_last_error message for a shape that is not served */
size_t tag_crosspairs_ws_bytes(int B, int T, int P, int L, int D);
size_t tag_crosspairs_backward_ws_bytes(int B, int T, int P, int L, int D);
/* sim (B,B,N,T) with sim[i,j,n,t] = the score of clip i, frame t against phrase n of clip j, 0 where n >= pnum[j];
 * alpha (B,P,T,L) and dyfac (B,P,T) are kept for the backward; simp (B,P,T) is scratch */
int tag_crosspairs_forward(const float* a, const float* aq, const float* gu, const float* w, const float* ak,
                           const float* ws_tok, const float* v, const float* b_s, const long* alen, const long* wlen,
                           const long* pnum_host, float* sim, float* alpha, float* dyfac, float* simp, int B, int T, int P,
                           int L, int D, int N, int scale, void* stream);
/* from dsim (B,B,N,T): daq, da (the term through u only), dgu (B,T,D); dak, dw (the term through c only), dws (P,L,D);
 * dv, db_s (D).  Entries of dsim with n >= pnum[j] are not read.  The frame side and the token side are separate kernels that
 * each recompute the tanh; dscore (B,P,T,L) is formed once, in ws, between them. */
int tag_crosspairs_backward(const float* a, const float* aq, const float* gu, const float* w, const float* ak,
                            const float* ws_tok, const float* v, const float* b_s, const long* alen, const long* wlen,
                            const long* pnum_host, const float* alpha, const float* dyfac, const float* dsim, float* daq,
                            float* da, float* dgu, float* dak, float* dw, float* dws, float* dv, float* db_s, int B, int T,
                            int P, int L, int D, int N, void* ws, void* stream);
/* g = sigmoid(z): dz = dg * g * (1 - g) (dgu of tag_crosspairs_backward -> the fc_u pre-activation); dz may be dg */
int tag_sigmoid_backward(const float* dg, const float* g, float* dz, long n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weak supervision (next row of the scope table): MultiTextBiEncoder (models/audio_text_model.py:101-229) -- N phrases
 * per clip scored against the SAME audio embedding (no (B*N,T,D) expansion), pooled by linear_softmax_with_lens
 * (models/utils.py:75-76); ClipBceLoss (losses.py:38-43) is tag_frame_bce_* over the (B,N) clip matrix.
 * ------------------------------------------------------------------------------------------- */
/* sim[(b*N+n), t] = sigmoid(audio[b,t] . text[b*N+n] [/sqrt(D)]).clamp(1e-7,1);  N <= 16 in backward */
int tag_match_group_forward(const float* audio /*(B,T,D)*/, const float* text /*(B*N,D)*/, float* sim /*(B*N,T)*/,
                            int scale, int B, int N, int T, int D, void* stream);
int tag_match_group_backward(const float* audio, const float* text, const float* dsim, float* daudio /*(B,T,D)*/,
                             float* dtext /*(B*N,D)*/, int scale, int B, int N, int T, int D, void* stream);
/* clip[r] = sum_{t<len} f^2 / sum_{t<len} f over rows of frame probabilities (rows, T); len = length[r / group] */
int tag_linear_softmax_pool_forward(const float* fs, const long* length, float* clip, long rows, int T, int group,
                                    void* stream);
int tag_linear_softmax_pool_backward(const float* fs, const long* length, const float* dclip, float* dfs, long rows,
                                     int T, int group, void* stream);

/* align-by-phrase (models/audio_text_model.py:907-976): sim_pooling.AudioMeanTextMean over the (B,B,T,N) matrix of
 * tag_align_dot_forward (models/sim_pooling.py:6-22) and MaxMarginRankingLoss(fix_norm=True) (losses.py:226-264) */
int tag_meanmean_pool_forward(const float* sim, const long* audio_len, const long* text_len, float* out /*(B,B)*/, int B,
                              int T, int N, void* stream);
int tag_meanmean_pool_backward(const float* dout, const long* audio_len, const long* text_len, float* dsim, int B, int T,
                               int N, void* stream);
/* fix_norm != 0 (the reference's default): mean over the 2 n (n-1) off-diagonal pairs; 0: the diagonal pairs stay in
 * (losses.py:249-264) */
int tag_maxmargin_forward(const float* x /*(n,n)*/, int n, float margin, float lamda1, int fix_norm, float* loss,
                          void* stream);
int tag_maxmargin_backward(const float* x, int n, float margin, float lamda1, int fix_norm, const float* dloss, float* dx,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * EmbeddingAgg(aggregation="attention") = AttentionPooling, models/text_encoder.py:46-58,79-86: x (B,L,D) token embeddings,
 * lens (B), fc.weight w (D), fc.bias (1) -> weight (B,L) softmax over the valid tokens (-1e10 fill), out (B,D).
 * backward: dx (B,L,D) (to be ADDED to any other gradient of the tokens by the caller), gw (B,D) / gb (B) = per-phrase terms
 * of d fc.weight / d fc.bias (fold with tag_colsum).
 * BiEncoder(upsample=True), models/audio_text_model.py:90-97: F.interpolate(mode="linear", align_corners=False) of the
 * frame scores x (R,T) -> (R, T*ratio); backward gathers (no atomics).
 * ------------------------------------------------------------------------------------------- */
int tag_attnpool_forward(const float* x, const long* lens, const float* w, const float* bias, float* weight, float* out,
                         int B, int L, int D, void* stream);
int tag_attnpool_backward(const float* x, const float* w, const float* weight, const float* dout, float* dx, float* gw,
                          float* gb, int B, int L, int D, void* stream);
int tag_upsample_linear_forward(const float* x, float* out, long R, int T, int ratio, void* stream);
int tag_upsample_linear_backward(const float* dout, float* dx, long R, int T, int ratio, void* stream);
/* MultiTextBiEncoder with a cross-encoder (models/audio_text_model.py:165-168, audio_emb.unsqueeze(1).expand(-1, text_num,
 * -1, -1).reshape): out[(b*N + n)][0..R) = x[b][0..R); backward = sum over the N copies in ascending order. */
int tag_group_expand_forward(const float* x, float* out, long B, int N, long R, void* stream);
int tag_group_expand_backward(const float* dout, float* dx, long B, int N, long R, void* stream);

/* ---------------------------------------------------------------------------------------------
 * General similarity pooling: models/utils.py:22-105 (mean/max/linear_softmax/exp_softmax _with_lens), all twelve reducers
 * of models/sim_pooling.py:6-204 and the pooling modes of MultiTextBiEncoder (models/audio_text_model.py:205-215).
 * sim (R,T,N) fp32, T frames, N tokens/phrases innermost; alen indexed by r / a_div, tlen by r % t_mod.
 * amode (frames < alen): 0 mean, 1 max (first maximum), 2 linear softmax sum f^2 / sum f, 3 exp softmax sum softmax(f) f.
 * tmode (tokens < tlen): 0 mean, 1 sum, 2 max (first), 3 mean + sum; -1 = none: out is (R,N), else (R).
 * backward writes the whole dsim (R,T,N) (zeros outside the valid region).
 * ------------------------------------------------------------------------------------------- */
int tag_sim_pool_forward(const float* sim, const long* alen, const long* tlen /* nullable iff tmode < 0 */, float* out,
                         long R, int T, int N, int a_div, int t_mod, int amode, int tmode, void* stream);
int tag_sim_pool_backward(const float* sim, const long* alen, const long* tlen, const float* dout, float* dsim, long R,
                          int T, int N, int a_div, int t_mod, int amode, int tmode, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BASELINE configs[3], the head named in the config text: match.CrossAttention (models/match.py:63-88) =
 * nn.MultiheadAttention(embed_dim E, heads H, dropout p, batch_first, kdim = vdim = kvdim) of every audio frame over the
 * phrase tokens -> audio + dropout(out) -> LayerNorm(E) -> Linear(E,1) -> sigmoid.  The four projections are tag_gemm
 * calls; these entry points are the attention core and the fused residual/LayerNorm/head, forward and backward.
 *   q (B,T,E) projected frames; k, v (B,L,E) projected tokens (L <= 32); klen (B) int64 valid tokens (key_padding_mask);
 *   attn (B,T,H,L) softmax weights BEFORE dropout (saved for backward); ctx (B,T,E).  head_dim = E/H in {16, 32} or a
 *   multiple of 64, E <= 1024.  drop_p / seed: dropout on the attention weights (train), counter-based like A2.
 * backward: dq (B,T,E), dk, dv (B,L,E) (sums over frames folded from per-tile partials in a fixed order).
 *   klen[b] > L (up to INT_MAX) means L (nothing is masked), on the MFMA and on the VALU path alike.  klen[b] = 0 is a softmax over no token:
 *   forward writes NaN to attn of THAT clip and to its ctx (as nn.MultiheadAttention does; loud, not a silent 0; with dropout, a
 *   (frame, head) all of whose weights were dropped reads 0) and leaves the other clips untouched; backward reads no weight of
 *   such a clip and returns exact zeros for its dq, dk and dv.
 * tag_resln_head_*: x = audio, r = out_proj(ctx); sim (rows) = sigmoid(LayerNorm(x + dropout(r)) . w + b); mu / rstd (rows)
 * saved.  backward: dx, dr (rows,E) and the per-row terms gw = d logit * n, gg = dn * xhat, gb = dn, ds = d logit, whose
 * column sums (tag_colsum) are the gradients of linear.weight, norm.weight, norm.bias and linear.bias.
 * ------------------------------------------------------------------------------------------- */
int tag_mha_cross_forward(const float* q, const float* k, const float* v, const long* klen, float* attn, float* ctx,
                          int B, int T, int L, int E, int H, float drop_p, uint64_t seed, void* stream);
size_t tag_mha_cross_backward_ws_bytes(int B, int T, int L, int E);
int tag_mha_cross_backward(const float* q, const float* k, const float* v, const float* attn, const float* dctx,
                           const long* klen, float* dq, float* dk, float* dv, int B, int T, int L, int E, int H,
                           float drop_p, uint64_t seed, void* ws, void* stream);
int tag_resln_head_forward(const float* x, const float* r, const float* gamma, const float* beta, const float* w,
                           const float* bias, float* sim, float* mu, float* rstd, long rows, int E, float eps,
                           float drop_p, uint64_t seed, void* stream);
int tag_resln_head_backward(const float* x, const float* r, const float* gamma, const float* beta, const float* w,
                            const float* mu, const float* rstd, const float* sim, const float* dsim, float* dx, float* dr,
                            float* gw, float* gg, float* gb, float* ds, long rows, int E, float drop_p, uint64_t seed,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * BASELINE configs[2]: bf16 ACTIVATION STORAGE.  The big tensors of the conv stack -- raw conv outputs, pooled block
 * outputs and the gradients of both -- are bf16 in HBM (void* here: raw 16-bit patterns, channels-last as before);
 * every product is bf16 x bf16 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; BatchNorm statistics (from the fp32
 * accumulators / values before rounding), scale/shift, the per-channel gradient sums (fp64), weight gradients, the
 * GRU, the heads, the loss and the master weights stay fp32.  Outputs are rounded to nearest-even.  Same argument
 * meaning as the fp32 entry points of the same name (models/panns.py:46-62, models/audio_encoder.py:202-212).
 * tag_conv3x3_forward_x3_bf16 / tag_conv3x3_wgrad_x3_bf16 take the ONE-product weight pack
 * (tag_pack_conv_weight_x3(..., products = 1)).
 * ------------------------------------------------------------------------------------------- */
int tag_conv3x3_c1_forward_stats_bf16(const float* x, const float* col_scale, const float* col_shift, const float* w,
                                      void* y, float* stats /* nullable */, int B, int H, int W, int Cout, void* stream);
int tag_conv3x3_c1_backward_bf16(const float* x, const float* col_scale, const float* col_shift, const void* dy,
                                 const float* w, float* dw, float* dx, int B, int H, int W, int Cout, void* ws,
                                 void* stream);
int tag_conv3x3_c1_backward_bnrelu_bf16(const float* x, const float* col_scale, const float* col_shift, const void* da,
                                        const void* yref, const float* bn_scale, const float* bn_shift,
                                        const float* bn_mean, const float* bn_invstd, const float* gamma,
                                        const float* dgamma, const float* dbeta, int bn_train, const float* w, float* dw,
                                        float* dx, int B, int H, int W, int Cout, void* ws, void* stream);
int tag_conv3x3_forward_x3_bf16(const void* x, const void* wpack, int prologue, const float* in_scale,
                                const float* in_shift, void* y, float* stats, int B, int H, int W, int Cin, int Cout,
                                void* stream);
int tag_conv3x3_wgrad_x3_bf16(const void* x, int prologue, const float* in_scale, const float* in_shift, const void* dy,
                              float* dw, int B, int H, int W, int Cin, int Cout, void* ws, void* stream);
int tag_bnact_pool_forward_bf16(const void* y, const float* scale, const float* shift, void* out, int B, int H, int W,
                                int C, int ph, int pw, int act, int pool, float drop_p, uint64_t seed, void* stream);
int tag_bnrelu_pool_backward_bf16(const void* y, const float* scale, const float* shift, const float* mean,
                                  const float* invstd, const float* gamma, const void* dout, void* dy, float* dgamma,
                                  float* dbeta, int B, int H, int W, int C, int ph, int pw, int pool, float drop_p,
                                  uint64_t seed, int bn_train, void* ws, void* stream);
/* bf16 twins of tag_conv3x3_dgrad_bnsums / tag_bnrelu_backward_apply (BASELINE configs[2] mode): the sums are taken from the
 * fp32 accumulators of the dgrad conv before its output is rounded to bf16; bnpart rows [P][2][Cout],
 * P = tag_conv3x3_x3_bf16_stats_rows(B,H,W,Cin,Cout,0) (the row-streaming kernel writes one row per strip and wave M-group, not
 * one per tile: tag_conv3x3_x3_stats_rows is the count of the fp32 entry only).  Argument rules of tag_conv3x3_forward_x3_bf16. */
int tag_conv3x3_dgrad_bnsums_bf16(const void* dy, const void* wpack, void* da, const void* yref, const float* bn_scale,
                                  const float* bn_shift, const float* bn_mean, const float* bn_invstd, float* bnpart,
                                  int B, int H, int W, int Cin, int Cout, void* stream);
int tag_bnrelu_backward_apply_bf16(const void* y, const float* scale, const float* shift, const float* mean,
                                   const float* invstd, const float* gamma, const void* da, void* dy,
                                   const float* dgamma, const float* dbeta, long rows, int C, int bn_train, void* stream);
int tag_bnrelu_backward_bf16(const void* y, const float* scale, const float* shift, const float* mean,
                             const float* invstd, const float* gamma, const void* da, void* dy, float* dgamma,
                             float* dbeta, long rows, int C, int bn_train, void* ws, void* stream);
int tag_mean_w_forward_bf16(const void* x, long rows, int W, int C, float drop_p, uint64_t seed, float* out, void* stream);
int tag_mean_w_backward_bf16(const float* dout, long rows, int W, int C, float drop_p, uint64_t seed, void* dx,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * Early-fusion CrossCnn8_Rnn (models/audio_text_model.py:571-840): the text enters every conv layer as a per-(clip, channel)
 * bias between BatchNorm and ReLU, relu(bn(y) + bias[b, c]), and again at fc1 and after the GRU.  fp32, channels-last.
 * A reducing entry writes clip (B, 2, C) doubles, [b][sum a | sum b] of its two quantities over clip b, folded in a fixed order
 * from fp64 partial rows that never straddle two clips; the channel totals are folded from those (no atomics).
 * ws: tag_clip_reduce_ws_bytes(B, C) bytes.  The clips are the y dimension of the launch grid: every entry of this group but
 * tag_rowgroup_bias_relu and tag_frame_head_forward refuses B > 65535 with TAG_EINVAL before it launches anything.
 *   tag_bias_bnrelu_forward       out = relu(y*scale + shift + bias[b]) over (B, HW, C)
 *   tag_bias_bnrelu_pool_forward  tag_bnact_pool_forward (act 1; pool 0 avg+max | 2 avg | 3 max) with the bias
 *   tag_bias_bnrelu_pool_backward its backward: clip = [sum dz | sum dz*xhat], dbeta / dgamma their totals, dy
 *   tag_bias_bnrelu_backward      backward of tag_bias_bnrelu_forward; dt (B, C) or null = this site's clip sum dz + prev's
 *                                 slot 0 (prev: the clip sums of the block's other site, or null)
 *   tag_rowgroup_bias_relu        out = relu(x + bias[row / T]) over (B*T, N) (fc1 + fc1_text(e)); in place allowed
 *   tag_rowgroup_colsum           dgroup (B, N) = column sums of each group of T rows, dtotal (N) = their total
 *   tag_frame_head_forward        sig = sigmoid((y + rb[row / T]) . w + b0), prob = clamp(sig, 1e-7, 1) per row
 *   tag_frame_head_backward       dlogit = dprob*(1-sig)*sig where 1e-7 <= sig <= 1, else 0; dy = dlogit*w,
 *                                 dw = sum dlogit*(y + rb), dsum[n] = sum dlogit (= d b0), drb[b] = (sum_t dlogit)*w
 */
size_t tag_clip_reduce_ws_bytes(int B, int C);
int tag_bias_bnrelu_forward(const float* y, const float* scale, const float* shift, const float* bias, float* out, int B,
                            long HW, int C, void* stream);
int tag_bias_bnrelu_pool_forward(const float* y, const float* scale, const float* shift, const float* bias, float* out,
                                 int B, int H, int W, int C, int ph, int pw, int pool, float drop_p, uint64_t seed,
                                 void* stream);
int tag_bias_bnrelu_pool_backward(const float* y, const float* scale, const float* shift, const float* mean,
                                  const float* invstd, const float* gamma, const float* bias, const float* dout, float* dy,
                                  float* dgamma, float* dbeta, double* clip, int B, int H, int W, int C, int ph, int pw,
                                  int pool, float drop_p, uint64_t seed, int bn_train, void* ws, void* stream);
int tag_bias_bnrelu_backward(const float* y, const float* scale, const float* shift, const float* mean,
                             const float* invstd, const float* gamma, const float* bias, const float* da, float* dy,
                             float* dgamma, float* dbeta, double* clip, const double* prev, float* dt, int B, long HW,
                             int C, int bn_train, void* ws, void* stream);
int tag_rowgroup_bias_relu(const float* x, const float* bias, float* out, int B, int T, int N, void* stream);
int tag_rowgroup_colsum(const float* x, int B, int T, int N, float* dgroup, float* dtotal, double* clip, void* ws,
                        void* stream);
int tag_frame_head_forward(const float* y, const float* rb, const float* w, const float* b0, float* sig, float* prob, int B,
                           int T, int N, void* stream);
int tag_frame_head_backward(const float* y, const float* rb, const float* w, const float* sig, const float* dprob, float* dy,
                            float* dw, float* dsum, float* drb, double* clip, int B, int T, int N, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Early-fusion CrossCDur (models/audio_text_model.py:461-568): BatchNorm sits in FRONT of each conv and the text is added to the
 * RAW conv output, leaky(conv(bn(x)) + bias[b, c]), so the bias is one add in the conv kernel's epilogue and the forward has
 * no pass of its own for it.  fp32, channels-last; bias (B, Cout).  With an all-zero bias the output equals the unbiased
 * entry's bit for bit.  A shape without an instance returns TAG_EINVAL (tag_last_error names the entry), it is not launched.
 *   tag_conv3x3_forward_bias     y = conv(prologue(x)) + bias[b]: the halo-tile kernel (EPI == 4) at W 16 | 4, Cin 32 | 128,
 *                                Cout 128, prologue 2 (scale*leaky(x)+shift) | 3 (scale*x+shift); wpack of tag_pack_conv_weight
 *   tag_conv3x3_c1_forward_bias  the Cin = 1 conv (x (B,H,W), optional per-column affine) + bias[b]: W % 4 == 0, Cout / 4 a
 *                                divisor of 256; a workgroup may hold rows of two clips, the bias row is the pixel's own clip
 *   tag_leaky_forward / _backward  leaky_relu(z, 0.1) and dz = dout * (z > 0 ? 1 : 0.1) over n % 4 == 0 floats: the activation of a
 *                                CDurTextBlock used outside the model (inside it the pool pass / the next conv's prologue has it)
 * The gradient of the bias is the per-clip sum of dz, dt[b, c] = sum over (h, w) of dz[b, h, w, c]: emitted by the pass that
 * writes dz (below), or tag_rowgroup_colsum over dz viewed as (B, H*W, C) in a pass of its own.
 *   tag_lppool_leaky_backward_clip  tag_lppool_leaky_backward + dt (B, C); clip (B, 2, C) doubles (slot 0 = the sums),
 *                                ws: tag_clip_reduce_ws_bytes(B, C) bytes.  dy bit-identical to the plain entry's
 *   tag_bn_act_backward_clip     tag_bn_act_backward over x (B, HW, C) + dt (B, C) of dx; ws: tag_bn_backward_ws_bytes(B*HW, C),
 *                                ws_clip: tag_clip_reduce_ws_bytes(B, C).  dx, dgamma, dbeta bit-identical to the plain entry's
 * Both fold fp64 partial rows that never straddle two clips in a fixed order (no atomics): bitwise repeatable.
 * The frame head is tag_frame_head_forward / _backward at N = 256, the x4 upsampling tag_upsample_linear_*.
 */
int tag_conv3x3_forward_bias(const float* x, const float* wpack, int prologue, const float* in_scale, const float* in_shift,
                             const float* bias, float* y, int B, int H, int W, int Cin, int Cout, void* stream);
int tag_conv3x3_c1_forward_bias(const float* x, const float* col_scale, const float* col_shift, const float* w,
                                const float* bias, float* y, int B, int H, int W, int Cout, void* stream);
int tag_lppool_leaky_backward_clip(const float* y, const float* dout, float* dy, float* dt, double* clip, int B, int H, int W,
                                   int C, int ph, int pw, float drop_p, uint64_t seed, void* ws, void* stream);
int tag_bn_act_backward_clip(const float* x, int pre_op, const float* mean, const float* invstd, const float* gamma,
                             const float* du, float* dx, float* dgamma, float* dbeta, float* dt, double* clip, int B, long HW,
                             int C, int bn_train, void* ws, void* ws_clip, void* stream);
int tag_leaky_forward(const float* z, float* out, long n, void* stream);
int tag_leaky_backward(const float* z, const float* dout, float* dz, long n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The class-mapping baseline AudioTagging (models/audio_text_model.py:405-458): encoder -> fc_output -> sigmoid -> pooling
 * over time, trained with ClipBceLoss / MaskedFrameBceLoss / ClipMaskedFrameBceLoss (losses.py:38-43, 157-183).  The three
 * products of the head are tag_gemm (act 5 = sigmoid for logits -> prob) and the bias gradient is tag_colsum; the passes
 * below are fp32 on the native (B, T, C) layout, classes innermost, any C and T (rows need 4-byte alignment only): the lanes
 * of a wave run over the classes, workgroups over (clip, class tile[, frame slab]).  Sums over frames are folded in a fixed
 * order (no atomics): bitwise repeatable.  length: int64 (B); frames t >= min(length[b], T) are outside every reduction.
 *   tag_class_pool_forward        clip (B, C) = *_with_lens(prob, length) (models/utils.py:49-84); mode 0 mean | 1 max |
 *                                 2 linear_softmax sum p^2 / sum p | 3 exp_softmax sum e^p p / sum e^p (p in [0, 1]: no
 *                                 stabiliser, equal to the reference's max-subtracted form to rounding).  aux (B, C) is what
 *                                 the backward needs: 2: sum p; 3: sum e^p; 1: index of the FIRST maximum, as a float; 0: zero
 *   tag_tagging_head_backward     dlogit (B, T, C) = (dprob + dclip * d clip / d prob) * prob * (1 - prob) in one pass:
 *                                 the pooling term (0: 1 / len; 1: 1 at the stored index; 2: (2 p - clip) / sum p;
 *                                 3: e^p / sum e^p * (1 + p - clip)) is zero outside the valid frames.  dprob (B, ld_dprob, C)
 *                                 with ld_dprob >= T frames per clip, or null; dclip (B, C) or null; dlogit may BE dprob
 *                                 (then ld_dprob == T)
 *   tag_masked_frame_bce_forward  MaskedFrameBceLoss (losses.py:157-170): loss[0] = sum(bce * len_mask * cls_mask) /
 *                                 sum(len_mask * cls_mask) over the first Tt frames, len_mask from clamp(length, 1, Tt),
 *                                 cls_mask (B, C) or null = all ones (an all-zero mask gives the reference's 0 / 0).  BCE as
 *                                 tag_frame_bce_*: logs clamped at -100.  prob (B, ld_t, C), label (B, ld_label_t, C) with
 *                                 ld_t, ld_label_t >= Tt FRAMES PER CLIP (views truncated in time need no copy).  fp64
 *                                 partials, one per workgroup, folded in a fixed order
 *   tag_masked_frame_bce_backward dprob (B, Tt, C), contiguous: dloss[0] / den * cls_mask * (p - y) / max(p (1 - p), 1e-12),
 *                                 zero where masked
 *   ws of both: tag_masked_frame_bce_ws_bytes(B, Tt, C) bytes.
 */
int tag_class_pool_forward(const float* prob, const int64_t* length, float* clip, float* aux, int B, int T, int C, int mode,
                           void* stream);
int tag_tagging_head_backward(const float* prob, const float* dprob, const float* dclip, const float* clip, const float* aux,
                              const int64_t* length, float* dlogit, int B, int T, int C, int mode, int ld_dprob,
                              void* stream);
size_t tag_masked_frame_bce_ws_bytes(int B, int Tt, int C);
int tag_masked_frame_bce_forward(const float* prob, int ld_t, const float* label, int ld_label_t, const int64_t* length,
                                 const float* cls_mask, int B, int Tt, int C, float* loss, void* ws, void* stream);
int tag_masked_frame_bce_backward(const float* prob, int ld_t, const float* label, int ld_label_t, const int64_t* length,
                                  const float* cls_mask, int B, int Tt, int C, const float* dloss, float* dprob, void* ws,
                                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sentence-level contrastive objectives (contrastive.hip): fp32 in, fp32 out, cross-thread sums in fp64 in a fixed order,
 * no atomics (two runs give the same bits).  x (n,n) contiguous = the clip-versus-caption matrix "sim"; any n >= 1 (n = 1:
 * loss 0, gradient 0).  One forward and one backward launch for n <= 128; above that the forward is two launches.
 * ws: tag_contrastive_ws_bytes(n) bytes (n = B for MilNce), written by the forward and READ by the backward of the same
 * input -- the backward is one elementwise pass with no reduction of its own.
 *   tag_infonce_*   InfoNceLoss (losses.py:267): z = x / tau, loss = 1/2 [mean_i(LSE_j z_ij - z_ii) + mean_j(LSE_i z_ij - z_jj)];
 *                   ws holds the row and column log-sum-exp.  The maximum is subtracted before every exponential
 *   tag_triplet_*   mode 0 MaxTripletLoss (:285): (sum_i max_{j!=i} relu(m + x_ij - x_ii) + sum_j max_{i!=j} relu(m + x_ij -
 *                   x_jj)) / n; mode 1 WeightedTripletLoss (:355): a row of x or x^T with q = max off-diagonal, p = diagonal
 *                   and q + m > p adds clamp(0.2 p^2 - 0.7 p + 0.5, 0) + clamp(0.9 q^2 - 0.4 q + 0.03, 0), total / n.  ws holds
 *                   the row and column argmax of the RAW entries (exact ties: the lowest index), -1 where inactive.
 *                   mode 2 RandomTripletLoss (:319): s_index / a_index (n) device int32 drawn by the caller,
 *                   (sum_i relu(m + x[i][s_i] - x[i][i]) + sum_i relu(m + x[i][a_i] - x[a_i][a_i])) / n, a draw of the
 *                   diagonal (or outside [0,n)) adds nothing; the index pointers may be null in modes 0 and 1
 *   tag_milnce_*    MilNceLoss (:46): clip_sim, label (B,N) contiguous, loss = mean_b[LSE_n(c / tau) - LSE_n(c l / tau)];
 *                   dclip (B,N), label gets no gradient.  One wave per row, any N >= 1
 * TAG_EINVAL (message in tag_last_error) for n < 1, tau <= 0 or a null pointer.
 */
size_t tag_contrastive_ws_bytes(int n);
int tag_infonce_forward(const float* x, int n, double tau, float* loss, void* ws, void* stream);
int tag_infonce_backward(const float* x, int n, double tau, const float* dloss, float* dx, const void* ws, void* stream);
int tag_triplet_forward(const float* x, int n, int mode, double margin, const int* s_index, const int* a_index, float* loss,
                        void* ws, void* stream);
int tag_triplet_backward(const float* x, int n, int mode, double margin, const int* s_index, const int* a_index,
                         const float* dloss, float* dx, const void* ws, void* stream);
int tag_milnce_forward(const float* clip_sim, const float* label, int B, int N, double tau, float* loss, void* ws,
                       void* stream);
int tag_milnce_backward(const float* clip_sim, const float* label, int B, int N, double tau, const float* dloss, float* dclip,
                        const void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Clip-level BCE objectives of weak phrase training (clip_bce.hip) over the flattened (B,N) clip matrix of M elements: fp32 in,
 * fp32 out, every element term and the sum over M in fp64, in a fixed order, no atomics (two runs give the same bits).
 * p = clip_sim, y = label (hard or soft in [0,1]), aux (M) = the weight of mode 1 / the prior of mode 4 (may be null otherwise).
 *   loss[0] = (1/M) sum_i e_i,   dp_i = dloss[0] / M * de_i/dp_i,   y and aux get no gradient
 *   bce(x,t)  = -(t max(ln x, -100) + (1 - t) max(ln(1 - x), -100)),   bce'(x,t) = (x - t) / max(x (1 - x), 1e-12)
 *   (torch's own guards; every 1e-12 here is its fp32 constant 1e-12f)
 *   mode 0  FocalClipBceLoss (losses.py:59), c0 = gamma, c1 = alpha:
 *           e = -alpha (1-p)^gamma y ln p - (1-alpha) p^gamma (1-y) ln(1-p), with the clamped logarithms of bce, x^0 = 1,
 *           d(x^gamma) = gamma x^gamma / max(x, 1e-12) and d ln p = -bce'(p,1), d ln(1-p) = -bce'(p,0): finite at p = 0 and
 *           p = 1 (the reference is NaN/inf there), and gamma = 0, alpha = 1/2 is half of the plain BCE everywhere
 *   mode 1  ClipBceLossFreqWeight (:75): e = w bce(p,y), w = (y == 0 ? 1 : aux)
 *   mode 2  SymmetricClipBceLoss (:90), c0 = eps: e = bce(p,y) + bce(yc,p), yc = clamp(y, eps, 1-eps);
 *           de = bce'(p,y) + ln(1-yc) - ln yc with both logarithms clamped at -100 (forward and backward alike)
 *   mode 3  OriginSymmetricClipBceLoss (:107), c0 = a, c1 = b, c2 = A = ln eps: e = a bce(p,y) - b A (y (1-p) + (1-y) p)
 *   mode 4  PriorAdjustedClipBceLoss (:125), c0 = tau, aux = prior pi in (0,1): u = pi^tau, v = (1-pi)^tau, s = p u + (1-p) v,
 *           e = bce(p u / s, y), de = bce'(p u / s, y) u v / s^2
 * The forward is one launch of a single workgroup up to an internal M (dispatch.CLIP_BCE_ONE_LAUNCH_MAX); above it the forward
 * is two launches with fp64 partials in ws (tag_clip_bce_ws_bytes(M) bytes; ws may be null for the one-launch sizes).  The
 * backward is one elementwise launch; dp may not alias p.  Any M >= 1.
 * TAG_EINVAL (message in tag_last_error) for M < 1, a mode outside 0..4, a null p / y / loss / dp / dloss, a null aux in modes
 * 1 and 4, or a NaN constant.
 */
size_t tag_clip_bce_ws_bytes(long M);
int tag_clip_bce_forward(const float* p, const float* y, const float* aux, long M, int mode, double c0, double c1, double c2,
                         float* loss, void* ws, void* stream);
int tag_clip_bce_backward(const float* p, const float* y, const float* aux, long M, int mode, double c0, double c1, double c2,
                          const float* dloss, float* dp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Thresholded similarity count (phrase_sim.hip; utils/data/calc_phrase_sim_count.py of the reference without its N x N matrix):
 *   out[i] = sum_j weight[j] * [ sum_d q[i,d] * bank[j,d] >= threshold ]          i < M, j < N
 * q (M, D) with row stride ldq, bank (N, D) with row stride ldb (both >= D, in floats), rows taken as given (the caller
 * normalises them); weight (N) int64, null = all ones; out (M) int64.  The products are fp32 on the exact-fp32 MFMA (operands
 * are not rounded), the comparison is >= on the fp32 sum, the counts are int64.  A workgroup owns 128 query rows and one slice
 * of the bank's columns and leaves its sums in ws[slice][row]; a second launch adds the slices in slice order: no atomics, ws
 * needs no zeroing, the same bits on every run.  ws (tag_phrase_sim_count_ws_bytes, a function of the shape alone) and out are
 * the only device memory: no M x N or chunk x N scores exist.  Any M, N, D >= 1 (the D tail is zero-filled); q may equal bank.
 * TAG_EINVAL before any launch, the limit named in tag_last_error: M, N or D < 1, ldq / ldb < D, a null q / bank / out / ws, M
 * or N above 2^31 - 129, or a launch of more than 2^31 - 1 workgroups.
 */
size_t tag_phrase_sim_count_ws_bytes(int M, int N, int D);
int tag_phrase_sim_count(const float* q, int ldq, const float* bank, int ldb, const long long* weight, float threshold,
                         long long* out, int M, int N, int D, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device k-means (kmeans.hip; python_scripts/clustering/kmeans_emb.py of the reference runs sklearn on the host).  x (N, D) with
 * row stride ldx, centers (K, D) with row stride ldc (both >= D, in floats), all fp32.  Every *_ws_bytes is a function of the
 * shape alone (0 for a shape the call would refuse); ws is never zeroed; no atomics: the same bits on every run.
 *
 * tag_kmeans_assign: label[i] (int32) = argmin_k (||c_k||^2 - 2 x_i . c_k), the products fp32 on the exact-fp32 MFMA (operands
 *   not rounded), ||c_k||^2 computed once per call into ws; ties go to the lowest k (identical centre rows score identically
 *   bit for bit); a column past K never wins.  dist2[i] (fp32) = sum_d (x_id - c_label,d)^2 from the differences, not from the
 *   expansion.  No (N, K) scores exist on the device.
 * tag_kmeans_update: sums (K x D, fp64, dense) = sum of the rows of each label, count (K, int64), centers[k] = sums[k] / count[k]
 *   for count > 0; a row of centers with count 0 is left untouched.  Row slices leave fp32 partials in ws (MFMA with a one-hot
 *   operand formed in registers), a second launch folds them in fp64 in slice order.  A label outside [0, K) is counted nowhere
 *   (the caller checks the range).
 * tag_kmeans_seed_step: closest[i] = min(closest[i], ||x_i - x_p||^2), p = *pick read on the device (int64); first != 0 writes
 *   the distance without the min.  A pick outside [0, N) writes nothing.
 * TAG_EINVAL before any launch, the numbers named in tag_last_error: N, K or D < 1, a row stride < D, a null pointer, N above
 * 2^31 - 129, K above 65535 * 32.
 */
size_t tag_kmeans_assign_ws_bytes(int N, int K, int D);
int tag_kmeans_assign(const float* x, int ldx, const float* centers, int ldc, int* label, float* dist2, int N, int K, int D,
                      void* ws, void* stream);
size_t tag_kmeans_update_ws_bytes(int N, int K, int D);
int tag_kmeans_update(const float* x, int ldx, const int* label, double* sums, long long* count, float* centers, int ldc, int N,
                      int K, int D, void* ws, void* stream);
int tag_kmeans_seed_step(const float* x, int ldx, const long long* pick, float* closest, int first, int N, int D, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device DBSCAN (dbscan.hip; python_scripts/clustering/dbscan_emb.py of the reference runs sklearn's DBSCAN(metric="precomputed")
 * on an N x N float matrix on the host).  The graph is a BIT matrix adj (N x W int32 words, W = tag_dbscan_words(N) =
 * 4 ceil(N / 128): whole 128-column tiles, 16-byte aligned rows; bit j % 32 of word j / 32 of row i is the pair (i, j)),
 * caller-owned: N^2 / 8 bytes, and no other device memory scales with N^2.  core_bits (W words) is one such row.
 *
 * tag_dbscan_words: W, or 0 for an N the calls would refuse.
 * tag_dbscan_graph: adj[i][j] = [sum_d x[i,d] * x[j,d] >= threshold], the products fp32 on the exact-fp32 MFMA (operands not
 *   rounded; phrase_sim.hip's marching kernel with q = bank = x, rows taken as given: the caller normalises them), x (N, D) with
 *   row stride ldx >= D in floats.  The diagonal is computed like any other pair.  EVERY word of adj is written, and bits at
 *   columns >= N are 0.  degree[i] (int32) = popcount of row i (a second launch).  The same bits on every run.
 * tag_dbscan_core: core_bits = the flags degree[i] >= min_samples, bits at rows >= N are 0.
 * tag_dbscan_hook: one FastSV pass on the parent array f (int32, N; 0 .. N - 1 before the first pass, every value a row index):
 *   with gf = f_in[f_in] and m_i = min of gf[j] over the core neighbours j of core row i,  f_out[f_in[i]] = min(.., m_i) and
 *   f_out[i] = min(.., m_i, gf[i]),  f_out starting as a copy of f_in (f_out != f_in).  The scatter-min is an integer atomicMin:
 *   the result does not depend on the order.  *changed (device int32) = 1 if f_out differs from f_in, else 0.  At the fixed
 *   point f[i] is the lowest index of core row i's component of the core-core graph.
 * tag_dbscan_roots: root[i] (int32) = f[i] for a core row, otherwise the smallest f[j] over the core neighbours j of row i, or -1.
 * TAG_EINVAL before any launch, the numbers named in tag_last_error: N or D < 1, ldx < D, a null pointer, N above 2^31 - 129.
 */
int tag_dbscan_words(int N);
int tag_dbscan_graph(const float* x, int ldx, float threshold, int* adj, int* degree, int N, int D, void* stream);
int tag_dbscan_core(const int* degree, int min_samples, int* core_bits, int N, void* stream);
int tag_dbscan_hook(const int* adj, const int* core_bits, const int* f_in, int* f_out, int* changed, int N, void* stream);
int tag_dbscan_roots(const int* adj, const int* core_bits, const int* f, int* root, int N, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device average-linkage clustering over the cosine distance (agc.hip; python_scripts/clustering/agc_emb.py of the reference runs
 * sklearn's AgglomerativeClustering(linkage="average") on the N x N float matrix 1 - cosine_similarity on the host).  For unit rows
 * the average distance of two clusters is 1 - m_A . m_B, m = (sum of the cluster's rows) / size, so a cluster is its fp64 sum
 * vector and its fp32 mean, and all reciprocal-nearest-neighbour pairs of a round merge at once (average linkage is reducible:
 * the dendrogram is the serial one).  A fit is rounds of tag_agc_nearest + tag_agc_merge on M = N, ..., 1 clusters.  Device memory
 * of a fit at (N, D): two (N, D) fp64 sum buffers and one (N, D) fp32 mean buffer (20 N D bytes), two sets of sizes (int64) and
 * node ids (int32), nn, dist, the log (16 (N - 1) bytes) and the two workspaces (at most 8 x 23 N and 8 N bytes): nothing scales
 * with N^2.  Every *_ws_bytes is a function of the shape alone (0 for a shape the call would refuse); ws is never zeroed; no
 * atomics, no cooperative launch, no device-side waiting: the same bits on every run.
 *
 * tag_agc_nearest: m (M, D) fp32 with row stride ldm >= D (floats).  nn[i] (int32) = the j != i with the largest m_i . m_j,
 *   dist[i] (fp32) = 1 - m_i . m_nn[i]; the products fp32 on the exact-fp32 MFMA with unrounded operands, the D tail zero-filled.
 *   Ties go to the lowest j; a column >= M and the diagonal never win.  The scores are BIT-SYMMETRIC: score(i, j) == score(j, i)
 *   (the same chain of k-steps in the same order for both, a product is commutative and nothing else scales a score), so the
 *   lowest row that attains the largest score of the call and its nn name each other: every round of a fit merges a pair.
 *   A workgroup owns 128 rows and one slice of the column tiles and leaves (score, index) per row and slice in ws; a second
 *   launch folds the slices in slice order on (score, index).  The slice count depends on M alone.  No (M, M) array exists.
 *   M = 1 writes nn = -1, dist = +inf; so does a row all of whose scores are NaN.
 * tag_agc_merge: one round's bookkeeping.  Row a is the left half of a pair when b = nn[a] lies in [0, M), b != a, nn[b] == a and
 *   a < b; with P pairs the output has M - P rows: the M - 2 P survivors in their relative order, then the merged clusters in
 *   ascending a with sum = sum_a + sum_b (fp64, dense (M, D)), size = size_a + size_b (int64) and node id next_id + rank (int32).
 *   means_out[o] = (float)(sum / size) is written for EVERY output row (row stride ldm); a pair of rank r writes
 *   log_dist[log_off + r] = dist[a] and log_ids[log_off + r] = {id_a, id_b, next_id + r} (log_ids is (log_rows, 3) int32).
 *   counts (2 x int32 on the device) = {P, M - P}: the round's one host read.  The *_out buffers differ from the inputs (rows
 *   move); means_out may be the buffer nearest read.
 * TAG_EINVAL before any launch, the numbers named in tag_last_error: M or D < 1, ldm < D, a null pointer, M above 2^31 - 129,
 * an output that aliases its input, log_off or next_id negative or above 2^31 - 1 - M, log_off + M / 2 > log_rows.
 */
size_t tag_agc_nearest_ws_bytes(int M, int D);
int tag_agc_nearest(const float* m, int ldm, int* nn, float* dist, int M, int D, void* ws, void* stream);
size_t tag_agc_merge_ws_bytes(int M, int D);
int tag_agc_merge(const int* nn, const float* dist, const double* sums_in, const long long* sizes_in, const int* ids_in,
                  double* sums_out, long long* sizes_out, int* ids_out, float* means_out, int ldm, float* log_dist, int* log_ids,
                  int log_rows, int log_off, int next_id, int* counts, int M, int D, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device spectral clustering over the cosine affinity (spectral.hip; python_scripts/clustering/spectral_emb.py of the reference runs
 * sklearn's SpectralClustering(affinity="precomputed") on the dense N x N fp64 matrix (cos + 1) / 2 on the host).  With unit rows u
 * and W = [u | 1] the affinity is W W^T / 2, rank D + 1, and sklearn's operator is M = Y Y^T - diag(e) with Y = diag(s) W / sqrt 2,
 * s = deg^-1/2, e = a_ii / deg, a_ii = (u_i . u_i + 1) / 2, deg_i = W_i . (W^T 1) / 2 - a_ii (the Laplacian ignores the diagonal).
 * All tensors fp32 with row strides in floats unless stated; ws is never zeroed; no atomics: the same bits on every run.
 *
 * tag_spectral_gram: out (p x q, fp64, row stride ldo >= q in doubles) = sum_i w_i P[i][a] Q[i][b] over N rows; P (N, p), Q (N, q),
 *   w (N) or null (w = 1).  The rows are cut into slices of TAG_SPECTRAL_CHAIN rows whatever the shape is.  Inside a slice the
 *   products are fp32 on the exact-fp32 MFMA (operands not rounded; w_i P[i][a] is one fp32 product) on two alternating
 *   accumulator sets, so a term passes through at most TAG_SPECTRAL_CHAIN / 2 + 3 roundings; the slices' partials go to ws and a
 *   second launch adds them in fp64 in slice order:  |err_ab| <= TAG_SPECTRAL_CHAIN 2^-24 sum_i |w_i P[i][a] Q[i][b]| (+ the fp64
 *   rounding of that sum) for every N.  P == Q with ldp == ldq and p == q: only tiles on or above the diagonal are computed and
 *   element (min(a, b), max(a, b)) serves both (a, b) and (b, a): out is bit-symmetric.  tag_spectral_gram_ws_bytes =
 *   4 ceil(N / TAG_SPECTRAL_CHAIN) p q, a function of the shape alone (0 for a shape the call would refuse).
 * tag_spectral_rows: u (N, D) unit rows (a zero row is fine), t (D, fp64) = sum_i u_i.  Per row, in fp64:
 *   deg = (u_i . t + N) / 2 - a_ii;  s[i] = deg^-1/2, e[i] = a_ii / deg and Y[i] = s_i / sqrt 2 * [u_i, 1] (D + 1 columns, ldy >=
 *   D + 1) are rounded to fp32 once.  A row whose deg is <= 0 or not finite is reported: s[i] = e[i] = 0 and a zero row of Y (a
 *   valid row has s > 0).
 * tag_spectral_apply: out (N, b) = Y T - e * X:  Y (N, Dp), T (Dp, b), e (N), X (N, b); the products as above with k = the column
 *   of Y in ascending order, the epilogue acc - e[i] * X[i][j] in fp32: |err| <= (Dp + 2) 2^-24 (|Y||T| + |e * X|).  out may be X.
 *   No workspace.
 * TAG_EINVAL before any launch, the numbers named in tag_last_error: a size < 1, a row stride below the width, a null pointer
 *   (w excepted), N above 2^31 - 1 - TAG_SPECTRAL_CHAIN (gram) or 2^31 - 129 (apply), p or q above 32768, a grid above 2^31 - 1.
 */
#define TAG_SPECTRAL_CHAIN 256
int tag_spectral_chain(void);
size_t tag_spectral_gram_ws_bytes(int N, int p, int q);
int tag_spectral_gram(const float* P, int ldp, const float* Q, int ldq, const float* w, double* out, int ldo, int N, int p, int q,
                      void* ws, void* stream);
int tag_spectral_rows(const float* u, int ldu, const double* t, float* Y, int ldy, float* s, float* e, int N, int D, void* stream);
int tag_spectral_apply(const float* Y, int ldy, const float* T, int ldt, const float* e, const float* X, int ldx, float* out,
                       int ldo, int N, int Dp, int b, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Operating-point counts of the grounding evaluation (grounding_eval.hip; utils/eval_util.py:296-330 and :136-225 of the
 * reference, as utils/grounding_eval.py restates them on the host): one launch behind tag_segments, one wave per
 * (clip, threshold) pair.  regions (B,NT,max_regions,2) int64 rows [onset, offset) in frames and counts (B,NT) int32 are
 * tag_segments' outputs; gt (B,max_gt,2) double [onset, offset] in seconds, gt_count (B) int32 rows in use per clip.
 * out (B,NT,4) int32 = {tp_preds, tp_refs, psds_tp, psds_fp} of the pair taken as one file: the integers that
 * evaluate_detections (tp_preds, tp_refs) and psds_operating_point (psds_tp, psds_fp) of utils/grounding_eval.py add up, with
 * det = regions * time_resolution in fp64 -- EXACTLY theirs: fp64 with IEEE division and numpy's order of additions (the
 * file's header states the rule; no floating-point value crosses lanes).  No detection: all four 0; no ground truth:
 * psds_fp = the number of detections, the rest 0.  EVERY entry of out is written.  counts[b][t] > max_regions and
 * gt_count[b] > max_gt (or negative values) are clamped, never read out of bounds.  Rows beyond the counts are not read.
 * TAG_EINVAL before any launch: a null pointer (gt may be null when max_gt == 0), B or NT < 1, B * NT above 2^31 - 1,
 * max_regions outside 1 .. 32768, max_gt outside 0 .. 128, time_resolution <= 0, dtc or gtc outside [0, 1].
 * ------------------------------------------------------------------------------------------- */
int tag_grounding_counts(const int64_t* regions, const int32_t* counts, int max_regions, const double* gt,
                         const int32_t* gt_count, int max_gt, int B, int NT, double time_resolution, double dtc, double gtc,
                         int32_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Event-based and segment-based counts of the sed_eval protocol (sed_eval.hip; utils/eval_util.py:354-425 compute_sed_eval of
 * the reference, every (clip, phrase) pair one file with a single label; utils/sed_metrics.py restates the published
 * definitions on the host and is the yardstick): one launch behind tag_segments / tag_segments_double, one wave per
 * (clip, operating point) pair.  regions, counts, gt, gt_count as for tag_grounding_counts, det = regions * time_resolution in
 * fp64 formed the same way.  PRECONDITION: the regions in use of a pair ascend and are disjoint, as tag_segments* write them
 * (the matching relies on it; other inputs give some count, never an access out of bounds); ground-truth times are >= 0.
 * out (B,NT,5) int32 = {ev_tp, seg_tp, seg_fp, seg_fn, seg_n} of the pair taken as one file, EXACTLY the host function's:
 *   ev_tp   the MAXIMUM cardinality of a matching of ground truths and detections (event_matching_type 'optimal'), an edge iff
 *           fabs(on_g - on_d) <= t_collar and fabs(off_g - off_d) <= max(t_collar, percentage_of_length * (off_g - on_g)), the
 *           same fp64 operations as on the host.  (Event FP = counts - ev_tp, FN = gt_count - ev_tp: one label, no substitution.)
 *   seg_*   event rolls at segment_resolution: an event covers segments floor(onset / r) .. ceil(offset / r) - 1 (IEEE fp64
 *           division), both rolls padded to seg_n = ceil(largest offset of either side / r) segments; per segment TP = both
 *           active, FP = detection only, FN = reference only.
 * seg_n is limited to TAG_SED_MAX_SEGMENTS per pair (the time of the word-at-a-time roll, not a buffer).  A pair above it is
 * never truncated: all five of its entries are -1.  No detection and no ground truth: all 0.  EVERY entry of out is written.
 * No floating-point value crosses lanes, no atomics.  counts[b][t] > max_regions and gt_count[b] > max_gt (or negative
 * values) are clamped, never read out of bounds.  Rows beyond the counts are not read.
 * TAG_EINVAL before any launch: a null pointer (gt may be null when max_gt == 0), B or NT < 1, B * NT above 2^31 - 1,
 * max_regions outside 1 .. 32768, max_gt outside 0 .. 128, time_resolution or segment_resolution <= 0, t_collar or
 * percentage_of_length < 0.
 * ------------------------------------------------------------------------------------------- */
#define TAG_SED_MAX_SEGMENTS 16384
int tag_sed_counts(const int64_t* regions, const int32_t* counts, int max_regions, const double* gt, const int32_t* gt_count,
                   int max_gt, int B, int NT, double time_resolution, double t_collar, double percentage_of_length,
                   double segment_resolution, int32_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Score-based PSDS: the PSDS counts of EVERY decision threshold a pair's frame scores define (psds_scores.hip;
 * utils/eval_util.py:226-292 compute_psds_sed_scores of the reference hands the raw scores to sed_scores_eval's
 * intersection_based.psd_roc, where every distinct score is a threshold; utils/psds_scores.py restates that on the host over
 * utils/grounding_eval.py psds_operating_point and is the yardstick).  One launch, one workgroup per pair.
 * sim (B rows of T fp32 frame scores, row stride ld >= T in floats); gt (B,max_gt,2) double [onset, offset] in seconds and
 * gt_count (B) int32 rows in use per pair, as for tag_grounding_counts.  With v_1 < ... < v_m the distinct non-NaN scores of a
 * row (-0.0 and +0.0 are one value, written as +0.0; a NaN score is never active and is no value), v_0 = -inf, and
 * c_k = {psds_tp, psds_fp} of the detections of regime k -- the maximal runs [on, off) of frames with score > v_k, as seconds
 * ((double)frame * time_resolution), no median filter and no connect step -- against the pair's ground truths taken as one
 * file, EXACTLY psds_operating_point's integers (fp64, IEEE division, numpy's order of additions; c_m = {0, 0}):
 *   values   (B,T)   fp32   v_1 .. v_m ascending, then +inf
 *   deltas   (B,T,2) int32  deltas[b][j] = c_{j+1} - c_j for j < m, then 0
 *   base     (B,2)   int32  c_0
 *   n_values (B)     int32  m; it is authoritative: a genuine +inf score is a value like any other (its regime counts {0, 0})
 * so the counts of the pair at a threshold theta are base + the deltas of every value <= theta.  EVERY entry of the four outputs
 * is written.  A pair without a ground truth: psds_tp = 0 and every detection is a false positive.  No atomics, no host read, no
 * floating-point value crosses lanes: the same bits on every run.  gt_count[b] > max_gt (or negative) is clamped, never read
 * out of bounds.
 * TAG_EINVAL before any launch, the numbers named in tag_last_error: a null pointer (gt may be null when max_gt == 0), B < 1,
 * T outside 1 .. TAG_PSDS_SCORES_MAX_T, ld < T, max_gt outside 0 .. 128, time_resolution <= 0, dtc or gtc outside [0, 1].
 * ------------------------------------------------------------------------------------------- */
#define TAG_PSDS_SCORES_MAX_T 1024
int tag_psds_score_deltas(const float* sim, int ld, int B, int T, const double* gt, const int32_t* gt_count, int max_gt,
                          double time_resolution, double dtc, double gtc, float* values, int32_t* deltas, int32_t* base,
                          int32_t* n_values, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Phrase-to-label cosine map (label_map.hip; ASMapping*Dataset of datasets/class_mapping_dataset.py in the reference call
 * sklearn's cosine_similarity(phrase, label_embs) on the host per item).  x (N, D) phrases with row stride ldx, e (C, D) labels
 * with row stride lde (both >= D, in floats), all fp32.  ws (tag_label_map_ws_bytes = 4 (N + C), a function of the shape alone,
 * 0 for a shape the call would refuse) is never zeroed; no atomics: the same bits on every run.
 *
 * tag_label_map: s[i][c] = x_i . e_c / (||x_i|| ||e_c||) in fp32, a zero row's norm taken as 1 (its s is exactly 0): the
 *   products on the exact-fp32 MFMA (operands not rounded), 1 / ||row|| once per call into ws (from an fp64 sum of squares),
 *   s = (x_i . e_c * 1/||x_i||) * 1/||e_c||:  |s - exact| <= (D + 8) 2^-24.  Label c is in the WINDOW of row i when
 *   th0 <= s <= th1 && s != 0 (fp32 comparisons).  Written for every row:
 *     best[i] (int32) = argmax_c s, ties to the lowest c;  best_sim[i] (fp32) that value;  min_sim[i] (fp32) = min_c s;
 *     win_best[i] (int32) = the argmax over the window, ties to the lowest c, -1 for an empty window;  win_count[i] (int32) = the
 *     window's size;  win_bits (N x ceil(C / 32) uint32, dense): bit c % 32 of word c / 32 is set exactly for the window members,
 *     bits past C are 0;
 *     sim (N, C) fp32 with row stride lds >= C, or NULL: then no (N, C) array exists anywhere.
 *   Every selection is made on the very values sim receives, and every other output has the same bits with and without sim.
 *   Identical label rows score identically bit for bit.  A column past C never wins, is in no window and is never written.
 *   A NaN input may give any selection (best stays inside [0, C)), never an access out of bounds.
 * tag_label_map_topk: idx (N x k int32, dense) = the window members of each row of sim (as tag_label_map wrote it, same th0 and
 *   th1) in descending s, ties to the lowest c, padded with -1; column 0 is win_best.  1 <= k <= TAG_LABEL_MAP_MAX_TOPK.
 * TAG_EINVAL before any launch, the numbers named in tag_last_error: N, C or D < 1, a row stride below the width, a null pointer
 * (sim of tag_label_map excepted), N or C above 2^31 - 129, k outside its range.
 */
#define TAG_LABEL_MAP_MAX_TOPK 32
size_t tag_label_map_ws_bytes(int N, int C, int D);
int tag_label_map(const float* x, int ldx, const float* e, int lde, float th0, float th1, int* best, float* best_sim,
                  float* min_sim, int* win_best, int* win_count, unsigned* win_bits, float* sim, int lds, int N, int C, int D,
                  void* ws, void* stream);
int tag_label_map_topk(const float* sim, int lds, float th0, float th1, int* idx, int N, int C, int k, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BERTScore phrase-to-label map (bertscore.hip; utils/data/create_phrase_event_mapping/prepare_phrase_bertscore.py in the
 * reference scores every (phrase, label) pair with bert_score.score and keeps the arg-max F1).  Greedy matching of token vectors,
 * all pairs, without a token x token score matrix:
 *   a  phrase tokens, N items of slot_a consecutive rows each: (N * slot_a, D) fp32, row stride lda >= D (in floats);
 *   b  label tokens, C items of slot_b rows each: (C * slot_b, D) fp32, row stride ldb >= D;
 *   a_len (N), b_len (C) int32: the valid rows of an item are its first len; a value outside 1 .. slot is taken as the nearest
 *      end of that range (nothing is ever read out of bounds on account of a length);
 *   a_w (N, slot_a), b_w (C, slot_b) fp32, dense: token weights; entries at and past the length are not read as weights.
 * The ACCEPTED SLOTS are 8, 16 and 32 (slot_a and slot_b independently): a slot is a power of two that divides the 128-row
 * tile, so no item straddles one.  The rows are used as they are (the caller normalises: bert_score normalises, then multiplies).
 * With s_ij = a[n,i] . b[c,j] on the exact-fp32 MFMA (operands not rounded), i < a_len[n], j < b_len[c]:
 *   P = sum_i a_w[n,i] max_j s_ij / sum_i a_w[n,i],  R = sum_j b_w[c,j] max_i s_ij / sum_j b_w[c,j],  F = 2 P R / (P + R);
 *   a zero weight sum gives P = 0 (R = 0), P + R == 0 gives F = 0.  A row or column past the length enters NO maximum and no sum
 *   (masked by the length; the contents of such rows do not matter as long as they are finite).
 * Written for every phrase n: best[n] (int32) = argmax_c F, ties to the lowest c; best_f, best_p, best_r (fp32) = F, P, R there.
 * scores: (3, N, C) fp32 dense = P, R, F of every pair, or NULL: the other outputs have the same bits either way.
 * ws (tag_bertscore_map_ws_bytes, a function of the shape and the slots alone, 0 for a call that would be refused) is never
 * zeroed; no atomics: the same bits on every run, and identical label items score identically bit for bit wherever they stand.
 * TAG_EINVAL before any launch, the numbers named in tag_last_error: N, C or D < 1, a slot other than 8, 16, 32, a row stride
 * below D, a null pointer (scores excepted), N * slot_a or C * slot_b above 2^31 - 129.
 */
size_t tag_bertscore_map_ws_bytes(int N, int C, int D, int slot_a, int slot_b);
int tag_bertscore_map(const float* a, int lda, const int32_t* a_len, const float* a_w, const float* b, int ldb,
                      const int32_t* b_len, const float* b_w, int slot_a, int slot_b, int N, int C, int D, int* best, float* best_f,
                      float* best_p, float* best_r, float* scores, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAG_HIP_H */
