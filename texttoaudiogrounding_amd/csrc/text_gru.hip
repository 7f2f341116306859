// T3: row-local GRU recurrence of the text side (models/text_encoder.py:91-125: nn.GRU(batch_first=True) over the padded
// token batch, then mean_with_lens, models/utils.py).  PyTorch gate order (r, z, n), h0 = 0, ALL L padded positions.
//
// Text is the opposite regime of the audio recurrence (gru.hip): R = B*N phrases (64 ... 2048 rows) of L <= ~20 tokens, any
// hidden size, one or two directions, stacked layers.  Rows never interact, so a workgroup owns 16 rows x ALL H units of one
// direction for the whole sequence: the hidden state (backward: the gate gradients) lives in LDS, W_hh streams through L2
// every step (3H x H fp32 = 786 KB at H = 256: it does not fit LDS and is not rounded), the four waves split the unit tiles.
// ONE launch per layer covers all directions and all L steps; there is no exchange between workgroups, no co-residency
// requirement, no spin, no atomic: two runs are bit-identical.  Arithmetic is exact fp32 (v_mfma_f32_16x16x4_f32 = an fmaf
// chain over k, cdna_hip_programming.md 'FP32-input MFMA').
//
// The input projections (x W_ih^T + b_ih, all directions in one GEMM) and the parameter-gradient GEMMs / column sums stay
// with the caller (dispatch.text_gru_forward / text_gru_backward), as for the audio GRU.
//
// MFMA operand maps (16x16x4 f32): lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; D has
// col = l & 15, row = 4 (l >> 4) + reg.  The k ORDER inside a chunk of 16 is free as long as A and B agree: a lane takes the
// four consecutive k = k0 + 4 (l >> 4) + i, i = 0..3, of a chunk in its four MFMAs, so that its h / dgh values are one
// 16-byte LDS read and (forward) its W_hh values one 16-byte global read -- 16 rows x 64 contiguous bytes per load instruction.
#include "tag_common.h"

namespace {

__device__ __forceinline__ float tg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

constexpr int TG_ROWS = 16;          // rows of a workgroup = the MFMA tile
constexpr int TG_THREADS = 256;      // 4 waves: unit tile nt belongs to wave nt % 4
constexpr int TG_PAD = 4;            // floats behind every LDS row: 16-byte aligned rows that start 4 banks apart

__host__ __device__ inline int tg_up16(int n) { return (n + 15) & ~15; }

// LDS: h of the previous and of the current step, [2][16][HS], HS = up16(H) + 4; columns >= H stay zero (the K padding).
// VEC: H % 4 == 0 and w_hh 16-byte aligned -> the four k of a lane are ONE 16-byte read of its W_hh row, else four predicated reads.
template <bool VEC>
__global__ __launch_bounds__(TG_THREADS) void text_gru_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ w_hh,
                                                                  const float* __restrict__ b_hh,
                                                                  const int64_t* __restrict__ text_len, float* __restrict__ y,
                                                                  float* __restrict__ gates, float* __restrict__ seq_mean,
                                                                  int R, int L, int H, int dirs) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int K16 = tg_up16(H), HS = K16 + TG_PAD;
    const int dir = blockIdx.y, r0 = blockIdx.x * TG_ROWS;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    for (int i = threadIdx.x; i < 2 * TG_ROWS * HS; i += TG_THREADS) smem[i] = 0.0f;
    __syncthreads();
    const size_t HH = (size_t)H * H;
    const float* w = w_hh + (size_t)dir * 3 * HH;
    const float* bias = b_hh + (size_t)dir * 3 * H;
    const int ntiles = K16 / 16;
    for (int s = 0; s < L; ++s) {
        const int t = dir == 0 ? s : L - 1 - s;
        const float* hc = smem + (size_t)(s & 1) * TG_ROWS * HS;            // h_{t-1} (zeros at s = 0)
        float* hn = smem + (size_t)((s & 1) ^ 1) * TG_ROWS * HS;           // h_t
        for (int nt = wid; nt < ntiles; nt += 4) {
            const int j = nt * 16 + li;
            const bool jin = j < H;
            const int jc = jin ? j : H - 1;
            // the input projections of this lane's 4 rows x 3 gates: issued before the MFMA chain, consumed after it
            float gx[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + lk * 4 + r;
                const bool ok = jin && row < R;
                const float* gp = gi + (((size_t)(ok ? row : 0) * L + t) * dirs + dir) * 3 * H + jc;
#pragma unroll
                for (int g = 0; g < 3; ++g) gx[r][g] = ok ? gp[(size_t)g * H] : 0.0f;
            }
            f32x4 acc[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            if (s > 0) {
                const float* wr = w + (size_t)jc * H;                       // row g H + j of W_hh: + g HH
                const float* hr = hc + li * HS;
                for (int k0 = 0; k0 < K16; k0 += 16) {
                    const int kk = k0 + 4 * lk;
                    const f32x4 a = *reinterpret_cast<const f32x4*>(hr + kk);
                    f32x4 b[3];
                    if constexpr (VEC) {
                        const bool kin = kk < H;                            // H % 4 == 0: the four k are in or out together
#pragma unroll
                        for (int g = 0; g < 3; ++g)
                            b[g] = kin ? *reinterpret_cast<const f32x4*>(wr + (size_t)g * HH + kk) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                    } else {
#pragma unroll
                        for (int g = 0; g < 3; ++g)
#pragma unroll
                            for (int i = 0; i < 4; ++i) b[g][i] = kk + i < H ? wr[(size_t)g * HH + kk + i] : 0.0f;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int g = 0; g < 3; ++g)
                            acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[g][i], acc[g], 0, 0, 0);
                }
            }
            const float b_r = bias[jc], b_z = bias[H + jc], b_n = bias[2 * H + jc];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = lk * 4 + r, row = r0 + rl;
                const float ghn = acc[2][r] + b_n;
                const float rg = tg_sigmoid(gx[r][0] + (acc[0][r] + b_r));
                const float zg = tg_sigmoid(gx[r][1] + (acc[1][r] + b_z));
                const float ng = tanhf(gx[r][2] + rg * ghn);
                const float hp = hc[rl * HS + jc];
                const float h = (1.0f - zg) * ng + zg * hp;
                if (jin) {
                    const bool rin = row < R;
                    hn[rl * HS + j] = rin ? h : 0.0f;
                    if (rin) {
                        const size_t cell = ((size_t)row * L + t) * dirs + dir;
                        y[cell * H + j] = h;
                        if (gates) {
                            float* gs = gates + cell * 4 * H;
                            gs[j] = rg; gs[H + j] = zg; gs[2 * H + j] = ng; gs[3 * H + j] = ghn;
                        }
                    }
                }
            }
        }
        __syncthreads();     // h_t complete; the buffer read in this step is rewritten in the next one
    }
    // mean over the valid tokens (mean_with_lens): the workgroup wrote every step of its rows; the barrier above orders those
    // stores before these loads (same workgroup).  t ascending whatever the direction: one summation order for both halves.
    if (seq_mean) {
        for (int i = threadIdx.x; i < TG_ROWS * H; i += TG_THREADS) {
            const int rl = i / H, j = i - rl * H, row = r0 + rl;
            if (row >= R) continue;
            const int64_t len = text_len[row];
            const int n = len < (int64_t)L ? (int)(len > 0 ? len : 0) : L;
            float sum = 0.0f;
            for (int t = 0; t < n; ++t) sum += y[(((size_t)row * L + t) * dirs + dir) * H + j];
            seq_mean[((size_t)row * dirs + dir) * H + j] = sum / (float)len;
        }
    }
}

// Backward, reverse time order.  LDS: the gate gradients of the step processed just before, [16][KS] (KS = up16(3H) + 4,
// columns >= 3H stay zero), and dhs [16][up16(H)] = the part of dh_t that arrives through h_t's successor: after the
// element pass it holds dh_{t'} z_{t'} of the step just done, the matrix pass of the next step adds dgh_{t'} W_hh to it.
// Two barriers per step: matrix pass (reads the gate gradients) | element pass (rewrites them).
__global__ __launch_bounds__(TG_THREADS) void text_gru_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dseq,
                                                                  const int64_t* __restrict__ text_len,
                                                                  const float* __restrict__ y, const float* __restrict__ gates,
                                                                  const float* __restrict__ w_hh, float* __restrict__ dgi,
                                                                  float* __restrict__ dgh, float* __restrict__ hprev_out,
                                                                  int R, int L, int H, int dirs) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int K = 3 * H, K16 = tg_up16(K), KS = K16 + TG_PAD, H16 = tg_up16(H);
    float* dghs = smem;
    float* dhs = smem + TG_ROWS * KS;
    const int dir = blockIdx.y, r0 = blockIdx.x * TG_ROWS;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    for (int i = threadIdx.x; i < TG_ROWS * (KS + H16); i += TG_THREADS) smem[i] = 0.0f;
    __syncthreads();
    const float* w = w_hh + (size_t)dir * K * H;
    const int ntiles = H16 / 16;
    for (int s = 0; s < L; ++s) {
        const int t = dir == 0 ? L - 1 - s : s;              // the reverse of the forward order
        const int tp = dir == 0 ? t - 1 : t + 1;             // forward-order predecessor (h_{t-1})
        const bool has_prev = s + 1 < L;
        if (s > 0) {
            for (int nt = wid; nt < ntiles; nt += 4) {
                const int j = nt * 16 + li;
                const bool jin = j < H;
                const float* wc = w + (jin ? j : H - 1);
                const float* ar = dghs + li * KS;
                f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int k0 = 0; k0 < K16; k0 += 16) {
                    const int kk = k0 + 4 * lk;
                    const f32x4 a = *reinterpret_cast<const f32x4*>(ar + kk);
                    float b[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int k = kk + i;
                        b[i] = (jin && k < K) ? wc[(size_t)(k < K ? k : K - 1) * H] : 0.0f;
                    }
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc1, 0, 0, 0);
                }
                if (jin) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) dhs[(lk * 4 + r) * H16 + j] += acc0[r] + acc1[r];
                }
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < TG_ROWS * H; i += TG_THREADS) {
            const int rl = i / H, j = i - rl * H, row = r0 + rl;
            if (row >= R) continue;
            const size_t cell = ((size_t)row * L + t) * dirs + dir;
            const float* gs = gates + cell * 4 * H;
            const float rg = gs[j], zg = gs[H + j], ng = gs[2 * H + j], ghn = gs[3 * H + j];
            float dh = dhs[rl * H16 + j];
            if (dy) dh += dy[cell * H + j];
            if (dseq) {                                       // d mean_with_lens: dseq / len at the valid positions
                const int64_t len = text_len[row];
                if ((int64_t)t < len) dh += dseq[((size_t)row * dirs + dir) * H + j] / (float)len;
            }
            const float hp = has_prev ? y[(((size_t)row * L + tp) * dirs + dir) * H + j] : 0.0f;
            const float dn = dh * (1.0f - zg);
            const float dz = dh * (hp - ng);
            const float dn_pre = dn * (1.0f - ng * ng);
            const float dz_pre = dz * zg * (1.0f - zg);
            const float dr_pre = dn_pre * ghn * rg * (1.0f - rg);
            const float dnr = dn_pre * rg;
            float* gi_o = dgi + cell * 3 * H;
            float* gh_o = dgh + cell * 3 * H;
            gi_o[j] = dr_pre; gi_o[H + j] = dz_pre; gi_o[2 * H + j] = dn_pre;
            gh_o[j] = dr_pre; gh_o[H + j] = dz_pre; gh_o[2 * H + j] = dnr;
            hprev_out[cell * H + j] = hp;
            float* ds = dghs + rl * KS;
            ds[j] = dr_pre; ds[H + j] = dz_pre; ds[2 * H + j] = dnr;
            dhs[rl * H16 + j] = dh * zg;
        }
        __syncthreads();
    }
}

size_t tg_fwd_lds(int H) { return (size_t)2 * TG_ROWS * (tg_up16(H) + TG_PAD) * sizeof(float); }
size_t tg_bwd_lds(int H) { return (size_t)TG_ROWS * (tg_up16(3 * H) + TG_PAD + tg_up16(H)) * sizeof(float); }
constexpr int TG_MAX_H = 512;        // LDS: forward 66,048 B, backward 131,328 B at H = 512 (160 KB per CU)

template <class K>
void tg_allow_lds(K kernel, bool* done) {
    if (!*done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)tg_bwd_lds(TG_MAX_H));
        *done = true;
    }
}

bool tg_shape_ok(int R, int L, int H, int dirs) {
    return R > 0 && L > 0 && H >= 1 && H <= TG_MAX_H && (dirs == 1 || dirs == 2);
}

}  // namespace

extern "C" int tag_text_gru_forward(const float* gi, const float* w_hh, const float* b_hh, const int64_t* text_len, float* y,
                                    float* gates, float* seq_mean, int R, int L, int H, int dirs, void* stream) {
    TAG_CHECK_ARG(gi && w_hh && b_hh && y);
    TAG_CHECK_ARG(tg_shape_ok(R, L, H, dirs));
    TAG_CHECK_ARG(!seq_mean || text_len);
    const dim3 grid((R + TG_ROWS - 1) / TG_ROWS, dirs);
    const size_t lds = tg_fwd_lds(H);
    // 16-byte reads of W_hh rows need H % 4 == 0 AND a 16-byte aligned base (a flat-parameter view may start anywhere)
    if (H % 4 == 0 && (reinterpret_cast<uintptr_t>(w_hh) & 15) == 0) {
        static bool attr_set = false;
        tg_allow_lds(text_gru_fwd_kernel<true>, &attr_set);
        hipLaunchKernelGGL(text_gru_fwd_kernel<true>, grid, dim3(TG_THREADS), lds, as_stream(stream), gi, w_hh, b_hh, text_len, y,
                           gates, seq_mean, R, L, H, dirs);
    } else {
        static bool attr_set = false;
        tg_allow_lds(text_gru_fwd_kernel<false>, &attr_set);
        hipLaunchKernelGGL(text_gru_fwd_kernel<false>, grid, dim3(TG_THREADS), lds, as_stream(stream), gi, w_hh, b_hh, text_len, y,
                           gates, seq_mean, R, L, H, dirs);
    }
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_text_gru_backward(const float* dy, const float* dseq, const int64_t* text_len, const float* y,
                                     const float* gates, const float* w_hh, float* dgi, float* dgh, float* hprev, int R, int L,
                                     int H, int dirs, void* stream) {
    TAG_CHECK_ARG(y && gates && w_hh && dgi && dgh && hprev);
    TAG_CHECK_ARG(dy || dseq);
    TAG_CHECK_ARG(!dseq || text_len);
    TAG_CHECK_ARG(tg_shape_ok(R, L, H, dirs));
    const dim3 grid((R + TG_ROWS - 1) / TG_ROWS, dirs);
    static bool attr_set = false;
    tg_allow_lds(text_gru_bwd_kernel, &attr_set);
    hipLaunchKernelGGL(text_gru_bwd_kernel, grid, dim3(TG_THREADS), tg_bwd_lds(H), as_stream(stream), dy, dseq, text_len, y, gates,
                       w_hh, dgi, dgh, hprev, R, L, H, dirs);
    TAG_LAUNCH_CHECK();
    return 0;
}
