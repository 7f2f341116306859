// T4: the text side's self-attention (models/text_encoder.py:240-268: cls token + sinusoidal positions + dropout, then ONE
// nn.MultiheadAttention(batch_first=True) over the phrase with a key-padding mask).  The projections are tag_gemm calls; this
// file holds the scaled-dot-product core over the PACKED in-projection (R, S, 3E) = [q|k|v], forward and backward, and the
// element-wise kernels that build the attention input.
//
// Text is the opposite regime of the audio-over-tokens core (mha.hip): R = B*N phrases (thousands of rows) of S = L + 1 <= 64
// positions.  Rows and heads never interact, so ONE WAVE owns a (row, head) pair for the whole computation: the S x S weights
// live in wave-private LDS, dq / dk / dv of the pair are complete sums formed in a fixed order by the lanes that store them.
// No partials, no workspace, no atomics, no workgroup barrier: two runs are bit-identical.  Waves of a workgroup are independent.
//
// Products run on the VALU (fmaf chains, exact fp32), not on MFMA: at S ~ 10 a 16x16 tile is under 40 % full and an S = 33 one
// needs 3 x 3 tiles for 1089 of 2304 cells, the fp32 MFMA rate equals the VALU rate (cdna_hip_programming.md 'FP32-input
// MFMA'), and the core moves ~2 flop per byte of qkv: it is bound by memory and latency, not by arithmetic.
//
// Phases of the forward (lanes):   scores: one (query, key) pair per lane, fmaf over head_dim, 16-byte reads when qkv is 16-byte
// aligned (VEC) else the same chain from 4-byte reads (same bits) | softmax: one query row per lane | store attn, apply dropout:
// flat over S x S | ctx: flat over (query, channel), keys ascending -- reads of v and stores of ctx are contiguous over channels.
#include "tag_common.h"

namespace {

constexpr int TA_MAX_S = 64;
constexpr int TA_MAX_E = 1024;

// same wave: LDS writes of some lanes are read by others.  The LDS queue of a wave is in order; the fences keep the compiler
// from moving accesses across, the barrier is its scheduling boundary.
__device__ __forceinline__ void ta_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum_d a[d] b[d], d ascending, one fmaf per product: VEC and scalar forms give the same bits
template <bool VEC>
__device__ __forceinline__ float ta_dot(const float* __restrict__ a, const float* __restrict__ b, int dh) {
    float acc = 0.0f;
    if constexpr (VEC) {
        for (int d = 0; d < dh; d += 4) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(a + d);
            const f32x4 y = *reinterpret_cast<const f32x4*>(b + d);
            acc = fmaf(x[0], y[0], acc);
            acc = fmaf(x[1], y[1], acc);
            acc = fmaf(x[2], y[2], acc);
            acc = fmaf(x[3], y[3], acc);
        }
    } else {
        for (int d = 0; d < dh; ++d) acc = fmaf(a[d], b[d], acc);
    }
    return acc;
}

__device__ __forceinline__ int ta_klen(const int64_t* klen, int row, int S) {
    const int64_t n = klen[row];
    return n < 1 ? 1 : (n > (int64_t)S ? S : (int)n);
}

// LDS per wave: w[S*S] (scores -> weights -> dropped weights)
template <bool VEC>
__global__ __launch_bounds__(256) void text_selfattn_fwd_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ klen,
                                                                float* __restrict__ ctx, float* __restrict__ attn, int R, int S,
                                                                int E, int H, float scale, float drop_p, uint64_t seed) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const long pair = (long)blockIdx.x * waves + wid;
    if (pair >= (long)R * H) return;                       // whole waves leave: nothing below spans waves
    const int row = (int)(pair / H), h = (int)(pair - (long)row * H);
    const int dh = E / H, SS = S * S, kl = ta_klen(klen, row, S);
    float* w = smem + (size_t)wid * SS;
    const size_t E3 = (size_t)3 * E;
    const float* q = qkv + (size_t)row * S * E3 + (size_t)h * dh;      // position s: + s * 3E;  k: + E;  v: + 2E
    for (int p = lane; p < SS; p += 64) {
        const int i = p / S, j = p - i * S;
        w[p] = j < kl ? ta_dot<VEC>(q + i * E3, q + j * E3 + E, dh) * scale : 0.0f;
    }
    ta_wave_sync();
    if (lane < S) {
        float* wr = w + lane * S;
        float m = wr[0];
        for (int j = 1; j < kl; ++j) m = fmaxf(m, wr[j]);
        float sum = 0.0f;
        for (int j = 0; j < kl; ++j) {
            const float e = expf(wr[j] - m);
            wr[j] = e;
            sum += e;
        }
        for (int j = 0; j < kl; ++j) wr[j] = wr[j] / sum;
    }
    ta_wave_sync();
    const size_t abase = ((size_t)row * H + h) * SS;
    const float keep_scale = 1.0f / (1.0f - drop_p);
    if (attn || drop_p > 0.0f) {
        for (int p = lane; p < SS; p += 64) {
            const float a = w[p];                           // exactly 0 at keys >= klen
            if (attn) attn[abase + p] = a;                  // the weights BEFORE dropout
            if (drop_p > 0.0f) w[p] = tag_keep(seed, (uint64_t)(abase + p), drop_p) ? a * keep_scale : 0.0f;
        }
        ta_wave_sync();
    }
    const float* v = q + 2 * (size_t)E;
    float* c = ctx + (size_t)row * S * E + (size_t)h * dh;
    for (int e = lane; e < S * dh; e += 64) {
        const int i = e / dh, d = e - i * dh;
        const float* wr = w + i * S;
        float acc = 0.0f;
        for (int j = 0; j < kl; ++j) acc = fmaf(wr[j], v[j * E3 + d], acc);
        c[(size_t)i * E + d] = acc;
    }
}

// LDS per wave: pd[S*S] dropped weights, ds[S*S] (d weights -> d scores, scaled)
template <bool VEC>
__global__ __launch_bounds__(256) void text_selfattn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ attn,
                                                                const float* __restrict__ dctx, const int64_t* __restrict__ klen,
                                                                float* __restrict__ dqkv, int R, int S, int E, int H, float scale,
                                                                float drop_p, uint64_t seed) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const long pair = (long)blockIdx.x * waves + wid;
    if (pair >= (long)R * H) return;
    const int row = (int)(pair / H), h = (int)(pair - (long)row * H);
    const int dh = E / H, SS = S * S, kl = ta_klen(klen, row, S);
    float* pd = smem + (size_t)wid * 2 * SS;
    float* ds = pd + SS;
    const size_t E3 = (size_t)3 * E;
    const float* q = qkv + (size_t)row * S * E3 + (size_t)h * dh;
    const float* k = q + E;
    const float* v = q + 2 * (size_t)E;
    const float* dc = dctx + (size_t)row * S * E + (size_t)h * dh;
    const size_t abase = ((size_t)row * H + h) * SS;
    const float* ar = attn + abase;
    const float keep_scale = 1.0f / (1.0f - drop_p);
    // d(dropped weights)[i][j] = dctx_i . v_j, through the dropout on the weights
    for (int p = lane; p < SS; p += 64) {
        const int i = p / S, j = p - i * S;
        float a = 0.0f, g = 0.0f;
        if (j < kl) {
            a = ar[p];
            g = ta_dot<VEC>(dc + (size_t)i * E, v + j * E3, dh);
            if (drop_p > 0.0f) {
                const bool keep = tag_keep(seed, (uint64_t)(abase + p), drop_p);
                g = keep ? g * keep_scale : 0.0f;
                a = keep ? a * keep_scale : 0.0f;
            }
        }
        pd[p] = a;
        ds[p] = g;
    }
    ta_wave_sync();
    // softmax backward of one query row per lane: ds = a (g - sum_j a g), times the score scale
    if (lane < S) {
        float* gr = ds + lane * S;
        const float* a = ar + lane * S;
        float t = 0.0f;
        for (int j = 0; j < kl; ++j) t = fmaf(a[j], gr[j], t);
        for (int j = 0; j < kl; ++j) gr[j] = a[j] * (gr[j] - t) * scale;
    }
    ta_wave_sync();
    float* dq = dqkv + (size_t)row * S * E3 + (size_t)h * dh;
    for (int e = lane; e < S * dh; e += 64) {
        const int s = e / dh, d = e - s * dh;
        float aq = 0.0f, ak = 0.0f, av = 0.0f;
        const float* gr = ds + s * S;
        for (int j = 0; j < kl; ++j) aq = fmaf(gr[j], k[j * E3 + d], aq);          // dq_s = sum_j ds[s][j] k_j
        if (s < kl) {
            for (int i = 0; i < S; ++i) {                                          // key s: sums over ALL queries
                ak = fmaf(ds[i * S + s], q[i * E3 + d], ak);
                av = fmaf(pd[i * S + s], dc[(size_t)i * E + d], av);
            }
        }
        float* o = dq + s * E3 + d;
        o[0] = aq;
        o[E] = ak;
        o[2 * (size_t)E] = av;
    }
}

// x (R, S, E) = dropout([cls ; tok] + pe[:S]), S = L + 1; keep mask indexed over the flat (R, S, E)
__global__ __launch_bounds__(256) void text_cls_pe_fwd_kernel(const float* __restrict__ tok, const float* __restrict__ cls,
                                                              const float* __restrict__ pe, float* __restrict__ x, long total,
                                                              int S, int E, float drop_p, uint64_t seed) {
    const float ks = 1.0f / (1.0f - drop_p);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int e = (int)(i % E);
        const long rs = i / E;
        const int s = (int)(rs % S);
        const long r = rs / S;
        float val = (s == 0 ? cls[e] : tok[(r * (S - 1) + (s - 1)) * E + e]) + pe[(long)s * E + e];
        if (drop_p > 0.0f) val = tag_keep(seed, (uint64_t)i, drop_p) ? val * ks : 0.0f;
        x[i] = val;
    }
}

// dx (R, S, E) -> dtok (R, L, E) (nullable) and the cls rows dcls_rows (R, E) (nullable), both through the same mask
__global__ __launch_bounds__(256) void text_cls_pe_bwd_kernel(const float* __restrict__ dx, float* __restrict__ dtok,
                                                              float* __restrict__ dcls_rows, long total, int S, int E,
                                                              float drop_p, uint64_t seed) {
    const float ks = 1.0f / (1.0f - drop_p);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int e = (int)(i % E);
        const long rs = i / E;
        const int s = (int)(rs % S);
        const long r = rs / S;
        float g = dx[i];
        if (drop_p > 0.0f) g = tag_keep(seed, (uint64_t)i, drop_p) ? g * ks : 0.0f;
        if (s == 0) {
            if (dcls_rows) dcls_rows[r * E + e] = g;
        } else if (dtok) {
            dtok[(r * (S - 1) + (s - 1)) * E + e] = g;
        }
    }
}

bool ta_shape_ok(int R, int S, int E, int H) {
    if (R < 1 || S < 2 || S > TA_MAX_S || E < 1 || E > TA_MAX_E || H < 1 || E % H != 0) return false;
    const int dh = E / H;
    return dh == 16 || dh == 32 || dh % 64 == 0;            // the rule of tag_mha_cross
}

// waves per workgroup: four, fewer when the wave-private LDS would pass 64 KB (no opt-in to large dynamic LDS needed)
int ta_waves(size_t lds_per_wave) {
    const size_t fit = (size_t)65536 / lds_per_wave;
    return fit >= 4 ? 4 : (fit >= 1 ? (int)fit : 1);
}

int ta_elementwise_blocks(long total) {
    const long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace

extern "C" int tag_text_selfattn_forward(const float* qkv, const int64_t* klen, float* ctx, float* attn, int R, int S, int E, int H,
                                         float drop_p, uint64_t seed, void* stream) {
    TAG_CHECK_ARG(qkv && klen && ctx);
    TAG_CHECK_ARG(ta_shape_ok(R, S, E, H));
    TAG_CHECK_ARG(drop_p >= 0.0f && drop_p < 1.0f);
    const size_t lds_wave = (size_t)S * S * sizeof(float);
    const int waves = ta_waves(lds_wave);
    const long pairs = (long)R * H;
    const dim3 grid((unsigned)((pairs + waves - 1) / waves)), block(64 * waves);
    const float scale = 1.0f / sqrtf((float)(E / H));
    // head slices start at multiples of 16 channels and rows are 3E floats apart: 16-byte reads need only an aligned base
    if (aligned16(qkv))
        hipLaunchKernelGGL(text_selfattn_fwd_kernel<true>, grid, block, lds_wave * waves, as_stream(stream), qkv, klen, ctx, attn, R, S,
                           E, H, scale, drop_p, seed);
    else
        hipLaunchKernelGGL(text_selfattn_fwd_kernel<false>, grid, block, lds_wave * waves, as_stream(stream), qkv, klen, ctx, attn, R,
                           S, E, H, scale, drop_p, seed);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_text_selfattn_backward(const float* qkv, const float* attn, const float* dctx, const int64_t* klen, float* dqkv,
                                          int R, int S, int E, int H, float drop_p, uint64_t seed, void* stream) {
    TAG_CHECK_ARG(qkv && attn && dctx && klen && dqkv);
    TAG_CHECK_ARG(ta_shape_ok(R, S, E, H));
    TAG_CHECK_ARG(drop_p >= 0.0f && drop_p < 1.0f);
    const size_t lds_wave = (size_t)2 * S * S * sizeof(float);
    const int waves = ta_waves(lds_wave);
    const long pairs = (long)R * H;
    const dim3 grid((unsigned)((pairs + waves - 1) / waves)), block(64 * waves);
    const float scale = 1.0f / sqrtf((float)(E / H));
    if (aligned16(qkv) && aligned16(dctx))
        hipLaunchKernelGGL(text_selfattn_bwd_kernel<true>, grid, block, lds_wave * waves, as_stream(stream), qkv, attn, dctx, klen,
                           dqkv, R, S, E, H, scale, drop_p, seed);
    else
        hipLaunchKernelGGL(text_selfattn_bwd_kernel<false>, grid, block, lds_wave * waves, as_stream(stream), qkv, attn, dctx, klen,
                           dqkv, R, S, E, H, scale, drop_p, seed);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_text_cls_pe_forward(const float* tok, const float* cls, const float* pe, float* x, int R, int L, int E,
                                       float drop_p, uint64_t seed, void* stream) {
    TAG_CHECK_ARG(tok && cls && pe && x);
    TAG_CHECK_ARG(R >= 1 && L >= 1 && E >= 1);
    TAG_CHECK_ARG(drop_p >= 0.0f && drop_p < 1.0f);
    const long total = (long)R * (L + 1) * E;
    hipLaunchKernelGGL(text_cls_pe_fwd_kernel, dim3(ta_elementwise_blocks(total)), dim3(256), 0, as_stream(stream), tok, cls, pe, x,
                       total, L + 1, E, drop_p, seed);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_text_cls_pe_backward(const float* dx, float* dtok, float* dcls_rows, int R, int L, int E, float drop_p,
                                        uint64_t seed, void* stream) {
    TAG_CHECK_ARG(dx && (dtok || dcls_rows));
    TAG_CHECK_ARG(R >= 1 && L >= 1 && E >= 1);
    TAG_CHECK_ARG(drop_p >= 0.0f && drop_p < 1.0f);
    const long total = (long)R * (L + 1) * E;
    hipLaunchKernelGGL(text_cls_pe_bwd_kernel, dim3(ta_elementwise_blocks(total)), dim3(256), 0, as_stream(stream), dx, dtok,
                       dcls_rows, total, L + 1, E, drop_p, seed);
    TAG_LAUNCH_CHECK();
    return 0;
}
