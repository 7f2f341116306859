// T5: the text side's IntraAttention encoder (models/text_encoder.py:147-237: per layer an UNSCALED dot-product attention of
// the phrase over itself, computed from two separately dropped copies of x + positions, whose message feeds a ConvGRUCell
// shared by all layers).  The three gate products are tag_gemm calls; this file holds the attention core, forward and
// backward, and the cell's element-wise kernels.
//
// Core: rows never interact, so ONE WORKGROUP (4 waves) owns a phrase for the whole computation: its L x L scores live in LDS,
// every output element is a complete sum formed in a fixed order by the lane that stores it.  No partials, no workspace, no
// atomics: two runs are bit-identical.  The (L, E) tile is NOT staged (256 KB at (64, 1024) against 160 KB of LDS): x and pe
// are read from global memory where they are used -- a phrase is 20 KB at (10, 512) and stays in L1 / L2.  What IS staged
// beside the scores are the two keep masks as BITS (2 x L*E/8 bytes, 16 KB at the corner), so that a keep decision costs one
// LDS read instead of one hash per use.
//
// Products run on the VALU (fmaf chains, exact fp32), not on MFMA: at L ~ 10 a 16x16 tile is under 40 % full and L = 33 needs
// 3 x 3 tiles for 1089 of 2304 cells; the fp32 MFMA rate equals the VALU rate (cdna_hip_programming.md 'FP32-input MFMA');
// the operands of the score product do not exist in memory (x + pe, dropped twice) and would have to be built into LDS
// fragments first; and with scores in the hundreds the rounding of the product matters: each score is ONE sum over
// (x + pe) * (x + pe), never expanded into four products.  The core is 4 L^2 E flop per row forward, a few hundred MFLOP per
// batch against ~32 GFLOP of gate GEMMs per layer.
//
// Phases of the forward (lanes):   keep bits: one 32-bit word per lane | scores: one query row per wave, a_i kept in
// registers (E / 64 <= 16 per lane), lanes stride the channels, keys ascending, wave_sum per cell; dead cells (query or key
// >= text_len) are filled with 1e-10 | softmax over ALL L cells: one query row per lane | store attn flat | message: flat
// over (query, channel), keys ascending over ALL L -- reads of x and stores of message are contiguous over channels.
#include "tag_common.h"

namespace {

constexpr int TI_MAX_L = 64;
constexpr int TI_MAX_E = 1024;
constexpr int TI_EPL = TI_MAX_E / 64;      // channels per lane
constexpr float TI_DEAD = 1e-10f;          // masked_fill(mask == 0, 1e-10)

__device__ __forceinline__ int ti_len(const int64_t* text_len, int row, int L) {
    const int64_t n = text_len[row];
    return n < 0 ? 0 : (n > (int64_t)L ? L : (int)n);
}

// keep bits of the first n elements of the phrase whose flat index starts at base: bit (i & 31) of word (i >> 5)
__device__ __forceinline__ void ti_keep_bits(unsigned* __restrict__ bits, uint64_t seed, uint64_t base, int n, float p) {
    for (int w = threadIdx.x; w * 32 < n; w += blockDim.x) {
        unsigned v = 0;
        const int hi = n - w * 32 < 32 ? n - w * 32 : 32;
        for (int b = 0; b < hi; ++b) v |= (unsigned)tag_keep(seed, base + (uint64_t)(w * 32 + b), p) << b;
        bits[w] = v;
    }
}

template <bool DROP>
__device__ __forceinline__ float ti_drop(float v, const unsigned* bits, int idx, float ks) {
    if constexpr (DROP) return (bits[idx >> 5] >> (idx & 31)) & 1u ? v * ks : 0.0f;
    return v;
}

// LDS: w[L*L] (scores -> weights), then DROP: bits_a[words], bits_b[words]
template <bool DROP>
__global__ __launch_bounds__(256) void text_intra_fwd_kernel(const float* __restrict__ x, const float* __restrict__ pe,
                                                             const int64_t* __restrict__ text_len, float* __restrict__ msg,
                                                             float* __restrict__ attn, int L, int E, float drop_p,
                                                             uint64_t seed_a, uint64_t seed_b) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int row = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int LL = L * L, LE = L * E, len = ti_len(text_len, row, L);
    float* w = smem;
    unsigned* ba = reinterpret_cast<unsigned*>(smem + LL);
    unsigned* bb = ba + (LE + 31) / 32;
    const float* xr = x + (size_t)row * LE;
    const float ks = 1.0f / (1.0f - drop_p);
    if constexpr (DROP) {
        ti_keep_bits(ba, seed_a, (uint64_t)row * LE, len * E, drop_p);
        ti_keep_bits(bb, seed_b, (uint64_t)row * LE, len * E, drop_p);
    }
    for (int p = threadIdx.x; p < LL; p += blockDim.x) {
        const int i = p / L, j = p - i * L;
        if (i >= len || j >= len) w[p] = TI_DEAD;
    }
    __syncthreads();
    for (int i = wid; i < len; i += waves) {
        float a[TI_EPL];
#pragma unroll
        for (int k = 0; k < TI_EPL; ++k) {
            const int e = lane + 64 * k;
            a[k] = e < E ? ti_drop<DROP>(xr[i * E + e] + pe[i * E + e], ba, i * E + e, ks) : 0.0f;
        }
        for (int j = 0; j < len; ++j) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < TI_EPL; ++k) {
                const int e = lane + 64 * k;
                if (e < E) acc = fmaf(a[k], ti_drop<DROP>(xr[j * E + e] + pe[j * E + e], bb, j * E + e, ks), acc);
            }
            acc = wave_sum(acc);
            if (lane == 0) w[i * L + j] = acc;
        }
    }
    __syncthreads();
    if (threadIdx.x < L) {
        float* wr = w + threadIdx.x * L;
        float m = wr[0];
        for (int j = 1; j < L; ++j) m = fmaxf(m, wr[j]);
        float sum = 0.0f;
        for (int j = 0; j < L; ++j) {
            const float e = expf(wr[j] - m);
            wr[j] = e;
            sum += e;
        }
        for (int j = 0; j < L; ++j) wr[j] = wr[j] / sum;
    }
    __syncthreads();
    if (attn)
        for (int p = threadIdx.x; p < LL; p += blockDim.x) attn[(size_t)row * LL + p] = w[p];
    float* mr = msg + (size_t)row * LE;
    for (int q = threadIdx.x; q < LE; q += blockDim.x) {
        const int i = q / E, e = q - i * E;
        const float* wr = w + i * L;
        float acc = 0.0f;
        for (int j = 0; j < L; ++j) acc = fmaf(wr[j], xr[j * E + e], acc);
        mr[q] = acc;
    }
}

// LDS: at[L*L] the weights, ds[L*L] (d weights -> d scores, 0 at dead cells), then DROP: bits_a, bits_b.
// dx[s] = sum_i at[i][s] dmsg_i  (message = attn @ x)
//       + keep_a[s] ks sum_j ds[s][j] b_j + keep_b[s] ks sum_i ds[i][s] a_i   (score = a b^T; s, i, j < text_len only)
template <bool DROP>
__global__ __launch_bounds__(256) void text_intra_bwd_kernel(const float* __restrict__ dmsg, const float* __restrict__ x,
                                                             const float* __restrict__ pe, const float* __restrict__ attn,
                                                             const int64_t* __restrict__ text_len, float* __restrict__ dx,
                                                             int accumulate, int L, int E, float drop_p, uint64_t seed_a,
                                                             uint64_t seed_b) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int row = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int LL = L * L, LE = L * E, len = ti_len(text_len, row, L);
    float* at = smem;
    float* ds = smem + LL;
    unsigned* ba = reinterpret_cast<unsigned*>(smem + 2 * LL);
    unsigned* bb = ba + (LE + 31) / 32;
    const float* xr = x + (size_t)row * LE;
    const float* gr = dmsg + (size_t)row * LE;
    const float ks = 1.0f / (1.0f - drop_p);
    if constexpr (DROP) {
        ti_keep_bits(ba, seed_a, (uint64_t)row * LE, len * E, drop_p);
        ti_keep_bits(bb, seed_b, (uint64_t)row * LE, len * E, drop_p);
    }
    for (int p = threadIdx.x; p < LL; p += blockDim.x) at[p] = attn[(size_t)row * LL + p];
    // d weights[i][j] = dmsg_i . x_j over ALL cells: dead cells carry weight in the softmax
    for (int i = wid; i < L; i += waves) {
        float g[TI_EPL];
#pragma unroll
        for (int k = 0; k < TI_EPL; ++k) {
            const int e = lane + 64 * k;
            g[k] = e < E ? gr[i * E + e] : 0.0f;
        }
        for (int j = 0; j < L; ++j) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < TI_EPL; ++k) {
                const int e = lane + 64 * k;
                if (e < E) acc = fmaf(g[k], xr[j * E + e], acc);
            }
            acc = wave_sum(acc);
            if (lane == 0) ds[i * L + j] = acc;
        }
    }
    __syncthreads();
    // softmax backward of one query row per lane; nothing flows through a dead cell
    if (threadIdx.x < L) {
        const int i = threadIdx.x;
        float* dr = ds + i * L;
        const float* a = at + i * L;
        float t = 0.0f;
        for (int j = 0; j < L; ++j) t = fmaf(a[j], dr[j], t);
        for (int j = 0; j < L; ++j) dr[j] = (i < len && j < len) ? a[j] * (dr[j] - t) : 0.0f;
    }
    __syncthreads();
    float* o = dx + (size_t)row * LE;
    for (int q = threadIdx.x; q < LE; q += blockDim.x) {
        const int s = q / E, e = q - s * E;
        float acc = 0.0f;
        for (int i = 0; i < L; ++i) acc = fmaf(at[i * L + s], gr[i * E + e], acc);
        if (s < len) {
            float da = 0.0f, db = 0.0f;
            for (int j = 0; j < len; ++j) {
                const float v = xr[j * E + e] + pe[j * E + e];
                da = fmaf(ds[s * L + j], ti_drop<DROP>(v, bb, j * E + e, ks), da);
                db = fmaf(ds[j * L + s], ti_drop<DROP>(v, ba, j * E + e, ks), db);
            }
            acc += ti_drop<DROP>(da, ba, q, ks) + ti_drop<DROP>(db, bb, q, ks);
        }
        o[q] = accumulate ? o[q] + acc : acc;
    }
}

__device__ __forceinline__ float ti_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// after the u / r GEMMs: u = sigmoid(u), r = sigmoid(r) in place, xr = x * r (the out gate's second operand)
__global__ __launch_bounds__(256) void convgru_gates_fwd_kernel(float* __restrict__ u, float* __restrict__ r,
                                                                const float* __restrict__ x, float* __restrict__ xr, long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const float rv = ti_sigmoid(r[i]);
        u[i] = ti_sigmoid(u[i]);
        r[i] = rv;
        xr[i] = x[i] * rv;
    }
}

// after the o GEMM: o = tanh(o) in place, xnew = x (1 - u) + o u; one (row, channel) per lane over the L positions, so the mean
// over the valid positions (seq_mean, nullable) is a fixed-order sum in a register
__global__ __launch_bounds__(256) void convgru_update_fwd_kernel(float* __restrict__ o, const float* __restrict__ u,
                                                                 const float* __restrict__ x, float* __restrict__ xnew,
                                                                 const int64_t* __restrict__ text_len, float* __restrict__ seq_mean,
                                                                 long RE, int L, int E) {
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < RE; q += (long)gridDim.x * 256) {
        const long row = q / E;
        const int e = (int)(q - row * E);
        const int64_t len = seq_mean ? text_len[row] : 0;
        float s = 0.0f;
        for (int t = 0; t < L; ++t) {
            const size_t i = ((size_t)row * L + t) * E + e;
            const float ov = tanhf(o[i]), uv = u[i];
            const float v = fmaf(ov, uv, x[i] * (1.0f - uv));
            o[i] = ov;
            xnew[i] = v;
            if (t < len) s += v;
        }
        if (seq_mean) seq_mean[q] = s / (float)len;
    }
}

// g = dnew + [t < text_len] dseq / text_len -> do_pre = g u (1 - o^2), du_pre = g (o - x) u (1 - u), dx = g (1 - u)
__global__ __launch_bounds__(256) void convgru_update_bwd_kernel(const float* __restrict__ dnew, const float* __restrict__ dseq,
                                                                 const int64_t* __restrict__ text_len, const float* __restrict__ x,
                                                                 const float* __restrict__ u, const float* __restrict__ o,
                                                                 float* __restrict__ do_pre, float* __restrict__ du_pre,
                                                                 float* __restrict__ dx, long RE, int L, int E) {
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < RE; q += (long)gridDim.x * 256) {
        const long row = q / E;
        const int e = (int)(q - row * E);
        const int64_t len = dseq ? text_len[row] : 0;
        const float share = dseq ? dseq[q] / (float)len : 0.0f;
        for (int t = 0; t < L; ++t) {
            const size_t i = ((size_t)row * L + t) * E + e;
            float g = dnew ? dnew[i] : 0.0f;
            if (t < len) g += share;
            const float uv = u[i], ov = o[i];
            do_pre[i] = g * uv * (1.0f - ov * ov);
            du_pre[i] = g * (ov - x[i]) * uv * (1.0f - uv);
            dx[i] = g * (1.0f - uv);
        }
    }
}

// dxr = do_pre W_o[:, E:] -> dr_pre = dxr x r (1 - r), dx += dxr r
__global__ __launch_bounds__(256) void convgru_gates_bwd_kernel(const float* __restrict__ dxr, const float* __restrict__ x,
                                                                const float* __restrict__ r, float* __restrict__ dr_pre,
                                                                float* __restrict__ dx, long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const float g = dxr[i], rv = r[i];
        dr_pre[i] = g * x[i] * rv * (1.0f - rv);
        dx[i] = fmaf(g, rv, dx[i]);
    }
}

bool ti_shape_ok(int R, int L, int E) { return R >= 1 && L >= 1 && L <= TI_MAX_L && E >= 2 && E <= TI_MAX_E && E % 2 == 0; }

size_t ti_lds_bytes(int L, int E, int score_tiles, bool drop) {
    return (size_t)score_tiles * L * L * sizeof(float) + (drop ? (size_t)2 * (((size_t)L * E + 31) / 32) * sizeof(unsigned) : 0);
}

int ti_blocks(long total) {
    const long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace

extern "C" int tag_text_intra_forward(const float* x, const float* pe, const int64_t* text_len, float* message, float* attn, int R,
                                      int L, int E, float drop_p, uint64_t seed_a, uint64_t seed_b, void* stream) {
    TAG_CHECK_ARG(x && pe && text_len && message);
    TAG_CHECK_ARG(ti_shape_ok(R, L, E));
    TAG_CHECK_ARG(drop_p >= 0.0f && drop_p < 1.0f);
    const bool drop = drop_p > 0.0f;
    const size_t lds = ti_lds_bytes(L, E, 1, drop);           // <= 16 KB + 16 KB
    if (drop)
        hipLaunchKernelGGL(text_intra_fwd_kernel<true>, dim3(R), dim3(256), lds, as_stream(stream), x, pe, text_len, message, attn, L,
                           E, drop_p, seed_a, seed_b);
    else
        hipLaunchKernelGGL(text_intra_fwd_kernel<false>, dim3(R), dim3(256), lds, as_stream(stream), x, pe, text_len, message, attn, L,
                           E, drop_p, seed_a, seed_b);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_text_intra_backward(const float* dmessage, const float* x, const float* pe, const float* attn,
                                       const int64_t* text_len, float* dx, int accumulate, int R, int L, int E, float drop_p,
                                       uint64_t seed_a, uint64_t seed_b, void* stream) {
    TAG_CHECK_ARG(dmessage && x && pe && attn && text_len && dx);
    TAG_CHECK_ARG(ti_shape_ok(R, L, E));
    TAG_CHECK_ARG(drop_p >= 0.0f && drop_p < 1.0f);
    const bool drop = drop_p > 0.0f;
    const size_t lds = ti_lds_bytes(L, E, 2, drop);           // <= 32 KB + 16 KB
    if (drop)
        hipLaunchKernelGGL(text_intra_bwd_kernel<true>, dim3(R), dim3(256), lds, as_stream(stream), dmessage, x, pe, attn, text_len,
                           dx, accumulate, L, E, drop_p, seed_a, seed_b);
    else
        hipLaunchKernelGGL(text_intra_bwd_kernel<false>, dim3(R), dim3(256), lds, as_stream(stream), dmessage, x, pe, attn, text_len,
                           dx, accumulate, L, E, drop_p, seed_a, seed_b);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_convgru_gates_forward(float* u, float* r, const float* x, float* xr, long M, int E, void* stream) {
    TAG_CHECK_ARG(u && r && x && xr && M >= 1 && E >= 1);
    const long total = M * E;
    hipLaunchKernelGGL(convgru_gates_fwd_kernel, dim3(ti_blocks(total)), dim3(256), 0, as_stream(stream), u, r, x, xr, total);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_convgru_update_forward(float* o, const float* u, const float* x, float* xnew, const int64_t* text_len,
                                          float* seq_mean, int R, int L, int E, void* stream) {
    TAG_CHECK_ARG(o && u && x && xnew && R >= 1 && L >= 1 && E >= 1);
    TAG_CHECK_ARG(!seq_mean || text_len);
    const long RE = (long)R * E;
    hipLaunchKernelGGL(convgru_update_fwd_kernel, dim3(ti_blocks(RE)), dim3(256), 0, as_stream(stream), o, u, x, xnew, text_len,
                       seq_mean, RE, L, E);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_convgru_update_backward(const float* dnew, const float* dseq, const int64_t* text_len, const float* x,
                                           const float* u, const float* o, float* do_pre, float* du_pre, float* dx, int R, int L,
                                           int E, void* stream) {
    TAG_CHECK_ARG((dnew || dseq) && x && u && o && do_pre && du_pre && dx && R >= 1 && L >= 1 && E >= 1);
    TAG_CHECK_ARG(!dseq || text_len);
    const long RE = (long)R * E;
    hipLaunchKernelGGL(convgru_update_bwd_kernel, dim3(ti_blocks(RE)), dim3(256), 0, as_stream(stream), dnew, dseq, text_len, x, u, o,
                       do_pre, du_pre, dx, RE, L, E);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_convgru_gates_backward(const float* dxr, const float* x, const float* r, float* dr_pre, float* dx, long M, int E,
                                          void* stream) {
    TAG_CHECK_ARG(dxr && x && r && dr_pre && dx && M >= 1 && E >= 1);
    const long total = M * E;
    hipLaunchKernelGGL(convgru_gates_bwd_kernel, dim3(ti_blocks(total)), dim3(256), 0, as_stream(stream), dxr, x, r, dr_pre, dx, total);
    TAG_LAUNCH_CHECK();
    return 0;
}
