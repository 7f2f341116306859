// The class-mapping baseline AudioTagging (models/audio_text_model.py:405-458 in the reference) behind its fc_output GEMM:
// time pooling of the frame probabilities (models/utils.py:49-84 *_with_lens), the backward of the whole head
// (pooling + sigmoid) in one pass, and MaskedFrameBceLoss (losses.py:157-170), forward and backward.
//
// Every pass works on the native (B, T, C) layout with the classes innermost.  C is in the hundreds (527 AudioSet labels)
// where the phrase-innermost passes of heads.hip (one wave per row, the innermost entries taken one after another) were
// laid out for N <= 16, so here the LANES run over the classes: a wave-level load or store is 64 consecutive floats, and
// the workgroups are spread over (clip, class tile[, frame slab]).  C = 527 is odd: rows are 4-byte aligned only and
// nothing below assumes more.  Sums over frames are folded in a fixed order (registers, then LDS): no atomics, the
// same bits every run.  Frames t >= min(length[b], T) are outside every reduction.
#include "tag_common.h"

namespace {

constexpr int CT = 64;        // classes per workgroup = one wave across
constexpr int PG = 8;         // frame groups (waves) of a pooling workgroup
constexpr int HG = 4;         // frame groups (waves) of a head-backward workgroup
constexpr int BCE_THREADS = 256;

__device__ __forceinline__ int valid_frames(int64_t l, int T) { return (int)(l < 0 ? 0 : (l > T ? T : l)); }
__device__ __forceinline__ int clamp_len(int64_t l, int Tt) { return (int)(l < 1 ? 1 : (l > Tt ? Tt : l)); }

// clip[b][c] = pool_t prob[b][t][c] over the valid frames; aux[b][c]: linear sum p | exp sum e^p | max index of the FIRST
// maximum (as a float: T < 2^24) | mean unused.  Workgroup = (class tile, clip); wave g takes the frames g, g + PG, ...
template <int MODE>
__global__ __launch_bounds__(CT * PG) void class_pool_fwd_kernel(const float* __restrict__ prob,
                                                                 const int64_t* __restrict__ length,
                                                                 float* __restrict__ clip, float* __restrict__ aux, int T,
                                                                 int C) {
    __shared__ float s1[PG][CT];
    __shared__ float s2[PG][CT];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * CT + lane, b = blockIdx.y;
    const int len = valid_frames(length[b], T);
    float a1 = MODE == 1 ? -3.0e38f : 0.0f, a2 = MODE == 1 ? 2.0e9f : 0.0f;
    if (c < C) {
        const float* p = prob + (size_t)b * T * C + c;
#pragma unroll 4
        for (int t = g; t < len; t += PG) {
            const float v = p[(size_t)t * C];
            if (MODE == 0) a1 += v;
            else if (MODE == 1) { if (v > a1) { a1 = v; a2 = (float)t; } }
            else if (MODE == 2) { a1 += v; a2 = fmaf(v, v, a2); }
            else { const float e = expf(v); a1 += e; a2 = fmaf(e, v, a2); }
        }
    }
    s1[g][lane] = a1;
    s2[g][lane] = a2;
    __syncthreads();
    if (g == 0 && c < C) {
        float r1 = s1[0][lane], r2 = s2[0][lane];
#pragma unroll
        for (int q = 1; q < PG; ++q) {
            const float o1 = s1[q][lane], o2 = s2[q][lane];
            if (MODE == 1) { if (o1 > r1 || (o1 == r1 && o2 < r2)) { r1 = o1; r2 = o2; } }
            else { r1 += o1; r2 += o2; }
        }
        const size_t o = (size_t)b * C + c;
        if (MODE == 0) { clip[o] = r1 / (float)len; aux[o] = 0.0f; }
        else if (MODE == 1) { clip[o] = r1; aux[o] = r2; }
        else { clip[o] = r2 / r1; aux[o] = r1; }
    }
}

// dlogit = (dprob + dclip * d clip / d p) * p (1 - p).  Workgroup = (class tile, frame slab, clip): the per-(clip, class)
// terms sit in registers, wave g takes the frames of its slab g, g + HG, ...  dlogit may alias dprob (same element, read
// before written by the same thread).
template <int MODE>
__global__ __launch_bounds__(CT * HG) void tagging_head_bwd_kernel(const float* __restrict__ prob, const float* dprob,
                                                                   const float* __restrict__ dclip,
                                                                   const float* __restrict__ clip,
                                                                   const float* __restrict__ aux,
                                                                   const int64_t* __restrict__ length, float* dlogit, int T,
                                                                   int C, int ld_dprob, int slab) {
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * CT + lane, b = blockIdx.z;
    if (c >= C) return;
    const int len = valid_frames(length[b], T);
    const int t0 = blockIdx.y * slab, t1 = min(T, t0 + slab);
    const size_t o = (size_t)b * C + c;
    const float dc = dclip ? dclip[o] : 0.0f;
    const float cl = clip[o], ax = aux[o];
    const float k = MODE == 0 ? dc / (float)len : (MODE == 1 ? dc : dc / ax);
    const int arg = MODE == 1 ? (int)ax : 0;
    const float* p = prob + (size_t)b * T * C + c;
    const float* dp = dprob ? dprob + (size_t)b * ld_dprob * C + c : nullptr;
    float* dl = dlogit + (size_t)b * T * C + c;
#pragma unroll 2
    for (int t = t0 + g; t < t1; t += HG) {
        const float v = p[(size_t)t * C];
        float gr = dp ? dp[(size_t)t * C] : 0.0f;
        if (t < len) {
            if (MODE == 0) gr += k;
            else if (MODE == 1) gr += t == arg ? k : 0.0f;
            else if (MODE == 2) gr = fmaf(k, 2.0f * v - cl, gr);
            else gr = fmaf(k * expf(v), 1.0f + v - cl, gr);
        }
        dl[(size_t)t * C] = gr * v * (1.0f - v);
    }
}

// ---- MaskedFrameBceLoss: sum(bce * len_mask * cls_mask) / sum(len_mask * cls_mask) ----
// The valid frames of a clip are ONE contiguous run of len * C floats in prob and in label (frame stride C in both), so a
// workgroup = (chunk of that run, clip) streams it whatever C is; the class of an element is tracked incrementally.
// Partial sums are fp64, one per workgroup, folded by bce_final_kernel in a fixed order.
__global__ __launch_bounds__(BCE_THREADS) void masked_bce_fwd_kernel(const float* __restrict__ prob, int ld_t,
                                                                     const float* __restrict__ label, int ld_label_t,
                                                                     const int64_t* __restrict__ length,
                                                                     const float* __restrict__ cls_mask, int Tt, int C,
                                                                     long chunk, double* __restrict__ partials) {
    __shared__ double red[BCE_THREADS / 64];
    const int b = blockIdx.y;
    const long n = (long)clamp_len(length[b], Tt) * C;
    const long i0 = (long)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
    const float* p = prob + (size_t)b * ld_t * C;
    const float* y = label + (size_t)b * ld_label_t * C;
    const float* m = cls_mask ? cls_mask + (size_t)b * C : nullptr;
    double s = 0.0;
    long i = i0 + threadIdx.x;
    int c = (int)(i % C);
    const int step = BCE_THREADS % C;
    for (; i < i1; i += BCE_THREADS) {
        const float pv = p[i], yv = y[i];
        const float lp = fmaxf(logf(pv), -100.0f), lq = fmaxf(logf(1.0f - pv), -100.0f);
        float l = (yv - 1.0f) * lq - yv * lp;
        if (m) l *= m[c];
        s += (double)l;
        c += step;
        if (c >= C) c -= C;
    }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < BCE_THREADS / 64; ++w) t += red[w];
        partials[(size_t)b * gridDim.x + blockIdx.x] = t;
    }
}

// den = sum_b len_b * sum_c mask[b][c] (fp64, fixed order); with partials: loss = sum(partials) / den, else out = den
__global__ __launch_bounds__(256) void masked_bce_final_kernel(const double* __restrict__ partials, int npart,
                                                               const int64_t* __restrict__ length,
                                                               const float* __restrict__ cls_mask, int B, int Tt, int C,
                                                               float* __restrict__ loss, double* __restrict__ den_out) {
    __shared__ double rs[4], rd[4];
    double s = 0.0, den = 0.0;
    for (int i = threadIdx.x; i < npart; i += 256) s += partials[i];
    if (cls_mask) {
        for (int i = threadIdx.x; i < B * C; i += 256) den += (double)clamp_len(length[i / C], Tt) * (double)cls_mask[i];
    } else {
        for (int b = threadIdx.x; b < B; b += 256) den += (double)clamp_len(length[b], Tt) * (double)C;
    }
    s = wave_sum_d(s);
    den = wave_sum_d(den);
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = s; rd[threadIdx.x >> 6] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double st = rs[0] + rs[1] + rs[2] + rs[3], dt = rd[0] + rd[1] + rd[2] + rd[3];
        if (loss) loss[0] = (float)(st / dt);
        if (den_out) den_out[0] = dt;
    }
}

// dprob (B, Tt, C) contiguous: dloss / den * mask * (p - y) / max(p (1 - p), 1e-12) inside the valid run, zero after it
__global__ __launch_bounds__(BCE_THREADS) void masked_bce_bwd_kernel(const float* __restrict__ prob, int ld_t,
                                                                     const float* __restrict__ label, int ld_label_t,
                                                                     const int64_t* __restrict__ length,
                                                                     const float* __restrict__ cls_mask, int Tt, int C,
                                                                     long chunk, const float* __restrict__ dloss,
                                                                     const double* __restrict__ den,
                                                                     float* __restrict__ dprob) {
    const int b = blockIdx.y;
    const long n = (long)clamp_len(length[b], Tt) * C, total = (long)Tt * C;
    const long i0 = (long)blockIdx.x * chunk, i1 = min(total, i0 + chunk);
    const float* p = prob + (size_t)b * ld_t * C;
    const float* y = label + (size_t)b * ld_label_t * C;
    const float* m = cls_mask ? cls_mask + (size_t)b * C : nullptr;
    float* d = dprob + (size_t)b * Tt * C;
    const float k = dloss[0] / (float)den[0];
    long i = i0 + threadIdx.x;
    int c = (int)(i % C);
    const int step = BCE_THREADS % C;
    for (; i < i1; i += BCE_THREADS) {
        float gr = 0.0f;
        if (i < n) {
            const float pv = p[i], yv = y[i];
            gr = k * (pv - yv) / fmaxf((1.0f - pv) * pv, 1e-12f);
            if (m) gr *= m[c];
        }
        d[i] = gr;
        c += step;
        if (c >= C) c -= C;
    }
}

// chunks of the per-clip run of Tt * C floats: enough workgroups to fill the chip, at least 4 elements per thread
int bce_chunks(int B, int Tt, int C) {
    const long total = (long)Tt * C;
    long want = (2048 + B - 1) / B;
    const long most = (total + 4 * BCE_THREADS - 1) / (4 * BCE_THREADS);
    if (want > most) want = most;
    return (int)(want < 1 ? 1 : want);
}
long bce_chunk_len(int B, int Tt, int C) {
    const long total = (long)Tt * C;
    const int S = bce_chunks(B, Tt, C);
    return (total + S - 1) / S;
}
bool index_range_ok(int B, int T, int C) { return (long)T * C < (1L << 31) && (long)B * C < (1L << 31) && B <= 65535; }

}  // namespace

extern "C" int tag_class_pool_forward(const float* prob, const int64_t* length, float* clip, float* aux, int B, int T,
                                      int C, int mode, void* stream) {
    TAG_CHECK_ARG(prob && length && clip && aux && B > 0 && T > 0 && C > 0 && mode >= 0 && mode <= 3);
    TAG_CHECK_ARG(index_range_ok(B, T, C) && T < (1 << 24));
    const dim3 grid(cdiv(C, CT), B), block(CT * PG);
    hipStream_t st = as_stream(stream);
    if (mode == 0) hipLaunchKernelGGL(class_pool_fwd_kernel<0>, grid, block, 0, st, prob, length, clip, aux, T, C);
    else if (mode == 1) hipLaunchKernelGGL(class_pool_fwd_kernel<1>, grid, block, 0, st, prob, length, clip, aux, T, C);
    else if (mode == 2) hipLaunchKernelGGL(class_pool_fwd_kernel<2>, grid, block, 0, st, prob, length, clip, aux, T, C);
    else hipLaunchKernelGGL(class_pool_fwd_kernel<3>, grid, block, 0, st, prob, length, clip, aux, T, C);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_tagging_head_backward(const float* prob, const float* dprob, const float* dclip, const float* clip,
                                         const float* aux, const int64_t* length, float* dlogit, int B, int T, int C,
                                         int mode, int ld_dprob, void* stream) {
    TAG_CHECK_ARG(prob && clip && aux && length && dlogit && B > 0 && T > 0 && C > 0 && mode >= 0 && mode <= 3);
    TAG_CHECK_ARG(index_range_ok(B, T, C) && (!dprob || ld_dprob >= T) && (dlogit != dprob || ld_dprob == T));
    // frame slabs: about 2048 workgroups in all, at least 4 frames per wave
    const int ctiles = cdiv(C, CT);
    int nslab = cdiv(2048, (long)ctiles * B);
    const int most = cdiv(T, 4 * HG);
    if (nslab > most) nslab = most;
    if (nslab < 1) nslab = 1;
    const int slab = cdiv(T, nslab);
    const dim3 grid(ctiles, cdiv(T, slab), B), block(CT * HG);
    hipStream_t st = as_stream(stream);
#define LAUNCH(M)                                                                                                     \
    hipLaunchKernelGGL(tagging_head_bwd_kernel<M>, grid, block, 0, st, prob, dprob, dclip, clip, aux, length, dlogit, T, C, \
                       ld_dprob, slab)
    if (mode == 0) LAUNCH(0);
    else if (mode == 1) LAUNCH(1);
    else if (mode == 2) LAUNCH(2);
    else LAUNCH(3);
#undef LAUNCH
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t tag_masked_frame_bce_ws_bytes(int B, int Tt, int C) {
    if (B <= 0 || Tt <= 0 || C <= 0) return 0;
    return ((size_t)B * bce_chunks(B, Tt, C) + 1) * sizeof(double);
}

extern "C" int tag_masked_frame_bce_forward(const float* prob, int ld_t, const float* label, int ld_label_t,
                                            const int64_t* length, const float* cls_mask, int B, int Tt, int C, float* loss,
                                            void* ws, void* stream) {
    TAG_CHECK_ARG(prob && label && length && loss && ws && B > 0 && Tt > 0 && C > 0 && ld_t >= Tt && ld_label_t >= Tt);
    TAG_CHECK_ARG(index_range_ok(B, ld_t, C) && index_range_ok(B, ld_label_t, C));
    const int S = bce_chunks(B, Tt, C);
    double* partials = static_cast<double*>(ws);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(masked_bce_fwd_kernel, dim3(S, B), dim3(BCE_THREADS), 0, st, prob, ld_t, label, ld_label_t, length,
                       cls_mask, Tt, C, bce_chunk_len(B, Tt, C), partials);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(masked_bce_final_kernel, dim3(1), dim3(256), 0, st, partials, B * S, length, cls_mask, B, Tt, C, loss,
                       (double*)nullptr);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_masked_frame_bce_backward(const float* prob, int ld_t, const float* label, int ld_label_t,
                                             const int64_t* length, const float* cls_mask, int B, int Tt, int C,
                                             const float* dloss, float* dprob, void* ws, void* stream) {
    TAG_CHECK_ARG(prob && label && length && dloss && dprob && ws && B > 0 && Tt > 0 && C > 0 && ld_t >= Tt &&
                  ld_label_t >= Tt);
    TAG_CHECK_ARG(index_range_ok(B, ld_t, C) && index_range_ok(B, ld_label_t, C));
    const int S = bce_chunks(B, Tt, C);
    double* den = static_cast<double*>(ws);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(masked_bce_final_kernel, dim3(1), dim3(256), 0, st, (const double*)nullptr, 0, length, cls_mask, B, Tt,
                       C, (float*)nullptr, den);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(masked_bce_bwd_kernel, dim3(S, B), dim3(BCE_THREADS), 0, st, prob, ld_t, label, ld_label_t, length,
                       cls_mask, Tt, C, bce_chunk_len(B, Tt, C), dloss, den, dprob);
    TAG_LAUNCH_CHECK();
    return 0;
}
