// The row kernels that text_clap.hip (RoBERTa-style tower) and text_bert.hip (BERT embedding block and sentence poolings) share:
// the register layout of a row, the LayerNorm forward of a row and its backward over rows, and the deterministic table gather.
//
// Row kernels: ONE WAVE per row of D <= 1024 channels, the row in registers as NQ groups of 4 consecutive channels per lane
// (channel = 256 i + 4 lane + j), so a row is read and written once with 16-byte accesses when every row is 16-byte aligned
// (D % 4 == 0 and aligned bases: VEC), and with 4-byte accesses of the SAME channels otherwise (same bits).  The two row sums go
// through wave_sum.  Sums over rows (dgamma, dbeta) are partial rows per wave, rows taken in a fixed stride, folded by tag_colsum;
// the table gradients are a first-occurrence gather like tag_embed_tokens_backward's: no atomics, two runs are bit-identical.
// Everything here has internal linkage: each translation unit that includes the header gets its own instances.
#pragma once
#include "tag_common.h"

namespace {

constexpr int TC_MAX_D = 1024;
constexpr int TC_MAX_PART_BLOCKS = 512;          // backward: at most 4 * 512 waves, each with one partial row of dgamma | dbeta

template <bool VEC>
__device__ __forceinline__ f32x4 tc_ld4(const float* __restrict__ p, int c, int D) {
    if constexpr (VEC) {
        return c < D ? *reinterpret_cast<const f32x4*>(p + c) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    } else {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c + j < D ? p[c + j] : 0.0f;
        return v;
    }
}

template <bool VEC>
__device__ __forceinline__ void tc_st4(float* __restrict__ p, int c, int D, f32x4 v) {
    if constexpr (VEC) {
        if (c < D) *reinterpret_cast<f32x4*>(p + c) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < D) p[c + j] = v[j];
    }
}

// v: the pre-norm row, zero beyond D.  Writes y, and xhat / rstd when asked (what the backward reads).
template <int NQ, bool VEC>
__device__ __forceinline__ void tc_ln_row(const f32x4 (&v)[NQ], int D, int lane, const float* __restrict__ gamma,
                                          const float* __restrict__ beta, float eps, float* __restrict__ y,
                                          float* __restrict__ xhat, float* __restrict__ rstd) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    const float mean = wave_sum(s) / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = (256 * i + 4 * lane + j < D) ? v[i][j] - mean : 0.0f;
            q = fmaf(d, d, q);
        }
    }
    const float inv = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int c = 256 * i + 4 * lane;
        const f32x4 g = tc_ld4<VEC>(gamma, c, D), b = tc_ld4<VEC>(beta, c, D);
        f32x4 xh, o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xh[j] = (v[i][j] - mean) * inv;
            o[j] = xh[j] * g[j] + b[j];
        }
        tc_st4<VEC>(y, c, D, o);
        if (xhat) tc_st4<VEC>(xhat, c, D, xh);
    }
    if (rstd && lane == 0) *rstd = inv;
}

// g = dy gamma;  ds = rstd (g - mean(g) - xhat mean(g xhat));  dgamma += dy xhat, dbeta += dy over the rows of this wave.
// part: (4 gridDim.x, 2, D), EVERY wave writes its row (zeros when it had no row).
template <int NQ, bool VEC>
__global__ __launch_bounds__(256) void tc_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                        const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                        float* __restrict__ ds, float* __restrict__ part, long rows, int D) {
    const int lane = threadIdx.x & 63;
    const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
    f32x4 gm[NQ], ag[NQ], ab[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        gm[i] = tc_ld4<VEC>(gamma, 256 * i + 4 * lane, D);
        ag[i] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        ab[i] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    const float invD = 1.0f / (float)D;
    for (long row = gw; row < rows; row += nw) {
        f32x4 g[NQ], xh[NQ];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int c = 256 * i + 4 * lane;
            const f32x4 d = tc_ld4<VEC>(dy + row * D, c, D);
            xh[i] = tc_ld4<VEC>(xhat + row * D, c, D);
#pragma unroll
            for (int j = 0; j < 4; ++j) {                      // channels beyond D were read as zeros
                g[i][j] = d[j] * gm[i][j];
                s1 += g[i][j];
                s2 = fmaf(g[i][j], xh[i][j], s2);
                ag[i][j] = fmaf(d[j], xh[i][j], ag[i][j]);
                ab[i][j] += d[j];
            }
        }
        const float m1 = wave_sum(s1) * invD, m2 = wave_sum(s2) * invD, r = rstd[row];
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int c = 256 * i + 4 * lane;
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = r * ((g[i][j] - m1) - xh[i][j] * m2);
            tc_st4<VEC>(ds + row * D, c, D, o);
        }
    }
    if (part) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int c = 256 * i + 4 * lane;
            tc_st4<VEC>(part + (gw * 2) * D, c, D, ag[i]);
            tc_st4<VEC>(part + (gw * 2 + 1) * D, c, D, ab[i]);
        }
    }
}

// Deterministic table gradient (no atomics): dtable[idx[p]] += the rows src[q] with idx[q] == idx[p], q ascending.  One workgroup
// per row p; the one whose p is the FIRST occurrence of its index owns the table row (every table row has one writer), as in
// tag_embed_tokens_backward, and forms the same sums in the same order (same bits) -- but the walk over the later rows takes 256
// index compares per step (ballots through LDS) instead of one: the walk is the latency of a launch with thousands of rows.
// Rows whose index is skip_id (the padding index) or outside [0, V) contribute nothing and touch nothing.  D <= 1024.
__global__ __launch_bounds__(256) void tc_scatter_rows_kernel(const float* __restrict__ src, const int64_t* __restrict__ idx,
                                                              float* __restrict__ dtable, int P, int D, int V, int skip_id) {
    __shared__ unsigned long long hits[4];
    __shared__ int earlier;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int64_t tok = idx[p];
    if (tok < 0 || tok >= V || tok == skip_id) return;        // uniform over the workgroup
    if (tid == 0) earlier = 0;
    __syncthreads();
    int found = 0;
    for (int q = tid; q < p; q += 256) found |= (idx[q] == tok);
    if (found) earlier = 1;                                   // benign race: every writer stores 1
    __syncthreads();
    if (earlier) return;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};                  // channels tid + 256 i
    for (int q0 = p; q0 < P; q0 += 256) {
        const int q = q0 + tid;
        const unsigned long long m = __ballot(q < P && idx[q] == tok);
        __syncthreads();                                      // the previous step's readers are done
        if ((tid & 63) == 0) hits[tid >> 6] = m;
        __syncthreads();
        for (int w = 0; w < 4; ++w) {
            unsigned long long mm = hits[w];
            while (mm) {                                      // uniform: every thread walks the same bits, ascending
                const int b = __ffsll((long long)mm) - 1;
                mm &= mm - 1;
                const float* row = src + (size_t)(q0 + 64 * w + b) * D;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (tid + 256 * i < D) acc[i] += row[tid + 256 * i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (tid + 256 * i < D) dtable[(size_t)tok * D + tid + 256 * i] += acc[i];
}

int tc_part_blocks(long rows) {
    const long b = (rows + 3) / 4;
    return (int)(b > TC_MAX_PART_BLOCKS ? TC_MAX_PART_BLOCKS : b);
}

size_t tc_part_floats(long rows, int D) { return (size_t)tc_part_blocks(rows) * 4 * 2 * D; }

#define TC_BY_NQ(D, VEC, CALL)                          \
    if (VEC) {                                          \
        if ((D) <= 256) { CALL(1, true) }               \
        else if ((D) <= 512) { CALL(2, true) }          \
        else if ((D) <= 768) { CALL(3, true) }          \
        else { CALL(4, true) }                          \
    } else {                                            \
        if ((D) <= 256) { CALL(1, false) }              \
        else if ((D) <= 512) { CALL(2, false) }         \
        else if ((D) <= 768) { CALL(3, false) }         \
        else { CALL(4, false) }                         \
    }

int tc_launch_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* ds, float* part, long rows,
                     int D, void* stream) {
    const bool vec = D % 4 == 0 && aligned16(dy) && aligned16(xhat) && aligned16(gamma) && aligned16(ds) &&
                     aligned16(part);
    const int nblk = tc_part_blocks(rows);
#define CALL(NQ, V)                                                                                                        \
    hipLaunchKernelGGL((tc_ln_bwd_kernel<NQ, V>), dim3(nblk), dim3(256), 0, as_stream(stream), dy, xhat, rstd, gamma, ds, \
                       part, rows, D);
    TC_BY_NQ(D, vec, CALL)
#undef CALL
    TAG_LAUNCH_CHECK();
    return 0;
}

// dgamma / dbeta from the partial rows (np, 2, D); cws: the column sum's own workspace
int tc_fold_parts(const float* part, long np, int D, float* dgamma, float* dbeta, void* cws, void* stream) {
    if (dgamma) {
        const int rc = tag_colsum(part, 2 * D, np, D, dgamma, cws, stream);
        if (rc) return rc;
    }
    if (dbeta) {
        const int rc = tag_colsum(part + D, 2 * D, np, D, dbeta, cws, stream);
        if (rc) return rc;
    }
    return 0;
}

size_t tc_max(size_t a, size_t b) { return a > b ? a : b; }

}  // namespace
