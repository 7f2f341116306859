// Sentence-level contrastive objectives over the (n,n) clip-versus-caption matrix (losses.py in the reference: InfoNceLoss :267,
// MaxTripletLoss :285, RandomTripletLoss :319, WeightedTripletLoss :355) and MilNceLoss (:46) over the (B,N) clip matrix.
//
// n is 32-128 per rank: these passes cost launch latency, not bandwidth, so every objective is ONE forward and ONE backward
// launch for n <= SINGLE_MAX (a single workgroup walks the rows, then the column tiles, and folds the loss itself).  Above that
// the same kernel runs on many workgroups, each leaves one fp64 partial, and a second launch folds them in a fixed order.
// The forward leaves what the backward needs in the workspace (row / column log-sum-exp, or row / column argmax with -1 =
// inactive), so the backward is one elementwise pass in which the owner of dx[i][j] writes it: no atomics, the same bits every
// run.  Both reductions read the matrix along its rows: a row is one wave with the lanes over the columns; a tile of 64 columns
// is one workgroup with the lanes over the columns and the waves striding down the rows, folded through LDS in wave order.
// Nothing of size n^2 lives in LDS or registers; every kernel serves any n >= 1.
#include "tag_common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int MAXW = 16;            // waves of the single-workgroup form
constexpr int MULTI_THREADS = 256;  // workgroup of the many-workgroup form and of the backward passes
constexpr int SINGLE_MAX = 128;     // largest n (or B of MilNce) served by one forward launch
constexpr int MAX_BLOCKS = 256;     // = fp64 partials in the workspace
constexpr int N_MAX = 32768;        // n * n stays below 2^31

enum { MODE_MAX = 0, MODE_WEIGHTED = 1, MODE_RANDOM = 2 };

// workspace: d0[n] d1[n] part[MAX_BLOCKS] (fp64), then i0[n] i1[n] (int32)
struct Ws {
    double *d0, *d1, *part;
    int *i0, *i1;
};
__host__ __device__ inline Ws ws_split(void* ws, int n) {
    Ws w;
    w.d0 = static_cast<double*>(ws);
    w.d1 = w.d0 + n;
    w.part = w.d1 + n;
    w.i0 = reinterpret_cast<int*>(w.part + MAX_BLOCKS);
    w.i1 = w.i0 + n;
    return w;
}

int fwd_blocks(int n) { return n <= SINGLE_MAX ? 1 : (cdiv(n, 4) < MAX_BLOCKS ? cdiv(n, 4) : MAX_BLOCKS); }
int fwd_threads(int n) { return n <= SINGLE_MAX ? 64 * MAXW : MULTI_THREADS; }
int bwd_blocks(int rows) { return cdiv(rows, 4) < 1024 ? cdiv(rows, 4) : 1024; }

// acc: per-lane loss terms of this workgroup -> loss[0] = scale * sum when the grid is one workgroup, else part[blockIdx.x]
__device__ __forceinline__ void block_finish(double acc, double scale, double* __restrict__ part, float* __restrict__ loss) {
    __shared__ double sred[MAXW];
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sred[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < nw; ++w) s += sred[w];
        if (gridDim.x == 1) loss[0] = (float)(s * scale);
        else part[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void fold_partials_kernel(const double* __restrict__ part, int nb, double scale,
                                                            float* __restrict__ loss) {
    __shared__ double sred[4];
    double s = (int)threadIdx.x < nb ? part[threadIdx.x] : 0.0;
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)(((sred[0] + sred[1]) + (sred[2] + sred[3])) * scale);
}

// exp((a - b) * inv) for a <= b (or a = -inf): the difference in fp64, the exponential in fp32
__device__ __forceinline__ float exp_scaled(float a, float b, double inv) { return expf((float)(((double)a - (double)b) * inv)); }

// ---------------------------------------------------------------------------------------------------------------- InfoNce
// z = x / tau.  R[i] = LSE_j z_ij -> d0, C[j] = LSE_i z_ij -> d1, loss terms (R_i - z_ii) + (C_j - z_jj).
__global__ __launch_bounds__(64 * MAXW) void infonce_fwd_kernel(const float* __restrict__ x, int n, double inv_tau,
                                                                double* __restrict__ R, double* __restrict__ C,
                                                                double* __restrict__ part, float* __restrict__ loss) {
    __shared__ float smax[MAXW][64];
    __shared__ double ssum[MAXW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double acc = 0.0;
    for (int i = blockIdx.x * nw + wave; i < n; i += gridDim.x * nw) {
        const float* row = x + (size_t)i * n;
        float m = -INFINITY;
        for (int j = lane; j < n; j += 64) m = fmaxf(m, row[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        double s = 0.0;
        for (int j = lane; j < n; j += 64) s += (double)exp_scaled(row[j], m, inv_tau);
        const double r = (double)m * inv_tau + log(wave_sum_d(s));
        if (lane == 0) {
            R[i] = r;
            acc += r - (double)row[i] * inv_tau;
        }
    }
    const int ntile = (n + 63) >> 6;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int j = tile * 64 + lane;
        float m = -INFINITY;
        double s = 0.0;
        if (j < n) {
            for (int i = wave; i < n; i += nw) {
                const float v = x[(size_t)i * n + j];
                const float mn = fmaxf(m, v);
                s = s * (double)exp_scaled(m, mn, inv_tau) + (double)exp_scaled(v, mn, inv_tau);
                m = mn;
            }
        }
        smax[wave][lane] = m;
        ssum[wave][lane] = s;
        __syncthreads();
        if (wave == 0 && j < n) {            // wave 0 holds row 0: its (m, s) is never empty
            double S = s;
            for (int g = 1; g < nw; ++g) {
                const float mg = smax[g][lane];
                const double sg = ssum[g][lane];
                if (sg == 0.0) continue;     // a wave without rows
                const float mn = fmaxf(m, mg);
                S = S * (double)exp_scaled(m, mn, inv_tau) + sg * (double)exp_scaled(mg, mn, inv_tau);
                m = mn;
            }
            const double c = (double)m * inv_tau + log(S);
            C[j] = c;
            acc += c - (double)x[(size_t)j * n + j] * inv_tau;
        }
        __syncthreads();
    }
    block_finish(acc, 0.5 / n, part, loss);
}

// dx_ij = g / (2 n tau) * (exp(z_ij - R_i) + exp(z_ij - C_j) - 2 [i == j]); one wave per row
__global__ __launch_bounds__(MULTI_THREADS) void infonce_bwd_kernel(const float* __restrict__ x, int n, double inv_tau,
                                                                    const double* __restrict__ R,
                                                                    const double* __restrict__ C,
                                                                    const float* __restrict__ dloss, float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const double k = (double)dloss[0] * inv_tau * 0.5 / n;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        const double r = R[i];
        for (int j = lane; j < n; j += 64) {
            const double z = (double)x[(size_t)i * n + j] * inv_tau;
            const double e = (double)expf((float)(z - r)) + (double)expf((float)(z - C[j])) - (i == j ? 2.0 : 0.0);
            dx[(size_t)i * n + j] = (float)(k * e);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- triplets
__device__ __forceinline__ double pos_poly(double p) { return 0.2 * p * p - 0.7 * p + 0.5; }
__device__ __forceinline__ double neg_poly(double q) { return 0.9 * q * q - 0.4 * q + 0.03; }

// one row of x (or of x^T): p = its diagonal, q = its largest off-diagonal -> active?, its loss term
template <int MODE>
__device__ __forceinline__ bool triplet_term(double margin, float p, float q, double& term) {
    const double h = margin + (double)q - (double)p;
    term = 0.0;
    if (!(h > 0.0)) return false;
    if (MODE == MODE_MAX) term = h;
    else term = fmax(pos_poly(p), 0.0) + fmax(neg_poly(q), 0.0);
    return true;
}

__device__ __forceinline__ void argmax_take(float& best, int& bi, float ov, int oi) {   // exact ties: the lowest index
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
}

// rarg[i] = argmax_{j != i} x_ij, carg[j] = argmax_{i != j} x_ij on the RAW inputs (the hinge is monotonic in x_ij), -1 where the
// row / column is inactive (or n == 1)
template <int MODE>
__global__ __launch_bounds__(64 * MAXW) void triplet_fwd_kernel(const float* __restrict__ x, int n, double margin,
                                                                int* __restrict__ rarg, int* __restrict__ carg,
                                                                double* __restrict__ part, float* __restrict__ loss) {
    __shared__ float sval[MAXW][64];
    __shared__ int sidx[MAXW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double acc = 0.0;
    for (int i = blockIdx.x * nw + wave; i < n; i += gridDim.x * nw) {
        const float* row = x + (size_t)i * n;
        float best = -INFINITY;
        int bi = INT_MAX;
        for (int j = lane; j < n; j += 64) {
            if (j == i) continue;
            const float v = row[j];
            if (v > best || bi == INT_MAX) { best = v; bi = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oi != INT_MAX && (bi == INT_MAX || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
        }
        if (lane == 0) {
            double term = 0.0;
            const bool on = bi != INT_MAX && triplet_term<MODE>(margin, row[i], best, term);
            rarg[i] = on ? bi : -1;
            acc += term;
        }
    }
    const int ntile = (n + 63) >> 6;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int j = tile * 64 + lane;
        float best = -INFINITY;
        int bi = INT_MAX;
        if (j < n) {
            for (int i = wave; i < n; i += nw) {
                if (i == j) continue;
                const float v = x[(size_t)i * n + j];
                if (v > best || bi == INT_MAX) { best = v; bi = i; }
            }
        }
        sval[wave][lane] = best;
        sidx[wave][lane] = bi;
        __syncthreads();
        if (wave == 0 && j < n) {
            for (int g = 1; g < nw; ++g) {
                const float ov = sval[g][lane];
                const int oi = sidx[g][lane];
                if (oi == INT_MAX) continue;
                if (bi == INT_MAX) { best = ov; bi = oi; }
                else argmax_take(best, bi, ov, oi);
            }
            double term = 0.0;
            const bool on = bi != INT_MAX && triplet_term<MODE>(margin, x[(size_t)j * n + j], best, term);
            carg[j] = on ? bi : -1;
            acc += term;
        }
        __syncthreads();
    }
    block_finish(acc, 1.0 / n, part, loss);
}

// MaxTriplet: an active row puts +g/n on its argmax and -g/n on its diagonal, an active column likewise.  WeightedTriplet:
// the derivative of the clamped polynomials, of q on the argmax and of p on the diagonal.  The owner of (i,j) gathers all four.
template <int MODE>
__global__ __launch_bounds__(MULTI_THREADS) void triplet_bwd_kernel(const float* __restrict__ x, int n,
                                                                    const int* __restrict__ rarg,
                                                                    const int* __restrict__ carg,
                                                                    const float* __restrict__ dloss, float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const double k = (double)dloss[0] / n;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        const int ri = rarg[i];
        for (int j = lane; j < n; j += 64) {
            const double v = (double)x[(size_t)i * n + j];
            double g = 0.0;
            if (j == i) {
                const double d = MODE == MODE_MAX ? -1.0 : (pos_poly(v) > 0.0 ? 0.4 * v - 0.7 : 0.0);
                g = d * ((ri >= 0 ? 1.0 : 0.0) + (carg[i] >= 0 ? 1.0 : 0.0));
            } else {
                const double d = MODE == MODE_MAX ? 1.0 : (neg_poly(v) > 0.0 ? 1.8 * v - 0.4 : 0.0);
                g = d * ((j == ri ? 1.0 : 0.0) + (carg[j] == i ? 1.0 : 0.0));
            }
            dx[(size_t)i * n + j] = (float)(k * g);
        }
    }
}

// RandomTriplet: row i against column s[i] (hinge on x_ii) and against column a[i] (hinge on the diagonal of THAT column); a draw
// of the diagonal itself (or an index outside [0,n)) contributes nothing
__device__ __forceinline__ bool random_on(const float* __restrict__ x, int n, double margin, int i, int j, int diag) {
    if (j == i || j < 0 || j >= n) return false;
    return margin + (double)x[(size_t)i * n + j] - (double)x[(size_t)diag * n + diag] > 0.0;
}

__global__ __launch_bounds__(256) void random_triplet_fwd_kernel(const float* __restrict__ x, int n, double margin,
                                                                 const int* __restrict__ s_index,
                                                                 const int* __restrict__ a_index, float* __restrict__ loss) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int s = s_index[i], a = a_index[i];
        if (random_on(x, n, margin, i, s, i)) acc += margin + (double)x[(size_t)i * n + s] - (double)x[(size_t)i * n + i];
        if (random_on(x, n, margin, i, a, a)) acc += margin + (double)x[(size_t)i * n + a] - (double)x[(size_t)a * n + a];
    }
    block_finish(acc, 1.0 / n, nullptr, loss);
}

// one wave per row i writes the whole row: +g/n per active draw on (i, s_i) and (i, a_i); the diagonal loses g/n for the row's
// own s-draw and for EVERY row k whose a-draw is column i, counted by this wave over a_index
__global__ __launch_bounds__(MULTI_THREADS) void random_triplet_bwd_kernel(const float* __restrict__ x, int n, double margin,
                                                                           const int* __restrict__ s_index,
                                                                           const int* __restrict__ a_index,
                                                                           const float* __restrict__ dloss,
                                                                           float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const double k = (double)dloss[0] / n;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        const int s = s_index[i], a = a_index[i];
        const bool s_on = random_on(x, n, margin, i, s, i), a_on = random_on(x, n, margin, i, a, a);
        float cnt = 0.0f;                      // a count below 2^24: exact in fp32 whatever the order
        for (int r = lane; r < n; r += 64)
            if (a_index[r] == i && random_on(x, n, margin, r, i, i)) cnt += 1.0f;
        cnt = wave_sum(cnt) + (s_on ? 1.0f : 0.0f);
        for (int j = lane; j < n; j += 64) {
            double g = 0.0;
            if (j == i) g = -(double)cnt;
            else g = (s_on && j == s ? 1.0 : 0.0) + (a_on && j == a ? 1.0 : 0.0);
            dx[(size_t)i * n + j] = (float)(k * g);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- MilNce
// one wave per row b: D[b] = LSE_n(c / tau) -> d0, U[b] = LSE_n(c l / tau) -> d1, loss term D - U
__global__ __launch_bounds__(64 * MAXW) void milnce_fwd_kernel(const float* __restrict__ c, const float* __restrict__ l, int B,
                                                               int N, double inv_tau, double* __restrict__ D,
                                                               double* __restrict__ U, double* __restrict__ part,
                                                               float* __restrict__ loss) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double acc = 0.0;
    for (int b = blockIdx.x * nw + wave; b < B; b += gridDim.x * nw) {
        const float* cr = c + (size_t)b * N;
        const float* lr = l + (size_t)b * N;
        double m1 = -INFINITY, m2 = -INFINITY;
        for (int j = lane; j < N; j += 64) {
            const double v = (double)cr[j];
            m1 = fmax(m1, v);
            m2 = fmax(m2, v * (double)lr[j]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            m1 = fmax(m1, __shfl_xor(m1, o, 64));
            m2 = fmax(m2, __shfl_xor(m2, o, 64));
        }
        double s1 = 0.0, s2 = 0.0;
        for (int j = lane; j < N; j += 64) {
            const double v = (double)cr[j];
            s1 += (double)expf((float)((v - m1) * inv_tau));
            s2 += (double)expf((float)((v * (double)lr[j] - m2) * inv_tau));
        }
        const double d = m1 * inv_tau + log(wave_sum_d(s1));
        const double u = m2 * inv_tau + log(wave_sum_d(s2));
        if (lane == 0) {
            D[b] = d;
            U[b] = u;
            acc += d - u;
        }
    }
    block_finish(acc, 1.0 / B, part, loss);
}

// dc = g / (B tau) * (softmax(c / tau) - l softmax(c l / tau))
__global__ __launch_bounds__(MULTI_THREADS) void milnce_bwd_kernel(const float* __restrict__ c, const float* __restrict__ l,
                                                                   int B, int N, double inv_tau, const double* __restrict__ D,
                                                                   const double* __restrict__ U,
                                                                   const float* __restrict__ dloss, float* __restrict__ dc) {
    const int lane = threadIdx.x & 63;
    const double k = (double)dloss[0] * inv_tau / B;
    for (int b = blockIdx.x * 4 + (threadIdx.x >> 6); b < B; b += gridDim.x * 4) {
        const double d = D[b], u = U[b];
        for (int j = lane; j < N; j += 64) {
            const double v = (double)c[(size_t)b * N + j], lab = (double)l[(size_t)b * N + j];
            const double e = (double)expf((float)(v * inv_tau - d)) - lab * (double)expf((float)(v * lab * inv_tau - u));
            dc[(size_t)b * N + j] = (float)(k * e);
        }
    }
}

int fold(const Ws& w, int n, double scale, float* loss, hipStream_t st) {
    if (fwd_blocks(n) == 1) return 0;
    hipLaunchKernelGGL(fold_partials_kernel, dim3(1), dim3(256), 0, st, w.part, fwd_blocks(n), scale, loss);
    TAG_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" size_t tag_contrastive_ws_bytes(int n) {
    if (n < 1 || n > N_MAX) return 0;
    return ((size_t)2 * n + MAX_BLOCKS) * sizeof(double) + (size_t)2 * n * sizeof(int);
}

extern "C" int tag_infonce_forward(const float* x, int n, double tau, float* loss, void* ws, void* stream) {
    TAG_CHECK_ARG(x && loss && ws && n >= 1 && n <= N_MAX && tau > 0.0);
    const Ws w = ws_split(ws, n);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(infonce_fwd_kernel, dim3(fwd_blocks(n)), dim3(fwd_threads(n)), 0, st, x, n, 1.0 / tau, w.d0, w.d1, w.part,
                       loss);
    TAG_LAUNCH_CHECK();
    return fold(w, n, 0.5 / n, loss, st);
}

extern "C" int tag_infonce_backward(const float* x, int n, double tau, const float* dloss, float* dx, const void* ws,
                                    void* stream) {
    TAG_CHECK_ARG(x && dloss && dx && ws && n >= 1 && n <= N_MAX && tau > 0.0);
    const Ws w = ws_split(const_cast<void*>(ws), n);
    hipLaunchKernelGGL(infonce_bwd_kernel, dim3(bwd_blocks(n)), dim3(MULTI_THREADS), 0, as_stream(stream), x, n, 1.0 / tau, w.d0,
                       w.d1, dloss, dx);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_triplet_forward(const float* x, int n, int mode, double margin, const int* s_index, const int* a_index,
                                   float* loss, void* ws, void* stream) {
    TAG_CHECK_ARG(x && loss && ws && n >= 1 && n <= N_MAX && mode >= MODE_MAX && mode <= MODE_RANDOM);
    TAG_CHECK_ARG(mode != MODE_RANDOM || (s_index && a_index));
    const Ws w = ws_split(ws, n);
    hipStream_t st = as_stream(stream);
    if (mode == MODE_RANDOM) {
        hipLaunchKernelGGL(random_triplet_fwd_kernel, dim3(1), dim3(256), 0, st, x, n, margin, s_index, a_index, loss);
        TAG_LAUNCH_CHECK();
        return 0;
    }
    const dim3 grid(fwd_blocks(n)), block(fwd_threads(n));
    if (mode == MODE_MAX)
        hipLaunchKernelGGL(triplet_fwd_kernel<MODE_MAX>, grid, block, 0, st, x, n, margin, w.i0, w.i1, w.part, loss);
    else
        hipLaunchKernelGGL(triplet_fwd_kernel<MODE_WEIGHTED>, grid, block, 0, st, x, n, margin, w.i0, w.i1, w.part, loss);
    TAG_LAUNCH_CHECK();
    return fold(w, n, 1.0 / n, loss, st);
}

extern "C" int tag_triplet_backward(const float* x, int n, int mode, double margin, const int* s_index, const int* a_index,
                                    const float* dloss, float* dx, const void* ws, void* stream) {
    TAG_CHECK_ARG(x && dloss && dx && ws && n >= 1 && n <= N_MAX && mode >= MODE_MAX && mode <= MODE_RANDOM);
    TAG_CHECK_ARG(mode != MODE_RANDOM || (s_index && a_index));
    const Ws w = ws_split(const_cast<void*>(ws), n);
    hipStream_t st = as_stream(stream);
    const dim3 grid(bwd_blocks(n)), block(MULTI_THREADS);
    if (mode == MODE_RANDOM)
        hipLaunchKernelGGL(random_triplet_bwd_kernel, grid, block, 0, st, x, n, margin, s_index, a_index, dloss, dx);
    else if (mode == MODE_MAX)
        hipLaunchKernelGGL(triplet_bwd_kernel<MODE_MAX>, grid, block, 0, st, x, n, w.i0, w.i1, dloss, dx);
    else
        hipLaunchKernelGGL(triplet_bwd_kernel<MODE_WEIGHTED>, grid, block, 0, st, x, n, w.i0, w.i1, dloss, dx);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_milnce_forward(const float* clip_sim, const float* label, int B, int N, double tau, float* loss, void* ws,
                                  void* stream) {
    TAG_CHECK_ARG(clip_sim && label && loss && ws && B >= 1 && B <= N_MAX && N >= 1 && tau > 0.0);
    TAG_CHECK_ARG((long)B * N < (1L << 31));
    const Ws w = ws_split(ws, B);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(milnce_fwd_kernel, dim3(fwd_blocks(B)), dim3(fwd_threads(B)), 0, st, clip_sim, label, B, N, 1.0 / tau,
                       w.d0, w.d1, w.part, loss);
    TAG_LAUNCH_CHECK();
    return fold(w, B, 1.0 / B, loss, st);
}

extern "C" int tag_milnce_backward(const float* clip_sim, const float* label, int B, int N, double tau, const float* dloss,
                                   float* dclip, const void* ws, void* stream) {
    TAG_CHECK_ARG(clip_sim && label && dloss && dclip && ws && B >= 1 && B <= N_MAX && N >= 1 && tau > 0.0);
    TAG_CHECK_ARG((long)B * N < (1L << 31));
    const Ws w = ws_split(const_cast<void*>(ws), B);
    hipLaunchKernelGGL(milnce_bwd_kernel, dim3(bwd_blocks(B)), dim3(MULTI_THREADS), 0, as_stream(stream), clip_sim, label, B, N,
                       1.0 / tau, w.d0, w.d1, dloss, dclip);
    TAG_LAUNCH_CHECK();
    return 0;
}
