// Clip-level BCE objectives of weak phrase training over the flattened (B,N) clip matrix of M elements (losses.py in the
// reference: FocalClipBceLoss :59, ClipBceLossFreqWeight :75, SymmetricClipBceLoss :90, OriginSymmetricClipBceLoss :107,
// PriorAdjustedClipBceLoss :125).  p = clip_sim, y = label (hard or soft in [0,1]), aux = the per-element weight or prior.
//
// M is 512 in the weak-phrase step and at most about 10^4: these passes cost launch latency.  Every element term is evaluated in
// fp64 from the fp32 inputs (1 - p is exact, the powers and logarithms carry no fp32 rounding), so the only rounding a caller sees
// is the final one to fp32.  The forward is ONE launch of a single workgroup for M <= ONE_LAUNCH_MAX; above that many workgroups
// leave one fp64 partial each and a second launch folds them in a fixed order.  No atomics: two runs give the same bits.  The
// backward is one elementwise pass with no reduction of its own.
//
// bce(x,t) = -(t max(ln x, -100) + (1 - t) max(ln(1 - x), -100)) and bce'(x,t) = (x - t) / max(x (1 - x), 1e-12) are torch's (and
// tag_frame_bce_*'s).  The focal mode takes the same clamped logarithms, and its 1/p and 1/(1-p) are bce'(p,1) and bce'(p,0), so
// that every mode is finite at p = 0 and p = 1 and gamma = 0, alpha = 1/2 is half of the plain BCE everywhere.
#include "tag_common.h"
#include <math.h>

namespace {

constexpr int ONE_THREADS = 1024;         // the single-workgroup forward
constexpr int MULTI_THREADS = 256;        // the many-workgroup forward and the backward
constexpr long ONE_LAUNCH_MAX = 4096;     // largest M served by one forward launch (dispatch.CLIP_BCE_ONE_LAUNCH_MAX)
constexpr int MAX_BLOCKS = 256;           // = fp64 partials in the workspace
constexpr int PER_BLOCK = 1024;           // elements per workgroup of the many-workgroup forward, until MAX_BLOCKS is reached

enum { MODE_FOCAL = 0, MODE_FREQ = 1, MODE_SYM = 2, MODE_ORIGIN = 3, MODE_PRIOR = 4, N_MODES = 5 };

constexpr double GUARD = (double)1e-12f;  // torch's binary_cross_entropy guards its derivative with the fp32 constant

struct Consts { double c0, c1, c2; };

__device__ __forceinline__ double clog(double x) { return fmax(log(x), -100.0); }
__device__ __forceinline__ double bce(double x, double t) { return -(t * clog(x) + (1.0 - t) * clog(1.0 - x)); }
__device__ __forceinline__ double dbce(double x, double t) { return (x - t) / fmax(x * (1.0 - x), GUARD); }

// prior-adjusted probability q = p u / s with u = pi^tau, v = (1 - pi)^tau, s = p u + (1 - p) v; dq/dp = u v / s^2
__device__ __forceinline__ double prior_adjust(double p, double prior, double tau, double& dq) {
    const double u = pow(prior, tau), v = pow(1.0 - prior, tau);
    const double s = p * u + (1.0 - p) * v;
    dq = u * v / (s * s);
    return p * u / s;
}

template <int MODE>
__device__ __forceinline__ double term(double p, double y, double a, const Consts& k) {
    if (MODE == MODE_FOCAL) {             // c0 = gamma, c1 = alpha; pow(0, 0) = 1
        return -k.c1 * pow(1.0 - p, k.c0) * y * clog(p) - (1.0 - k.c1) * pow(p, k.c0) * (1.0 - y) * clog(1.0 - p);
    } else if (MODE == MODE_FREQ) {
        return (y == 0.0 ? 1.0 : a) * bce(p, y);
    } else if (MODE == MODE_SYM) {        // c0 = eps
        return bce(p, y) + bce(fmin(fmax(y, k.c0), 1.0 - k.c0), p);
    } else if (MODE == MODE_ORIGIN) {     // c0 = a, c1 = b, c2 = A = ln eps
        return k.c0 * bce(p, y) - k.c1 * k.c2 * (y * (1.0 - p) + (1.0 - y) * p);
    } else {                              // c0 = tau
        double dq;
        return bce(prior_adjust(p, a, k.c0, dq), y);
    }
}

template <int MODE>
__device__ __forceinline__ double dterm(double p, double y, double a, const Consts& k) {
    if (MODE == MODE_FOCAL) {
        const double g = k.c0, al = k.c1;
        const double pw1 = pow(1.0 - p, g), pw0 = pow(p, g), den = fmax(p * (1.0 - p), GUARD);
        const double d_pw1 = -g * pw1 / fmax(1.0 - p, GUARD), d_pw0 = g * pw0 / fmax(p, GUARD);
        const double d_lp = (1.0 - p) / den, d_lq = -p / den;
        return -al * y * (d_pw1 * clog(p) + pw1 * d_lp) - (1.0 - al) * (1.0 - y) * (d_pw0 * clog(1.0 - p) + pw0 * d_lq);
    } else if (MODE == MODE_FREQ) {
        return (y == 0.0 ? 1.0 : a) * dbce(p, y);
    } else if (MODE == MODE_SYM) {
        const double yc = fmin(fmax(y, k.c0), 1.0 - k.c0);
        return dbce(p, y) + clog(1.0 - yc) - clog(yc);
    } else if (MODE == MODE_ORIGIN) {
        return k.c0 * dbce(p, y) - k.c1 * k.c2 * (1.0 - 2.0 * y);
    } else {
        double dq;
        const double q = prior_adjust(p, a, k.c0, dq);
        return dbce(q, y) * dq;
    }
}

constexpr bool reads_aux(int mode) { return mode == MODE_FREQ || mode == MODE_PRIOR; }

// one workgroup (loss[0] = sum / M) or many (part[blockIdx.x] = sum): lanes stride the elements, the waves fold through LDS in
// wave order
template <int MODE>
__global__ __launch_bounds__(ONE_THREADS) void clip_bce_fwd_kernel(const float* __restrict__ p, const float* __restrict__ y,
                                                                   const float* __restrict__ aux, long M, Consts k,
                                                                   double* __restrict__ part, float* __restrict__ loss) {
    __shared__ double sred[ONE_THREADS / 64];
    double acc = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (long)gridDim.x * blockDim.x)
        acc += term<MODE>((double)p[i], (double)y[i], reads_aux(MODE) ? (double)aux[i] : 0.0, k);
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += sred[w];
        if (gridDim.x == 1) loss[0] = (float)(s / (double)M);
        else part[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(MAX_BLOCKS) void clip_bce_fold_kernel(const double* __restrict__ part, int nb, long M,
                                                                   float* __restrict__ loss) {
    __shared__ double sred[MAX_BLOCKS / 64];
    double s = (int)threadIdx.x < nb ? part[threadIdx.x] : 0.0;
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)(((sred[0] + sred[1]) + (sred[2] + sred[3])) / (double)M);
}

template <int MODE>
__global__ __launch_bounds__(MULTI_THREADS) void clip_bce_bwd_kernel(const float* __restrict__ p, const float* __restrict__ y,
                                                                     const float* __restrict__ aux, long M, Consts k,
                                                                     const float* __restrict__ dloss, float* __restrict__ dp) {
    const double scale = (double)dloss[0] / (double)M;
    for (long i = (long)blockIdx.x * MULTI_THREADS + threadIdx.x; i < M; i += (long)gridDim.x * MULTI_THREADS)
        dp[i] = (float)(scale * dterm<MODE>((double)p[i], (double)y[i], reads_aux(MODE) ? (double)aux[i] : 0.0, k));
}

int fwd_blocks(long M) { return M <= ONE_LAUNCH_MAX ? 1 : (cdiv(M, PER_BLOCK) < MAX_BLOCKS ? cdiv(M, PER_BLOCK) : MAX_BLOCKS); }

template <int MODE>
void launch_fwd(const float* p, const float* y, const float* aux, long M, Consts k, double* part, float* loss, hipStream_t st) {
    const int nb = fwd_blocks(M);
    hipLaunchKernelGGL(clip_bce_fwd_kernel<MODE>, dim3(nb), dim3(nb == 1 ? ONE_THREADS : MULTI_THREADS), 0, st, p, y, aux, M, k,
                       part, loss);
}

template <int MODE>
void launch_bwd(const float* p, const float* y, const float* aux, long M, Consts k, const float* dloss, float* dp,
                hipStream_t st) {
    const int nb = cdiv(M, MULTI_THREADS) < 1024 ? cdiv(M, MULTI_THREADS) : 1024;
    hipLaunchKernelGGL(clip_bce_bwd_kernel<MODE>, dim3(nb), dim3(MULTI_THREADS), 0, st, p, y, aux, M, k, dloss, dp);
}

}  // namespace

#define CLIP_BCE_CHECK_COMMON()                                              \
    TAG_CHECK_ARG(M >= 1 && mode >= 0 && mode < N_MODES && p && y);          \
    TAG_CHECK_ARG(aux || !reads_aux(mode));                                  \
    TAG_CHECK_ARG(c0 == c0 && c1 == c1 && c2 == c2)

extern "C" size_t tag_clip_bce_ws_bytes(long M) { return M < 1 ? 0 : (size_t)MAX_BLOCKS * sizeof(double); }

extern "C" int tag_clip_bce_forward(const float* p, const float* y, const float* aux, long M, int mode, double c0, double c1,
                                    double c2, float* loss, void* ws, void* stream) {
    CLIP_BCE_CHECK_COMMON();
    TAG_CHECK_ARG(loss && (ws || M <= ONE_LAUNCH_MAX));
    const Consts k = {c0, c1, c2};
    double* part = static_cast<double*>(ws);
    hipStream_t st = as_stream(stream);
    switch (mode) {
        case MODE_FOCAL: launch_fwd<MODE_FOCAL>(p, y, aux, M, k, part, loss, st); break;
        case MODE_FREQ: launch_fwd<MODE_FREQ>(p, y, aux, M, k, part, loss, st); break;
        case MODE_SYM: launch_fwd<MODE_SYM>(p, y, aux, M, k, part, loss, st); break;
        case MODE_ORIGIN: launch_fwd<MODE_ORIGIN>(p, y, aux, M, k, part, loss, st); break;
        default: launch_fwd<MODE_PRIOR>(p, y, aux, M, k, part, loss, st); break;
    }
    TAG_LAUNCH_CHECK();
    if (fwd_blocks(M) > 1) {
        hipLaunchKernelGGL(clip_bce_fold_kernel, dim3(1), dim3(MAX_BLOCKS), 0, st, part, fwd_blocks(M), M, loss);
        TAG_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int tag_clip_bce_backward(const float* p, const float* y, const float* aux, long M, int mode, double c0, double c1,
                                     double c2, const float* dloss, float* dp, void* stream) {
    CLIP_BCE_CHECK_COMMON();
    TAG_CHECK_ARG(dloss && dp && dp != p);
    const Consts k = {c0, c1, c2};
    hipStream_t st = as_stream(stream);
    switch (mode) {
        case MODE_FOCAL: launch_bwd<MODE_FOCAL>(p, y, aux, M, k, dloss, dp, st); break;
        case MODE_FREQ: launch_bwd<MODE_FREQ>(p, y, aux, M, k, dloss, dp, st); break;
        case MODE_SYM: launch_bwd<MODE_SYM>(p, y, aux, M, k, dloss, dp, st); break;
        case MODE_ORIGIN: launch_bwd<MODE_ORIGIN>(p, y, aux, M, k, dloss, dp, st); break;
        default: launch_bwd<MODE_PRIOR>(p, y, aux, M, k, dloss, dp, st); break;
    }
    TAG_LAUNCH_CHECK();
    return 0;
}
