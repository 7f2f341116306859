// Device spectral clustering over the cosine affinity (python_scripts/clustering/spectral_emb.py in the reference, which runs
// sklearn's SpectralClustering(affinity="precomputed") on the dense N x N fp64 matrix (cos + 1) / 2 on the host;
// utils/phrase_cluster.py drives these three entry points).
//
// With u_i = x_i / max(||x_i||, 1e-12) and W = [u | 1] (N x (D + 1)) the affinity is A = W W^T / 2: rank D + 1.  sklearn takes the
// largest eigenpairs of the normalised operator M = Y Y^T - diag(e), Y = diag(s) W / sqrt 2, s = deg^-1/2, e = a_ii / deg (scipy's
// Laplacian ignores the diagonal), so M x = Y (Y^T x) - e * x needs a few tall-skinny products and no N x N array.
//
// tag_spectral_gram:  out (p x q, fp64) = P^T diag(w) Q over N rows.  The reduction index is the ROW, so an MFMA fragment of either
//   operand is 32 consecutive floats of one row: lanes 0 .. 31 read row i, lanes 32 .. 63 row i + 1, straight from the row-major
//   arrays -- no transpose, no LDS, no barrier.  A workgroup owns one 128 x 128 tile of out and one SLICE of TAG_SPECTRAL_CHAIN
//   rows (a constant: the shape never changes it) and leaves its fp32 partial in ws[slice]; a second launch folds the slices in
//   fp64 in slice order.  Inside a slice the products are fp32 on v_mfma_f32_32x32x2_f32 with unrounded operands (w_i P_ia is one
//   fp32 product), on two alternating accumulator sets that are added at the end: a term passes through at most
//   TAG_SPECTRAL_CHAIN / 2 + 3 roundings, so |err_ab| <= TAG_SPECTRAL_CHAIN 2^-24 sum_i |w_i P_ia Q_ib| whatever N is.
//   P == Q (same pointer and stride): only tiles on or above the diagonal are computed and the fold reads element (min, max) for
//   both (a, b) and (b, a), so out is bit-symmetric.
// tag_spectral_rows:  one wave per row, fp64: deg, s, e and the row of Y.
// tag_spectral_apply: out = Y T - e * X, a 128 x 128 tile per workgroup on the same MFMA with k = the column of Y (a lane reads
//   four consecutive floats of its row of Y and the four matching rows of T), the row epilogue fused.
//
// No atomics, no cooperative launch; ws is never zeroed; the same bits on every run.
#include "tag_common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int L = TAG_SPECTRAL_CHAIN;   // rows per slice
constexpr int T = 128;                  // tile edge of a workgroup (4 waves, 64 x 64 each)
constexpr int UN = 4;                   // row pairs per group of loads: 16 loads in flight per lane
static_assert(L % (2 * UN) == 0 && UN % 2 == 0, "a slice is whole groups, a group feeds both accumulator sets alike");

// ------------------------------------------------------------------------------------------------------------------------
// gram
// ------------------------------------------------------------------------------------------------------------------------
struct GramPlan { int tp, tq, tiles, slices; long blocks; };
GramPlan gram_plan(int N, int p, int q, bool sym) {
    GramPlan g;
    g.tp = cdiv(p, T);
    g.tq = cdiv(q, T);
    g.tiles = sym ? (int)((long)g.tp * (g.tp + 1) / 2) : g.tp * g.tq;
    g.slices = cdiv(N, L);
    g.blocks = (long)g.tiles * g.slices;
    return g;
}

// tile edges are ints (p + 127), a row of ws has q floats, the grid is one-dimensional
bool gram_shape_ok(int N, int p, int q) {
    if (N < 1 || p < 1 || q < 1 || N > INT_MAX - L || p > 32768 || q > 32768) return false;
    return gram_plan(N, p, q, false).blocks <= INT_MAX;
}

template <bool HASW>
__global__ __launch_bounds__(256, 2) void spectral_gram_kernel(const float* __restrict__ P, int ldp, const float* __restrict__ Q,
                                                               int ldq, const float* __restrict__ w, float* __restrict__ ws, int N,
                                                               int p, int q, int tp, int tq, int tiles, bool sym) {
    // tile fastest: the workgroups of one slice read the same rows side by side
    const int slice = blockIdx.x / tiles;
    int t = blockIdx.x % tiles, ta = 0, tb;
    if (sym) {                                  // row ta of the upper triangle has tp - ta tiles
        while (t >= tp - ta) { t -= tp - ta; ++ta; }
        tb = ta + t;
    } else {
        ta = t / tq;
        tb = t % tq;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int kl = lane >> 5, ml = lane & 31;
    const int a0 = ta * T + (wid >> 1) * 64, b0 = tb * T + (wid & 1) * 64;
    const int lo = slice * L;
    const int hi = N - lo < L ? N : lo + L;

    bool aok[2], bok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        aok[i] = a0 + 32 * i + ml < p;
        bok[i] = b0 + 32 * i + ml < q;
    }
    const float* pa = P + a0 + ml;
    const float* pb = Q + b0 + ml;

    f32x16 acc[2][2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][i][j][r] = 0.0f;

    // a group = UN row pairs: 4 UN loads per lane, then 4 UN MFMAs, alternating between the two accumulator sets.  Rows >= hi are
    // zero-filled without a read.  (Issuing the next group's loads ahead of the MFMAs by hand, two register sets and scheduling
    // barriers, measured 7 % slower than leaving the order to the compiler and the second resident workgroup.)
    for (int r0 = lo; r0 < hi; r0 += 2 * UN) {
        float av[UN][2], bv[UN][2];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int row = r0 + 2 * u + kl;
            const bool rok = row < hi;
            float wi = 1.0f;
            if (HASW && rok) wi = w[row];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float a = 0.0f, b = 0.0f;
                if (rok && aok[i]) a = pa[(size_t)row * ldp + 32 * i];
                if (rok && bok[i]) b = pb[(size_t)row * ldq + 32 * i];
                av[u][i] = HASW ? a * wi : a;
                bv[u][i] = b;
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[u & 1][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][i], bv[u][j], acc[u & 1][i][j], 0, 0, 0);
    }

    // register r of acc[.][i][j] is row a0 + 32 i + (r & 3) + 8 (r >> 2) + 4 kl, column b0 + 32 j + ml of out
    float* o = ws + (size_t)slice * p * q;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int b = b0 + 32 * j + ml;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int a = a0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * kl;
                if (a < p && b < q) o[(size_t)a * q + b] = acc[0][i][j][r] + acc[1][i][j][r];
            }
        }
}

// out[a][b] = the slices' partials added in fp64 in slice order; sym: element (min, max) serves both (a, b) and (b, a), and a tile
// below the diagonal, which nobody wrote, is never read
__global__ __launch_bounds__(256) void spectral_gram_fold_kernel(const float* __restrict__ ws, int slices, int p, int q,
                                                                 double* __restrict__ out, int ldo, bool sym) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)p * q) return;
    const int a = (int)(idx / q), b = (int)(idx % q);
    const int ra = sym && a > b ? b : a, rb = sym && a > b ? a : b;
    const float* s = ws + (size_t)ra * q + rb;
    double sum = 0.0;
    for (int z = 0; z < slices; ++z) sum += (double)s[(size_t)z * p * q];
    out[(size_t)a * ldo + b] = sum;
}

// ------------------------------------------------------------------------------------------------------------------------
// rows
// ------------------------------------------------------------------------------------------------------------------------
constexpr int ROWS_PER_WG = 4;    // one wave per row

// deg_i = (u_i . t + N) / 2 - a_ii, a_ii = (u_i . u_i + 1) / 2: the affinity's row sum without its diagonal, in fp64 (the lanes'
// partial sums fold in the fixed order of wave_sum_d).  A row with deg <= 0 or a deg that is not finite is REPORTED: s = e = 0 and
// a zero row of Y (a valid row has s > 0).
__global__ __launch_bounds__(256) void spectral_rows_kernel(const float* __restrict__ u, int ldu, const double* __restrict__ t,
                                                            float* __restrict__ Y, int ldy, float* __restrict__ s,
                                                            float* __restrict__ e, int N, int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* ur = u + (size_t)row * ldu;
    double ut = 0.0, uu = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = (double)ur[d];
        ut += v * t[d];
        uu += v * v;
    }
    ut = wave_sum_d(ut);
    uu = wave_sum_d(uu);
    const double aii = 0.5 * (uu + 1.0);
    const double deg = 0.5 * (ut + (double)N) - aii;
    const bool ok = deg > 0.0 && deg <= 1.79769313486231570e308;
    const double sd = ok ? 1.0 / sqrt(deg) : 0.0;
    const double ys = sd / sqrt(2.0);
    float* yr = Y + (size_t)row * ldy;
    for (int d = lane; d < D; d += 64) yr[d] = (float)(ys * (double)ur[d]);
    if (lane == 0) {
        yr[D] = (float)ys;
        s[row] = (float)sd;
        e[row] = ok ? (float)(aii / deg) : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// apply
// ------------------------------------------------------------------------------------------------------------------------
// MFMA step e of an 8-column group g of Y multiplies column k = 8 g + 4 kl + e: the lane's four consecutive floats of its row of Y
// (one 16-byte load when the rows are aligned) against rows k of T, 32 consecutive floats each.
__global__ __launch_bounds__(256, 2) void spectral_apply_kernel(const float* __restrict__ Y, int ldy, const float* __restrict__ Tm,
                                                                int ldt, const float* __restrict__ ev, const float* __restrict__ X,
                                                                int ldx, float* __restrict__ out, int ldo, int N, int Dp, int b,
                                                                int tn, bool al) {
    const int tile_m = blockIdx.x / tn, tile_n = blockIdx.x % tn;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int kl = lane >> 5, ml = lane & 31;
    const int m0 = tile_m * T + (wid >> 1) * 64, n0 = tile_n * T + (wid & 1) * 64;

    bool mok[2], nok[2];
    const float* ya[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + 32 * i + ml;
        mok[i] = m < N;
        ya[i] = Y + (size_t)(mok[i] ? m : 0) * ldy;
        nok[i] = n0 + 32 * i + ml < b;
    }
    const float* tb = Tm + n0 + ml;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    for (int k0 = 0; k0 < Dp; k0 += 8) {
        const int k = k0 + 4 * kl;
        const int n = Dp - k;                   // columns of Y left from k on
        f32x4 af[2];
        float bf[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (mok[i] && n > 0) {
                const float* y = ya[i] + k;
                if (n >= 4 && al) {
                    v = *reinterpret_cast<const f32x4*>(y);
                } else {
                    v.x = y[0];
                    if (n > 1) v.y = y[1];
                    if (n > 2) v.z = y[2];
                    if (n > 3) v.w = y[3];
                }
            }
            af[i] = v;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = 0.0f;
                if (nok[j] && e < n) v = tb[(size_t)(k + e) * ldt + 32 * j];
                bf[j][e] = v;
            }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
    }

    // register r of acc[i][j] is row m0 + 32 i + (r & 3) + 8 (r >> 2) + 4 kl, column n0 + 32 j + ml
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * kl;
            if (m >= N) continue;
            const float em = ev[m];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + 32 * j + ml;
                if (n < b) out[(size_t)m * ldo + n] = acc[i][j][r] - em * X[(size_t)m * ldx + n];
            }
        }
}

}  // namespace

extern "C" int tag_spectral_chain(void) { return L; }

extern "C" size_t tag_spectral_gram_ws_bytes(int N, int p, int q) {
    if (!gram_shape_ok(N, p, q)) return 0;
    return (size_t)cdiv(N, L) * p * q * sizeof(float);
}

extern "C" int tag_spectral_gram(const float* P, int ldp, const float* Q, int ldq, const float* w, double* out, int ldo, int N, int p,
                                 int q, void* ws, void* stream) {
    TAG_CHECK_ARG(P && Q && out && ws);
    if (N < 1 || p < 1 || q < 1) {
        tag_set_error("tag_spectral_gram: N, p, q must be >= 1 (got %d, %d, %d)", N, p, q);
        return TAG_EINVAL;
    }
    if (!gram_shape_ok(N, p, q)) {
        tag_set_error("tag_spectral_gram: N = %d, p = %d, q = %d: N at most %d, p and q at most 32768, and tiles x slices at most %d",
                      N, p, q, INT_MAX - L, INT_MAX);
        return TAG_EINVAL;
    }
    if (ldp < p || ldq < q || ldo < q) {
        tag_set_error("tag_spectral_gram: row strides ldp = %d, ldq = %d, ldo = %d must be >= p = %d, q = %d, q = %d", ldp, ldq, ldo,
                      p, q, q);
        return TAG_EINVAL;
    }
    const bool sym = P == Q && ldp == ldq && p == q;
    const GramPlan g = gram_plan(N, p, q, sym);
    hipStream_t st = as_stream(stream);
    float* part = static_cast<float*>(ws);
    if (w)
        hipLaunchKernelGGL(spectral_gram_kernel<true>, dim3((unsigned)g.blocks), dim3(256), 0, st, P, ldp, Q, ldq, w, part, N, p, q,
                           g.tp, g.tq, g.tiles, sym);
    else
        hipLaunchKernelGGL(spectral_gram_kernel<false>, dim3((unsigned)g.blocks), dim3(256), 0, st, P, ldp, Q, ldq, w, part, N, p, q,
                           g.tp, g.tq, g.tiles, sym);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(spectral_gram_fold_kernel, dim3(cdiv((long)p * q, 256)), dim3(256), 0, st, part, g.slices, p, q, out, ldo, sym);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_spectral_rows(const float* u, int ldu, const double* t, float* Y, int ldy, float* s, float* e, int N, int D,
                                 void* stream) {
    TAG_CHECK_ARG(u && t && Y && s && e);
    if (N < 1 || D < 1 || D == INT_MAX) {
        tag_set_error("tag_spectral_rows: N, D must be >= 1 and D + 1 an int (got %d, %d)", N, D);
        return TAG_EINVAL;
    }
    if (ldu < D || ldy < D + 1) {
        tag_set_error("tag_spectral_rows: row strides ldu = %d, ldy = %d must be >= D = %d, D + 1 = %d", ldu, ldy, D, D + 1);
        return TAG_EINVAL;
    }
    hipLaunchKernelGGL(spectral_rows_kernel, dim3(cdiv(N, ROWS_PER_WG)), dim3(256), 0, as_stream(stream), u, ldu, t, Y, ldy, s, e, N,
                       D);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_spectral_apply(const float* Y, int ldy, const float* Tm, int ldt, const float* e, const float* X, int ldx,
                                  float* out, int ldo, int N, int Dp, int b, void* stream) {
    TAG_CHECK_ARG(Y && Tm && e && X && out);
    if (N < 1 || Dp < 1 || b < 1) {
        tag_set_error("tag_spectral_apply: N, Dp, b must be >= 1 (got %d, %d, %d)", N, Dp, b);
        return TAG_EINVAL;
    }
    const long blocks = (long)cdiv(N, T) * cdiv(b, T);
    if (N > INT_MAX - T || b > INT_MAX - T || Dp > INT_MAX - 32 || blocks > INT_MAX) {
        tag_set_error("tag_spectral_apply: N = %d, Dp = %d, b = %d: N and b at most %d, Dp at most %d, and %ld tiles at most %d", N,
                      Dp, b, INT_MAX - T, INT_MAX - 32, blocks, INT_MAX);
        return TAG_EINVAL;
    }
    if (ldy < Dp || ldt < b || ldx < b || ldo < b) {
        tag_set_error("tag_spectral_apply: row strides ldy = %d, ldt = %d, ldx = %d, ldo = %d must be >= Dp = %d, b = %d, b, b", ldy,
                      ldt, ldx, ldo, Dp, b);
        return TAG_EINVAL;
    }
    const bool al = aligned16(Y) && ldy % 4 == 0;
    hipLaunchKernelGGL(spectral_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), Y, ldy, Tm, ldt, e, X, ldx, out,
                       ldo, N, Dp, b, cdiv(b, T), al);
    TAG_LAUNCH_CHECK();
    return 0;
}
