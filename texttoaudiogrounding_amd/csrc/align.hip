// align.ExpNegL2 (models/align.py:34-64 in the reference): every clip's frames against every clip's phrases,
//   out[a][i][t][j] = exp(-|| an[a,t,:] - tn[i,j,:] ||_2)        an, tn = the F.normalize'd rows of audio (B,T,D) / text (B,N,D)
// in the (B,B,T,N) layout of align.DotProduct.  The rows are normalised by a row pass of this file that DIVIDES by the norm
// (tag_l2norm_rows_forward multiplies by its reciprocal: x * (1/|x|) is not always +-1, so at D = 1, where the true gradient is
// identically zero, and between rows that are multiples of each other, the quotient form is exact and the product form is not).
// With M = B*T audio rows and P = B*N text rows the rest is three passes over row pairs:
//   forward      dist[m][p] = sqrt(sum_d (an[m][d] - tn[p][d])^2),  out = exp(-dist)
//   coefficient  g[m][p]    = -dout * exp(-dist) / dist  (0 where dist == 0, as torch.norm's backward) -- the distance is
//                             RECOMPUTED by the forward's own loop (same bits), not recovered as -log(out)
//   pair sums    dan[m][:]  = sum_p g[m][p] (an[m] - tn[p]),   dtn[p][:] = sum_m g[m][p] (tn[p] - an[m])
// The squared distance is the sum of squared differences (no 2 - 2 cos: at distance 0.07 that form loses two digits), and
// the pair sums multiply the differences themselves instead of composing (sum g) an - G tn from two GEMMs, whose terms
// cancel as the rows approach each other.  (a - b)^2 has no MFMA form: these are VALU kernels tiled like a GEMM -- a 64 x 64
// tile of pairs per 256-thread workgroup, 4 x 4 accumulators per lane, both operand tiles in LDS per chunk of D (or of the
// summed rows), 16-byte loads where D is a multiple of 4 and the base is aligned, scalar loads otherwise.  Every sum runs in
// a fixed order (chunk sums of 32 terms, then the chunks in order, then the slices of a cut pass in order): no atomics, the
// same bits on every run.  Any B, T, N,
// D >= 1 within the index limits checked by the launchers; nothing of size (M, P, D) exists anywhere.
#include "tag_common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int TILE = 64;          // rows of either operand (and columns of D in the pair sums) per workgroup
constexpr int KC = 32;            // chunk of the summed index held in LDS
constexpr int LDK = KC + 4;       // row stride of a [TILE][KC] tile: 16-byte aligned rows, and 16 rows (stride 36 floats) start on
                                  // 16 different 4-bank slots, so the b128 reads of a 16-lane group do not conflict
constexpr int LDD = TILE + 4;     // row stride of a [KC][TILE] tile
constexpr long GRID_Y_MAX = 65535;

// dst[r][c] (stride ld) = src[(row0 + r) * D + col0 + c] for r < ROWS, c < COLS; zero outside rows_total x D.
// COLS is a multiple of 4; vec: D % 4 == 0 and a 16-byte aligned base, so a group of 4 columns is inside or outside as a whole.
template <int ROWS, int COLS>
__device__ __forceinline__ void load_tile(float* __restrict__ dst, int ld, const float* __restrict__ src, long rows_total,
                                          long row0, int col0, int D, bool vec) {
    constexpr int Q = COLS / 4;
    for (int idx = threadIdx.x; idx < ROWS * Q; idx += 256) {
        const int r = idx / Q, c = (idx % Q) * 4;
        const long row = row0 + r;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (row < rows_total) {
            const float* p = src + row * D + col0 + c;
            if (vec) {
                if (col0 + c < D) v = *reinterpret_cast<const f32x4*>(p);
            } else {
                if (col0 + c + 0 < D) v.x = p[0];
                if (col0 + c + 1 < D) v.y = p[1];
                if (col0 + c + 2 < D) v.z = p[2];
                if (col0 + c + 3 < D) v.w = p[3];
            }
        }
        *reinterpret_cast<f32x4*>(dst + r * ld + c) = v;
    }
}

// Squared distances of a 64 x 64 tile of (audio row, text row) pairs; lane (tx, ty) owns rows m0 + ty + 16 i and p0 + tx + 16 j.
// MODE 0: out (B,B,T,N) = exp(-dist).   MODE 1: g (M,P) = -dout * exp(-dist) / dist, dout in the (B,B,T,N) layout.
template <int MODE>
__global__ __launch_bounds__(256) void expnegl2_pairs_kernel(const float* __restrict__ an, const float* __restrict__ tn,
                                                             const float* __restrict__ dout, float* __restrict__ res, int B,
                                                             int T, int N, int D, int vec) {
    __shared__ __attribute__((aligned(16))) float As[TILE * LDK];
    __shared__ __attribute__((aligned(16))) float Bs[TILE * LDK];
    const long M = (long)B * T, P = (long)B * N;
    const long m0 = (long)blockIdx.x * TILE, p0 = (long)blockIdx.y * TILE;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < D; k0 += KC) {
        load_tile<TILE, KC>(As, LDK, an, M, m0, k0, D, vec != 0);
        load_tile<TILE, KC>(Bs, LDK, tn, P, p0, k0, D, vec != 0);
        __syncthreads();
        float part[4][4] = {};
#pragma unroll 2
        for (int k = 0; k < KC; k += 4) {
            f32x4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(As + (ty + 16 * i) * LDK + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const f32x4*>(Bs + (tx + 16 * j) * LDK + k);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d0 = a[i].x - b[j].x, d1 = a[i].y - b[j].y, d2 = a[i].z - b[j].z, d3 = a[i].w - b[j].w;
                    part[i][j] = fmaf(d3, d3, fmaf(d2, d2, fmaf(d1, d1, fmaf(d0, d0, part[i][j]))));
                }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += part[i][j];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long m = m0 + ty + 16 * i;
        if (m >= M) continue;
        const long a = m / T, t = m % T;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long p = p0 + tx + 16 * j;
            if (p >= P) continue;
            const long c = p / N, n = p % N;
            const size_t o = (((size_t)a * B + c) * T + t) * N + n;
            const float dist = sqrtf(acc[i][j]);
            const float e = expf(-dist);
            if (MODE == 0) res[o] = e;
            else res[(size_t)m * P + p] = dist > 0.0f ? -dout[o] * e / dist : 0.0f;
        }
    }
}

// dx[r][:] = sum_s c(r,s) (x[r][:] - y[s][:]) for R rows x, S rows y;  c(r,s) = g[r * S + s], or g[s * R + r] when TRANS.
// A 64-row x 64-column tile of dx per workgroup; lane (tx, ty) owns rows r0 + ty + 16 i and columns d0 + 4 tx .. + 3.
// blockIdx.z = slice of the summed rows (chunks_per_slice chunks of KC rows each): with more than one slice every slice
// leaves its sum in its own (R, D) slab of dx and expnegl2_fold_kernel adds the slabs in slice order.
template <bool TRANS>
__global__ __launch_bounds__(256) void expnegl2_pairsum_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                               const float* __restrict__ y, float* __restrict__ dx, long R,
                                                               long S, int D, int vec, int chunks_per_slice) {
    __shared__ __attribute__((aligned(16))) float Cs[TILE * LDK];
    __shared__ __attribute__((aligned(16))) float Ys[KC * LDD];
    const long r0 = (long)blockIdx.x * TILE;
    const int d0 = blockIdx.y * TILE;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int dc = d0 + 4 * tx;
    float xr[4][4], acc[4][4] = {};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long r = r0 + ty + 16 * i;
#pragma unroll
        for (int q = 0; q < 4; ++q) xr[i][q] = (r < R && dc + q < D) ? x[r * D + dc + q] : 0.0f;
    }
    const long s_lo = (long)blockIdx.z * chunks_per_slice * KC;
    const long s_hi = s_lo + (long)chunks_per_slice * KC < S ? s_lo + (long)chunks_per_slice * KC : S;
    dx += (size_t)blockIdx.z * R * D;
    for (long s0 = s_lo; s0 < s_hi; s0 += KC) {
        // coefficients Cs[r][s]: lanes run along the contiguous index of g
        for (int idx = threadIdx.x; idx < TILE * KC; idx += 256) {
            const int r = TRANS ? idx % TILE : idx / KC, s = TRANS ? idx / TILE : idx % KC;
            const long gr = r0 + r, gs = s0 + s;
            float c = 0.0f;
            if (gr < R && gs < S) c = TRANS ? g[(size_t)gs * R + gr] : g[(size_t)gr * S + gs];
            Cs[r * LDK + s] = c;
        }
        load_tile<KC, TILE>(Ys, LDD, y, S, s0, d0, D, vec != 0);
        __syncthreads();
        float part[4][4] = {};
#pragma unroll 2
        for (int s = 0; s < KC; s += 4) {
            f32x4 c[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = *reinterpret_cast<const f32x4*>(Cs + (ty + 16 * i) * LDK + s);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f32x4 yv = *reinterpret_cast<const f32x4*>(Ys + (s + u) * LDD + 4 * tx);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float ci = u == 0 ? c[i].x : u == 1 ? c[i].y : u == 2 ? c[i].z : c[i].w;
                    part[i][0] = fmaf(ci, xr[i][0] - yv.x, part[i][0]);
                    part[i][1] = fmaf(ci, xr[i][1] - yv.y, part[i][1]);
                    part[i][2] = fmaf(ci, xr[i][2] - yv.z, part[i][2]);
                    part[i][3] = fmaf(ci, xr[i][3] - yv.w, part[i][3]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][q] += part[i][q];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long r = r0 + ty + 16 * i;
        if (r >= R) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (dc + q < D) dx[r * D + dc + q] = acc[i][q];
    }
}

// y = x / max(||x||, 1e-12) (F.normalize), one wave per row
__global__ __launch_bounds__(256) void expnegl2_normalize_kernel(const float* __restrict__ x, float* __restrict__ y, long rows,
                                                                 int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float s = 0.0f;
    for (int d = lane; d < D; d += 64) { const float v = x[row * D + d]; s = fmaf(v, v, s); }
    const float n = fmaxf(sqrtf(wave_sum(s)), 1e-12f);
    for (int d = lane; d < D; d += 64) y[row * D + d] = x[row * D + d] / n;
}

// backward of F.normalize from the stored unit rows u: dx = (du - u (u . du)) / ||x||, or du / 1e-12 below the clamp (the
// clamped norm is a constant there), as autograd's
__global__ __launch_bounds__(256) void expnegl2_normalize_bwd_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                                     const float* __restrict__ du, float* __restrict__ dx,
                                                                     long rows, int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float ss = 0.0f, ud = 0.0f;
    for (int d = lane; d < D; d += 64) {
        const float v = x[row * D + d];
        ss = fmaf(v, v, ss);
        ud = fmaf(u[row * D + d], du[row * D + d], ud);
    }
    const float n = sqrtf(wave_sum(ss));
    ud = wave_sum(ud);
    for (int d = lane; d < D; d += 64)
        dx[row * D + d] = n > 1e-12f ? (du[row * D + d] - u[row * D + d] * ud) / n : du[row * D + d] / 1e-12f;
}

// dx[i] = part[0][i] + part[1][i] + ... in slice order, n = R * D elements per slab
__global__ __launch_bounds__(256) void expnegl2_fold_kernel(const float* __restrict__ part, int slices, long n,
                                                            float* __restrict__ dx) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float v = part[i];
        for (int z = 1; z < slices; ++z) v += part[(size_t)z * n + i];
        dx[i] = v;
    }
}

// Slices of the summed rows of one pair-sum pass: the text-side pass has few output tiles (B*N x D / 64^2 = 64 at the benched
// shape, a quarter of the CUs) and B*T rows to sum, so it is cut until about four workgroups per CU exist, a slice keeping at
// least two chunks.  A function of the shape alone: the same shape always sums in the same order.
struct Slices { int n, chunks_each; };
Slices pairsum_slices(long R, long S, int D) {
    const long tiles = (long)cdiv(R, TILE) * cdiv(D, TILE), chunks = (S + KC - 1) / KC;
    long want = (1024 + tiles - 1) / tiles;
    if (want > (chunks + 1) / 2) want = (chunks + 1) / 2;
    if (want < 1) want = 1;
    const long each = (chunks + want - 1) / want;
    return {(int)((chunks + each - 1) / each), (int)each};
}
size_t slab_floats(long R, long S, int D) {
    const Slices sl = pairsum_slices(R, S, D);
    return sl.n > 1 ? (size_t)sl.n * R * D : 0;
}

template <bool TRANS>
void launch_pairsum(const float* g, const float* x, const float* y, float* dx, float* slabs, long R, long S, int D, int vec,
                    hipStream_t st) {
    const Slices sl = pairsum_slices(R, S, D);
    hipLaunchKernelGGL(expnegl2_pairsum_kernel<TRANS>, dim3(cdiv(R, TILE), cdiv(D, TILE), sl.n), dim3(256), 0, st, g, x, y,
                       sl.n > 1 ? slabs : dx, R, S, D, vec, sl.chunks_each);
    if (sl.n > 1) {
        const long n = R * D;
        hipLaunchKernelGGL(expnegl2_fold_kernel, dim3((int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, st,
                           slabs, sl.n, n, dx);
    }
}

// index limits shared by the launchers: row counts and the (M, P) / (B,B,T,N) element count as used by the kernels
int check_shape(const char* what, int B, int T, int N, int D) {
    if (B < 1 || T < 1 || N < 1 || D < 1) {
        tag_set_error("%s: B, T, N, D must be >= 1 (got %d, %d, %d, %d)", what, B, T, N, D);
        return TAG_EINVAL;
    }
    const long M = (long)B * T, P = (long)B * N;
    if (M > INT_MAX || P > GRID_Y_MAX * TILE || (long)cdiv(D, TILE) > GRID_Y_MAX) {
        tag_set_error("%s: B*T = %ld exceeds %d, or B*N = %ld exceeds %ld, or D = %d exceeds %ld (grid and row-index limits)",
                      what, M, INT_MAX, P, GRID_Y_MAX * TILE, D, GRID_Y_MAX * TILE);
        return TAG_EINVAL;
    }
    return 0;
}

}  // namespace

extern "C" int tag_align_expnegl2_normalize(const float* x, float* y, long rows, int D, void* stream) {
    TAG_CHECK_ARG(x && y && rows > 0 && rows <= 4L * INT_MAX && D > 0);
    hipLaunchKernelGGL(expnegl2_normalize_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, as_stream(stream), x, y, rows, D);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_align_expnegl2_normalize_backward(const float* x, const float* u, const float* du, float* dx, long rows,
                                                     int D, void* stream) {
    TAG_CHECK_ARG(x && u && du && dx && rows > 0 && rows <= 4L * INT_MAX && D > 0);
    hipLaunchKernelGGL(expnegl2_normalize_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, as_stream(stream), x, u, du, dx, rows,
                       D);
    TAG_LAUNCH_CHECK();
    return 0;
}

// workspace: g (B*T, B*N), then the slabs of whichever pair-sum pass needs more
extern "C" size_t tag_align_expnegl2_ws_bytes(int B, int T, int N, int D) {
    if (B < 1 || T < 1 || N < 1 || D < 1) return 0;
    const long M = (long)B * T, P = (long)B * N;
    const size_t a = slab_floats(M, P, D), t = slab_floats(P, M, D);
    return ((size_t)M * P + (a > t ? a : t)) * sizeof(float);
}

extern "C" int tag_align_expnegl2_forward(const float* an, const float* tn, float* out, int B, int T, int N, int D,
                                          void* stream) {
    TAG_CHECK_ARG(an && tn && out);
    if (int rc = check_shape("tag_align_expnegl2_forward", B, T, N, D)) return rc;
    const int vec = D % 4 == 0 && aligned16(an) && aligned16(tn);
    hipLaunchKernelGGL(expnegl2_pairs_kernel<0>, dim3(cdiv((long)B * T, TILE), cdiv((long)B * N, TILE)), dim3(256), 0,
                       as_stream(stream), an, tn, static_cast<const float*>(nullptr), out, B, T, N, D, vec);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_align_expnegl2_backward(const float* an, const float* tn, const float* dout, float* dan, float* dtn, int B,
                                           int T, int N, int D, void* ws, void* stream) {
    TAG_CHECK_ARG(an && tn && dout && dan && dtn && ws);
    if (int rc = check_shape("tag_align_expnegl2_backward", B, T, N, D)) return rc;
    const long M = (long)B * T, P = (long)B * N;
    const int vec = D % 4 == 0 && aligned16(an) && aligned16(tn);
    float* g = static_cast<float*>(ws);
    hipLaunchKernelGGL(expnegl2_pairs_kernel<1>, dim3(cdiv(M, TILE), cdiv(P, TILE)), dim3(256), 0, as_stream(stream), an, tn,
                       dout, g, B, T, N, D, vec);
    TAG_LAUNCH_CHECK();
    float* slabs = g + (size_t)M * P;          // the first pass's fold has read them before the second pass writes (stream order)
    launch_pairsum<false>(g, an, tn, dan, slabs, M, P, D, vec, as_stream(stream));
    TAG_LAUNCH_CHECK();
    launch_pairsum<true>(g, tn, an, dtn, slabs, P, M, D, vec, as_stream(stream));
    TAG_LAUNCH_CHECK();
    return 0;
}
