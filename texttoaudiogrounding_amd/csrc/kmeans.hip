// Device k-means for phrase clustering (python_scripts/clustering/kmeans_emb.py in the reference, which runs sklearn's KMeans on
// the host; utils/phrase_cluster.py drives these three entry points).
//
// tag_kmeans_assign:  label[i] = argmin_k (||c_k||^2 - 2 x_i . c_k), ties to the lowest k, and dist2[i] = sum_d (x_id - c_label,d)^2.
//   The products are the marching kernel of march_f32.h: a workgroup owns 128 rows of x and walks ALL 128-column tiles of the
//   centres on the exact-fp32 MFMA.  When a tile's K loop ends each lane turns its 64 accumulator values into scores and keeps a
//   running (score, index) pair per row it holds (32 rows); a column past K scores +inf (a zero-filled centre would score 0 and
//   beat every positive real score).  A lane sees its columns in ascending order and replaces on < only; at the end the 64 lanes
//   that share a row fold through LDS on (score, index), so the lowest k wins a tie.  Identical centre rows give bit-identical
//   scores in any column (the same chain of k-steps, the same ||c||^2 kernel), so that rule is exact.  No (N, K) scores exist.
//   ||c_k||^2 goes to ws once per call (K floats); dist2 comes from the differences in a second small launch, one wave per row
//   (never from the expansion: inertia and the datasets' distance percentile read it).
//
// tag_kmeans_update:  sums = onehot^T . x as an MFMA reduction over the rows.  A wave owns one 32-column tile of d and KT
//   32-cluster tiles (KT = 1, 2 or 4 by K); per MFMA it takes two rows: the A operand is formed in registers from
//   label[i] == k (no one-hot matrix in memory), the B operand is x[i][d0 + lane % 32], a coalesced read, and is reused by the
//   KT products.  The four waves of a workgroup take quarters of one row slice and add their accumulators through LDS in wave
//   order; the slice's fp32 partial goes to ws[slice][k][d] and its integer counts to the tail of ws.  A second launch folds the
//   slices in fp64 in slice order, writes sums and count, and divides where count > 0 (a row with count 0 is left untouched).
//   No atomics, ws is never zeroed, the same bits on every run.  (A NaN in x reaches every cluster's sum of its column: 0 * NaN.)
//
// tag_kmeans_seed_step:  closest[i] = min(closest[i], ||x_i - x_p||^2) with p read from a device int64 (k-means++ without a host
//   round trip); first != 0 writes the distance without the min.  Row-wise fp32 differences, one wave per row.
#include "march_f32.h"
#include <math.h>

namespace {

using namespace march;

// ------------------------------------------------------------------------------------------------------------------------
// assignment
// ------------------------------------------------------------------------------------------------------------------------
constexpr size_t LDS_BYTES = STAGE_BYTES;
static_assert((size_t)2 * T * RED_LD * sizeof(float) <= LDS_BYTES, "the fold reuses the stage buffers");

template <bool FX, bool FC>
__global__ __launch_bounds__(256, 2) void kmeans_assign_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ c,
                                                               int ldc, const float* __restrict__ cnorm, int* __restrict__ label,
                                                               int N, int K, int D, bool x_al, bool c_al) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int m0 = blockIdx.x * T;
    const Lanes l = lanes();

    float best[2][16];
    int bidx[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            best[i][r] = INFINITY;
            bidx[i][r] = 0;
        }

    // This lane meets its columns in ascending order (tile, then j) and replaces on < only.
    march_tiles<FX, FC>(smem, Rows{x, ldx, N, x_al}, Rows{c, ldc, K, c_al}, m0, 0, (K + T - 1) / T, D,
                        [&](int tile, const f32x16 (&acc)[2][2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = tile * T + l.wn0 + j * 32 + l.ml;
            const bool real = n < K;
            const float cn = real ? cnorm[n] : 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float s = real ? cn - 2.0f * acc[i][j][r] : INFINITY;
                    const bool take = s < best[i][r];
                    best[i][r] = take ? s : best[i][r];
                    bidx[i][r] = take ? n : bidx[i][r];
                }
        }
    });

    // fold the 64 lanes (2 waves x 32 columns) that share a row on (score, index); the stage buffers are free after the last barrier
    float* rs = smem;
    int* ri = reinterpret_cast<int*>(smem + T * RED_LD);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = fold_slot(l, i, r);
            rs[o] = best[i][r];
            ri[o] = bidx[i][r];
        }
    __syncthreads();
    if (threadIdx.x < T && m0 + (int)threadIdx.x < N) {
        float bs = rs[threadIdx.x * RED_LD];
        int bn = ri[threadIdx.x * RED_LD];
        for (int e = 1; e < 64; ++e) {
            const float s = rs[threadIdx.x * RED_LD + e];
            const int n = ri[threadIdx.x * RED_LD + e];
            if (s < bs || (s == bs && n < bn)) {
                bs = s;
                bn = n;
            }
        }
        label[m0 + threadIdx.x] = bn;
    }
}

// sum_d (a[d] - b[d])^2 of one row pair by one wave, lanes striding d (coalesced), then a butterfly: every lane gets the sum
__device__ __forceinline__ float wave_sqdist(const float* __restrict__ a, const float* __restrict__ b, int D, int lane) {
    float s = 0.0f;
    for (int d = lane; d < D; d += 64) {
        const float t = a[d] - b[d];
        s += t * t;
    }
    return wave_sum(s);
}

constexpr int ROWS_PER_WG = 4;    // one wave per row

__global__ __launch_bounds__(256) void kmeans_cnorm_kernel(const float* __restrict__ c, int ldc, float* __restrict__ cnorm, int K,
                                                           int D) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (k >= K) return;
    const float* row = c + (size_t)k * ldc;
    float s = 0.0f;
    for (int d = lane; d < D; d += 64) s += row[d] * row[d];
    s = wave_sum(s);
    if (lane == 0) cnorm[k] = s;
}

__global__ __launch_bounds__(256) void kmeans_dist2_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ c, int ldc,
                                                           const int* __restrict__ label, float* __restrict__ dist2, int N, int D) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (i >= N) return;
    const float s = wave_sqdist(x + (size_t)i * ldx, c + (size_t)label[i] * ldc, D, lane);
    if (lane == 0) dist2[i] = s;
}

__global__ __launch_bounds__(256) void kmeans_seed_kernel(const float* __restrict__ x, int ldx, const long long* __restrict__ pick,
                                                          float* __restrict__ closest, int first, int N, int D) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    const long long p = *pick;
    if (i >= N || p < 0 || p >= N) return;          // (a pick outside the rows writes nothing)
    const float s = wave_sqdist(x + (size_t)i * ldx, x + (size_t)p * ldx, D, lane);
    if (lane == 0) closest[i] = first ? s : fminf(closest[i], s);
}

// ------------------------------------------------------------------------------------------------------------------------
// update
// ------------------------------------------------------------------------------------------------------------------------
// Row slices (host, a function of the shape alone).  A workgroup is one (32-column tile of d, group of KT 32-cluster tiles, row
// slice); the launch wants UPD_WGS workgroups, so the rows are cut into want = ceil(UPD_WGS / (d tiles x cluster groups))
// slices of rows_each = max(UPD_ROWS_MIN, ceil(N / want)) rows, rounded up to a multiple of 8 (four waves x two rows per MFMA);
// slices = ceil(N / rows_each), the last one short.  ws = slices x K x (D floats + one int).
constexpr int UPD_WGS = 512;
constexpr int UPD_ROWS_MIN = 128;
constexpr int UPD_U = 8;          // row pairs in flight per wave
constexpr int NO_ROW = 1 << 30;   // added to label - cluster for a row past the end: equals no 32 t
struct UPlan { int kt, d_tiles, k_groups, rows_each, slices; };
UPlan make_uplan(int N, int K, int D) {
    UPlan p;
    p.kt = K <= 32 ? 1 : K <= 64 ? 2 : 4;
    p.d_tiles = cdiv(D, 32);
    p.k_groups = cdiv(K, 32 * p.kt);
    const long units = (long)p.d_tiles * p.k_groups;
    const long want = units >= UPD_WGS ? 1 : (UPD_WGS + units - 1) / units;
    long each = ((long)N + want - 1) / want;
    if (each < UPD_ROWS_MIN) each = UPD_ROWS_MIN;
    each = (each + 7) / 8 * 8;
    p.rows_each = (int)each;
    p.slices = cdiv(N, each);
    return p;
}

template <int KT>
__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ x, int ldx, const int* __restrict__ label,
                                                            float* __restrict__ part, int* __restrict__ pcnt, int N, int K, int D,
                                                            int rows_each) {
    __shared__ float red[3][KT * 16][64];
    __shared__ int cred[4][KT][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int half = lane >> 5, ml = lane & 31;
    const int d = blockIdx.x * 32 + ml;
    const int k0 = blockIdx.y * 32 * KT;
    const int slice = blockIdx.z;
    const int quarter = rows_each / 4;              // even: a row pair never straddles two waves
    const long lo = (long)slice * rows_each + (long)wid * quarter;
    long hi = lo + quarter;
    if (hi > N) hi = N;
    const bool dok = d < D;

    f32x16 acc[KT];
    int cnt[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        cnt[t] = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    }
    // MFMA lane roles: A[m = ml][k = half] = (label[row + half] == k0 + 32 t + ml), B[k = half][n = ml] = x[row + half][d].
    // The loads of a batch of UPD_U row pairs are UNCONDITIONAL on a clamped row and column (always inside x and label): a load
    // under a lane predicate becomes a branch with its own s_waitcnt vmcnt(0), which serialises the batch on the memory
    // latency.  A row past the end repeats the wave's last row with a label offset that matches no cluster (its products are
    // 0 * x); a column past D repeats column D - 1 and is never stored.
    const int dc = dok ? d : D - 1;
    for (long i = lo; i < hi; i += 2 * UPD_U) {
        float xv[UPD_U];
        int rel[UPD_U];
#pragma unroll
        for (int u = 0; u < UPD_U; ++u) {
            const long row = i + 2 * u + half;
            const long rc = row < hi ? row : hi - 1;
            rel[u] = label[rc];
            xv[u] = x[(size_t)rc * ldx + dc];
        }
        // all loads of the batch first and nothing that reads them: interleaved with their uses, each is waited for on its own
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UPD_U; ++u) rel[u] += (i + 2 * u + half < hi ? 0 : NO_ROW) - k0 - ml;
#pragma unroll
        for (int u = 0; u < UPD_U; ++u)
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const bool hit = rel[u] == 32 * t;
                cnt[t] += hit ? 1 : 0;
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(hit ? 1.0f : 0.0f, xv[u], acc[t], 0, 0, 0);
            }
    }

    // the four quarters of the slice: waves 1..3 hand their accumulators to wave 0, which adds them in wave order
    if (wid > 0) {
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) red[wid - 1][t * 16 + r][lane] = acc[t][r];
    }
#pragma unroll
    for (int t = 0; t < KT; ++t) cred[wid][t][lane] = cnt[t];
    __syncthreads();
    if (wid == 0) {
#pragma unroll 1                  // (unrolled, the 3 x 16 KT LDS reads are all hoisted: 320 VGPRs at KT = 4)
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] += red[w][t * 16 + r][lane];
        // register r of acc[t] is cluster k0 + 32 t + (r & 3) + 8 (r >> 2) + 4 half, column d
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = k0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (k < K && dok) part[((size_t)slice * K + k) * D + d] = acc[t][r];
            }
    }
    if (blockIdx.x == 0 && threadIdx.x < 32 * KT) {
        const int t = threadIdx.x >> 5, m = threadIdx.x & 31;
        const int k = k0 + 32 * t + m;
        int n = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) n += cred[w][t][m] + cred[w][t][m + 32];
        if (k < K) pcnt[(size_t)slice * K + k] = n;
    }
}

// one workgroup per cluster: count[k] = sum of the slices' counts, sums[k][d] = the slices' partials added in fp64 in slice order,
// centers[k][d] = sums / count where count > 0
__global__ __launch_bounds__(256) void kmeans_update_fold_kernel(const float* __restrict__ part, const int* __restrict__ pcnt,
                                                                 int slices, double* __restrict__ sums, long long* __restrict__ count,
                                                                 float* __restrict__ centers, int ldc, int K, int D) {
    __shared__ long long wsum[4];
    const int k = blockIdx.x;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    long long n = 0;
    for (int z = threadIdx.x; z < slices; z += 256) n += pcnt[(size_t)z * K + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) wsum[wid] = n;
    __syncthreads();
    n = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (threadIdx.x == 0) count[k] = n;
    for (int d = threadIdx.x; d < D; d += 256) {
        double s = 0.0;
#pragma unroll 8
        for (int z = 0; z < slices; ++z) s += (double)part[((size_t)z * K + k) * D + d];
        sums[(size_t)k * D + d] = s;
        if (n > 0) centers[(size_t)k * ldc + d] = (float)(s / (double)n);
    }
}


// row and tile origins (N + 127, K + 127, D + 31) are ints; the assign grid is one-dimensional, the update grid's y and z are
// cluster groups (<= 65535) and slices (<= UPD_WGS)
constexpr int K_MAX = 65535 * 32;
int check_shape(const char* fn, int N, int K, int D) {
    if (N < 1 || K < 1 || D < 1) {
        tag_set_error("%s: N, K, D must be >= 1 (got %d, %d, %d)", fn, N, K, D);
        return TAG_EINVAL;
    }
    if (int rc = check_index_limit(fn, "N", N, T, "row")) return rc;
    if (K > K_MAX) {
        tag_set_error("%s: K = %d exceeds %d (cluster group limit of the launch grid)", fn, K, K_MAX);
        return TAG_EINVAL;
    }
    if (int rc = check_index_limit(fn, "D", D, KC, "chunk")) return rc;
    return 0;
}

template <bool FX, bool FC>
void launch_assign(const float* x, int ldx, const float* c, int ldc, const float* cnorm, int* label, int N, int K, int D, bool x_al,
                   bool c_al, hipStream_t st) {
    static bool attr_set = false;         // (once per process, as gemm.hip's launchers: the library drives one device per process)
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&kmeans_assign_kernel<FX, FC>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
        attr_set = true;
    }
    hipLaunchKernelGGL((kmeans_assign_kernel<FX, FC>), dim3(cdiv(N, T)), dim3(256), LDS_BYTES, st, x, ldx, c, ldc, cnorm, label, N,
                       K, D, x_al, c_al);
}

template <int KT>
void launch_update(const float* x, int ldx, const int* label, float* part, int* pcnt, int N, int K, int D, const UPlan& p,
                   hipStream_t st) {
    hipLaunchKernelGGL(kmeans_update_kernel<KT>, dim3(p.d_tiles, p.k_groups, p.slices), dim3(256), 0, st, x, ldx, label, part, pcnt,
                       N, K, D, p.rows_each);
}

bool shape_ok(int N, int K, int D) { return N >= 1 && K >= 1 && D >= 1 && N <= INT_MAX - T && K <= K_MAX && D <= INT_MAX - KC; }

}  // namespace

extern "C" size_t tag_kmeans_assign_ws_bytes(int N, int K, int D) {
    if (!shape_ok(N, K, D)) return 0;
    return (size_t)K * sizeof(float);
}

extern "C" int tag_kmeans_assign(const float* x, int ldx, const float* centers, int ldc, int* label, float* dist2, int N, int K,
                                 int D, void* ws, void* stream) {
    TAG_CHECK_ARG(x && centers && label && dist2 && ws);
    if (int rc = check_shape("tag_kmeans_assign", N, K, D)) return rc;
    if (ldx < D || ldc < D) {
        tag_set_error("tag_kmeans_assign: row strides ldx = %d, ldc = %d must be >= D = %d", ldx, ldc, D);
        return TAG_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    float* cnorm = static_cast<float*>(ws);
    hipLaunchKernelGGL(kmeans_cnorm_kernel, dim3(cdiv(K, ROWS_PER_WG)), dim3(256), 0, st, centers, ldc, cnorm, K, D);
    TAG_LAUNCH_CHECK();
    const bool x_al = aligned16(x) && ldx % 4 == 0, c_al = aligned16(centers) && ldc % 4 == 0;
    const bool fx = x_al && N % T == 0 && D % KC == 0, fc = c_al && K % T == 0 && D % KC == 0;
    if (fx && fc) launch_assign<true, true>(x, ldx, centers, ldc, cnorm, label, N, K, D, x_al, c_al, st);
    else if (fx) launch_assign<true, false>(x, ldx, centers, ldc, cnorm, label, N, K, D, x_al, c_al, st);
    else if (fc) launch_assign<false, true>(x, ldx, centers, ldc, cnorm, label, N, K, D, x_al, c_al, st);
    else launch_assign<false, false>(x, ldx, centers, ldc, cnorm, label, N, K, D, x_al, c_al, st);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(kmeans_dist2_kernel, dim3(cdiv(N, ROWS_PER_WG)), dim3(256), 0, st, x, ldx, centers, ldc, label, dist2, N, D);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t tag_kmeans_update_ws_bytes(int N, int K, int D) {
    if (!shape_ok(N, K, D)) return 0;
    return (size_t)make_uplan(N, K, D).slices * K * ((size_t)D * sizeof(float) + sizeof(int));
}

extern "C" int tag_kmeans_update(const float* x, int ldx, const int* label, double* sums, long long* count, float* centers, int ldc,
                                 int N, int K, int D, void* ws, void* stream) {
    TAG_CHECK_ARG(x && label && sums && count && centers && ws);
    if (int rc = check_shape("tag_kmeans_update", N, K, D)) return rc;
    if (ldx < D || ldc < D) {
        tag_set_error("tag_kmeans_update: row strides ldx = %d, ldc = %d must be >= D = %d", ldx, ldc, D);
        return TAG_EINVAL;
    }
    const UPlan p = make_uplan(N, K, D);
    hipStream_t st = as_stream(stream);
    float* part = static_cast<float*>(ws);
    int* pcnt = reinterpret_cast<int*>(part + (size_t)p.slices * K * D);
    if (p.kt == 1) launch_update<1>(x, ldx, label, part, pcnt, N, K, D, p, st);
    else if (p.kt == 2) launch_update<2>(x, ldx, label, part, pcnt, N, K, D, p, st);
    else launch_update<4>(x, ldx, label, part, pcnt, N, K, D, p, st);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(kmeans_update_fold_kernel, dim3(K), dim3(256), 0, st, part, pcnt, p.slices, sums, count, centers, ldc, K, D);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_kmeans_seed_step(const float* x, int ldx, const long long* pick, float* closest, int first, int N, int D,
                                    void* stream) {
    TAG_CHECK_ARG(x && pick && closest);
    if (int rc = check_shape("tag_kmeans_seed_step", N, 1, D)) return rc;
    if (ldx < D) {
        tag_set_error("tag_kmeans_seed_step: row stride ldx = %d must be >= D = %d", ldx, D);
        return TAG_EINVAL;
    }
    hipLaunchKernelGGL(kmeans_seed_kernel, dim3(cdiv(N, ROWS_PER_WG)), dim3(256), 0, as_stream(stream), x, ldx, pick, closest, first, N, D);
    TAG_LAUNCH_CHECK();
    return 0;
}
