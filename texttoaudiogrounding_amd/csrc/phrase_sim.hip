// Thresholded similarity count (utils/data/calc_phrase_sim_count.py in the reference, which calls cosine_similarity once per
// phrase and keeps the phrases at or above a threshold):
//   out[i] = sum_j weight[j] * [ sum_d q[i,d] * bank[j,d] >= threshold ]
// The N x N score matrix never exists: a workgroup owns 128 query rows and one SLICE of the bank's 128-column tiles and marches
// over the slice on the exact-fp32 MFMA (march_f32.h: the loop, the LDS image and the column-slice plan; a cosine lands on the
// side of the threshold where fp32 numpy puts it).  When a tile's K loop ends each lane compares its 64 accumulator values with
// the threshold and adds the column's weight into one int64 register per row it holds (32 rows).  At the end of the slice the
// 64 lanes that share a row fold their sums through LDS in lane order and the row's partial goes to ws[slice][row]; a second
// launch adds the slices in a fixed order.  Integer sums do not depend on the order, but the two-launch form keeps the library
// free of atomics and ws free of any zeroing.  ws = slices x M int64: 2 MB at M = N = 32768.
#include "march_f32.h"

namespace {

using namespace march;
constexpr size_t LDS_BYTES = STAGE_BYTES;
static_assert((size_t)T * RED_LD * sizeof(long long) <= LDS_BYTES, "the fold reuses the stage buffers");

Plan plan_of(int M, int N) { return make_plan(cdiv(M, T), cdiv(N, T)); }

template <bool FAST>
__global__ __launch_bounds__(256, 2) void phrase_sim_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ bank,
                                                            int ldb, const long long* __restrict__ weight, float thr,
                                                            long long* __restrict__ ws, int M, int N, int D, int m_tiles,
                                                            int n_tiles, int group, int slices, int tiles_each, bool q_al,
                                                            bool b_al) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Share sh = plan_share(n_tiles, group, slices, tiles_each);
    if (sh.mt >= m_tiles) return;
    const int m0 = sh.mt * T, slice = sh.slice;
    const Lanes l = lanes();

    long long cnt[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) cnt[i][r] = 0;

    // A column past N (its bank rows were zero-filled: score 0) weighs nothing.
    march_tiles<FAST, FAST>(smem, Rows{q, ldq, M, q_al}, Rows{bank, ldb, N, b_al}, m0, sh.t_lo, sh.t_hi, D,
                            [&](int tile, const f32x16 (&acc)[2][2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = tile * T + l.wn0 + j * 32 + l.ml;
            const long long w = n < N ? (weight ? weight[n] : 1LL) : 0LL;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) cnt[i][r] += acc[i][j][r] >= thr ? w : 0LL;
        }
    });

    // fold the 64 lanes (2 waves x 32 columns) that share a row, in lane order; the stage buffers are free after the last barrier
    long long* red = reinterpret_cast<long long*>(smem);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[fold_slot(l, i, r)] = cnt[i][r];
    __syncthreads();
    if (threadIdx.x < T && m0 + (int)threadIdx.x < M) {
        long long s = 0;
        for (int c = 0; c < 64; ++c) s += red[threadIdx.x * RED_LD + c];
        ws[(size_t)slice * M + m0 + threadIdx.x] = s;
    }
}

// out[m] = ws[0][m] + ws[1][m] + ...: 16 rows per workgroup, 16 threads per row; thread g of a row adds slices g, g + 16, ...
// in slice order and the row's 16 sums are added in thread order.  (One thread per row walking all slices took 62 us for the
// 256 slices of M = 128, N = 32768 -- a chain of dependent-latency loads longer than the main kernel's 42 us.)
constexpr int FOLD_ROWS = 16, FOLD_WAYS = 16;
__global__ __launch_bounds__(256) void phrase_sim_fold_kernel(const long long* __restrict__ ws, int slices, int M,
                                                              long long* __restrict__ out) {
    __shared__ long long part[FOLD_WAYS][FOLD_ROWS];
    const int r = threadIdx.x % FOLD_ROWS, g = threadIdx.x / FOLD_ROWS;
    const int m = blockIdx.x * FOLD_ROWS + r;
    long long s = 0;
    if (m < M) {
#pragma unroll 4
        for (int z = g; z < slices; z += FOLD_WAYS) s += ws[(size_t)z * M + m];
    }
    part[g][r] = s;
    __syncthreads();
    if (g == 0 && m < M) {
        long long t = 0;
#pragma unroll
        for (int k = 0; k < FOLD_WAYS; ++k) t += part[k][r];
        out[m] = t;
    }
}

int check_shape(int M, int N, int D) {
    if (M < 1 || N < 1 || D < 1) {
        tag_set_error("tag_phrase_sim_count: M, N, D must be >= 1 (got %d, %d, %d)", M, N, D);
        return TAG_EINVAL;
    }
    // tile origins (tile * 128 <= N + 127, m0 + 127) and the chunk origin (D + 31) are ints; the grid is one-dimensional
    if (int rc = check_index_limit("tag_phrase_sim_count", "M", M, T, "row")) return rc;
    if (int rc = check_index_limit("tag_phrase_sim_count", "N", N, T, "row")) return rc;
    if (int rc = check_index_limit("tag_phrase_sim_count", "D", D, KC, "chunk")) return rc;
    const Plan p = plan_of(M, N);
    if (p.blocks > INT_MAX) {
        tag_set_error("tag_phrase_sim_count: M = %d, N = %d need %ld workgroups (%d query blocks x %d slices), more than the grid "
                      "limit %d", M, N, p.blocks, p.m_tiles, p.slices, INT_MAX);
        return TAG_EINVAL;
    }
    return 0;
}

template <bool FAST>
void launch_main(const float* q, int ldq, const float* bank, int ldb, const long long* weight, float thr, long long* ws, int M,
                 int N, int D, const Plan& p, bool q_al, bool b_al, hipStream_t st) {
    static bool attr_set = false;         // (once per process, as gemm.hip's launchers: the library drives one device per process)
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&phrase_sim_kernel<FAST>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)LDS_BYTES);
        attr_set = true;
    }
    hipLaunchKernelGGL(phrase_sim_kernel<FAST>, dim3((unsigned)p.blocks), dim3(256), LDS_BYTES, st, q, ldq, bank, ldb, weight, thr,
                       ws, M, N, D, p.m_tiles, p.n_tiles, p.group, p.slices, p.tiles_each, q_al, b_al);
}

}  // namespace

extern "C" size_t tag_phrase_sim_count_ws_bytes(int M, int N, int D) {
    if (M < 1 || N < 1 || D < 1 || M > INT_MAX - T || N > INT_MAX - T) return 0;
    return (size_t)plan_of(M, N).slices * M * sizeof(long long);
}

extern "C" int tag_phrase_sim_count(const float* q, int ldq, const float* bank, int ldb, const long long* weight, float threshold,
                                    long long* out, int M, int N, int D, void* ws, void* stream) {
    TAG_CHECK_ARG(q && bank && out && ws);
    if (int rc = check_shape(M, N, D)) return rc;
    if (ldq < D || ldb < D) {
        tag_set_error("tag_phrase_sim_count: row strides ldq = %d, ldb = %d must be >= D = %d", ldq, ldb, D);
        return TAG_EINVAL;
    }
    const Plan p = plan_of(M, N);
    const bool q_al = aligned16(q) && ldq % 4 == 0, b_al = aligned16(bank) && ldb % 4 == 0;
    const bool fast = q_al && b_al && M % T == 0 && N % T == 0 && D % KC == 0;
    hipStream_t st = as_stream(stream);
    long long* part = static_cast<long long*>(ws);
    if (fast) launch_main<true>(q, ldq, bank, ldb, weight, threshold, part, M, N, D, p, q_al, b_al, st);
    else launch_main<false>(q, ldq, bank, ldb, weight, threshold, part, M, N, D, p, q_al, b_al, st);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(phrase_sim_fold_kernel, dim3(cdiv(M, FOLD_ROWS)), dim3(256), 0, st, part, p.slices, M, out);
    TAG_LAUNCH_CHECK();
    return 0;
}
