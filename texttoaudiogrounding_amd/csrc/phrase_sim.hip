// Thresholded similarity count (utils/data/calc_phrase_sim_count.py in the reference, which calls cosine_similarity once per
// phrase and keeps the phrases at or above a threshold):
//   out[i] = sum_j weight[j] * [ sum_d q[i,d] * bank[j,d] >= threshold ]
// The N x N score matrix never exists: a workgroup owns 128 query rows and one SLICE of the bank's 128-column tiles and marches
// over the slice tile by tile on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, operands not rounded: a cosine lands on the
// side of the threshold where fp32 numpy puts it).  Both operands are k-contiguous and use gemm.hip's row-major LDS image
// (S[r][32 k + 4 pad], 16-byte LDS writes, a fragment = one ds_read_b128 = the lane's operands of four k-steps; k-step j of an
// 8-k group multiplies k = 8 g + 4 kl + j in BOTH operands, so the permutation cancels in the sum).  The K chunks of all tiles
// of a slice form ONE double-buffered sequence: the loads of the next tile's first chunk are in flight while the last chunk of
// this one multiplies.  When a tile's K loop ends each lane compares its 64 accumulator values with the threshold, adds the
// column's weight into one int64 register per row it holds (32 rows), and clears the accumulators.  At the end of the slice the
// 64 lanes that share a row fold their sums through LDS in lane order and the row's partial goes to ws[slice][row]; a second
// launch adds the slices in a fixed order.  Integer sums do not depend on the order, but the two-launch form keeps the library
// free of atomics and ws free of any zeroing.
#include "tag_common.h"
#include <limits.h>

namespace {

constexpr int T = 128;            // query rows per workgroup, bank rows per tile
constexpr int KC = 32;            // K chunk per barrier
constexpr int LD = KC + 4;        // LDS row stride (144-byte rows: conflict-free b128 reads, as gemm.hip)
constexpr int SZ = T * LD;        // floats per stage buffer
constexpr int NL = T * KC / 1024; // float4 per thread, operand and chunk
constexpr int RQ = KC / 4;        // float4 per row of a chunk
constexpr int RED_LD = 65;        // int64 row stride of the end-of-slice fold (64 partials per row + 1 pad)
constexpr size_t LDS_BYTES = (size_t)4 * SZ * sizeof(float);
static_assert((size_t)T * RED_LD * sizeof(long long) <= LDS_BYTES, "the fold reuses the stage buffers");

// Column slices.  The launch wants FILL_WGS workgroups (two per CU of 256 by LDS), so few query blocks against a large bank
// are cut into many slices; with many query blocks SLICES_MIN slices remain, because the workgroups resident on one XCD
// then are G query blocks x several slices -- G + 8 operand tiles of 128 x D floats in flight per XCD instead of 64 + 1, which is
// what its 4 MB L2 can hold at D = 512.  ws = slices x M int64: 2 MB at M = N = 32768.  A function of the shape alone.
constexpr int FILL_WGS = 512;
constexpr int SLICES_MIN = 8;
constexpr int GROUP = 8;          // query blocks that run side by side over the same slices
struct Plan { int m_tiles, n_tiles, group, slices, tiles_each; long blocks; };
Plan make_plan(int M, int N) {
    Plan p;
    p.m_tiles = cdiv(M, T);
    p.n_tiles = cdiv(N, T);
    p.group = p.m_tiles < GROUP ? p.m_tiles : GROUP;
    int want = cdiv(FILL_WGS, p.m_tiles);
    if (want < SLICES_MIN) want = SLICES_MIN;
    if (want > p.n_tiles) want = p.n_tiles;
    p.tiles_each = cdiv(p.n_tiles, want);
    p.slices = cdiv(p.n_tiles, p.tiles_each);
    p.blocks = (long)cdiv(p.m_tiles, p.group) * p.group * p.slices;
    return p;
}

// FAST: whole tiles, whole K chunks and 16-byte aligned rows (checked by the launcher): plain float4 loads, no tail tests
template <bool FAST>
__device__ __forceinline__ void load_rows(f32x4 (&reg)[NL], const float* __restrict__ base, int ld, int r0, int rmax, int k0, int D,
                                          bool al) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int idx = threadIdx.x + 256 * i;
        const int r = r0 + idx / RQ, k = k0 + (idx % RQ) * 4;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (FAST) {
            v = *reinterpret_cast<const f32x4*>(base + (size_t)r * ld + k);
        } else if (r < rmax) {
            const float* p = base + (size_t)r * ld + k;
            const int n = D - k;
            if (n >= 4 && al) {
                v = *reinterpret_cast<const f32x4*>(p);
            } else {
                if (n > 0) v.x = p[0];
                if (n > 1) v.y = p[1];
                if (n > 2) v.z = p[2];
                if (n > 3) v.w = p[3];
            }
        }
        reg[i] = v;
    }
}

__device__ __forceinline__ void store_rows(float* s, const f32x4 (&reg)[NL]) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int idx = threadIdx.x + 256 * i;
        *reinterpret_cast<f32x4*>(s + (idx / RQ) * LD + (idx % RQ) * 4) = reg[i];
    }
}

template <bool FAST>
__global__ __launch_bounds__(256, 2) void phrase_sim_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ bank,
                                                            int ldb, const long long* __restrict__ weight, float thr,
                                                            long long* __restrict__ ws, int M, int N, int D, int m_tiles,
                                                            int n_tiles, int group, int slices, int tiles_each, bool q_al,
                                                            bool b_al) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;             // [2][SZ]
    float* Bs = smem + 2 * SZ;    // [2][SZ]
    // logical order (query group, slice, query block of the group), an XCD taking a contiguous run of it
    const int L = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
    const int mt = (L / (group * slices)) * group + L % group;
    const int slice = (L / group) % slices;
    if (mt >= m_tiles) return;    // (the last group of query blocks may be short; the whole workgroup leaves)
    const int m0 = mt * T;
    const int t_lo = slice * tiles_each;
    const int t_hi = t_lo + tiles_each < n_tiles ? t_lo + tiles_each : n_tiles;
    const int kiters = (D + KC - 1) / KC;
    const int total = (t_hi - t_lo) * kiters;

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm0 = (wid >> 1) * 64, wn0 = (wid & 1) * 64;
    const int kl = lane >> 5, ml = lane & 31;

    f32x16 acc[2][2];
    long long cnt[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            cnt[i][r] = 0;
            acc[i][0][r] = 0.0f;
            acc[i][1][r] = 0.0f;
        }

    f32x4 ra[NL], rb[NL];
    int ld_tile = t_lo, ld_k = 0;         // the chunk the next load requests
    auto load_next = [&]() {
        load_rows<FAST>(ra, q, ldq, m0, M, ld_k * KC, D, q_al);
        load_rows<FAST>(rb, bank, ldb, ld_tile * T, N, ld_k * KC, D, b_al);
        if (++ld_k == kiters) { ld_k = 0; ++ld_tile; }
    };
    load_next();
    store_rows(As, ra);
    store_rows(Bs, rb);
    __syncthreads();

    int tile = t_lo, kc = 0;
    for (int it = 0; it < total; ++it) {
        const int buf = it & 1;
        if (it + 1 < total) load_next();
        __builtin_amdgcn_sched_barrier(0);
        const float* a = As + buf * SZ + (wm0 + ml) * LD + kl * 4;
        const float* b = Bs + buf * SZ + (wn0 + ml) * LD + kl * 4;
        f32x4 af[2][2], bf[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            af[0][i] = *reinterpret_cast<const f32x4*>(a + i * 32 * LD);
            bf[0][i] = *reinterpret_cast<const f32x4*>(b + i * 32 * LD);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < KC / 8; ++g) {
            if (g + 1 < KC / 8) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    af[(g + 1) & 1][i] = *reinterpret_cast<const f32x4*>(a + i * 32 * LD + 8 * (g + 1));
                    bf[(g + 1) & 1][i] = *reinterpret_cast<const f32x4*>(b + i * 32 * LD + 8 * (g + 1));
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g & 1][i][e], bf[g & 1][j][e], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (it + 1 < total) {
            store_rows(As + (buf ^ 1) * SZ, ra);
            store_rows(Bs + (buf ^ 1) * SZ, rb);
        }
        if (++kc == kiters) {
            // the tile's scores are complete: register r of acc[i][j] is row wm0 + 32 i + (r & 3) + 8 (r >> 2) + 4 kl, column
            // wn0 + 32 j + ml.  A column past N (its bank rows were zero-filled: score 0) weighs nothing.
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = tile * T + wn0 + j * 32 + ml;
                const long long w = n < N ? (weight ? weight[n] : 1LL) : 0LL;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        cnt[i][r] += acc[i][j][r] >= thr ? w : 0LL;
                        acc[i][j][r] = 0.0f;
                    }
            }
            kc = 0;
            ++tile;
        }
        __syncthreads();
    }

    // fold the 64 lanes (2 waves x 32 columns) that share a row, in lane order; the stage buffers are free after the last barrier
    long long* red = reinterpret_cast<long long*>(smem);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl) * RED_LD + (wid & 1) * 32 + ml] = cnt[i][r];
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

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int check_shape(int M, int N, int D) {
    if (M < 1 || N < 1 || D < 1) {
        tag_set_error("tag_phrase_sim_count: M, N, D must be >= 1 (got %d, %d, %d)", M, N, D);
        return TAG_EINVAL;
    }
    // tile origins (tile * 128 <= N + 127, m0 + 127) and the chunk origin (D + 31) are ints; the grid is one-dimensional
    if (M > INT_MAX - T) {
        tag_set_error("tag_phrase_sim_count: M = %d exceeds %d (row index limit)", M, INT_MAX - T);
        return TAG_EINVAL;
    }
    if (N > INT_MAX - T) {
        tag_set_error("tag_phrase_sim_count: N = %d exceeds %d (row index limit)", N, INT_MAX - T);
        return TAG_EINVAL;
    }
    if (D > INT_MAX - KC) {
        tag_set_error("tag_phrase_sim_count: D = %d exceeds %d (chunk index limit)", D, INT_MAX - KC);
        return TAG_EINVAL;
    }
    const Plan p = make_plan(M, N);
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
    return (size_t)make_plan(M, N).slices * M * sizeof(long long);
}

extern "C" int tag_phrase_sim_count(const float* q, int ldq, const float* bank, int ldb, const long long* weight, float threshold,
                                    long long* out, int M, int N, int D, void* ws, void* stream) {
    TAG_CHECK_ARG(q && bank && out && ws);
    if (int rc = check_shape(M, N, D)) return rc;
    if (ldq < D || ldb < D) {
        tag_set_error("tag_phrase_sim_count: row strides ldq = %d, ldb = %d must be >= D = %d", ldq, ldb, D);
        return TAG_EINVAL;
    }
    const Plan p = make_plan(M, N);
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
