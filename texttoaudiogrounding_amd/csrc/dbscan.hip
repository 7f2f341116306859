// Device DBSCAN for phrase clustering (python_scripts/clustering/dbscan_emb.py in the reference, which runs sklearn's
// DBSCAN(metric="precomputed") on the N x N float matrix (1 - cosine_similarity).clip(0); utils/phrase_cluster.py drives these
// entry points).  Everything lives on an N x W BIT matrix, W = 4 ceil(N / 128) 32-bit words per row (whole 128-column tiles,
// 16-byte aligned rows): N^2 / 8 bytes instead of 4 N^2.
//
// tag_dbscan_graph:  adj[i][j] = [x_i . x_j >= threshold] and degree[i] = popcount(adj[i]).  The products are phrase_sim.hip's
//   marching kernel with q = bank = x: a workgroup owns 128 rows and one SLICE of the 128-column tiles and marches over it on the
//   exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, operands not rounded, the same row-major LDS image, the K chunks of all tiles of a
//   slice one double-buffered sequence).  When a tile's K loop ends, register r of acc[i][j] holds row wm0 + 32 i + (r & 3) +
//   8 (r >> 2) + 4 (lane >> 5), column wn0 + 32 j + (lane & 31), so ONE 64-bit ballot of (acc[i][j][r] >= threshold) is two
//   finished adjacency words: the low half for that row of the lower 32 lanes, the high half for the row four further on.  The
//   ballot is ANDed with the ballot of (column < N) -- bits at columns >= N are 0, the degree and every later scan rely on it --
//   and its halves go into lane (row - wm0) of one of two registers with v_writelane_b32 (inline assembly: this compiler has no
//   builtin for it, and as a C++ select on the lane number each of the 64 ballots became an exec-masked branch); after the 64
//   ballots lane l holds the two words of row wm0 + l and stores them with one 8-byte vector store.  This replaces the int64
//   selects and adds of phrase_sim_kernel and its end-of-slice fold; no workspace exists.  A second launch takes the row
//   popcounts, one wave per row, lanes in word order and a butterfly: integers, the same bits on every run.
//
// tag_dbscan_core:   core_bits (W words) = the flags degree[i] >= min_samples, packed like a row of adj.
//
// tag_dbscan_hook:   one FastSV pass over the core-core graph on a parent array f (f = 0 .. N - 1 at the start).  With gf = f[f]
//   and m_i = min of gf[j] over the core neighbours j of core row i:  f'[f[i]] = min(f'[f[i]], m_i),  f'[i] = min(f'[i], m_i,
//   gf[i]).  f' (f_out) starts as a copy of f (f_in) and only f_in is read, so the number of passes is a function of the input
//   alone; the scatter-min is an integer atomicMin, whose result does not depend on the order of its operands.  One wave per core
//   row scans adj[i] & core_bits.  *changed = 1 when any entry of f_out ends below f_in (every writer stores the same value),
//   0 otherwise.  At the fixed point f[i] is the lowest index of i's component.  (Plain minimum-label propagation needs a
//   number of passes of the order of the graph's diameter; hooking needs about log2 N.)
//
// tag_dbscan_roots:  root[i] = f[i] for a core row; for any other row the smallest f[j] over its core neighbours j (sklearn grows
//   its clusters one at a time in the order of their lowest core index, so that cluster reaches a border row first), -1 for none.
#include "tag_common.h"
#include <limits.h>

namespace {

constexpr int T = 128;            // rows per workgroup, columns per tile
constexpr int KC = 32;            // K chunk per barrier
constexpr int LD = KC + 4;        // LDS row stride (144-byte rows: conflict-free b128 reads, as gemm.hip)
constexpr int SZ = T * LD;        // floats per stage buffer
constexpr int NL = T * KC / 1024; // float4 per thread, operand and chunk
constexpr int RQ = KC / 4;        // float4 per row of a chunk
constexpr size_t LDS_BYTES = (size_t)4 * SZ * sizeof(float);

// Column slices, as phrase_sim.hip's make_plan with M = N: the launch wants FILL_WGS workgroups, at least SLICES_MIN slices, and
// GROUP row blocks side by side over the same slice (they share the slice's operand tiles in one XCD's L2).  At most
// (2^24 + 8) * 8 workgroups for N <= 2^31 - 129: inside the grid limit.
constexpr int FILL_WGS = 512;
constexpr int SLICES_MIN = 8;
constexpr int GROUP = 8;
struct Plan { int tiles, group, slices, tiles_each; long blocks; };
Plan make_plan(int N) {
    Plan p;
    p.tiles = cdiv(N, T);
    p.group = p.tiles < GROUP ? p.tiles : GROUP;
    int want = cdiv(FILL_WGS, p.tiles);
    if (want < SLICES_MIN) want = SLICES_MIN;
    if (want > p.tiles) want = p.tiles;
    p.tiles_each = cdiv(p.tiles, want);
    p.slices = cdiv(p.tiles, p.tiles_each);
    p.blocks = (long)cdiv(p.tiles, p.group) * p.group * p.slices;
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
__global__ __launch_bounds__(256, 2) void dbscan_graph_kernel(const float* __restrict__ x, int ldx, float thr,
                                                              unsigned* __restrict__ adj, int N, int D, int W, int tiles, int group,
                                                              int slices, int tiles_each, bool al) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;             // [2][SZ]
    float* Bs = smem + 2 * SZ;    // [2][SZ]
    // logical order (row-block group, slice, row block of the group), an XCD taking a contiguous run of it
    const int L = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
    const int mt = (L / (group * slices)) * group + L % group;
    const int slice = (L / group) % slices;
    if (mt >= tiles) return;      // (the last group of row blocks may be short; the whole workgroup leaves)
    const int m0 = mt * T;
    const int t_lo = slice * tiles_each;
    const int t_hi = t_lo + tiles_each < tiles ? t_lo + tiles_each : tiles;
    const int kiters = (D + KC - 1) / KC;
    const int total = (t_hi - t_lo) * kiters;

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm0 = (wid >> 1) * 64, wn0 = (wid & 1) * 64;
    const int kl = lane >> 5, ml = lane & 31;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[i][0][r] = 0.0f;
            acc[i][1][r] = 0.0f;
        }

    f32x4 ra[NL], rb[NL];
    int ld_tile = t_lo, ld_k = 0;         // the chunk the next load requests
    auto load_next = [&]() {
        load_rows<FAST>(ra, x, ldx, m0, N, ld_k * KC, D, al);
        load_rows<FAST>(rb, x, ldx, ld_tile * T, N, ld_k * KC, D, al);
        if (++ld_k == kiters) { ld_k = 0; ++ld_tile; }
    };
    load_next();
    store_rows(As, ra);
    store_rows(Bs, rb);
    __syncthreads();

    const int row = m0 + wm0 + lane;      // the row whose two words this lane stores
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
            // the tile's scores are complete.  A column past N (its rows of x were zero-filled: score 0, which a threshold <= 0
            // would accept) is masked out of every ballot.
            int w[2] = {0, 0};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const unsigned long long real = __ballot(tile * T + wn0 + j * 32 + ml < N);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned long long hit = __ballot(acc[i][j][r] >= thr) & real;
                        const int rl = 32 * i + (r & 3) + 8 * (r >> 2);          // lane rl takes the low half, lane rl + 4 the high
                        asm("v_writelane_b32 %0, %1, %2" : "+v"(w[j]) : "s"((int)(unsigned)hit), "n"(rl));
                        asm("v_writelane_b32 %0, %1, %2" : "+v"(w[j]) : "s"((int)(unsigned)(hit >> 32)), "n"(rl + 4));
                        acc[i][j][r] = 0.0f;
                    }
            }
            if (row < N) {
                typedef int i32x2 __attribute__((ext_vector_type(2)));
                *reinterpret_cast<i32x2*>(adj + (size_t)row * W + tile * 4 + (wid & 1) * 2) = (i32x2){w[0], w[1]};
            }
            kc = 0;
            ++tile;
        }
        __syncthreads();
    }
}

constexpr int ROWS_PER_WG = 4;    // one wave per row
constexpr int NONE = INT_MAX;

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void dbscan_degree_kernel(const unsigned* __restrict__ adj, int* __restrict__ degree, int N, int W) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (i >= N) return;
    const unsigned* row = adj + (size_t)i * W;
    int n = 0;
    for (int w = lane; w < W; w += 64) n += __popc(row[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) degree[i] = n;
}

// thread t takes row blockIdx * 256 + t; a wave's ballot is the two words of its 64 rows
__global__ __launch_bounds__(256) void dbscan_core_kernel(const int* __restrict__ degree, int min_samples, unsigned* __restrict__ core,
                                                          int N, int W) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long b = __ballot(i < N && degree[i < N ? i : 0] >= min_samples);
    const int lane = threadIdx.x & 63;
    const long w = i >> 5;
    if ((lane & 31) == 0 && w < W) core[w] = lane ? (unsigned)(b >> 32) : (unsigned)b;
}

__device__ __forceinline__ bool core_bit(const unsigned* __restrict__ core, int i) { return (core[i >> 5] >> (i & 31)) & 1u; }

// min over the core neighbours j of row i of  GF ? f[f[j]] : f[j];  NONE without a core neighbour.  Every lane gets the result.
template <bool GF>
__device__ __forceinline__ int scan_row(const unsigned* __restrict__ adj, const unsigned* __restrict__ core, const int* __restrict__ f,
                                        int i, int W, int lane) {
    const unsigned* row = adj + (size_t)i * W;
    int m = NONE;
    for (int w = lane; w < W; w += 64) {
        unsigned bits = row[w] & core[w];
        while (bits) {
            const int j = 32 * w + __ffs(bits) - 1;         // (< N: bits at columns >= N are 0 in adj and in core)
            bits &= bits - 1;
            int v = f[j];
            if (GF) v = f[v];
            m = v < m ? v : m;
        }
    }
    return wave_min_i(m);
}

__global__ __launch_bounds__(256) void dbscan_hook_kernel(const unsigned* __restrict__ adj, const unsigned* __restrict__ core,
                                                          const int* __restrict__ f_in, int* __restrict__ f_out,
                                                          int* __restrict__ changed, int N, int W) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (i >= N || !core_bit(core, i)) return;
    const int m = scan_row<true>(adj, core, f_in, i, W, lane);
    if (lane != 0) return;
    const int fi = f_in[i], ffi = f_in[fi];                 // parent and grandparent (f[fi] <= fi <= i: both are rows)
    bool ch = false;
    if (m < ffi) {                                           // (otherwise f'[fi] <= f[fi] = ffi <= m already)
        atomicMin(f_out + fi, m);
        ch = true;
    }
    const int mi = m < ffi ? m : ffi;
    if (mi < fi) {
        atomicMin(f_out + i, mi);
        ch = true;
    }
    if (ch) *changed = 1;
}

__global__ __launch_bounds__(256) void dbscan_roots_kernel(const unsigned* __restrict__ adj, const unsigned* __restrict__ core,
                                                           const int* __restrict__ f, int* __restrict__ root, int N, int W) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (i >= N) return;
    if (core_bit(core, i)) {
        if (lane == 0) root[i] = f[i];
        return;
    }
    const int m = scan_row<false>(adj, core, f, i, W, lane);
    if (lane == 0) root[i] = m == NONE ? -1 : m;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// row and tile origins (N + 127) are ints; 32 W = 128 ceil(N / 128) <= 2^31 - 128
int check_rows(const char* fn, int N) {
    if (N < 1) {
        tag_set_error("%s: N must be >= 1 (got %d)", fn, N);
        return TAG_EINVAL;
    }
    if (N > INT_MAX - T) {
        tag_set_error("%s: N = %d exceeds %d (row index limit)", fn, N, INT_MAX - T);
        return TAG_EINVAL;
    }
    return 0;
}

template <bool FAST>
void launch_graph(const float* x, int ldx, float thr, unsigned* adj, int N, int D, int W, const Plan& p, bool al, hipStream_t st) {
    static bool attr_set = false;         // (once per process, as gemm.hip's launchers: the library drives one device per process)
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dbscan_graph_kernel<FAST>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)LDS_BYTES);
        attr_set = true;
    }
    hipLaunchKernelGGL(dbscan_graph_kernel<FAST>, dim3((unsigned)p.blocks), dim3(256), LDS_BYTES, st, x, ldx, thr, adj, N, D, W,
                       p.tiles, p.group, p.slices, p.tiles_each, al);
}

}  // namespace

extern "C" int tag_dbscan_words(int N) {
    if (N < 1 || N > INT_MAX - T) return 0;
    return 4 * cdiv(N, T);
}

extern "C" int tag_dbscan_graph(const float* x, int ldx, float threshold, int* adj, int* degree, int N, int D, void* stream) {
    TAG_CHECK_ARG(x && adj && degree);
    if (N < 1 || D < 1) {
        tag_set_error("tag_dbscan_graph: N, D must be >= 1 (got %d, %d)", N, D);
        return TAG_EINVAL;
    }
    if (int rc = check_rows("tag_dbscan_graph", N)) return rc;
    if (D > INT_MAX - KC) {
        tag_set_error("tag_dbscan_graph: D = %d exceeds %d (chunk index limit)", D, INT_MAX - KC);
        return TAG_EINVAL;
    }
    if (ldx < D) {
        tag_set_error("tag_dbscan_graph: row stride ldx = %d must be >= D = %d", ldx, D);
        return TAG_EINVAL;
    }
    const Plan p = make_plan(N);
    const int W = tag_dbscan_words(N);
    const bool al = aligned16(x) && ldx % 4 == 0;
    const bool fast = al && N % T == 0 && D % KC == 0;
    hipStream_t st = as_stream(stream);
    unsigned* bits = reinterpret_cast<unsigned*>(adj);
    if (fast) launch_graph<true>(x, ldx, threshold, bits, N, D, W, p, al, st);
    else launch_graph<false>(x, ldx, threshold, bits, N, D, W, p, al, st);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(dbscan_degree_kernel, dim3(cdiv(N, ROWS_PER_WG)), dim3(256), 0, st, bits, degree, N, W);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_dbscan_core(const int* degree, int min_samples, int* core_bits, int N, void* stream) {
    TAG_CHECK_ARG(degree && core_bits);
    if (int rc = check_rows("tag_dbscan_core", N)) return rc;
    const int W = tag_dbscan_words(N);
    hipLaunchKernelGGL(dbscan_core_kernel, dim3(cdiv((long)W * 32, 256)), dim3(256), 0, as_stream(stream), degree, min_samples,
                       reinterpret_cast<unsigned*>(core_bits), N, W);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_dbscan_hook(const int* adj, const int* core_bits, const int* f_in, int* f_out, int* changed, int N, void* stream) {
    TAG_CHECK_ARG(adj && core_bits && f_in && f_out && changed && f_in != f_out);
    if (int rc = check_rows("tag_dbscan_hook", N)) return rc;
    const int W = tag_dbscan_words(N);
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemcpyAsync(f_out, f_in, (size_t)N * sizeof(int), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(changed, 0, sizeof(int), st);
    if (e != hipSuccess) {
        tag_set_error("tag_dbscan_hook: preparing f_out and changed failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    hipLaunchKernelGGL(dbscan_hook_kernel, dim3(cdiv(N, ROWS_PER_WG)), dim3(256), 0, st, reinterpret_cast<const unsigned*>(adj),
                       reinterpret_cast<const unsigned*>(core_bits), f_in, f_out, changed, N, W);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_dbscan_roots(const int* adj, const int* core_bits, const int* f, int* root, int N, void* stream) {
    TAG_CHECK_ARG(adj && core_bits && f && root);
    if (int rc = check_rows("tag_dbscan_roots", N)) return rc;
    const int W = tag_dbscan_words(N);
    hipLaunchKernelGGL(dbscan_roots_kernel, dim3(cdiv(N, ROWS_PER_WG)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const unsigned*>(adj), reinterpret_cast<const unsigned*>(core_bits), f, root, N, W);
    TAG_LAUNCH_CHECK();
    return 0;
}
