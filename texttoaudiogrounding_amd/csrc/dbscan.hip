// Device DBSCAN for phrase clustering (python_scripts/clustering/dbscan_emb.py in the reference, which runs sklearn's
// DBSCAN(metric="precomputed") on the N x N float matrix (1 - cosine_similarity).clip(0); utils/phrase_cluster.py drives these
// entry points).  Everything lives on an N x W BIT matrix, W = 4 ceil(N / 128) 32-bit words per row (whole 128-column tiles,
// 16-byte aligned rows): N^2 / 8 bytes instead of 4 N^2.
//
// tag_dbscan_graph:  adj[i][j] = [x_i . x_j >= threshold] and degree[i] = popcount(adj[i]).  The products are the marching kernel
//   of march_f32.h with A = B = x: a workgroup owns 128 rows and one SLICE of the 128-column tiles and marches over it on the
//   exact-fp32 MFMA.  When a tile's K loop ends, ONE 64-bit ballot of (acc[i][j][r] >= threshold) is two finished adjacency words
//   (ballot_to_words).  The ballot is ANDed with the ballot of (column < N) -- bits at columns >= N are 0, the degree and every
//   later scan rely on it; after the 64 ballots lane l holds the two words of row wm0 + l and stores them with one 8-byte vector
//   store.  This replaces the int64 selects and adds of phrase_sim_kernel and its end-of-slice fold; no workspace exists.  A
//   second launch takes the row popcounts, one wave per row, lanes in word order and a butterfly: integers, the same bits on
//   every run.
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
#include "march_f32.h"

namespace {

using namespace march;
constexpr size_t LDS_BYTES = STAGE_BYTES;

// Column slices: the plan of march_f32.h with the columns = the rows themselves.  At most (2^24 + 8) * 8 workgroups for
// N <= 2^31 - 129: inside the grid limit.
Plan plan_of(int N) { return make_plan(cdiv(N, T), cdiv(N, T)); }

template <bool FAST>
__global__ __launch_bounds__(256, 2) void dbscan_graph_kernel(const float* __restrict__ x, int ldx, float thr,
                                                              unsigned* __restrict__ adj, int N, int D, int W, int tiles, int group,
                                                              int slices, int tiles_each, bool al) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Share sh = plan_share(tiles, group, slices, tiles_each);
    if (sh.mt >= tiles) return;
    const int m0 = sh.mt * T;
    const Lanes l = lanes();
    const int row = m0 + l.wm0 + l.lane;  // the row whose two words this lane stores

    // A column past N (its rows of x were zero-filled: score 0, which a threshold <= 0 would accept) is masked out of every ballot.
    march_tiles<FAST, FAST>(smem, Rows{x, ldx, N, al}, Rows{x, ldx, N, al}, m0, sh.t_lo, sh.t_hi, D,
                            [&](int tile, const f32x16 (&acc)[2][2]) {
        int w[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned long long real = __ballot(tile * T + l.wn0 + j * 32 + l.ml < N);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) ballot_to_words(w[j], __ballot(acc[i][j][r] >= thr) & real, acc_row(i, r));
        }
        if (row < N) {
            typedef int i32x2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<i32x2*>(adj + (size_t)row * W + tile * 4 + (l.wid & 1) * 2) = (i32x2){w[0], w[1]};
        }
    });
}

constexpr int ROWS_PER_WG = 4;    // one wave per row
constexpr int NONE = INT_MAX;

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

// row and tile origins (N + 127) are ints; 32 W = 128 ceil(N / 128) <= 2^31 - 128
int check_rows(const char* fn, int N) {
    if (N < 1) {
        tag_set_error("%s: N must be >= 1 (got %d)", fn, N);
        return TAG_EINVAL;
    }
    return check_index_limit(fn, "N", N, T, "row");
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
                       p.m_tiles, p.group, p.slices, p.tiles_each, al);
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
    if (int rc = check_index_limit("tag_dbscan_graph", "D", D, KC, "chunk")) return rc;
    if (ldx < D) {
        tag_set_error("tag_dbscan_graph: row stride ldx = %d must be >= D = %d", ldx, D);
        return TAG_EINVAL;
    }
    const Plan p = plan_of(N);
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
