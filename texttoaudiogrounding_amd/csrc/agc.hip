// Device average-linkage clustering over the cosine distance (python_scripts/clustering/agc_emb.py in the reference, which runs
// sklearn's AgglomerativeClustering(linkage="average") on the N x N matrix 1 - cosine_similarity on the host;
// utils/phrase_cluster.py drives these two entry points).
//
// For unit rows u the average of 1 - u_i . u_j over i in A, j in B is 1 - m_A . m_B with m_A = (sum_{i in A} u_i) / |A|: a cluster
// is its sum vector, a merge adds two sums, and "nearest cluster" is a row argmax of m m^T.  Average linkage is reducible, so all
// reciprocal-nearest-neighbour pairs of a round merge at once and the dendrogram is the one the serial algorithm builds: a fit is
// rounds of tag_agc_nearest + tag_agc_merge with one host read each (12 rounds on 40 x 8 rows, 526 at 32768 x 512: the count
// depends on the data, at most N - 1).  Device memory of a fit at (N, D): two (N, D) fp64
// sum buffers, one (N, D) fp32 mean buffer, O(N) vectors and the workspace below, about 20 N D + 64 N bytes; no (N, N) array.
//
// tag_agc_nearest:  nn[i] = the j != i with the largest m_i . m_j, ties to the lowest j, dist[i] = 1 - m_i . m_nn[i].  The products
//   are the marching kernel of march_f32.h with A = B = m: a workgroup owns 128 rows and one SLICE of the 128-column tiles of the
//   same matrix and walks the slice on the exact-fp32 MFMA (operands not rounded, the D tail zero-filled).  When a tile's K loop
//   ends each lane keeps a running (score, index) pair per row it holds; the diagonal and the columns >= M score -inf.  A lane
//   meets its columns in ascending order and replaces on > only; at the end of the slice the 64 lanes that share a row fold
//   through LDS on (score, index) and the row's pair goes to ws[slice][row]; a second launch folds the slices in slice order on
//   (score, index) and writes nn and dist.  M shrinks from N towards 1 during a fit, so the slice count comes from M alone
//   (the plan with the columns = the rows): few row blocks are cut into many slices and still fill the device.
//   The scores are BIT-SYMMETRIC, score(i, j) == score(j, i): both are the same chain of k-steps in the same order (k-step e of
//   a group multiplies the same k in both operands, a product a * b is commutative, and nothing else scales a score).  The fit
//   loop's progress argument needs it: the lowest row that attains the round's largest score and its nn name each other.
//
// tag_agc_merge:  one round's bookkeeping in two launches.  Row a is the LEFT half of a pair when nn[nn[a]] == a and a < nn[a]
//   (an nn outside [0, M) pairs with nothing).  agc_plan_kernel (one workgroup) scans the flags in row order: the survivors keep
//   their relative order at the front of the output, the merged clusters follow in ascending a; it writes each output row's two
//   source rows into ws and {pairs, new M} into counts.  agc_gather_kernel (one wave per output row, launched for M rows, rows
//   >= new M leave at once) adds the fp64 sums, writes sizes, node ids (next_id + rank for a merged row), the new means
//   (float)(sum / size) for EVERY output row, and the merge log row (dist[a], id_a, id_b, new id) at log_off + rank.
//
// No atomics, no cooperative launch, no device-side waiting; ws is never zeroed; the same bits on every run.
#include "march_f32.h"
#include <math.h>

namespace {

using namespace march;

// ------------------------------------------------------------------------------------------------------------------------
// nearest
// ------------------------------------------------------------------------------------------------------------------------
constexpr size_t LDS_BYTES = STAGE_BYTES;
static_assert((size_t)2 * T * RED_LD * sizeof(float) <= LDS_BYTES, "the fold reuses the stage buffers");
constexpr int NONE = INT_MAX;     // index of "no candidate yet": loses every tie

// Column slices: the plan of march_f32.h with the columns = the rows themselves.  ws = slices x M x (float + int).
Plan plan_of(int M) { return make_plan(cdiv(M, T), cdiv(M, T)); }

template <bool FAST>
__global__ __launch_bounds__(256, 2) void agc_nearest_kernel(const float* __restrict__ m, int ldm, float* __restrict__ ws_score,
                                                             int* __restrict__ ws_idx, int M, int D, int tiles, int group,
                                                             int slices, int tiles_each, bool al) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Share sh = plan_share(tiles, group, slices, tiles_each);
    if (sh.mt >= tiles) return;
    const int m0 = sh.mt * T, slice = sh.slice;
    const Lanes l = lanes();
    const int row0 = m0 + l.wm0 + 4 * l.kl;       // register r of acc[i][.] is row row0 + acc_row(i, r)

    float best[2][16];
    int bidx[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            best[i][r] = -INFINITY;
            bidx[i][r] = NONE;
        }

    // This lane meets its columns in ascending order (tile, then j) and replaces on > only; a column past M (zero-filled: score 0,
    // above every negative real score) and the diagonal never win.
    march_tiles<FAST, FAST>(smem, Rows{m, ldm, M, al}, Rows{m, ldm, M, al}, m0, sh.t_lo, sh.t_hi, D,
                            [&](int tile, const f32x16 (&acc)[2][2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = tile * T + l.wn0 + j * 32 + l.ml;
            const bool real = n < M;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row0 + acc_row(i, r);
                    const float s = acc[i][j][r];
                    const bool take = real && n != row && s > best[i][r];
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
    if (threadIdx.x < T && m0 + (int)threadIdx.x < M) {
        float bs = rs[threadIdx.x * RED_LD];
        int bn = ri[threadIdx.x * RED_LD];
        for (int e = 1; e < 64; ++e) {
            const float s = rs[threadIdx.x * RED_LD + e];
            const int n = ri[threadIdx.x * RED_LD + e];
            if (s > bs || (s == bs && n < bn)) {
                bs = s;
                bn = n;
            }
        }
        ws_score[(size_t)slice * M + m0 + threadIdx.x] = bs;
        ws_idx[(size_t)slice * M + m0 + threadIdx.x] = bn;
    }
}

// nn[i], dist[i] from the slices' pairs, in slice order on (score, index): one thread per row (the plan gives at most 23 slices).  A row without any candidate (M == 1, or scores that are all NaN) gets nn = -1, dist = +inf.
__global__ __launch_bounds__(256) void agc_nearest_fold_kernel(const float* __restrict__ ws_score, const int* __restrict__ ws_idx,
                                                               int slices, int M, int* __restrict__ nn, float* __restrict__ dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    float bs = -INFINITY;
    int bn = NONE;
    for (int z = 0; z < slices; ++z) {
        const float s = ws_score[(size_t)z * M + i];
        const int n = ws_idx[(size_t)z * M + i];
        if (s > bs || (s == bs && n < bn)) {
            bs = s;
            bn = n;
        }
    }
    nn[i] = bn == NONE ? -1 : bn;
    dist[i] = bn == NONE ? INFINITY : 1.0f - bs;
}

__global__ void agc_single_kernel(int* __restrict__ nn, float* __restrict__ dist) {
    nn[0] = -1;
    dist[0] = INFINITY;
}

bool shape_ok(int M, int D) { return M >= 1 && D >= 1 && M <= INT_MAX - T && D <= INT_MAX - KC && plan_of(M).blocks <= INT_MAX; }

// tile origins (M + 127) and the chunk origin (D + 31) are ints; the grid is one-dimensional
int check_shape(const char* fn, int M, int D) {
    if (M < 1 || D < 1) {
        tag_set_error("%s: M, D must be >= 1 (got %d, %d)", fn, M, D);
        return TAG_EINVAL;
    }
    if (int rc = check_index_limit(fn, "M", M, T, "row")) return rc;
    if (int rc = check_index_limit(fn, "D", D, KC, "chunk")) return rc;
    const Plan p = plan_of(M);
    if (p.blocks > INT_MAX) {
        tag_set_error("%s: M = %d needs %ld workgroups (%d row blocks x %d slices), more than the grid limit %d", fn, M, p.blocks,
                      p.m_tiles, p.slices, INT_MAX);
        return TAG_EINVAL;
    }
    return 0;
}

template <bool FAST>
void launch_nearest(const float* m, int ldm, float* ws_score, int* ws_idx, int M, int D, const Plan& p, bool al, hipStream_t st) {
    static bool attr_set = false;         // (once per process, as gemm.hip's launchers: the library drives one device per process)
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&agc_nearest_kernel<FAST>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)LDS_BYTES);
        attr_set = true;
    }
    hipLaunchKernelGGL(agc_nearest_kernel<FAST>, dim3((unsigned)p.blocks), dim3(256), LDS_BYTES, st, m, ldm, ws_score, ws_idx, M, D,
                       p.m_tiles, p.group, p.slices, p.tiles_each, al);
}

// ------------------------------------------------------------------------------------------------------------------------
// merge
// ------------------------------------------------------------------------------------------------------------------------
constexpr int PLAN_THREADS = 1024;

// role of row a: 1 = the left half of a pair, 2 = the right half, 0 = a survivor.  Every index is checked before it is used.
__device__ __forceinline__ int agc_role(const int* __restrict__ nn, int a, int M) {
    const int b = nn[a];
    if (b < 0 || b >= M || b == a) return 0;
    if (nn[b] != a) return 0;
    return a < b ? 1 : 2;
}

// exclusive scan over the workgroup of one (x, y) pair per thread -> the thread's offsets (ox, oy) and the totals (tx, ty)
__device__ __forceinline__ void block_scan2(int x, int y, int& ox, int& oy, int& tx, int& ty, int (*sh)[2]) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int ix = x, iy = y;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int px = __shfl_up(ix, o, 64), py = __shfl_up(iy, o, 64);
        if (lane >= o) { ix += px; iy += py; }
    }
    if (lane == 63) { sh[wid][0] = ix; sh[wid][1] = iy; }
    __syncthreads();
    int bx = 0, by = 0;
    tx = 0;
    ty = 0;
    for (int w = 0; w < PLAN_THREADS / 64; ++w) {
        if (w < wid) { bx += sh[w][0]; by += sh[w][1]; }
        tx += sh[w][0];
        ty += sh[w][1];
    }
    ox = bx + ix - x;
    oy = by + iy - y;
    __syncthreads();              // sh is reused by the next call
}

// One workgroup.  Every thread takes a contiguous run of rows (so that ranks follow the row order), counts its survivors and left
// halves, the workgroup scans the counts, and the thread writes the source rows of its output rows: src[o] = (a, -1) for the
// survivor of rank o, src[S + p] = (a, nn[a]) for the left half of rank p, S = M - 2 P survivors.  counts = {P, M - P}.
__global__ __launch_bounds__(PLAN_THREADS) void agc_plan_kernel(const int* __restrict__ nn, int M, int* __restrict__ src,
                                                                int* __restrict__ counts) {
    __shared__ int sh[PLAN_THREADS / 64][2];
    const int each = (M + PLAN_THREADS - 1) / PLAN_THREADS;
    const long lo_l = (long)threadIdx.x * each;
    const int lo = lo_l < M ? (int)lo_l : M;
    const int hi = lo_l + each < M ? (int)(lo_l + each) : M;
    int ns = 0, np = 0;
    for (int a = lo; a < hi; ++a) {
        const int r = agc_role(nn, a, M);
        ns += r == 0;
        np += r == 1;
    }
    int os, op, S, P;
    block_scan2(ns, np, os, op, S, P, sh);
    for (int a = lo; a < hi; ++a) {
        const int r = agc_role(nn, a, M);
        if (r == 0) {
            src[2 * (size_t)os] = a;
            src[2 * (size_t)os + 1] = -1;
            ++os;
        } else if (r == 1) {
            src[2 * ((size_t)S + op)] = a;
            src[2 * ((size_t)S + op) + 1] = nn[a];
            ++op;
        }
    }
    if (threadIdx.x == 0) {
        counts[0] = P;
        counts[1] = M - P;
    }
}

constexpr int ROWS_PER_WG = 4;    // one wave per output row

__global__ __launch_bounds__(256) void agc_gather_kernel(const int* __restrict__ src, const int* __restrict__ counts,
                                                         const float* __restrict__ dist, const double* __restrict__ sums_in,
                                                         const long long* __restrict__ sizes_in, const int* __restrict__ ids_in,
                                                         double* __restrict__ sums_out, long long* __restrict__ sizes_out,
                                                         int* __restrict__ ids_out, float* __restrict__ means_out, int ldm,
                                                         float* __restrict__ log_dist, int* __restrict__ log_ids, int log_off,
                                                         int next_id, int M, int D) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    const int P = counts[0], M2 = counts[1];
    if (o >= M2 || o >= M) return;
    const int a = src[2 * (size_t)o], b = src[2 * (size_t)o + 1];
    const bool pair = b >= 0;
    const long long size = sizes_in[a] + (pair ? sizes_in[b] : 0LL);
    const double dsize = (double)size;
    const double* sa = sums_in + (size_t)a * D;
    const double* sb = sums_in + (size_t)(pair ? b : a) * D;
    double* so = sums_out + (size_t)o * D;
    float* mo = means_out + (size_t)o * ldm;
    for (int d = lane; d < D; d += 64) {
        const double s = pair ? sa[d] + sb[d] : sa[d];
        so[d] = s;
        mo[d] = (float)(s / dsize);
    }
    if (lane == 0) {
        sizes_out[o] = size;
        if (pair) {
            const int rank = o - (M2 - P);
            const int id = next_id + rank;
            ids_out[o] = id;
            log_dist[(size_t)log_off + rank] = dist[a];
            int* row = log_ids + 3 * ((size_t)log_off + rank);
            row[0] = ids_in[a];
            row[1] = ids_in[b];
            row[2] = id;
        } else {
            ids_out[o] = ids_in[a];
        }
    }
}

}  // namespace

extern "C" size_t tag_agc_nearest_ws_bytes(int M, int D) {
    if (!shape_ok(M, D)) return 0;
    return (size_t)plan_of(M).slices * M * (sizeof(float) + sizeof(int));
}

extern "C" int tag_agc_nearest(const float* m, int ldm, int* nn, float* dist, int M, int D, void* ws, void* stream) {
    TAG_CHECK_ARG(m && nn && dist && ws);
    if (int rc = check_shape("tag_agc_nearest", M, D)) return rc;
    if (ldm < D) {
        tag_set_error("tag_agc_nearest: row stride ldm = %d must be >= D = %d", ldm, D);
        return TAG_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    if (M == 1) {
        hipLaunchKernelGGL(agc_single_kernel, dim3(1), dim3(1), 0, st, nn, dist);
        TAG_LAUNCH_CHECK();
        return 0;
    }
    const Plan p = plan_of(M);
    float* ws_score = static_cast<float*>(ws);
    int* ws_idx = reinterpret_cast<int*>(ws_score + (size_t)p.slices * M);
    const bool al = aligned16(m) && ldm % 4 == 0;
    const bool fast = al && M % T == 0 && D % KC == 0;
    if (fast) launch_nearest<true>(m, ldm, ws_score, ws_idx, M, D, p, al, st);
    else launch_nearest<false>(m, ldm, ws_score, ws_idx, M, D, p, al, st);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(agc_nearest_fold_kernel, dim3(cdiv(M, 256)), dim3(256), 0, st, ws_score, ws_idx, p.slices, M, nn, dist);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t tag_agc_merge_ws_bytes(int M, int D) {
    if (!shape_ok(M, D)) return 0;
    return (size_t)2 * M * sizeof(int);
}

extern "C" int tag_agc_merge(const int* nn, const float* dist, const double* sums_in, const long long* sizes_in, const int* ids_in,
                             double* sums_out, long long* sizes_out, int* ids_out, float* means_out, int ldm, float* log_dist,
                             int* log_ids, int log_rows, int log_off, int next_id, int* counts, int M, int D, void* ws,
                             void* stream) {
    TAG_CHECK_ARG(nn && dist && sums_in && sizes_in && ids_in && sums_out && sizes_out && ids_out && means_out && log_dist && log_ids &&
                  counts && ws);
    if (int rc = check_shape("tag_agc_merge", M, D)) return rc;
    if (ldm < D) {
        tag_set_error("tag_agc_merge: row stride ldm = %d must be >= D = %d", ldm, D);
        return TAG_EINVAL;
    }
    if (sums_in == sums_out || sizes_in == sizes_out || ids_in == ids_out) {
        tag_set_error("tag_agc_merge: sums_out, sizes_out and ids_out must be buffers other than the inputs (rows move)");
        return TAG_EINVAL;
    }
    if (log_off < 0 || next_id < 0 || log_off > INT_MAX - M || next_id > INT_MAX - M) {
        tag_set_error("tag_agc_merge: log_off = %d and next_id = %d must be >= 0 and at most %d (M = %d more fit an int)", log_off,
                      next_id, INT_MAX - M, M);
        return TAG_EINVAL;
    }
    if (log_off + M / 2 > log_rows) {
        tag_set_error("tag_agc_merge: a log of %d rows cannot take the up to %d pairs of M = %d rows at log_off = %d", log_rows, M / 2,
                      M, log_off);
        return TAG_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    int* src = static_cast<int*>(ws);
    hipLaunchKernelGGL(agc_plan_kernel, dim3(1), dim3(PLAN_THREADS), 0, st, nn, M, src, counts);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(agc_gather_kernel, dim3(cdiv(M, ROWS_PER_WG)), dim3(256), 0, st, src, counts, dist, sums_in, sizes_in, ids_in,
                       sums_out, sizes_out, ids_out, means_out, ldm, log_dist, log_ids, log_off, next_id, M, D);
    TAG_LAUNCH_CHECK();
    return 0;
}
