// The marching exact-fp32 MFMA tile loop shared by phrase_sim.hip, dbscan.hip, agc.hip, kmeans.hip and label_map.hip: all-pairs dot
// products of fp32 rows, A (rows x D) against B (rows x D), without the score matrix ever existing.
//
// A workgroup (256 threads, four waves as 2 x 2 quadrants of 64 x 64) owns T = 128 rows of A and a range [t_lo, t_hi) of B's
// 128-row tiles -- the columns of the score matrix -- and marches over the range tile by tile on v_mfma_f32_32x32x2_f32 (operands
// not rounded: a score lands on the side of a threshold where fp32 numpy puts it).  Both operands are k-contiguous and use
// gemm.hip's row-major LDS image: S[r][32 k + 4 pad], 16-byte LDS writes, a fragment = one ds_read_b128 = the lane's operands of
// four k-steps; k-step j of an 8-k group multiplies k = 8 g + 4 kl + j in BOTH operands, so the permutation cancels in the sum.
// The K chunks of all tiles of the range form ONE double-buffered sequence: the loads of the next tile's first chunk are in
// flight while the last chunk of this one multiplies.  Rows past an operand's end and the D tail are zero-filled (score 0).
// When a tile's K loop ends the caller's epilogue sees the 64 finished scores of each lane, and the accumulators are cleared.
// What an epilogue keeps (counts, running extrema, adjacency words) and how it is folded at the end is each kernel's own.
#pragma once
#include "tag_common.h"
#include <limits.h>

namespace march {

constexpr int T = 128;            // rows of A per workgroup, rows of B (score columns) per tile
constexpr int KC = 32;            // K chunk per barrier
constexpr int LD = KC + 4;        // LDS row stride (144-byte rows: conflict-free b128 reads, as gemm.hip)
constexpr int SZ = T * LD;        // floats per stage buffer
constexpr int NL = T * KC / 1024; // float4 per thread, operand and chunk
constexpr int RQ = KC / 4;        // float4 per row of a chunk
constexpr int RED_LD = 65;        // row stride of an end-of-march fold through LDS (64 partials per row + 1 pad)
constexpr size_t STAGE_BYTES = (size_t)4 * SZ * sizeof(float);        // As[2][SZ], Bs[2][SZ]; free for a fold after the march

// FAST: whole tiles, whole K chunks and 16-byte aligned rows (checked by the launcher, per operand): plain float4 loads, no
// tail tests
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

// Where a thread stands: wave wid owns the rows wm0 .. wm0 + 63 and the columns wn0 .. wn0 + 63 of a tile.  Register r of
// acc[i][j] is row wm0 + acc_row(i, r) + 4 kl, column wn0 + 32 j + ml.
struct Lanes { int lane, wid, wm0, wn0, kl, ml; };
__device__ __forceinline__ Lanes lanes() {
    Lanes l;
    l.lane = threadIdx.x & 63;
    l.wid = threadIdx.x >> 6;
    l.wm0 = (l.wid >> 1) * 64;
    l.wn0 = (l.wid & 1) * 64;
    l.kl = l.lane >> 5;
    l.ml = l.lane & 31;
    return l;
}
// row of accumulator register r of acc[i][.] inside the wave's 64 rows, for the lower 32 lanes (the upper 32 hold the row 4 on)
__host__ __device__ constexpr int acc_row(int i, int r) { return 32 * i + (r & 3) + 8 * (r >> 2); }
// The 64 lanes (2 waves x 32 columns) that share a row leave one partial each in a [T][RED_LD] LDS array; thread t < T then
// reads row t's 64 in lane order.
__device__ __forceinline__ int fold_slot(const Lanes& l, int i, int r) {
    return (l.wm0 + acc_row(i, r) + 4 * l.kl) * RED_LD + (l.wid & 1) * 32 + l.ml;
}

// One operand: rows x D floats, row stride ld, al = 16-byte aligned rows (base and ld)
struct Rows { const float* p; int ld, rows; bool al; };

// The march.  A's rows m0 .. m0 + 127 against B's tiles [t_lo, t_hi); smem = the STAGE_BYTES of dynamic LDS.  epi(tile, acc) runs
// when tile's scores are complete -- after the LDS stores of the next chunk and before the barrier, so its work overlaps the other
// waves' last MFMAs -- and acc is zero again afterwards.  After the return the last barrier has passed: the stage buffers are free.
// Two things keep an epilogue written as a lambda register-for-register what it is when written inside the loop (agc.hip: 230
// VGPRs either way, 245-252 otherwise): a running (value, index) pair is updated with selects (take ? s : best), not with an if
// around two assignments, which inside a lambda stays a branch in part; and a row origin such as m0 + wm0 + 4 kl is formed once
// outside the lambda, so that adding acc_row(i, r) to it is an OR of disjoint bits.  (label_map.hip, which lives at 256 VGPRs
// and spills into AGPRs, keeps its ifs: as selects it needed 8 to 20 more AGPRs.)
template <bool FA, bool FB, class Epi>
__device__ __forceinline__ void march_tiles(float* smem, const Rows& A, const Rows& B, int m0, int t_lo, int t_hi, int D, Epi&& epi) {
    float* As = smem;             // [2][SZ]
    float* Bs = smem + 2 * SZ;    // [2][SZ]
    const int kiters = (D + KC - 1) / KC;
    const int total = (t_hi - t_lo) * kiters;
    const Lanes l = lanes();

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
        load_rows<FA>(ra, A.p, A.ld, m0, A.rows, ld_k * KC, D, A.al);
        load_rows<FB>(rb, B.p, B.ld, ld_tile * T, B.rows, ld_k * KC, D, B.al);
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
        const float* a = As + buf * SZ + (l.wm0 + l.ml) * LD + l.kl * 4;
        const float* b = Bs + buf * SZ + (l.wn0 + l.ml) * LD + l.kl * 4;
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
            epi(tile, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    acc[i][0][r] = 0.0f;
                    acc[i][1][r] = 0.0f;
                }
            kc = 0;
            ++tile;
        }
        __syncthreads();
    }
}

// Column slices.  The launch wants FILL_WGS workgroups (two per CU of 256 by LDS), so few row blocks against many column tiles
// are cut into many slices; with many row blocks SLICES_MIN slices remain, because the workgroups resident on one XCD then are
// GROUP row blocks x several slices -- GROUP + 8 operand tiles of 128 x D floats in flight per XCD instead of 64 + 1, which is what
// its 4 MB L2 can hold at D = 512.  A function of the tile counts alone, so a workspace of slices x rows is one too.
constexpr int FILL_WGS = 512;
constexpr int SLICES_MIN = 8;
constexpr int GROUP = 8;          // row blocks that run side by side over the same slices
struct Plan { int m_tiles, n_tiles, group, slices, tiles_each; long blocks; };
inline Plan make_plan(int m_tiles, int n_tiles) {
    Plan p;
    p.m_tiles = m_tiles;
    p.n_tiles = n_tiles;
    p.group = p.m_tiles < GROUP ? p.m_tiles : GROUP;
    int want = cdiv(FILL_WGS, p.m_tiles);
    if (want < SLICES_MIN) want = SLICES_MIN;
    if (want > p.n_tiles) want = p.n_tiles;
    p.tiles_each = cdiv(p.n_tiles, want);
    p.slices = cdiv(p.n_tiles, p.tiles_each);
    p.blocks = (long)cdiv(p.m_tiles, p.group) * p.group * p.slices;
    return p;
}
// A workgroup's share of the plan: logical order (row-block group, slice, row block of the group), an XCD taking a contiguous
// run of it.  The last group of row blocks may be short: when mt >= m_tiles the whole workgroup leaves.
struct Share { int mt, slice, t_lo, t_hi; };
__device__ __forceinline__ Share plan_share(int n_tiles, int group, int slices, int tiles_each) {
    const int L = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
    Share s;
    s.mt = (L / (group * slices)) * group + L % group;
    s.slice = (L / group) % slices;
    s.t_lo = s.slice * tiles_each;
    s.t_hi = s.t_lo + tiles_each < n_tiles ? s.t_lo + tiles_each : n_tiles;
    return s;
}

// One 64-bit ballot over accumulator register r of acc[i][j] is two finished 32-column words: the low half belongs to row
// wm0 + rl (the lower 32 lanes' row, rl = acc_row(i, r)), the high half to row wm0 + rl + 4.  The halves go into lanes rl and
// rl + 4 of w, so that after the 32 ballots of a column half lane l holds the word of row wm0 + l.  v_writelane_b32 is inline
// assembly: this compiler has no builtin for it, and as a C++ select on the lane number each of the 64 ballots became an
// exec-masked branch.  rl must be a constant once the caller's loops are unrolled.
__device__ __forceinline__ void ballot_to_words(int& w, unsigned long long hit, int rl) {
    asm("v_writelane_b32 %0, %1, %2" : "+v"(w) : "s"((int)(unsigned)hit), "n"(rl));
    asm("v_writelane_b32 %0, %1, %2" : "+v"(w) : "s"((int)(unsigned)(hit >> 32)), "n"(rl + 4));
}

// "<fn>: <var> = <v> exceeds <INT_MAX - step> (<what> index limit)": origins v + step - 1 of rows, columns and chunks are ints
inline int check_index_limit(const char* fn, const char* var, int v, int step, const char* what) {
    if (v <= INT_MAX - step) return 0;
    tag_set_error("%s: %s = %d exceeds %d (%s index limit)", fn, var, v, INT_MAX - step, what);
    return TAG_EINVAL;
}

}  // namespace march
