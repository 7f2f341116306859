// Phrase-to-label cosine map of the AudioSet class-mapping datasets (datasets/class_mapping_dataset.py:15-293 in the reference,
// which calls sklearn's cosine_similarity(phrase, label_embs) on the host per item; utils/label_map.py drives these entry points).
//
// tag_label_map:  s[i][c] = x_i . e_c / (||x_i|| ||e_c||), a zero row's norm taken as 1 (its similarities are exactly 0).  The
//   products are the marching kernel of march_f32.h: a workgroup owns 128 rows of x and walks ALL 128-column tiles of the labels on
//   the exact-fp32 MFMA (operands not rounded).  A first small launch leaves 1 / ||row|| of both operands in ws (N + C floats; the
//   sum of squares in fp64, so the factor carries one rounding).  When a tile's K loop ends each lane turns its 64 accumulator
//   values into s = (acc * rx[row]) * re[column], the ONLY value every output is made of:
//     - sim (optional) gets s with plain 4-byte vector stores, columns past C and rows past N never;
//     - a running (max, index) pair, a running minimum and a running (max, index) pair over the window members
//       (th0 <= s <= th1 && s != 0) per row the lane holds (32 rows).  A lane meets its columns in ascending order and replaces on
//       > only; at the end the 64 lanes that share a row fold through LDS on (value, index), so the lowest c wins a tie.
//       Identical label rows give bit-identical s in any column (the same chain of k-steps, the same norm kernel), so that rule is
//       exact;
//     - ONE 64-bit ballot of the window predicate per accumulator register is two finished words of win_bits (ballot_to_words,
//       as dbscan.hip's epilogue).  The ballot is ANDed with the ballot of (column < C), and after the 64 ballots lane l holds
//       the two words of row wm0 + l: it stores those below ceil(C / 32) and adds their popcounts to the row's window size.
//   No atomics, ws is never zeroed, the same bits on every run, and nothing but the stores of sim depends on whether sim exists.
//
// tag_label_map_topk:  one wave per row of sim: k rounds of a wave argmax over the window members that follow the last pick in
//   the order (s descending, c ascending); the picks go to idx (N, k), -1 once the window is exhausted.  Round one is win_best.
#include "march_f32.h"
#include <math.h>

namespace {

using namespace march;
constexpr size_t LDS_BYTES = STAGE_BYTES + T * sizeof(float);                 // + 1 / ||x|| of the workgroup's rows
static_assert((size_t)2 * T * RED_LD * sizeof(float) + 2 * T * sizeof(int) <= STAGE_BYTES, "the fold reuses the stage buffers");

struct MapOut {
    int* best;
    float* best_sim;
    float* min_sim;
    int* win_best;
    int* win_count;
    unsigned* win_bits;
    float* sim;
    int lds;
};

template <bool FX, bool FE, bool SIM>
__global__ __launch_bounds__(256) void label_map_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ e, int lde,
                                                        const float* __restrict__ inv_x, const float* __restrict__ inv_e, float th0,
                                                        float th1, MapOut out, int N, int C, int D, int W, bool x_al, bool e_al) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* rxs = smem + 4 * SZ;   // [T]
    const int m0 = blockIdx.x * T;
    const Lanes l = lanes();
    const int wid = l.wid, wm0 = l.wm0, lane = l.lane;
    const int brow = m0 + wm0 + lane;     // the row whose window words this lane collects

    float best[2][16], wval[2][16], minv[2][16];
    int bidx[2][16], widx[2][16];
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            best[i][r] = -INFINITY;
            bidx[i][r] = 0;
            wval[i][r] = -INFINITY;
            widx[i][r] = -1;
            minv[i][r] = INFINITY;
        }

    if (threadIdx.x < T) rxs[threadIdx.x] = m0 + (int)threadIdx.x < N ? inv_x[m0 + threadIdx.x] : 1.0f;

    // This lane meets its columns in ascending order (tile, then j) and replaces on > only.  A column past C (its label rows were
    // zero-filled: s = 0) takes part in nothing.
    march_tiles<FX, FE>(smem, Rows{x, ldx, N, x_al}, Rows{e, lde, C, e_al}, m0, 0, (C + T - 1) / T, D,
                        [&](int tile, const f32x16 (&acc)[2][2]) {
        int w[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = tile * T + l.wn0 + j * 32 + l.ml;
            const bool real = n < C;
            const unsigned long long realb = __ballot(real);
            const float re = real ? inv_e[n] : 1.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = acc_row(i, r);             // row wm0 + rl + 4 kl
                    const float s = (acc[i][j][r] * rxs[wm0 + rl + 4 * l.kl]) * re;
                    const bool inw = real && s >= th0 && s <= th1 && s != 0.0f;
                    if constexpr (SIM) {
                        const int row = m0 + wm0 + rl + 4 * l.kl;
                        if (real && row < N) out.sim[(size_t)row * out.lds + n] = s;
                    }
                    if (real && s > best[i][r]) {
                        best[i][r] = s;
                        bidx[i][r] = n;
                    }
                    if (real && s < minv[i][r]) minv[i][r] = s;
                    if (inw && (widx[i][r] < 0 || s > wval[i][r])) {
                        wval[i][r] = s;
                        widx[i][r] = n;
                    }
                    ballot_to_words(w[j], __ballot(inw) & realb, rl);
                }
        }
        if (brow < N) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int word = tile * 4 + (wid & 1) * 2 + j;
                if (word < W) out.win_bits[(size_t)brow * W + word] = (unsigned)w[j];
            }
        }
        cnt += __popc((unsigned)w[0]) + __popc((unsigned)w[1]);
    });

    // fold the 64 lanes that share a row, one quantity after the other; the stage buffers are free after the last barrier
    float* rs = smem;
    int* ri = reinterpret_cast<int*>(smem + T * RED_LD);
    int* rc = reinterpret_cast<int*>(smem + 2 * T * RED_LD);      // [2][T] window sizes of the two column halves
    const int t = threadIdx.x;
    const bool owner = t < T && m0 + t < N;

    rc[(wid & 1) * T + wm0 + lane] = cnt;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = fold_slot(l, i, r);
            rs[o] = best[i][r];
            ri[o] = bidx[i][r];
        }
    __syncthreads();
    if (owner) {
        float bs = rs[t * RED_LD];
        int bn = ri[t * RED_LD];
        for (int c = 1; c < 64; ++c) {
            const float s = rs[t * RED_LD + c];
            const int n = ri[t * RED_LD + c];
            if (s > bs || (s == bs && n < bn)) {
                bs = s;
                bn = n;
            }
        }
        out.best[m0 + t] = bn;
        out.best_sim[m0 + t] = bs;
        out.win_count[m0 + t] = rc[t] + rc[T + t];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = fold_slot(l, i, r);
            rs[o] = wval[i][r];
            ri[o] = widx[i][r];
        }
    __syncthreads();
    if (owner) {
        float bs = 0.0f;
        int bn = -1;
        for (int c = 0; c < 64; ++c) {
            const float s = rs[t * RED_LD + c];
            const int n = ri[t * RED_LD + c];
            if (n >= 0 && (bn < 0 || s > bs || (s == bs && n < bn))) {
                bs = s;
                bn = n;
            }
        }
        out.win_best[m0 + t] = bn;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) rs[fold_slot(l, i, r)] = minv[i][r];
    __syncthreads();
    if (owner) {
        float bs = rs[t * RED_LD];
        for (int c = 1; c < 64; ++c) {
            const float s = rs[t * RED_LD + c];
            bs = s < bs ? s : bs;
        }
        out.min_sim[m0 + t] = bs;
    }
}

constexpr int ROWS_PER_WG = 4;    // one wave per row

// inv[r] = 1 / ||row r|| over the N rows of x and then the C rows of e; 1 for a zero row.  The sum of squares is fp64 (lanes
// striding d, a butterfly), so the fp32 factor is the exact one rounded once.
__global__ __launch_bounds__(256) void label_map_norm_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ e,
                                                             int lde, float* __restrict__ inv, int N, int C, int D) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (r >= (long)N + C) return;
    const float* row = r < N ? x + (size_t)r * ldx : e + (size_t)(r - N) * lde;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) s += (double)row[d] * (double)row[d];
    s = wave_sum_d(s);
    if (lane == 0) inv[r] = s > 0.0 ? (float)(1.0 / sqrt(s)) : 1.0f;
}

__device__ __forceinline__ bool in_window(float s, float th0, float th1) { return s >= th0 && s <= th1 && s != 0.0f; }

__global__ __launch_bounds__(256) void label_map_topk_kernel(const float* __restrict__ sim, int lds, float th0, float th1,
                                                             int* __restrict__ idx, int N, int C, int k) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (i >= N) return;
    const float* row = sim + (size_t)i * lds;
    float pv = 0.0f;              // the last pick; the members after it are s < pv, or s == pv at a column > pn
    int pn = -1;                  // -1: nothing picked yet, every member is a candidate
    for (int round = 0; round < k; ++round) {
        float bs = 0.0f;
        int bn = -1;
        if (round == 0 || pn >= 0) {      // (an exhausted window stays exhausted)
            for (int c = lane; c < C; c += 64) {
                const float s = row[c];
                const bool cand = in_window(s, th0, th1) && (round == 0 || s < pv || (s == pv && c > pn));
                if (cand && (bn < 0 || s > bs)) {         // ascending c: the first of equal values stays
                    bs = s;
                    bn = c;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float s = __shfl_xor(bs, o, 64);
                const int n = __shfl_xor(bn, o, 64);
                if (n >= 0 && (bn < 0 || s > bs || (s == bs && n < bn))) {
                    bs = s;
                    bn = n;
                }
            }
        }
        if (lane == 0) idx[(size_t)i * k + round] = bn;
        pv = bs;
        pn = bn;
    }
}

// row and tile origins (N + 127, C + 127, D + 31) are ints; the grids are one-dimensional (N / 128 and (N + C) / 4 workgroups)
bool shape_ok(int N, int C, int D) { return N >= 1 && C >= 1 && D >= 1 && N <= INT_MAX - T && C <= INT_MAX - T && D <= INT_MAX - KC; }

int check_shape(const char* fn, int N, int C, int D) {
    if (N < 1 || C < 1 || D < 1) {
        tag_set_error("%s: N, C, D must be >= 1 (got %d, %d, %d)", fn, N, C, D);
        return TAG_EINVAL;
    }
    if (int rc = check_index_limit(fn, "N", N, T, "row")) return rc;
    if (int rc = check_index_limit(fn, "C", C, T, "column")) return rc;
    if (int rc = check_index_limit(fn, "D", D, KC, "chunk")) return rc;
    return 0;
}

template <bool FX, bool FE, bool SIM>
void launch_map(const float* x, int ldx, const float* e, int lde, const float* inv, float th0, float th1, const MapOut& out, int N,
                int C, int D, bool x_al, bool e_al, hipStream_t st) {
    static bool attr_set = false;         // (once per process, as gemm.hip's launchers: the library drives one device per process)
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&label_map_kernel<FX, FE, SIM>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
        attr_set = true;
    }
    hipLaunchKernelGGL((label_map_kernel<FX, FE, SIM>), dim3(cdiv(N, T)), dim3(256), LDS_BYTES, st, x, ldx, e, lde, inv, inv + N, th0,
                       th1, out, N, C, D, cdiv(C, 32), x_al, e_al);
}

template <bool SIM>
void launch_map_forms(bool fx, bool fe, const float* x, int ldx, const float* e, int lde, const float* inv, float th0, float th1,
                      const MapOut& out, int N, int C, int D, bool x_al, bool e_al, hipStream_t st) {
    if (fx && fe) launch_map<true, true, SIM>(x, ldx, e, lde, inv, th0, th1, out, N, C, D, x_al, e_al, st);
    else if (fx) launch_map<true, false, SIM>(x, ldx, e, lde, inv, th0, th1, out, N, C, D, x_al, e_al, st);
    else if (fe) launch_map<false, true, SIM>(x, ldx, e, lde, inv, th0, th1, out, N, C, D, x_al, e_al, st);
    else launch_map<false, false, SIM>(x, ldx, e, lde, inv, th0, th1, out, N, C, D, x_al, e_al, st);
}

}  // namespace

extern "C" size_t tag_label_map_ws_bytes(int N, int C, int D) {
    if (!shape_ok(N, C, D)) return 0;
    return ((size_t)N + (size_t)C) * sizeof(float);
}

extern "C" int tag_label_map(const float* x, int ldx, const float* e, int lde, float th0, float th1, int* best, float* best_sim,
                             float* min_sim, int* win_best, int* win_count, unsigned* win_bits, float* sim, int lds, int N, int C,
                             int D, void* ws, void* stream) {
    TAG_CHECK_ARG(x && e && best && best_sim && min_sim && win_best && win_count && win_bits && ws);
    if (int rc = check_shape("tag_label_map", N, C, D)) return rc;
    if (ldx < D || lde < D) {
        tag_set_error("tag_label_map: row strides ldx = %d, lde = %d must be >= D = %d", ldx, lde, D);
        return TAG_EINVAL;
    }
    if (sim && lds < C) {
        tag_set_error("tag_label_map: row stride lds = %d of sim must be >= C = %d", lds, C);
        return TAG_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    float* inv = static_cast<float*>(ws);
    hipLaunchKernelGGL(label_map_norm_kernel, dim3(cdiv((long)N + C, ROWS_PER_WG)), dim3(256), 0, st, x, ldx, e, lde, inv, N, C, D);
    TAG_LAUNCH_CHECK();
    const bool x_al = aligned16(x) && ldx % 4 == 0, e_al = aligned16(e) && lde % 4 == 0;
    const bool fx = x_al && N % T == 0 && D % KC == 0, fe = e_al && C % T == 0 && D % KC == 0;
    const MapOut out = {best, best_sim, min_sim, win_best, win_count, win_bits, sim, lds};
    if (sim) launch_map_forms<true>(fx, fe, x, ldx, e, lde, inv, th0, th1, out, N, C, D, x_al, e_al, st);
    else launch_map_forms<false>(fx, fe, x, ldx, e, lde, inv, th0, th1, out, N, C, D, x_al, e_al, st);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_label_map_topk(const float* sim, int lds, float th0, float th1, int* idx, int N, int C, int k, void* stream) {
    TAG_CHECK_ARG(sim && idx);
    if (int rc = check_shape("tag_label_map_topk", N, C, 1)) return rc;
    if (lds < C) {
        tag_set_error("tag_label_map_topk: row stride lds = %d of sim must be >= C = %d", lds, C);
        return TAG_EINVAL;
    }
    if (k < 1 || k > TAG_LABEL_MAP_MAX_TOPK) {
        tag_set_error("tag_label_map_topk: k = %d must lie in [1, %d]", k, TAG_LABEL_MAP_MAX_TOPK);
        return TAG_EINVAL;
    }
    hipLaunchKernelGGL(label_map_topk_kernel, dim3(cdiv(N, ROWS_PER_WG)), dim3(256), 0, as_stream(stream), sim, lds, th0, th1, idx, N,
                       C, k);
    TAG_LAUNCH_CHECK();
    return 0;
}
