// BERTScore phrase-to-label map (utils/data/create_phrase_event_mapping/prepare_phrase_bertscore.py in the reference, which
// scores every (phrase, label) pair with bert_score.score -- the pair re-encoded each time -- and keeps the arg-max F1;
// utils/bertscore_map.py drives this entry point).  What the score needs is a function of the token vectors alone: with
// s_ij = a[n,i] . b[c,j] over the valid tokens of phrase n and label c,
//   P = sum_i a_w[n,i] max_j s_ij / sum_i a_w[n,i],  R = sum_j b_w[c,j] max_i s_ij / sum_j b_w[c,j],  F = 2 P R / (P + R).
//
// The products are the marching kernel of march_f32.h, its sixth client and the first whose epilogue reduces over SEGMENTS of
// rows and columns: the rows of A are phrase tokens, the rows of B (the score columns) label tokens, every item in a slot of
// SA (SB) consecutive rows, SA and SB in {8, 16, 32}, so no item straddles a 128-row tile, a wave's 64 x 64 quadrant or one of
// its four 32 x 32 accumulator blocks.  No token x token matrix exists; everything below happens in registers and across lanes
// when a tile's K loop ends (LDS holds the stage buffers and 1 KB of per-row weights and lengths: two workgroups per CU).
//
// A lane of acc[i][j] holds column 32 j + ml and the 16 rows 32 i + (r & 3) + 8 (r >> 2) + 4 kl.  A slot of SA >= 8 rows is the
// registers r of one group q = r / (SA / 2), in both lane halves (kl); a slot of SB columns is SB neighbouring lanes.  So
//   - the maximum over a label's columns of one row is a butterfly (xor 1 .. SB / 2) over the lanes, columns at or past b_len
//     entering as -inf; every lane of the slot then holds it, and the weighted sum over the phrase's rows runs in the lane
//     (ascending r) and is completed by the lane 32 on;
//   - the maximum over a phrase's rows of one column is taken in the lane (rows at or past a_len skipped) and completed by the
//     lane 32 on; its weighted sum over the label's columns is the same butterfly, as a sum.
// Both the butterflies and the in-lane order depend on the position INSIDE the slot alone, never on where the slot stands: a
// label copied to another index gets the same bits of P, R and F in any column, tile and slice (the dot products themselves
// are the same chain of k-steps in every column).  Padded slots are masked by the lengths; the zero fill is not relied on.
// Each lane keeps a running (F, index, P, R) per phrase it holds (2 x 32 / SA), meets its labels in ascending order and
// replaces on > only.  At the end of the slice the 64 lanes that share a phrase fold through LDS on (F, index), the lowest
// index winning a tie, into ws[slice][phrase]; a second launch folds the slices the same way.  No atomics, ws is never zeroed,
// the same bits on every run, and nothing but the stores of scores depends on whether scores exists.
#include "march_f32.h"
#include <math.h>

namespace {

using namespace march;

struct Best { float f; int idx; float p, r; };

constexpr int MAX_ITEMS = T / 8;                                      // phrases of a row block at the smallest slot
// + weight and length of the workgroup's 128 token rows and the weight sum of its phrases
constexpr size_t LDS_BYTES = STAGE_BYTES + (2 * T + MAX_ITEMS) * sizeof(float);
static_assert((size_t)4 * MAX_ITEMS * RED_LD * sizeof(float) <= STAGE_BYTES, "the fold reuses the stage buffers");

bool slot_ok(int s) { return s == 8 || s == 16 || s == 32; }

// over the S neighbouring lanes of a slot (S a power of two, the slot aligned to it): every lane ends with the same value
template <int S>
__device__ __forceinline__ float slot_max(float v) {
#pragma unroll
    for (int o = 1; o < S; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
template <int S>
__device__ __forceinline__ float slot_sum(float v) {
#pragma unroll
    for (int o = 1; o < S; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int clamp_len(int len, int slot) { return len < 1 ? 1 : (len > slot ? slot : len); }

template <int SA, int SB, bool FAST>
__global__ __launch_bounds__(256, 2) void bertscore_kernel(const float* __restrict__ a, int lda, const int* __restrict__ a_len,
                                                           const float* __restrict__ a_w, const float* __restrict__ b, int ldb,
                                                           const int* __restrict__ b_len, const float* __restrict__ b_w,
                                                           Best* __restrict__ ws, float* __restrict__ scores, int N, int C, int D,
                                                           int m_tiles, int n_tiles, int group, int slices, int tiles_each,
                                                           bool a_al, bool b_al) {
    constexpr int NPH = 32 / SA;          // phrases among the 16 rows a lane holds of acc[i][.]
    constexpr int RPP = 16 / NPH;         // accumulator registers per phrase and lane (the lane 32 on holds the other SA / 2 rows)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* aws = smem + 4 * SZ;                           // [T] a_w of the row, 0 at and past the length
    int* als = reinterpret_cast<int*>(aws + T);           // [T] a_len of the row's phrase, 0 for a phrase past N
    float* wss = aws + 2 * T;                             // [T / SA] sum_i a_w of the phrase, positions ascending
    const Share sh = plan_share(n_tiles, group, slices, tiles_each);
    if (sh.mt >= m_tiles) return;
    const int m0 = sh.mt * T, p0 = m0 / SA;               // first token row and first phrase of the row block
    const Lanes l = lanes();

    if (threadIdx.x < T) {
        const int t = threadIdx.x, ph = p0 + t / SA, pos = t % SA;
        int len = 0;
        float w = 0.0f;
        if (ph < N) {
            len = clamp_len(a_len[ph], SA);
            if (pos < len) w = a_w[(size_t)ph * SA + pos];
        }
        aws[t] = w;
        als[t] = len;
    }
    __syncthreads();
    if (threadIdx.x < T / SA) {
        float s = 0.0f;
        for (int pos = 0; pos < SA; ++pos) s += aws[threadIdx.x * SA + pos];
        wss[threadIdx.x] = s;
    }
    __syncthreads();

    // row r of acc[i][.] stands at position (r & 3) + 4 kl + 8 ((r >> 2) % (SA / 8)) of phrase q = r / RPP
    float bf[2][NPH], bp[2][NPH], br[2][NPH];
    int bi[2][NPH];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < NPH; ++q) {
            bf[i][q] = -INFINITY;
            bi[i][q] = 0;
            bp[i][q] = 0.0f;
            br[i][q] = 0.0f;
        }

    // This lane meets its labels in ascending order (tile, then j) and replaces on > only.  A label past C takes part in nothing.
    march_tiles<FAST, FAST>(smem, Rows{a, lda, N * SA, a_al}, Rows{b, ldb, C * SB, b_al}, m0, sh.t_lo, sh.t_hi, D,
                            [&](int tile, const f32x16 (&acc)[2][2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lab = (tile * T + l.wn0 + j * 32 + l.ml) / SB, cpos = l.ml % SB;
            const bool real = lab < C;
            const int blen = real ? clamp_len(b_len[lab], SB) : 0;
            const bool cvalid = cpos < blen;
            const float bw = cvalid ? b_w[(size_t)lab * SB + cpos] : 0.0f;
            const float wsb = slot_sum<SB>(bw);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < NPH; ++q) {
                    const int alen = als[l.wm0 + 32 * i + q * SA];
                    const float wsa = wss[(l.wm0 + 32 * i) / SA + q];
                    float ps = 0.0f, cm = -INFINITY;
#pragma unroll
                    for (int rr = 0; rr < RPP; ++rr) {
                        const int r = q * RPP + rr;
                        const int rl = acc_row(i, r) + 4 * l.kl;          // row wm0 + rl
                        const bool rvalid = rl % SA < alen;
                        const float s = acc[i][j][r];
                        const float rm = slot_max<SB>(cvalid ? s : -INFINITY);
                        ps += rvalid && real ? aws[l.wm0 + rl] * rm : 0.0f;
                        cm = rvalid ? fmaxf(cm, s) : cm;
                    }
                    ps = ps + __shfl_xor(ps, 32, 64);
                    cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
                    const float rs = slot_sum<SB>(cvalid && alen > 0 ? bw * cm : 0.0f);
                    const float P = wsa != 0.0f ? ps / wsa : 0.0f;
                    const float R = wsb != 0.0f ? rs / wsb : 0.0f;
                    const float F = P + R != 0.0f ? 2.0f * P * R / (P + R) : 0.0f;
                    if (scores != nullptr) {
                        const int ph = p0 + (l.wm0 + 32 * i) / SA + q;
                        if (real && cpos == 0 && l.kl == 0 && ph < N) {
                            const size_t plane = (size_t)N * C, o = (size_t)ph * C + lab;
                            scores[o] = P;
                            scores[plane + o] = R;
                            scores[2 * plane + o] = F;
                        }
                    }
                    const bool take = real && F > bf[i][q];
                    bf[i][q] = take ? F : bf[i][q];
                    bi[i][q] = take ? lab : bi[i][q];
                    bp[i][q] = take ? P : bp[i][q];
                    br[i][q] = take ? R : br[i][q];
                }
        }
    });

    // fold the 64 lanes (2 waves x 32 columns) that share a phrase; the stage buffers are free after the last barrier
    float* rf = smem;
    int* ri = reinterpret_cast<int*>(smem + MAX_ITEMS * RED_LD);
    float* rp = smem + 2 * MAX_ITEMS * RED_LD;
    float* rr_ = smem + 3 * MAX_ITEMS * RED_LD;
    if (l.kl == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < NPH; ++q) {
                const int o = ((l.wm0 + 32 * i) / SA + q) * RED_LD + (l.wid & 1) * 32 + l.ml;
                rf[o] = bf[i][q];
                ri[o] = bi[i][q];
                rp[o] = bp[i][q];
                rr_[o] = br[i][q];
            }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < T / SA && p0 + t < N) {
        int k = 0;
        float f = rf[t * RED_LD];
        int n = ri[t * RED_LD];
        for (int c = 1; c < 64; ++c) {
            const float fc = rf[t * RED_LD + c];
            const int nc = ri[t * RED_LD + c];
            if (fc > f || (fc == f && nc < n)) {
                f = fc;
                n = nc;
                k = c;
            }
        }
        ws[(size_t)sh.slice * N + p0 + t] = Best{f, n, rp[t * RED_LD + k], rr_[t * RED_LD + k]};
    }
}

// the slices of a phrase in ascending order, replacing on (F, index): one thread per phrase
__global__ __launch_bounds__(256) void bertscore_fold_kernel(const Best* __restrict__ ws, int slices, int N, int* __restrict__ best,
                                                             float* __restrict__ best_f, float* __restrict__ best_p,
                                                             float* __restrict__ best_r) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    Best v = ws[n];
#pragma unroll 4
    for (int z = 1; z < slices; ++z) {
        const Best c = ws[(size_t)z * N + n];
        if (c.f > v.f || (c.f == v.f && c.idx < v.idx)) v = c;
    }
    best[n] = v.idx;
    best_f[n] = v.f;
    best_p[n] = v.p;
    best_r[n] = v.r;
}

Plan plan_of(int N, int C, int sa, int sb) { return make_plan(cdiv((long)N * sa, T), cdiv((long)C * sb, T)); }

// token rows N * slot_a and C * slot_b, their tile origins and the chunk origin (D + 31) are ints; the grid is one-dimensional
int check_shape(int N, int C, int D, int sa, int sb) {
    const char* fn = "tag_bertscore_map";
    if (N < 1 || C < 1 || D < 1) {
        tag_set_error("%s: N, C, D must be >= 1 (got %d, %d, %d)", fn, N, C, D);
        return TAG_EINVAL;
    }
    if (!slot_ok(sa) || !slot_ok(sb)) {
        tag_set_error("%s: slot_a = %d, slot_b = %d: the accepted slots are 8, 16 and 32", fn, sa, sb);
        return TAG_EINVAL;
    }
    if ((long)N * sa > INT_MAX - T) {
        tag_set_error("%s: N = %d phrases of slot %d are more than %d token rows (row index limit)", fn, N, sa, INT_MAX - T);
        return TAG_EINVAL;
    }
    if ((long)C * sb > INT_MAX - T) {
        tag_set_error("%s: C = %d labels of slot %d are more than %d token rows (column index limit)", fn, C, sb, INT_MAX - T);
        return TAG_EINVAL;
    }
    if (int rc = check_index_limit(fn, "N * slot_a", N * sa, T, "row")) return rc;
    if (int rc = check_index_limit(fn, "C * slot_b", C * sb, T, "column")) return rc;
    if (int rc = check_index_limit(fn, "D", D, KC, "chunk")) return rc;
    const Plan p = plan_of(N, C, sa, sb);
    if (p.blocks > INT_MAX) {
        tag_set_error("%s: N = %d, C = %d need %ld workgroups (%d row blocks x %d slices), more than the grid limit %d", fn, N, C,
                      p.blocks, p.m_tiles, p.slices, INT_MAX);
        return TAG_EINVAL;
    }
    return 0;
}

struct Args {
    const float* a; int lda; const int* a_len; const float* a_w;
    const float* b; int ldb; const int* b_len; const float* b_w;
    Best* ws; float* scores; int N, C, D; bool a_al, b_al;
};

template <int SA, int SB, bool FAST>
void launch_main(const Args& g, const Plan& p, hipStream_t st) {
    static bool attr_set = false;         // (once per process, as gemm.hip's launchers: the library drives one device per process)
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&bertscore_kernel<SA, SB, FAST>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
        attr_set = true;
    }
    hipLaunchKernelGGL((bertscore_kernel<SA, SB, FAST>), dim3((unsigned)p.blocks), dim3(256), LDS_BYTES, st, g.a, g.lda, g.a_len,
                       g.a_w, g.b, g.ldb, g.b_len, g.b_w, g.ws, g.scores, g.N, g.C, g.D, p.m_tiles, p.n_tiles, p.group, p.slices,
                       p.tiles_each, g.a_al, g.b_al);
}

template <int SA, int SB>
void launch_form(bool fast, const Args& g, const Plan& p, hipStream_t st) {
    if (fast) launch_main<SA, SB, true>(g, p, st);
    else launch_main<SA, SB, false>(g, p, st);
}

template <int SA>
void launch_slot_b(int sb, bool fast, const Args& g, const Plan& p, hipStream_t st) {
    if (sb == 8) launch_form<SA, 8>(fast, g, p, st);
    else if (sb == 16) launch_form<SA, 16>(fast, g, p, st);
    else launch_form<SA, 32>(fast, g, p, st);
}

}  // namespace

extern "C" size_t tag_bertscore_map_ws_bytes(int N, int C, int D, int slot_a, int slot_b) {
    if (N < 1 || C < 1 || D < 1 || !slot_ok(slot_a) || !slot_ok(slot_b)) return 0;
    if ((long)N * slot_a > INT_MAX - T || (long)C * slot_b > INT_MAX - T || D > INT_MAX - KC) return 0;
    const Plan p = plan_of(N, C, slot_a, slot_b);
    if (p.blocks > INT_MAX) return 0;
    return (size_t)p.slices * N * sizeof(Best);
}

extern "C" int tag_bertscore_map(const float* a, int lda, const int32_t* a_len, const float* a_w, const float* b, int ldb,
                                 const int32_t* b_len, const float* b_w, int slot_a, int slot_b, int N, int C, int D, int* best,
                                 float* best_f, float* best_p, float* best_r, float* scores, void* ws, void* stream) {
    TAG_CHECK_ARG(a && a_len && a_w && b && b_len && b_w && best && best_f && best_p && best_r && ws);
    if (int rc = check_shape(N, C, D, slot_a, slot_b)) return rc;
    if (lda < D || ldb < D) {
        tag_set_error("tag_bertscore_map: row strides lda = %d, ldb = %d must be >= D = %d", lda, ldb, D);
        return TAG_EINVAL;
    }
    const Plan p = plan_of(N, C, slot_a, slot_b);
    Args g = {a, lda, a_len, a_w, b, ldb, b_len, b_w, static_cast<Best*>(ws), scores, N, C, D, false, false};
    g.a_al = aligned16(a) && lda % 4 == 0;
    g.b_al = aligned16(b) && ldb % 4 == 0;
    const bool fast = g.a_al && g.b_al && (N * slot_a) % T == 0 && (C * slot_b) % T == 0 && D % KC == 0;
    hipStream_t st = as_stream(stream);
    if (slot_a == 8) launch_slot_b<8>(slot_b, fast, g, p, st);
    else if (slot_a == 16) launch_slot_b<16>(slot_b, fast, g, p, st);
    else launch_slot_b<32>(slot_b, fast, g, p, st);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(bertscore_fold_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, g.ws, p.slices, N, best, best_f, best_p, best_r);
    TAG_LAUNCH_CHECK();
    return 0;
}
