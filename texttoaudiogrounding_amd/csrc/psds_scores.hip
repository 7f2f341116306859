// Score-based PSDS on the device: for every (clip, phrase) pair the PSDS counts of EVERY decision threshold its frame scores
// define, as deltas over the sorted distinct scores.  The yardstick is utils/psds_scores.py pair_regimes, which evaluates each
// regime through utils/grounding_eval.py psds_operating_point; the integers here equal its integers.
//
// With v_1 < ... < v_m the distinct non-NaN scores of the row and v_0 = -inf, regime k = 0 .. m has the active frames
// score > v_k, its detections are the maximal runs [on, off) of active frames, in seconds ((double)frame * res, as
// tag_grounding_counts forms them), and c_k = (psds_tp, psds_fp) of those detections against the pair's ground truths.  No median
// filter, no connect step.  A NaN score is never active and is no value; -0.0 and +0.0 are one value (+0.0 is written).
//
// One workgroup of four waves per pair:
//   1  the row goes to LDS twice: as it is (the active test) and as order-preserving 32-bit keys, NaN and the padding up to a
//      power of two as the largest key; a bitonic sort of the keys; wave 0 squeezes the duplicates out with ballots
//   2  the waves stride the m + 1 regimes.  Per regime a wave walks the row 64 frames at a time: one ballot per chunk, the
//      rising and falling edges of the mask are the onsets and offsets, which go to the wave's own list in LDS in order.  Then
//      the count arithmetic of grounding_counts_kernel phases 1 and 2 (psds_tp and psds_fp only) on that list: lanes stride the
//      detections (np_sum over the ground truths -> relevant), then the ground truths (the column sum over the relevant
//      detections, left to right for G >= 2, numpy's pairwise order for G == 1).  A regime is always recomputed from its
//      frames: the fp64 sums depend on the order of the detections, so nothing is carried from one regime to the next.
//   3  differences of consecutive regimes and the padding.
// No floating-point value crosses lanes, no atomics, no host read: the same bits on every run.  Every entry of the four
// outputs is written.
#include "grounding_pairs.h"
#include <limits.h>

namespace {

constexpr int MAX_GT = 128;                  // ground-truth rows per pair, as tag_grounding_counts
constexpr int MAX_T = TAG_PSDS_SCORES_MAX_T; // frames per pair: the row, its keys, its values and the counts live in LDS
constexpr int MAX_RUNS = MAX_T / 2;          // runs of active frames are separated by an inactive one
constexpr int WAVES = 4, THREADS = 64 * WAVES;
constexpr unsigned KEY_NONE = 0xffffffffu;   // NaN and padding: above the key of +inf (0xff800000)

__device__ __forceinline__ unsigned key_of(float x) {
    if (x != x) return KEY_NONE;
    if (x == 0.0f) x = 0.0f;                 // -0.0 -> +0.0
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// LDS written by some lanes of a wave and read by others of the SAME wave: the hardware keeps a wave's LDS operations in order, the
// compiler must not move them across this point
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(THREADS) void psds_score_deltas_kernel(const float* __restrict__ sim, int ld, int T,
                                                                    const double* __restrict__ gt,
                                                                    const int* __restrict__ gt_count, int max_gt, double res,
                                                                    double dtc, double gtc, float* __restrict__ values,
                                                                    int* __restrict__ deltas, int* __restrict__ base,
                                                                    int* __restrict__ n_values) {
    __shared__ float s_x[MAX_T];                     // the row
    __shared__ unsigned s_key[MAX_T];                // sort keys
    __shared__ float s_val[MAX_T];                   // distinct values, ascending
    __shared__ int s_cnt[MAX_T + 1][2];              // (psds_tp, psds_fp) per regime
    __shared__ double s_gt[MAX_GT][2];
    __shared__ unsigned short s_on[WAVES][MAX_RUNS], s_off[WAVES][MAX_RUNS];
    __shared__ unsigned char s_rel[WAVES][MAX_RUNS]; // relevant flag per detection
    __shared__ int s_m;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int G = gt_count[b];
    G = G < 0 ? 0 : (G > max_gt ? max_gt : G);       // (the wrapper refuses such inputs; here they must not read out of bounds)
    const float* row = sim + (size_t)b * ld;
    int N = 1;
    while (N < T) N <<= 1;                           // <= MAX_T, a power of two

    for (int i = tid; i < N; i += THREADS) {
        const float x = i < T ? row[i] : 0.0f;
        if (i < T) s_x[i] = x;
        s_key[i] = i < T ? key_of(x) : KEY_NONE;
    }
    const double* g_rows = gt + (size_t)b * max_gt * 2;
    for (int g = tid; g < G; g += THREADS) {
        s_gt[g][0] = g_rows[2 * g];
        s_gt[g][1] = g_rows[2 * g + 1];
    }
    __syncthreads();

    // 1: bitonic sort, ascending
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const unsigned a = s_key[i], c = s_key[p];
                    if ((a > c) == ((i & k) == 0)) {
                        s_key[i] = c;
                        s_key[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // distinct values: the first key of each run of equal keys, NaN / padding left out
    if (wave == 0) {
        int m = 0;
        for (int c = 0; c < N; c += 64) {
            const int i = c + lane;
            const unsigned key = i < N ? s_key[i] : KEY_NONE;
            const bool first = key != KEY_NONE && (i == 0 || s_key[i - 1] != key);
            const unsigned long long mask = __ballot(first);
            if (first) s_val[m + __popcll(mask & ((1ull << lane) - 1ull))] = value_of(key);
            m += __popcll(mask);
        }
        if (lane == 0) s_m = m;
    }
    __syncthreads();
    const int m = s_m;

    // 2: regime k, active = score > v_k
    for (int k = wave; k <= m; k += WAVES) {
        const float v = k == 0 ? -INFINITY : s_val[k - 1];
        int D = 0, n_off = 0;
        bool prev = false;                           // frame before the chunk active (wave-uniform)
        for (int c = 0; c <= T; c += 64) {           // frame T is never active: it closes a run that reaches the end
            const int t = c + lane;
            const bool act = t < T && s_x[t] > v;
            const unsigned long long mask = __ballot(act);
            const unsigned long long before = (mask << 1) | (prev ? 1ull : 0ull);
            const unsigned long long rise = mask & ~before, fall = ~mask & before;
            const unsigned long long below = (1ull << lane) - 1ull;
            if ((rise >> lane) & 1ull) s_on[wave][D + __popcll(rise & below)] = (unsigned short)t;
            if ((fall >> lane) & 1ull) s_off[wave][n_off + __popcll(fall & below)] = (unsigned short)t;
            D += __popcll(rise);
            n_off += __popcll(fall);
            prev = (mask >> 63) & 1ull;
        }
        wave_lds_sync();

        int tp = 0, fp = 0;
        if (G == 0) {
            fp = lane == 0 ? D : 0;
        } else if (D > 0) {
            for (int d = lane; d < D; d += 64) {
                const double on_d = (double)s_on[wave][d] * res, off_d = (double)s_off[wave][d] * res;
                const double rsum = np_sum<double>(G, [&](int g) { return pair_ratios(on_d, off_d, s_gt[g][0], s_gt[g][1]).det_prec; });
                const bool relevant = rsum >= dtc;
                fp += !relevant;
                s_rel[wave][d] = relevant;
            }
            wave_lds_sync();
            for (int g = lane; g < G; g += 64) {
                const double on_g = s_gt[g][0], off_g = s_gt[g][1];
                auto term = [&](int d) {
                    const double on_d = (double)s_on[wave][d] * res, off_d = (double)s_off[wave][d] * res;
                    return pair_ratios(on_d, off_d, on_g, off_g).gt_cov * (s_rel[wave][d] ? 1.0 : 0.0);
                };
                double col;
                if (G == 1) {
                    col = np_sum<double>(D, term);               // a (D, 1) array is contiguous along d
                } else {
                    col = 0.0;
                    for (int d = 0; d < D; ++d) col = col + term(d);
                }
                tp += col >= gtc;
            }
        }
        tp = wave_sum_i(tp);
        fp = wave_sum_i(fp);
        if (lane == 0) {
            s_cnt[k][0] = tp;
            s_cnt[k][1] = fp;
        }
        // the next regime overwrites the wave's lists: every lane is done reading them
        wave_lds_sync();
    }
    __syncthreads();

    // 3: outputs
    float* o_val = values + (size_t)b * T;
    int* o_del = deltas + (size_t)b * T * 2;
    for (int j = tid; j < T; j += THREADS) {
        const bool in = j < m;
        o_val[j] = in ? s_val[j] : INFINITY;
        o_del[2 * j] = in ? s_cnt[j + 1][0] - s_cnt[j][0] : 0;
        o_del[2 * j + 1] = in ? s_cnt[j + 1][1] - s_cnt[j][1] : 0;
    }
    if (tid < 2) base[(size_t)b * 2 + tid] = s_cnt[0][tid];
    if (tid == 2) n_values[b] = m;
}

}  // namespace

extern "C" int tag_psds_score_deltas(const float* sim, int ld, int B, int T, const double* gt, const int32_t* gt_count, int max_gt,
                                     double time_resolution, double dtc, double gtc, float* values, int32_t* deltas, int32_t* base,
                                     int32_t* n_values, void* stream) {
    TAG_CHECK_ARG(sim && gt_count && values && deltas && base && n_values);
    if (B < 1) {
        tag_set_error("tag_psds_score_deltas: B = %d: expected B >= 1", B);
        return TAG_EINVAL;
    }
    if (T < 1 || T > MAX_T) {
        tag_set_error("tag_psds_score_deltas: T = %d: expected 1 .. %d", T, MAX_T);
        return TAG_EINVAL;
    }
    if (ld < T) {
        tag_set_error("tag_psds_score_deltas: ld = %d: expected ld >= T = %d", ld, T);
        return TAG_EINVAL;
    }
    if (max_gt < 0 || max_gt > MAX_GT) {
        tag_set_error("tag_psds_score_deltas: max_gt = %d: expected 0 .. %d", max_gt, MAX_GT);
        return TAG_EINVAL;
    }
    if (max_gt > 0 && !gt) {
        tag_set_error("tag_psds_score_deltas: gt is null with max_gt = %d", max_gt);
        return TAG_EINVAL;
    }
    if (!(time_resolution > 0.0) || !(dtc >= 0.0 && dtc <= 1.0) || !(gtc >= 0.0 && gtc <= 1.0)) {
        tag_set_error("tag_psds_score_deltas: expected time_resolution > 0 and dtc, gtc in [0, 1] (got %g, %g, %g)",
                      time_resolution, dtc, gtc);
        return TAG_EINVAL;
    }
    hipLaunchKernelGGL(psds_score_deltas_kernel, dim3((unsigned)B), dim3(THREADS), 0, as_stream(stream), sim, ld, T, gt, gt_count,
                       max_gt, time_resolution, dtc, gtc, values, deltas, base, n_values);
    TAG_LAUNCH_CHECK();
    return 0;
}
