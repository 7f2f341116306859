// The second evaluation protocol of the reference on the device (utils/eval_util.py:354-425 compute_sed_eval, utils/sed_utils.py:
// 145-198 double_threshold): hysteresis post-processing of the frame scores, and per (clip, operating point) pair the integers
// that the event-based and the segment-based F-score of sed_eval add up for ONE file with a single label.  The host functions of
// utils/sed_metrics.py are the yardstick; the counts equal theirs exactly.
//
// tag_segments_double: one (clip, operating point) pair per thread, one pass over T like segments_kernel (heads.hip).  A run of
//   x > low is kept when one of its frames has x > high; the kept runs go through connect_ (gap <= n_connect) as they end, so the
//   filter comes before the connection.  Both comparisons are fp32 against the threshold ROUNDED to fp32 (numpy compares a
//   float32 array with a Python float that way); tag_segments compares in fp64.
//
// tag_sed_counts: one wave (= one workgroup of 64) per pair, the ground truths of the clip staged in LDS, the detections read
//   from global memory at a wave-uniform address and turned into seconds as tag_grounding_counts does, (double)frame * res.
//   No floating-point value crosses lanes; integers are folded with a butterfly, which is exact; no atomics; every entry of out
//   is written.
//   ev_tp    Every lane takes ground truths g = lane, lane + 64 and walks the detections once: the detections it may be matched
//            with (onset within t_collar AND offset within max(t_collar, percentage_of_length * length), the fp64 operations of
//            the host function) form ONE index range [lo, hi], because the detections ascend and rounding is monotone.  The
//            graph is convex, so Glover's rule gives a maximum matching: walk the detections in order and give each to the open,
//            unmatched ground truth whose range ends first (a wave-wide integer minimum of (hi << 8 | g) per detection).
//   seg_*    Segment s of 32-segment word w belongs to lane w % 64.  The lane ORs the bits of every event, floor(onset / r) ..
//            ceil(offset / r) - 1, into a reference and a detection word in registers and counts both / detection only /
//            reference only.  seg_n = max over the events of ceil(offset / r), equal to the ceiling of the largest quotient
//            because division and ceil are monotone.  A pair with more than TAG_SED_MAX_SEGMENTS segments is not truncated: all
//            five entries are -1 (the wrapper refuses such inputs before the launch when it is allowed a host read).
#include "tag_common.h"
#include <limits.h>

namespace {

constexpr int MAX_GT = 128;                          // ground-truth rows per clip (LDS staging; two per lane in the matching)
constexpr int MAX_REGIONS = 32768;                   // hi << 8 | g stays below INT_MAX
constexpr int MAX_SEGMENTS = TAG_SED_MAX_SEGMENTS;

__global__ __launch_bounds__(64) void segments_double_kernel(const float* __restrict__ sim, int ld, int B, int T,
                                                             const double* __restrict__ high, const double* __restrict__ low,
                                                             int NT, int n_connect, int64_t* __restrict__ regions,
                                                             int32_t* __restrict__ counts, int max_regions) {
    const int id = blockIdx.x * 64 + threadIdx.x;
    if (id >= B * NT) return;
    const int b = id / NT, ti = id % NT;
    const float* x = sim + (size_t)b * ld;
    const float hi = (float)high[ti], lo = (float)low[ti];
    int64_t* out = regions + (size_t)id * max_regions * 2;
    int n_out = 0;
    bool in_reg = false, has_high = false;
    int reg_start = 0;
    bool have_pending = false;
    int pend_start = 0, pend_end = 0;
    for (int i = 0; i <= T; ++i) {
        const float xi = i < T ? x[i] : 0.0f;
        const bool v = i < T && xi > lo;
        if (v) {
            if (!in_reg) { in_reg = true; reg_start = i; has_high = false; }
            has_high |= xi > hi;
        } else if (in_reg) {
            in_reg = false;
            if (has_high) {
                const int s = reg_start, e = i;
                if (have_pending && s - pend_end <= n_connect) {
                    pend_end = e;
                } else {
                    if (have_pending && n_out < max_regions) { out[2 * n_out] = pend_start; out[2 * n_out + 1] = pend_end; ++n_out; }
                    have_pending = true; pend_start = s; pend_end = e;
                }
            }
        }
    }
    if (have_pending && n_out < max_regions) { out[2 * n_out] = pend_start; out[2 * n_out + 1] = pend_end; ++n_out; }
    counts[id] = n_out;
}

// floor(t / r) and ceil(t / r) as segment indices in [0, MAX_SEGMENTS + 1]: negative, NaN -> 0; anything above the limit -> limit + 1
__device__ __forceinline__ int seg_floor(double t, double r) {
    const double q = floor(t / r);
    return !(q >= 0.0) ? 0 : (q > (double)MAX_SEGMENTS ? MAX_SEGMENTS + 1 : (int)q);
}
__device__ __forceinline__ int seg_ceil(double t, double r) {
    const double q = ceil(t / r);
    return !(q >= 0.0) ? 0 : (q > (double)MAX_SEGMENTS ? MAX_SEGMENTS + 1 : (int)q);
}
// bits of segments [s, e) that fall into the word of segments [base, base + 32)
__device__ __forceinline__ unsigned word_bits(int s, int e, int base) {
    const int a = s > base ? s - base : 0, z = e < base + 32 ? e - base : 32;
    if (a >= z) return 0u;
    const unsigned upto_z = z >= 32 ? 0xffffffffu : ((1u << z) - 1u);
    return upto_z & ~((1u << a) - 1u);
}

__global__ __launch_bounds__(64) void sed_counts_kernel(const long long* __restrict__ regions, const int* __restrict__ counts,
                                                        int max_regions, const double* __restrict__ gt,
                                                        const int* __restrict__ gt_count, int max_gt, int NT, double res,
                                                        double t_collar, double pct, double seg_res, int* __restrict__ out) {
    __shared__ double s_gt[MAX_GT][2];

    const int pair = blockIdx.x, b = pair / NT;
    const int lane = threadIdx.x;
    int D = counts[pair], G = gt_count[b];
    D = D < 0 ? 0 : (D > max_regions ? max_regions : D);        // (the wrapper refuses such inputs; here they must not read
    G = G < 0 ? 0 : (G > max_gt ? max_gt : G);                  //  out of bounds)
    int* dst = out + (size_t)pair * 5;
    const long long* reg = regions + (size_t)pair * max_regions * 2;
    const double* g_rows = gt + (size_t)b * max_gt * 2;
    for (int g = lane; g < G; g += 64) {
        s_gt[g][0] = g_rows[2 * g];
        s_gt[g][1] = g_rows[2 * g + 1];
    }
    __syncthreads();

    // ---- event-based: the index range of each ground truth, then Glover's rule
    int lo[2] = {INT_MAX, INT_MAX}, hi[2] = {-1, -1};
    int ev_tp = 0;
    if (D > 0 && G > 0) {                                       // (wave-uniform)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int g = lane + 64 * k;
            if (g < G) {
                const double on_g = s_gt[g][0], off_g = s_gt[g][1];
                const double by_len = pct * (off_g - on_g);
                const double off_collar = by_len > t_collar ? by_len : t_collar;
                for (int d = 0; d < D; ++d) {
                    const double on_d = (double)reg[2 * d] * res, off_d = (double)reg[2 * d + 1] * res;
                    if (fabs(on_g - on_d) <= t_collar && fabs(off_g - off_d) <= off_collar) {
                        if (lo[k] == INT_MAX) lo[k] = d;
                        hi[k] = d;
                    }
                }
            }
        }
        const int d0 = wave_min_i(lo[0] < lo[1] ? lo[0] : lo[1]);
        const int d1 = wave_max_i(hi[0] > hi[1] ? hi[0] : hi[1]);
        bool used[2] = {false, false};
        for (int d = d0; d <= d1; ++d) {                        // (empty when no ground truth has an edge: d0 = INT_MAX, d1 = -1)
            int key = INT_MAX;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!used[k] && lo[k] <= d && d <= hi[k]) {
                    const int mine = (hi[k] << 8) | (lane + 64 * k);
                    key = mine < key ? mine : key;
                }
            }
            key = wave_min_i(key);
            if (key != INT_MAX) {
                const int g = key & 255;
                if ((g & 63) == lane) used[g >> 6] = true;
                ++ev_tp;                                        // (the same count on every lane)
            }
        }
    }

    // ---- segment-based: the number of segments, then one 32-segment word at a time
    int n_seg = 0;
    for (int g = lane; g < G; g += 64) {
        const int e = seg_ceil(s_gt[g][1], seg_res);
        n_seg = e > n_seg ? e : n_seg;
    }
    for (int d = lane; d < D; d += 64) {
        const int e = seg_ceil((double)reg[2 * d + 1] * res, seg_res);
        n_seg = e > n_seg ? e : n_seg;
    }
    n_seg = wave_max_i(n_seg);
    if (n_seg > MAX_SEGMENTS) {                                 // (wave-uniform) never a truncated count
        if (lane < 5) dst[lane] = -1;
        return;
    }
    int seg_tp = 0, seg_fp = 0, seg_fn = 0;
    for (int base = lane * 32; base < n_seg; base += 64 * 32) {
        unsigned ref = 0u, sys = 0u;
        for (int g = 0; g < G; ++g) ref |= word_bits(seg_floor(s_gt[g][0], seg_res), seg_ceil(s_gt[g][1], seg_res), base);
        for (int d = 0; d < D; ++d)
            sys |= word_bits(seg_floor((double)reg[2 * d] * res, seg_res), seg_ceil((double)reg[2 * d + 1] * res, seg_res), base);
        seg_tp += __popc(ref & sys);
        seg_fp += __popc(sys & ~ref);
        seg_fn += __popc(ref & ~sys);
    }
    seg_tp = wave_sum_i(seg_tp);
    seg_fp = wave_sum_i(seg_fp);
    seg_fn = wave_sum_i(seg_fn);
    if (lane < 5) dst[lane] = lane == 0 ? ev_tp : lane == 1 ? seg_tp : lane == 2 ? seg_fp : lane == 3 ? seg_fn : n_seg;
}

}  // namespace

extern "C" int tag_segments_double(const float* sim, int ld, int B, int T, const double* high, const double* low, int NT,
                                   int n_connect, int64_t* regions, int32_t* counts, int max_regions, void* stream) {
    TAG_CHECK_ARG(sim && high && low && regions && counts);
    if (B < 1 || T < 1 || NT < 1 || ld < T || (long)B * NT > INT_MAX - 64) {
        tag_set_error("tag_segments_double: B, T, NT must be >= 1, ld >= T and B * NT <= %d (got %d, %d, %d, ld %d)", INT_MAX - 64,
                      B, T, NT, ld);
        return TAG_EINVAL;
    }
    if (n_connect < 0 || max_regions < (T + 1) / 2) {
        tag_set_error("tag_segments_double: n_connect = %d must be >= 0 and max_regions = %d >= (T + 1) / 2 = %d", n_connect,
                      max_regions, (T + 1) / 2);
        return TAG_EINVAL;
    }
    hipLaunchKernelGGL(segments_double_kernel, dim3(cdiv((long)B * NT, 64)), dim3(64), 0, as_stream(stream), sim, ld, B, T, high,
                       low, NT, n_connect, regions, counts, max_regions);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_sed_counts(const int64_t* regions, const int32_t* counts, int max_regions, const double* gt,
                              const int32_t* gt_count, int max_gt, int B, int NT, double time_resolution, double t_collar,
                              double percentage_of_length, double segment_resolution, int32_t* out, void* stream) {
    TAG_CHECK_ARG(regions && counts && gt_count && out);
    if (B < 1 || NT < 1 || (long)B * NT > INT_MAX) {
        tag_set_error("tag_sed_counts: B, NT must be >= 1 and B * NT <= %d (got %d, %d)", INT_MAX, B, NT);
        return TAG_EINVAL;
    }
    if (max_regions < 1 || max_regions > MAX_REGIONS) {
        tag_set_error("tag_sed_counts: max_regions = %d: expected 1 .. %d", max_regions, MAX_REGIONS);
        return TAG_EINVAL;
    }
    if (max_gt < 0 || max_gt > MAX_GT) {
        tag_set_error("tag_sed_counts: max_gt = %d: expected 0 .. %d", max_gt, MAX_GT);
        return TAG_EINVAL;
    }
    if (max_gt > 0 && !gt) {
        tag_set_error("tag_sed_counts: gt is null with max_gt = %d", max_gt);
        return TAG_EINVAL;
    }
    if (!(time_resolution > 0.0) || !(segment_resolution > 0.0) || !(t_collar >= 0.0) || !(percentage_of_length >= 0.0)) {
        tag_set_error("tag_sed_counts: expected time_resolution > 0, segment_resolution > 0, t_collar >= 0 and "
                      "percentage_of_length >= 0 (got %g, %g, %g, %g)", time_resolution, segment_resolution, t_collar,
                      percentage_of_length);
        return TAG_EINVAL;
    }
    hipLaunchKernelGGL(sed_counts_kernel, dim3((unsigned)(B * NT)), dim3(64), 0, as_stream(stream),
                       reinterpret_cast<const long long*>(regions), counts, max_regions, gt, gt_count, max_gt, NT, time_resolution,
                       t_collar, percentage_of_length, segment_resolution, out);
    TAG_LAUNCH_CHECK();
    return 0;
}
