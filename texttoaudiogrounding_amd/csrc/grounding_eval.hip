// Operating-point counts of the grounding evaluation on the device: for every (clip, threshold) pair the four integers that
// utils/grounding_eval.py's evaluate_detections (threshold-AUC: tp_preds, tp_refs) and psds_operating_point (psds_tp, psds_fp) add
// up for ONE file, from tag_segments' integer regions and the clip's ground-truth rows.  The host functions stay the yardstick:
// the counts equal theirs EXACTLY, also where a ratio sum lands on dtc / gtc up to rounding (segments on the frame grid do so all
// the time) and for zero-duration ground-truth rows (0/0 = NaN, which compares false).  That takes fp64 with IEEE division
// (-fno-fast-math -ffp-contract=off, csrc/Makefile) AND numpy's order of additions:
//
//   * a sum over the ground truths of one detection (det_prec.sum(1) and its masked variant) is numpy's contiguous fp64
//     reduction, np_sum of grounding_pairs.h: fewer than 8 terms left to right; up to 128 terms eight running lanes r[j] += a[i + j], combined as
//     ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the remainder added in order; above 128 terms the halves (the first rounded down to a
//     multiple of 8) summed on their own and added.
//   * a sum over the detections of one ground truth (gt_cov.sum(0) and its masked variants) is left to right in d when the file
//     has two or more ground truths (numpy adds row after row) -- and np_sum over d when it has exactly ONE: a (D, 1) array is
//     contiguous along d and numpy reduces it with the same pairwise routine.
//   * a masked term is the ratio times 0.0 or 1.0 and is still added (inf * 0 = NaN, as on the host).
//
// No floating-point value crosses lanes.  One wave (= one workgroup of 64) per (clip, threshold) pair:
//   phase 1  lanes stride the detections: row sum of det_prec in numpy's order -> the DTC flags (recall criterion: with "crosses
//            any ground truth"; PSDS relevance: without), one byte per detection in LDS; psds_fp counts the irrelevant ones
//   phase 2  lanes stride the ground truths: the three column sums of gt_cov (all detections / DTC-passing / relevant) ->
//            tp_refs, psds_tp and the GTC flags, one byte per ground truth in LDS
//   phase 3  lanes stride the detections again: row sum of det_prec over the GTC-passing ground truths -> tp_preds
// The ratios are recomputed where they are needed (the same operations give the same bits); the ground truths of the clip are
// staged in LDS, the detections are read from global memory at a wave-uniform address.  The integer counts are folded with a
// butterfly, which is exact.  No atomics; every entry of out is written.
#include "grounding_pairs.h"      // np_sum, pair_ratios, Sum3: shared with psds_scores.hip
#include <limits.h>

namespace {

constexpr int MAX_GT = 128;          // ground-truth rows per clip (LDS staging; numpy's pairwise block size, so row sums never recurse)
constexpr int MAX_REGIONS = 32768;   // detection flags: one byte each in dynamic LDS

constexpr unsigned char F_DTC = 1, F_RELEVANT = 2;

__global__ __launch_bounds__(64) void grounding_counts_kernel(const long long* __restrict__ regions, const int* __restrict__ counts,
                                                              int max_regions, const double* __restrict__ gt,
                                                              const int* __restrict__ gt_count, int max_gt, int NT, double res,
                                                              double dtc, double gtc, int* __restrict__ out) {
    __shared__ double s_gt[MAX_GT][2];
    __shared__ unsigned char s_gflag[MAX_GT];
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dflag[];     // [max_regions]

    const int pair = blockIdx.x, b = pair / NT;
    const int lane = threadIdx.x;
    int D = counts[pair], G = gt_count[b];
    D = D < 0 ? 0 : (D > max_regions ? max_regions : D);        // (the wrapper refuses such inputs; here they must not read
    G = G < 0 ? 0 : (G > max_gt ? max_gt : G);                  //  out of bounds)
    int* dst = out + (size_t)pair * 4;
    if (D == 0 || G == 0) {                                      // (wave-uniform: nobody reaches a barrier)
        if (lane < 4) dst[lane] = (lane == 3 && G == 0) ? D : 0;
        return;
    }
    const long long* reg = regions + (size_t)pair * max_regions * 2;
    const double* g_rows = gt + (size_t)b * max_gt * 2;
    for (int g = lane; g < G; g += 64) {
        s_gt[g][0] = g_rows[2 * g];
        s_gt[g][1] = g_rows[2 * g + 1];
    }
    __syncthreads();

    int tp_preds = 0, tp_refs = 0, psds_tp = 0, psds_fp = 0;

    // phase 1: detection d against every ground truth
    for (int d = lane; d < D; d += 64) {
        const double on_d = (double)reg[2 * d] * res, off_d = (double)reg[2 * d + 1] * res;
        bool any = false;
        const double row = np_sum<double>(G, [&](int g) {
            const Pair p = pair_ratios(on_d, off_d, s_gt[g][0], s_gt[g][1]);
            any |= p.cross;
            return p.det_prec;
        });
        const bool relevant = row >= dtc;
        psds_fp += !relevant;
        s_dflag[d] = (unsigned char)((relevant && any ? F_DTC : 0) | (relevant ? F_RELEVANT : 0));
    }
    __syncthreads();

    // phase 2: ground truth g against every detection
    for (int g = lane; g < G; g += 64) {
        const double on_g = s_gt[g][0], off_g = s_gt[g][1];
        bool any = false, any_pass = false;
        auto term = [&](int d) {
            const double on_d = (double)reg[2 * d] * res, off_d = (double)reg[2 * d + 1] * res;
            const Pair p = pair_ratios(on_d, off_d, on_g, off_g);
            const unsigned char f = s_dflag[d];
            any |= p.cross;
            any_pass |= p.cross && (f & F_DTC);
            return Sum3{p.gt_cov, p.gt_cov * ((f & F_DTC) ? 1.0 : 0.0), p.gt_cov * ((f & F_RELEVANT) ? 1.0 : 0.0)};
        };
        Sum3 col;
        if (G == 1) {
            col = np_sum<Sum3>(D, term);                        // a (D, 1) array is contiguous along d
        } else {
            col = Sum3{0.0, 0.0, 0.0};
            for (int d = 0; d < D; ++d) col = col + term(d);
        }
        tp_refs += (col.b >= gtc) && any_pass;
        psds_tp += col.c >= gtc;
        s_gflag[g] = (col.a >= gtc) && any;
    }
    __syncthreads();

    // phase 3: detection d against the ground truths that pass the GTC
    for (int d = lane; d < D; d += 64) {
        const double on_d = (double)reg[2 * d] * res, off_d = (double)reg[2 * d + 1] * res;
        bool any_pass = false;
        const double row = np_sum<double>(G, [&](int g) {
            const Pair p = pair_ratios(on_d, off_d, s_gt[g][0], s_gt[g][1]);
            const bool pass = s_gflag[g];
            any_pass |= p.cross && pass;
            return p.det_prec * (pass ? 1.0 : 0.0);
        });
        tp_preds += (row >= dtc) && any_pass;
    }

    tp_preds = wave_sum_i(tp_preds);
    tp_refs = wave_sum_i(tp_refs);
    psds_tp = wave_sum_i(psds_tp);
    psds_fp = wave_sum_i(psds_fp);
    if (lane < 4) dst[lane] = lane == 0 ? tp_preds : lane == 1 ? tp_refs : lane == 2 ? psds_tp : psds_fp;
}

}  // namespace

extern "C" int tag_grounding_counts(const int64_t* regions, const int32_t* counts, int max_regions, const double* gt,
                                    const int32_t* gt_count, int max_gt, int B, int NT, double time_resolution, double dtc,
                                    double gtc, int32_t* out, void* stream) {
    TAG_CHECK_ARG(regions && counts && gt_count && out);
    if (B < 1 || NT < 1 || (long)B * NT > INT_MAX) {
        tag_set_error("tag_grounding_counts: B, NT must be >= 1 and B * NT <= %d (got %d, %d)", INT_MAX, B, NT);
        return TAG_EINVAL;
    }
    if (max_regions < 1 || max_regions > MAX_REGIONS) {
        tag_set_error("tag_grounding_counts: max_regions = %d: expected 1 .. %d", max_regions, MAX_REGIONS);
        return TAG_EINVAL;
    }
    if (max_gt < 0 || max_gt > MAX_GT) {
        tag_set_error("tag_grounding_counts: max_gt = %d: expected 0 .. %d", max_gt, MAX_GT);
        return TAG_EINVAL;
    }
    if (max_gt > 0 && !gt) {
        tag_set_error("tag_grounding_counts: gt is null with max_gt = %d", max_gt);
        return TAG_EINVAL;
    }
    if (!(time_resolution > 0.0) || !(dtc >= 0.0 && dtc <= 1.0) || !(gtc >= 0.0 && gtc <= 1.0)) {
        tag_set_error("tag_grounding_counts: expected time_resolution > 0 and dtc, gtc in [0, 1] (got %g, %g, %g)", time_resolution,
                      dtc, gtc);
        return TAG_EINVAL;
    }
    const size_t lds = ((size_t)max_regions + 15) / 16 * 16;
    hipLaunchKernelGGL(grounding_counts_kernel, dim3((unsigned)(B * NT)), dim3(64), lds, as_stream(stream),
                       reinterpret_cast<const long long*>(regions), counts, max_regions, gt, gt_count, max_gt, NT, time_resolution,
                       dtc, gtc, out);
    TAG_LAUNCH_CHECK();
    return 0;
}
