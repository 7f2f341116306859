// The fp64 pair arithmetic of utils/grounding_eval.py that grounding_eval.hip and psds_scores.hip share: the two ratios of one
// (detection, ground truth) pair and numpy's order of additions.  Both files must give the host's integers EXACTLY, so both take
// these functions from here; grounding_eval.hip's header states the rules.
#pragma once
#include "tag_common.h"

namespace {

constexpr int PW_BLOCK = 128;        // numpy's PW_BLOCKSIZE
constexpr int PW_DEPTH = 12;         // halving 32768 terms down to PW_BLOCK takes 8 levels

struct Sum3 {                        // three sums carried through the same order of additions
    double a, b, c;
};
__device__ __forceinline__ Sum3 operator+(Sum3 x, Sum3 y) { return Sum3{x.a + y.a, x.b + y.b, x.c + y.c}; }

// numpy's pairwise_sum for n <= 128 terms term(lo) .. term(lo + n - 1)
template <class V, class F>
__device__ __forceinline__ V np_block(int lo, int n, F term) {
    if (n < 8) {
        V s{};
        for (int i = 0; i < n; ++i) s = s + term(lo + i);
        return s;
    }
    V r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = term(lo + j);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + term(lo + i + j);
    }
    V s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) s = s + term(lo + i);
    return s;
}

// numpy's pairwise_sum for any n <= 32768: the recursion pw(lo, n) = pw(lo, n2) + pw(lo + n2, n - n2), n2 = n / 2 rounded
// down to a multiple of 8, on an explicit stack
template <class V, class F>
__device__ __forceinline__ V np_sum(int n, F term) {
    if (n <= PW_BLOCK) return np_block<V>(0, n, term);
    int lo[PW_DEPTH], len[PW_DEPTH], state[PW_DEPTH];
    V left[PW_DEPTH];
    V ret{};
    int sp = 0;
    lo[0] = 0, len[0] = n, state[0] = 0;
    while (sp >= 0) {
        if (len[sp] <= PW_BLOCK) {
            ret = np_block<V>(lo[sp], len[sp], term);
            --sp;
            continue;
        }
        int n2 = len[sp] / 2;
        n2 -= n2 % 8;
        if (state[sp] == 0) {
            state[sp] = 1;
            lo[sp + 1] = lo[sp], len[sp + 1] = n2, state[sp + 1] = 0;
            ++sp;
        } else if (state[sp] == 1) {
            left[sp] = ret;
            state[sp] = 2;
            lo[sp + 1] = lo[sp] + n2, len[sp + 1] = len[sp] - n2, state[sp + 1] = 0;
            ++sp;
        } else {
            ret = left[sp] + ret;
            --sp;
        }
    }
    return ret;
}

// one (detection, ground truth) pair as utils/grounding_eval.py _pair_ratios computes it (np.minimum / np.maximum spelled out)
struct Pair {
    bool cross;
    double det_prec, gt_cov;
};
__device__ __forceinline__ Pair pair_ratios(double on_d, double off_d, double on_g, double off_g) {
    Pair p;
    p.cross = (on_d <= off_g) && (on_g <= off_d);
    const double lo = (on_d >= on_g || on_d != on_d) ? on_d : on_g;
    const double hi = (off_d <= off_g || off_d != off_d) ? off_d : off_g;
    const double inter = hi - lo;
    p.det_prec = p.cross ? inter / (off_d - on_d) : 0.0;
    p.gt_cov = p.cross ? inter / (off_g - on_g) : 0.0;
    return p;
}

}  // namespace
