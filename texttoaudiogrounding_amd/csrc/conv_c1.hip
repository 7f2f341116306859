// A1, block 1's first convolution: 3x3 / stride 1 / pad 1 / no bias with Cin = 1 (models/panns.py:25-33 on the (B, 1, T, mel)
// log-mel input).  With one input channel there is no K axis to put on the matrix pipe: the product is a 9-tap stencil over
// x (B, H, W) against w (Cout, 9), and every kernel here is bound by the HBM traffic of the (B, H, W, Cout) side.
//
// The column affine: bn0 is a BatchNorm2d over the mel axis, i.e. one (scale, shift) pair per COLUMN w of the input.  Every
// kernel that reads x takes cs / ct (both null or both given) and forms fmaf(x[h][w], cs[w], ct[w]) on load, BEFORE the zero
// padding (a padded tap is 0, not ct[w]), so the normalised input never exists in HBM.
//
// Which kernel serves which shape (the launchers below choose; anything else is TAG_EINVAL):
//   forward    W == 64 && Cout == 64       conv_c1_fwd_rows_kernel<TS>: input rows in an LDS ring, fp32 or bf16 output,
//                                          optionally the BatchNorm statistics of the output (the _forward_stats entries)
//              W % 4 == 0, 256 % (Cout/4) == 0   conv_c1_fwd4_kernel<false>: 4 pixels x 4 couts per thread
//              any other Cout % 4 == 0     conv_c1_fwd_kernel: 1 pixel x 4 couts per thread
//              + per-clip bias             conv_c1_fwd4_kernel<true> (the 4-pixel domain only)
//   backward   W == 64 && Cout == 64       conv_c1_bwd_kernel<TS, FUSE>: dw and dx in ONE pass over dy on the 16x16x4 fp32
//                                          MFMA; FUSE applies the backward of relu(bn1(.)) to dy as it arrives
//              Cout/4 a divisor of 64      conv_c1_wgrad_kernel<4> (W % 4 == 0) or <1>, fp64 partials per workgroup folded
//                                          by conv_c1_wgrad_finalize_kernel; conv_c1_dgrad_kernel
#include "tag_common.h"

namespace {

__device__ __forceinline__ float c1_in(const float* x, const float* cs, const float* ct, int H, int W, long m,
                                       int h, int w, int dy, int dx) {
    const int hh = h + dy, ww = w + dx;
    if (hh < 0 || hh >= H || ww < 0 || ww >= W) return 0.0f;
    const float v = x[m + (long)dy * W + dx];
    return cs ? fmaf(v, cs[ww], ct[ww]) : v;
}

__global__ __launch_bounds__(256) void conv_c1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ cs,
                                                          const float* __restrict__ ct, const float* __restrict__ w,
                                                          float* __restrict__ y, long M, int H, int W, int Cout) {
    const int C4 = Cout >> 2;
    const long total = M * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4) << 2;
        const long m = i / C4;
        const int hw = (int)(m % ((long)H * W));
        const int h = hw / W, ww = hw % W;
        float o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float v = c1_in(x, cs, ct, H, W, m, h, ww, tap / 3 - 1, tap % 3 - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fmaf(v, w[(c + j) * 9 + tap], o[j]);
        }
        *reinterpret_cast<float4*>(y + m * Cout + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// 4 consecutive pixels along W x 4 output channels per thread: the 3 x 6 input patch (bn0 affine applied once per
// value) is reused by 144 FMAs, weights live in registers.  Requires W % 4 == 0.
__device__ __forceinline__ void c1_patch(const float* x, const float* cs, const float* ct, int H, int W, long mrow,
                                         int h, int w0, float xin[3][6]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int hh = h + r - 1;
        const bool hok = (unsigned)hh < (unsigned)H;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const int ww = w0 + c - 1;
            const bool ok = hok & ((unsigned)ww < (unsigned)W);
            const int wc = ok ? ww : w0;
            const long off = ok ? (long)(r - 1) * W + (c - 1) : 0;
            const float v = x[mrow + off];
            const float a = cs ? fmaf(v, cs[wc], ct[wc]) : v;
            xin[r][c] = ok ? a : 0.0f;
        }
    }
}

// BIAS: a per-clip bias on the output (CrossCDur block 1), y = conv(affine(x)) + bias[b, cout].  The pixel groups run over the
// whole batch, so a workgroup may hold rows of two clips: the bias row is the group's own clip m / (H W).  The bias is added
// last, after the plain instance's sum: an all-zero table gives its output bit for bit.  The plain instance never touches `bias`.
template <bool BIAS>
__global__ __launch_bounds__(256) void conv_c1_fwd4_kernel(const float* __restrict__ x, const float* __restrict__ cs,
                                                           const float* __restrict__ ct, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y, long M,
                                                           int H, int W, int Cout) {
    const int C4 = Cout >> 2, gpi = 256 / C4;   // requires 256 % C4 == 0: a thread keeps its channel quad
    const long groups = M >> 2;                 // W % 4 == 0 -> M % 4 == 0 and a group never straddles a row
    const int c = (threadIdx.x % C4) << 2;
    const long HW = (long)H * W;
    float wr[4][9];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) wr[j][t] = w[(c + j) * 9 + t];
    for (long gi = (long)blockIdx.x * gpi + threadIdx.x / C4; gi < groups; gi += (long)gridDim.x * gpi) {
        const long m = gi << 2;
        const long b = m / HW;
        const int hw = (int)(m - b * HW);
        const int h = hw / W, w0 = hw % W;
        float4 bv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if constexpr (BIAS) bv = *reinterpret_cast<const float4*>(bias + b * Cout + c);
        float xin[3][6];
        c1_patch(x, cs, ct, H, W, m, h, w0, xin);
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            float o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaf(xin[tap / 3][px + tap % 3], wr[j][tap], o[j]);
            if constexpr (BIAS) { o[0] += bv.x; o[1] += bv.y; o[2] += bv.z; o[3] += bv.w; }
            *reinterpret_cast<float4*>(y + (m + px) * Cout + c) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// dw partials [nblk][Cout*9] doubles, one row per workgroup.  A thread keeps its channel quad and walks the pixels in steps of
// PX: 4-pixel groups through c1_patch (PX = 4, needs W % 4 == 0) or single pixels through c1_in (PX = 1).
template <int PX>
__global__ __launch_bounds__(256) void conv_c1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ cs,
                                                            const float* __restrict__ ct,
                                                            const float* __restrict__ dy, double* __restrict__ partials,
                                                            long M, int H, int W, int Cout) {
    extern __shared__ double sred[];         // [4 waves][64][36] (only lanes < tpr used)
    const int tpr = Cout >> 2, rpi = 256 / tpr;
    const int c = (threadIdx.x % tpr) << 2, rsub = threadIdx.x / tpr;
    float acc[4][9];
    double dacc[4][9];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) { acc[j][t] = 0.0f; dacc[j][t] = 0.0; }
    int cnt = 0;
    const long steps = M / PX;
    for (long s = (long)blockIdx.x * rpi + rsub; s < steps; s += (long)gridDim.x * rpi) {
        const long m = s * PX;
        const int hw = (int)(m % ((long)H * W));
        const int h = hw / W, w0 = hw % W;
        if constexpr (PX == 4) {
            float xin[3][6];
            c1_patch(x, cs, ct, H, W, m, h, w0, xin);
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const float4 g = *reinterpret_cast<const float4*>(dy + (m + px) * Cout + c);
                const float gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j][tap] = fmaf(xin[tap / 3][px + tap % 3], gv[j], acc[j][tap]);
            }
        } else {
            const float4 g = *reinterpret_cast<const float4*>(dy + m * Cout + c);
            const float gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float v = c1_in(x, cs, ct, H, W, m, h, w0, tap / 3 - 1, tap % 3 - 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j][tap] = fmaf(v, gv[j], acc[j][tap]);
            }
        }
        if (++cnt == 64 / PX) {   // flush the fp32 partial sums into fp64 every 64 pixels
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < 9; ++t) { dacc[j][t] += acc[j][t]; acc[j][t] = 0.0f; }
            cnt = 0;
        }
    }
    // threads sharing a channel quad sit tpr lanes apart: fold inside the wave, then across the 4 waves
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            double v = dacc[j][t] + (double)acc[j][t];
            for (int o = 32; o >= tpr; o >>= 1) v += __shfl_xor(v, o, 64);
            dacc[j][t] = v;
        }
    if (lane < tpr) {
        double* mine = sred + (wid * 64 + lane) * 36;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 9; ++t) mine[j * 9 + t] = dacc[j][t];
    }
    __syncthreads();
    if (threadIdx.x < tpr) {
        double* p = partials + (size_t)blockIdx.x * Cout * 9;
        for (int e = 0; e < 36; ++e) {
            double s = 0;
            for (int wv = 0; wv < 4; ++wv) s += sred[(wv * 64 + threadIdx.x) * 36 + e];
            p[(c + e / 9) * 9 + e % 9] = s;
        }
    }
}

__global__ __launch_bounds__(256) void conv_c1_wgrad_finalize_kernel(const double* __restrict__ partials, int nblk,
                                                                    int n, float* __restrict__ dw) {
    // 8 outputs x 32 interleaved parts per block (four independent chains per part keep the loads in flight), folded
    // through LDS in a fixed order
    __shared__ double sh[32][9];
    const int i = blockIdx.x * 8 + (threadIdx.x & 7), part = threadIdx.x >> 3;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    if (i < n) {
        int b = part;
        for (; b + 96 < nblk; b += 128) {
            s0 += partials[(size_t)b * n + i];
            s1 += partials[(size_t)(b + 32) * n + i];
            s2 += partials[(size_t)(b + 64) * n + i];
            s3 += partials[(size_t)(b + 96) * n + i];
        }
        for (; b < nblk; b += 32) s0 += partials[(size_t)b * n + i];
    }
    sh[part][threadIdx.x & 7] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (part == 0 && i < n) {
        double t = 0;
        for (int q = 0; q < 32; ++q) t += sh[q][threadIdx.x & 7];
        dw[i] = (float)t;
    }
}

// dx[m] = sum_tap sum_co dy[m - shift(tap)][co] * w[co][tap]; 16 lanes x float4 cover Cout = 64
__global__ __launch_bounds__(256) void conv_c1_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                            float* __restrict__ dx, long M, int H, int W, int Cout) {
    const int tpr = Cout >> 2, rpi = 256 / tpr;
    const int c = (threadIdx.x % tpr) << 2, rsub = threadIdx.x / tpr;
    float wr[4][9];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) wr[j][t] = w[(c + j) * 9 + t];
    const long iters = (M + (long)gridDim.x * rpi - 1) / ((long)gridDim.x * rpi);
    for (long itr = 0; itr < iters; ++itr) {
        const long m = ((long)itr * gridDim.x + blockIdx.x) * rpi + rsub;
        float s = 0.0f;
        if (m < M) {
            const int hw = (int)(m % ((long)H * W));
            const int h = hw / W, ww = hw % W;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                // output pixel m' = m - shift(tap) used x[m] through tap
                const int hh = h - (tap / 3 - 1), w2 = ww - (tap % 3 - 1);
                if (hh >= 0 && hh < H && w2 >= 0 && w2 < W) {
                    const float4 g =
                        *reinterpret_cast<const float4*>(dy + (m - (long)(tap / 3 - 1) * W - (tap % 3 - 1)) * Cout + c);
                    s = fmaf(g.x, wr[0][tap], s); s = fmaf(g.y, wr[1][tap], s);
                    s = fmaf(g.z, wr[2][tap], s); s = fmaf(g.w, wr[3][tap], s);
                }
            }
        }
        // reduce across the tpr lanes that share the pixel (tpr is a power of two <= 64, lane-aligned)
        for (int o = tpr >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (m < M && (threadIdx.x % tpr) == 0) dx[m] = s;
    }
}

constexpr int C1B_GW = 66, C1B_GT = 10;        // LDS ring rows: 64 + 2 halo pixels; G rows: 9 taps + 1 pad
// The W = 64 kernels keep the input rows around the current one in a 4-slot LDS ring, row r in slot (r + 8) & 3.  This stages
// row `row` of image `ximg` with its two halo columns: bn0 affine applied, zero outside the image (threads 0 .. 65).
__device__ __forceinline__ void c1_stage_row(float (*Xs)[C1B_GW], const float* ximg, const float* cs, const float* ct, int H,
                                             int row) {
    constexpr int W = 64;
    const int tid = threadIdx.x;
    if (tid < C1B_GW) {
        const int w = tid - 1;
        float v = 0.0f;
        if ((unsigned)row < (unsigned)H && (unsigned)w < (unsigned)W) {
            v = ximg[(size_t)row * W + w];
            if (cs) v = fmaf(v, cs[w], ct[w]);
        }
        Xs[(row + 8) & 3][tid] = v;
    }
}

// Forward of the Cin = 1 convolution for W = 64, Cout = 64: a workgroup walks down a strip of rows of one image; the
// three input rows of the current output row live in an LDS ring (bn0 affine and zero padding applied once per value),
// every thread produces 4 pixels x 4 couts per row (weights in registers) and stores 16 B per pixel -> the kernel is a
// pure 1 GB write stream.
template <class TS>
__global__ __launch_bounds__(256) void conv_c1_fwd_rows_kernel(const float* __restrict__ x, const float* __restrict__ cs,
                                                               const float* __restrict__ ct, const float* __restrict__ wgt,
                                                               TS* __restrict__ y, float* __restrict__ stats, int H,
                                                               int strips, int rows_per_strip) {
    constexpr int W = 64, Cout = 64;
    __shared__ float Xs[4][C1B_GW];
    const int img = blockIdx.x / strips, strip = blockIdx.x % strips;
    const int r0 = strip * rows_per_strip;
    int r1 = r0 + rows_per_strip;
    if (r1 > H) r1 = H;
    const int tid = threadIdx.x, c = (tid & 15) << 2, grp = tid >> 4;      // 16 pixel groups of 4 pixels
    float wr[4][9];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) wr[j][t] = wgt[(c + j) * 9 + t];
    const float* ximg = x + (size_t)img * H * W;
    // fused BatchNorm statistics (training): every thread keeps, for its 4 couts, a pivot K (its first output) and the
    // shifted sums r = sum(y - K), q = sum((y - K)^2) over its 4 pixels x the rows of the strip; the 16 threads of a pixel
    // group form one partial row [K | r | q] of 64 channels (same layout as the MFMA conv epilogues ->
    // tag_bn_stats_from_partials), so the 1 GB output is never re-read for its statistics.
    float sk[4] = {0, 0, 0, 0}, sr[4] = {0, 0, 0, 0}, sq[4] = {0, 0, 0, 0};
    bool have_pivot = false;
    c1_stage_row(Xs, ximg, cs, ct, H, r0 - 1);
    c1_stage_row(Xs, ximg, cs, ct, H, r0);
    c1_stage_row(Xs, ximg, cs, ct, H, r0 + 1);
    __syncthreads();
    for (int h = r0; h < r1; ++h) {
        if (h + 2 <= r1) c1_stage_row(Xs, ximg, cs, ct, H, h + 2);           // slot (h+2)&3 is not read by row h
        float xin[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 6; ++k) xin[r][k] = Xs[(h + r - 1 + 8) & 3][grp * 4 + k];
        TS* yrow = y + (((size_t)img * H + h) * W + grp * 4) * Cout + c;
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            float o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaf(xin[tap / 3][px + tap % 3], wr[j][tap], o[j]);
            Act<TS>::st4(yrow + (size_t)px * Cout, (f32x4){o[0], o[1], o[2], o[3]});
            if (stats) {
                if (!have_pivot) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) sk[j] = o[j];
                    have_pivot = true;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) { const float d = o[j] - sk[j]; sr[j] += d; sq[j] = fmaf(d, d, sq[j]); }
            }
        }
        __syncthreads();
    }
    if (stats) {
        const int P = gridDim.x * 16, prow = blockIdx.x * 16 + grp;
        float* ps = stats + (size_t)prow * 3 * Cout;
#pragma unroll
        for (int j = 0; j < 4; ++j) { ps[c + j] = sk[j]; ps[Cout + c + j] = sr[j]; ps[2 * Cout + c + j] = sq[j]; }
        if (c == 0) stats[(size_t)P * 3 * Cout + prow] = (float)((r1 - r0) * 4);
    }
}

// Fused backward of the Cin = 1 convolution for W = 64 mel bins, Cout = 64: ONE pass over dy (the 1 GB tensor at
// batch 64) produces both dw (64 x 9) and dx (the gradient of the bn0 output, needed for bn0's weight / bias).
// A workgroup walks down a strip of rows of one image; per row (64 pixels x 64 couts = 16 KB, one float4 per thread
// and 16-pixel quarter) every dy value is read once and feeds
//   wgrad:  dw[co][tap] += xin[h+ky-1][w+kx-1] * dy[h][w][co]             (xin rows in an LDS ring, bn0 affine applied)
//   dgrad:  G[h][w][tap] = sum_co dy[h][w][co] * wgt[co][tap], kept in an LDS ring of 4 rows;
//           dx[h-1][w] = sum_tap G[h-1-(ky-1)][w-(kx-1)][tap] once row h is in
// -- both products on v_mfma_f32_16x16x4_f32 (operand mapping inside the kernel).
// The next row's dy is in flight while the current one is processed; one barrier per row.
// FUSE: `dy` holds da = dL/d relu(bn1(yref)) (the raw dgrad output of block 1's second conv) and the backward of that
// BatchNorm + ReLU is applied as the values arrive -- dy = k0 * (dz - k1 - xhat * k2), dz = da where bn1(yref) > 0, the
// arithmetic of bnrelu_bwd_apply_kernel (bn_pool.hip) -- so the separate apply pass over the largest activation of the
// network (read y, read da, write dy) is replaced by one extra read of y here.
struct C1BnBwd {
    const void* yref; const float* scale; const float* shift; const float* mean; const float* invstd;
    const float* gamma; const float* dgamma; const float* dbeta; float invN; int bn_train;
};
template <class TS, bool FUSE>
__global__ __launch_bounds__(256) void conv_c1_bwd_kernel(const float* __restrict__ x, const float* __restrict__ cs,
                                                          const float* __restrict__ ct, const TS* __restrict__ dy,
                                                          const float* __restrict__ wgt, float* __restrict__ dx,
                                                          double* __restrict__ partials, int H, int strips,
                                                          int rows_per_strip, C1BnBwd bb) {
    constexpr int W = 64, Cout = 64;
    __shared__ float Gs[4][C1B_GW][C1B_GT];
    __shared__ float Xs[4][C1B_GW];
    __shared__ float red[4][16][36];
    const int img = blockIdx.x / strips, strip = blockIdx.x % strips;
    const int r0 = strip * rows_per_strip;
    int r1 = r0 + rows_per_strip;
    if (r1 > H) r1 = H;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int cq = lane & 15, c = cq << 2, psub = lane >> 4;             // channel quad, pixel inside a 4-pixel load
    // Both contractions run on v_mfma_f32_16x16x4_f32 (A[i = lane % 16][k = lane / 16], B[k = lane / 16][j = lane % 16],
    // D[i = 4 (lane / 16) + r][j = lane % 16]); a wave owns 16 pixels of the row.
    //   wgrad  dw[co][tap] += sum_px dy[px][co] * xin[px + shift(tap)]: the loaded layout IS the A operand (row = channel quad cq,
    //          k = pixel psub, one MFMA per item i and channel j); B = the input value under this lane's tap (tap = lane % 16);
    //   dgrad  G[px][tap]   = sum_co dy[px][co] * wgt[co][tap]: the contraction index has to move from lane % 16 to lane / 16, so the
    //          wave's 16 x 64 gradient tile goes through a wave-private LDS tile (68-float rows: conflict-free both ways) and
    //          comes back as A[row = pixel][k = channel], 16 MFMAs against the weights held as B fragments.
    // (The scalar form -- 36 FMAs, 36 DPP adds and 36 masked LDS stores per 4-channel item -- was VALU-bound at 2 x the HBM time.)
    const int tapl = lane & 15, kg = lane >> 4;
    const bool tap_ok = tapl < 9;
    const int tky = tap_ok ? tapl / 3 : 0, tkx = tap_ok ? tapl % 3 : 0;
    float wB[16];                                                        // B fragments of the dgrad product: wgt[kg*16 + step][tap]
#pragma unroll
    for (int q = 0; q < 16; ++q) wB[q] = tap_ok ? wgt[(kg * 16 + q) * 9 + tapl] : 0.0f;
    f32x4 accW[4];                                                       // dw[co = (4 kg + r) * 4 + j][tap = tapl] in accW[j][r]
#pragma unroll
    for (int j = 0; j < 4; ++j) accW[j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    __shared__ __attribute__((aligned(16))) float Ts[4][16][68];
    for (int i = tid; i < 4 * C1B_GW * C1B_GT; i += 256) (&Gs[0][0][0])[i] = 0.0f;      // halo columns stay zero
    const float* ximg = x + (size_t)img * H * W;
    const TS* dimg = dy + (size_t)img * H * W * Cout;
    typedef ActN<TS, 4> AN;
    typedef typename AN::raw_t raw_t;
    constexpr int NY = FUSE ? 4 : 1;
    f32x4 g[4];
    raw_t gn[4], yn[NY];                    // the next row, in flight as loaded (converted / transformed in take())
    // per-channel constants of the fused BatchNorm backward: in LDS and re-read after each row's barrier, so they do not
    // hold 28 registers through the accumulation (3 workgroups per CU stay resident)
    __shared__ float bnc[7][Cout];
    const TS* yimg = nullptr;
    if constexpr (FUSE) {
        yimg = static_cast<const TS*>(bb.yref) + (size_t)img * H * W * Cout;
        if (tid < Cout) {
            const float is = bb.invstd[tid];
            bnc[0][tid] = bb.scale[tid]; bnc[1][tid] = bb.shift[tid]; bnc[2][tid] = bb.mean[tid]; bnc[3][tid] = is;
            bnc[4][tid] = bb.gamma[tid] * is;
            bnc[5][tid] = bb.bn_train ? bb.dbeta[tid] * bb.invN : 0.0f;
            bnc[6][tid] = bb.bn_train ? bb.dgamma[tid] * bb.invN : 0.0f;
        }
    }
    auto load_dy = [&](int row) {
        const bool ok = (unsigned)row < (unsigned)H;
        const size_t off = ((size_t)(ok ? row : 0) * W + wid * 16 + psub) * Cout + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            gn[i] = AN::ldraw(dimg + off + (size_t)i * 4 * Cout);
            if constexpr (FUSE) yn[i] = AN::ldraw(yimg + off + (size_t)i * 4 * Cout);
            else if (!ok) gn[i] = AN::zero();
        }
    };
    auto take = [&](bool ok) {              // g <- the row in flight (FUSE: dy from da and yref; zero outside the image)
        if constexpr (FUSE) {
            float k[7][4];
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(&bnc[q][c]);
                k[q][0] = v.x; k[q][1] = v.y; k[q][2] = v.z; k[q][3] = v.w;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float av[4], vv[4], o[4];
                AN::unpack(gn[i], av);
                AN::unpack(yn[i], vv);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float dz = fmaf(vv[j], k[0][j], k[1][j]) > 0.0f ? av[j] : 0.0f;
                    o[j] = k[4][j] * (dz - k[5][j] - (vv[j] - k[2][j]) * k[3][j] * k[6][j]);
                    if (!ok) o[j] = 0.0f;
                }
                g[i] = (f32x4){o[0], o[1], o[2], o[3]};
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float av[4];
                AN::unpack(gn[i], av);
                g[i] = (f32x4){av[0], av[1], av[2], av[3]};
            }
        }
    };
    c1_stage_row(Xs, ximg, cs, ct, H, r0 - 1);
    c1_stage_row(Xs, ximg, cs, ct, H, r0);
    load_dy(r0 - 1);
    __syncthreads();
    take((unsigned)(r0 - 1) < (unsigned)H);
    for (int h = r0 - 1; h <= r1; ++h) {
        c1_stage_row(Xs, ximg, cs, ct, H, h + 2 > r1 + 1 ? -1 : h + 2);   // rows beyond r1+1 are never read
        if (h < r1) load_dy(h + 1);
        const bool own = h >= r0 && h < r1;
        const int gs = (h + 8) & 3;
        if (own) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float xb = tap_ok ? Xs[(h + tky - 1 + 8) & 3][wid * 16 + i * 4 + psub + tkx] : 0.0f;
                accW[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[i].x, xb, accW[0], 0, 0, 0);
                accW[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[i].y, xb, accW[1], 0, 0, 0);
                accW[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[i].z, xb, accW[2], 0, 0, 0);
                accW[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[i].w, xb, accW[3], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(&Ts[wid][i * 4 + psub][c]) = g[i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");           // the tile is wave-private: no barrier
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        f32x4 accG = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(&Ts[wid][tapl][kg * 16 + 4 * q4]);
            accG = __builtin_amdgcn_mfma_f32_16x16x4f32(v.x, wB[4 * q4 + 0], accG, 0, 0, 0);
            accG = __builtin_amdgcn_mfma_f32_16x16x4f32(v.y, wB[4 * q4 + 1], accG, 0, 0, 0);
            accG = __builtin_amdgcn_mfma_f32_16x16x4f32(v.z, wB[4 * q4 + 2], accG, 0, 0, 0);
            accG = __builtin_amdgcn_mfma_f32_16x16x4f32(v.w, wB[4 * q4 + 3], accG, 0, 0, 0);
        }
        if (tap_ok) {
            float* gp = &Gs[gs][wid * 16 + 4 * kg + 1][tapl];             // G[px = 4 kg + r][tap] in accG[r]
            gp[0] = accG.x; gp[C1B_GT] = accG.y; gp[2 * C1B_GT] = accG.z; gp[3 * C1B_GT] = accG.w;
        }
        __syncthreads();
        const int ho = h - 1;                                             // output row whose three G rows are now present
        if (ho >= r0 && ho < r1 && tid < W) {
            float sdx = 0.0f;
#pragma unroll
            for (int t = 0; t < 9; ++t)                                   // dx[p] = sum_tap G[p - shift(tap)][tap]
                sdx += Gs[(ho - (t / 3 - 1) + 8) & 3][tid + 1 - (t % 3 - 1)][t];
            dx[((size_t)img * H + ho) * W + tid] = sdx;
        }
        if (h < r1) take((unsigned)(h + 1) < (unsigned)H);
    }
    // dw partial of this workgroup: the MFMA has summed the wave's pixels; fold the 4 waves (fixed order), in fp64 across workgroups
    if (tap_ok) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            red[wid][4 * kg + 0][j * 9 + tapl] = accW[j].x;
            red[wid][4 * kg + 1][j * 9 + tapl] = accW[j].y;
            red[wid][4 * kg + 2][j * 9 + tapl] = accW[j].z;
            red[wid][4 * kg + 3][j * 9 + tapl] = accW[j].w;
        }
    }
    __syncthreads();
    for (int e = tid; e < 16 * 36; e += 256) {
        const int q = e / 36, r = e % 36;
        const double sum = ((double)red[0][q][r] + (double)red[1][q][r]) + ((double)red[2][q][r] + (double)red[3][q][r]);
        partials[(size_t)blockIdx.x * Cout * 9 + (q * 4 + r / 9) * 9 + r % 9] = sum;
    }
}

}  // namespace

static void c1_bwd_geom(int B, int H, int* strips, int* rows) {
    int s = 2048 / (B > 0 ? B : 1);
    if (s < 1) s = 1;
    int r = (H + s - 1) / s;
    if (r < 8) r = 8;                       // two halo rows are recomputed per strip
    *rows = r;
    *strips = (H + r - 1) / r;
}
// workgroups of a grid-stride launch: one per `per_block` items, at most 8192
static int c1_blocks(long items, long per_block) {
    const long nb = (items + per_block - 1) / per_block;
    return (int)(nb > 8192 ? 8192 : nb);
}
// the W = 64, Cout = 64 forward, fp32 or bf16 output, with the statistics partials of its output if `stats` is given
template <class TS>
static int c1_fwd_rows_launch(const float* x, const float* col_scale, const float* col_shift, const float* w, TS* y,
                              float* stats, int B, int H, void* stream) {
    int strips, rows;
    c1_bwd_geom(B, H, &strips, &rows);
    hipLaunchKernelGGL(conv_c1_fwd_rows_kernel<TS>, dim3(B * strips), dim3(256), 0, as_stream(stream), x, col_scale, col_shift, w,
                       y, stats, H, strips, rows);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_conv3x3_c1_forward(const float* x, const float* col_scale, const float* col_shift, const float* w,
                                      float* y, int B, int H, int W, int Cout, void* stream) {
    TAG_CHECK_ARG(x && w && y && B > 0 && H > 0 && W > 0 && Cout > 0);      // (Cout > 0 before 256 % (Cout / 4) below)
    TAG_CHECK_ARG(Cout % 4 == 0 && (col_scale == nullptr) == (col_shift == nullptr));
    const long M = (long)B * H * W;
    if (W == 64 && Cout == 64) return c1_fwd_rows_launch<float>(x, col_scale, col_shift, w, y, nullptr, B, H, stream);
    if (W % 4 == 0 && 256 % (Cout / 4) == 0)
        hipLaunchKernelGGL(conv_c1_fwd4_kernel<false>, dim3(c1_blocks((M / 4) * (Cout / 4), 256)), dim3(256), 0,
                           as_stream(stream), x, col_scale, col_shift, w, (const float*)nullptr, y, M, H, W, Cout);
    else
        hipLaunchKernelGGL(conv_c1_fwd_kernel, dim3(c1_blocks(M * (Cout / 4), 256)), dim3(256), 0, as_stream(stream), x,
                           col_scale, col_shift, w, y, M, H, W, Cout);
    TAG_LAUNCH_CHECK();
    return 0;
}

// y = conv(affine(x)) + bias[b, cout] of the Cin = 1 convolution (CrossCDur block 1): W % 4 == 0 and Cout in {4, 8, 16, 32, 64,
// 128, ...} with 256 % (Cout / 4) == 0 (the 4-pixel kernel); anything else is TAG_EINVAL.
extern "C" int tag_conv3x3_c1_forward_bias(const float* x, const float* col_scale, const float* col_shift, const float* w,
                                           const float* bias, float* y, int B, int H, int W, int Cout, void* stream) {
    TAG_CHECK_ARG(x && w && bias && y && B > 0 && H > 0 && (col_scale == nullptr) == (col_shift == nullptr));
    if (!(W > 0 && W % 4 == 0 && Cout >= 4 && Cout % 4 == 0 && 256 % (Cout / 4) == 0)) {
        tag_set_error("%s", "tag_conv3x3_c1_forward_bias: unserved shape (W a multiple of 4, Cout / 4 a divisor of 256)");
        return TAG_EINVAL;
    }
    const long M = (long)B * H * W;
    hipLaunchKernelGGL(conv_c1_fwd4_kernel<true>, dim3(c1_blocks((M / 4) * (Cout / 4), 256)), dim3(256), 0, as_stream(stream), x,
                       col_scale, col_shift, w, bias, y, M, H, W, Cout);
    TAG_LAUNCH_CHECK();
    return 0;
}

// Cin = 1 forward with the BatchNorm statistics of its output fused (W == 64, Cout == 64 only: tag_conv3x3_c1_stats_rows
// > 0); stats = [P][3][Cout] partial rows + [P] counts -> tag_bn_stats_from_partials
extern "C" int tag_conv3x3_c1_stats_rows(int B, int H, int W, int Cout) {
    if (!(W == 64 && Cout == 64 && B > 0 && H > 0)) return 0;
    int strips, rows;
    c1_bwd_geom(B, H, &strips, &rows);
    return B * strips * 16;
}
extern "C" int tag_conv3x3_c1_forward_stats(const float* x, const float* col_scale, const float* col_shift, const float* w,
                                            float* y, float* stats, int B, int H, int W, int Cout, void* stream) {
    TAG_CHECK_ARG(x && w && y && stats && W == 64 && Cout == 64 && B > 0 && H > 0);
    TAG_CHECK_ARG((col_scale == nullptr) == (col_shift == nullptr));
    return c1_fwd_rows_launch<float>(x, col_scale, col_shift, w, y, stats, B, H, stream);
}
// bf16 activation storage (BASELINE configs[2]): y is written as bf16, statistics come from the fp32 values
extern "C" int tag_conv3x3_c1_forward_stats_bf16(const float* x, const float* col_scale, const float* col_shift,
                                                 const float* w, void* y, float* stats, int B, int H, int W, int Cout,
                                                 void* stream) {
    TAG_CHECK_ARG(x && w && y && W == 64 && Cout == 64 && B > 0 && H > 0);
    TAG_CHECK_ARG((col_scale == nullptr) == (col_shift == nullptr));
    return c1_fwd_rows_launch<bf16_t>(x, col_scale, col_shift, w, static_cast<bf16_t*>(y), stats, B, H, stream);
}

extern "C" size_t tag_conv3x3_c1_wgrad_ws_bytes(int B, int H, int W, int Cout) {
    (void)B; (void)H; (void)W;
    return (size_t)1024 * Cout * 9 * sizeof(double);
}

extern "C" int tag_conv3x3_c1_wgrad(const float* x, const float* col_scale, const float* col_shift, const float* dy,
                                    float* dw, int B, int H, int W, int Cout, void* ws, void* stream) {
    TAG_CHECK_ARG(x && dy && dw && ws && B > 0 && H > 0 && W > 0 && Cout > 0);
    TAG_CHECK_ARG(Cout % 4 == 0 && Cout / 4 <= 64 && 64 % (Cout / 4) == 0);
    TAG_CHECK_ARG((col_scale == nullptr) == (col_shift == nullptr));
    const long M = (long)B * H * W;
    const int rpi = 256 / (Cout / 4);
    long nb = (M + (long)rpi * 64 - 1) / ((long)rpi * 64);
    const int nblk = (int)(nb > 1024 ? 1024 : (nb < 1 ? 1 : nb));
    double* partials = static_cast<double*>(ws);
    hipLaunchKernelGGL(W % 4 == 0 ? conv_c1_wgrad_kernel<4> : conv_c1_wgrad_kernel<1>, dim3(nblk), dim3(256),
                       4 * 64 * 36 * sizeof(double), as_stream(stream), x, col_scale, col_shift, dy, partials, M, H, W, Cout);
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(conv_c1_wgrad_finalize_kernel, dim3(cdiv(Cout * 9, 8)), dim3(256), 0, as_stream(stream),
                       partials, nblk, Cout * 9, dw);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_conv3x3_c1_dgrad(const float* dy, const float* w, float* dx, int B, int H, int W, int Cout,
                                    void* stream) {
    TAG_CHECK_ARG(dy && w && dx && B > 0 && H > 0 && W > 0 && Cout > 0);
    TAG_CHECK_ARG(Cout % 4 == 0 && Cout / 4 <= 64 && 64 % (Cout / 4) == 0);
    const long M = (long)B * H * W;
    const int rpi = 256 / (Cout / 4);
    hipLaunchKernelGGL(conv_c1_dgrad_kernel, dim3(c1_blocks(M, rpi)), dim3(256), 0, as_stream(stream), dy, w, dx, M, H, W, Cout);
    TAG_LAUNCH_CHECK();
    return 0;
}

// fused wgrad + dgrad of the Cin = 1 convolution (one pass over dy); W == 64 and Cout == 64 only
extern "C" size_t tag_conv3x3_c1_backward_ws_bytes(int B, int H, int W, int Cout) {
    (void)W;
    int strips, rows;
    c1_bwd_geom(B, H, &strips, &rows);
    return (size_t)B * strips * Cout * 9 * sizeof(double);
}
template <class TS>
static int c1_backward_impl(const float* x, const float* col_scale, const float* col_shift, const TS* dy, const float* w,
                            float* dw, float* dx, int B, int H, int W, int Cout, void* ws, void* stream, const C1BnBwd* bb) {
    TAG_CHECK_ARG(x && dy && w && dw && dx && ws && B > 0 && H > 0);
    TAG_CHECK_ARG(W == 64 && Cout == 64);
    TAG_CHECK_ARG((col_scale == nullptr) == (col_shift == nullptr));
    int strips, rows;
    c1_bwd_geom(B, H, &strips, &rows);
    double* partials = static_cast<double*>(ws);
    if (bb) {
        TAG_CHECK_ARG(bb->yref && bb->scale && bb->shift && bb->mean && bb->invstd && bb->gamma && bb->dgamma && bb->dbeta);
        hipLaunchKernelGGL((conv_c1_bwd_kernel<TS, true>), dim3(B * strips), dim3(256), 0, as_stream(stream), x, col_scale,
                           col_shift, dy, w, dx, partials, H, strips, rows, *bb);
    } else {
        hipLaunchKernelGGL((conv_c1_bwd_kernel<TS, false>), dim3(B * strips), dim3(256), 0, as_stream(stream), x, col_scale,
                           col_shift, dy, w, dx, partials, H, strips, rows, C1BnBwd{});
    }
    TAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(conv_c1_wgrad_finalize_kernel, dim3(cdiv(Cout * 9, 8)), dim3(256), 0, as_stream(stream),
                       partials, B * strips, Cout * 9, dw);
    TAG_LAUNCH_CHECK();
    return 0;
}
extern "C" int tag_conv3x3_c1_backward(const float* x, const float* col_scale, const float* col_shift, const float* dy,
                                       const float* w, float* dw, float* dx, int B, int H, int W, int Cout, void* ws,
                                       void* stream) {
    return c1_backward_impl<float>(x, col_scale, col_shift, dy, w, dw, dx, B, H, W, Cout, ws, stream, nullptr);
}
extern "C" int tag_conv3x3_c1_backward_bf16(const float* x, const float* col_scale, const float* col_shift, const void* dy,
                                            const float* w, float* dw, float* dx, int B, int H, int W, int Cout, void* ws,
                                            void* stream) {
    return c1_backward_impl<bf16_t>(x, col_scale, col_shift, static_cast<const bf16_t*>(dy), w, dw, dx, B, H, W, Cout, ws,
                                    stream, nullptr);
}
// the same pass with the backward of relu(bn(yref)) applied to `da` on the fly (C1BnBwd above): dgamma / dbeta hold
// sum(dz * xhat) / sum(dz) over all B*H*W rows, as tag_bn_grad_from_partials leaves them
static C1BnBwd c1_bn_bwd(const void* yref, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                         const float* bn_invstd, const float* gamma, const float* dgamma, const float* dbeta, int bn_train,
                         int B, int H, int W) {
    return C1BnBwd{yref, bn_scale, bn_shift, bn_mean, bn_invstd, gamma, dgamma, dbeta, 1.0f / (float)((long)B * H * W), bn_train};
}
extern "C" int tag_conv3x3_c1_backward_bnrelu(const float* x, const float* col_scale, const float* col_shift, const float* da,
                                              const float* yref, const float* bn_scale, const float* bn_shift,
                                              const float* bn_mean, const float* bn_invstd, const float* gamma,
                                              const float* dgamma, const float* dbeta, int bn_train, const float* w,
                                              float* dw, float* dx, int B, int H, int W, int Cout, void* ws, void* stream) {
    const C1BnBwd bb = c1_bn_bwd(yref, bn_scale, bn_shift, bn_mean, bn_invstd, gamma, dgamma, dbeta, bn_train, B, H, W);
    return c1_backward_impl<float>(x, col_scale, col_shift, da, w, dw, dx, B, H, W, Cout, ws, stream, &bb);
}
extern "C" int tag_conv3x3_c1_backward_bnrelu_bf16(const float* x, const float* col_scale, const float* col_shift,
                                                   const void* da, const void* yref, const float* bn_scale,
                                                   const float* bn_shift, const float* bn_mean, const float* bn_invstd,
                                                   const float* gamma, const float* dgamma, const float* dbeta, int bn_train,
                                                   const float* w, float* dw, float* dx, int B, int H, int W, int Cout,
                                                   void* ws, void* stream) {
    const C1BnBwd bb = c1_bn_bwd(yref, bn_scale, bn_shift, bn_mean, bn_invstd, gamma, dgamma, dbeta, bn_train, B, H, W);
    return c1_backward_impl<bf16_t>(x, col_scale, col_shift, static_cast<const bf16_t*>(da), w, dw, dx, B, H, W, Cout, ws,
                                    stream, &bb);
}
