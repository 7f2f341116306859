// Training-time augmentation of the bn0 output: SpecAugment (torchlibrosa augmentation.py DropStripes / SpecAugmentation,
// applied at models/audio_encoder.py:192-195) and mixup (utils/train_util.py:73-88 do_mixup, applied at :197-200).
//
// Both kernels are pure streaming passes over (B, F, NM) fp32 (frames x mel bins, mel bins innermost): one float4 of one
// row per lane and grid-stride, so a wave reads 1 KiB contiguous.  The stripe table (B, n_time + n_freq, 2) int32 [bgn, width]
// is read per clip by every lane of the clip (a few cached dwords); its values are only compared against the element's
// coordinates, never used to form an address, so a table outside the image masks nothing out of bounds.
#include "tag_common.h"

namespace {

constexpr int AUG_MAX_STRIPES = 8;       // per dropper (torchlibrosa's stripes_num; the reference uses 2)
constexpr int AUG_MAX_BLOCKS = 2048;

struct ClipMask {
    bool time;                           // the whole row (frame f) is inside a time stripe of this clip
    bool freq[4];                        // mel bins c .. c+3 inside a frequency stripe
};

__device__ __forceinline__ bool in_stripe(int i, const int* s) { return (unsigned)(i - s[0]) < (unsigned)s[1]; }

__device__ __forceinline__ ClipMask clip_mask(const int* __restrict__ stripes, int nt, int nf, int b, int f, int c) {
    ClipMask m = {false, {false, false, false, false}};
    if (!stripes) return m;
    const int* s = stripes + (size_t)b * (nt + nf) * 2;
    for (int k = 0; k < nt; ++k) m.time |= in_stripe(f, s + 2 * k);
    for (int k = nt; k < nt + nf; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) m.freq[j] |= in_stripe(c + j, s + 2 * k);
    return m;
}

// one clip's 4 values: bn0 affine exactly as the Cin = 1 convolutions form it on load (conv_c1.hip c1_in: fmaf(v, cs[w], ct[w])),
// then the stripes' zeros
__device__ __forceinline__ f32x4 bn0_masked(const float* __restrict__ lm, const float* __restrict__ cs,
                                            const float* __restrict__ ct, const int* __restrict__ stripes, int nt, int nf,
                                            int b, int f, int c, int F, int NM) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(lm + ((size_t)b * F + f) * NM + c);
    float v[4] = {x.x, x.y, x.z, x.w};
    const ClipMask m = clip_mask(stripes, nt, nf, b, f, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (cs) v[j] = fmaf(v[j], cs[c + j], ct[c + j]);
        v[j] = (m.time || m.freq[j]) ? 0.0f : v[j];
    }
    return (f32x4){v[0], v[1], v[2], v[3]};
}

// x0 (Bo, F, NM): Bo = B, or B / 2 with lam (x0[k] = x[2k] * lam[2k] + x[2k+1] * lam[2k+1], two products then one add)
__global__ __launch_bounds__(256) void augment_fwd_kernel(const float* __restrict__ lm, const float* __restrict__ cs,
                                                          const float* __restrict__ ct, const int* __restrict__ stripes,
                                                          int nt, int nf, const float* __restrict__ lam,
                                                          float* __restrict__ x0, int Bo, int F, int NM) {
    const int q = NM >> 2;
    const long total = (long)Bo * F * q;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % q) << 2;
        const long row = i / q;
        const int f = (int)(row % F);
        const int bo = (int)(row / F);
        f32x4 out;
        if (lam) {
            const f32x4 a = bn0_masked(lm, cs, ct, stripes, nt, nf, 2 * bo, f, c, F, NM);
            const f32x4 b = bn0_masked(lm, cs, ct, stripes, nt, nf, 2 * bo + 1, f, c, F, NM);
            const float l0 = lam[2 * bo], l1 = lam[2 * bo + 1];
            out = a * l0 + b * l1;                    // -ffp-contract=off: no fused multiply-add
        } else {
            out = bn0_masked(lm, cs, ct, stripes, nt, nf, bo, f, c, F, NM);
        }
        *reinterpret_cast<f32x4*>(x0 + (size_t)row * NM + c) = out;
    }
}

// dbn0 (B, F, NM) = mask[b] * lam[b] * dx0[b / 2]   (dx0[b] without lam); masked elements exactly 0
__global__ __launch_bounds__(256) void augment_bwd_kernel(const float* __restrict__ dx0, const int* __restrict__ stripes,
                                                          int nt, int nf, const float* __restrict__ lam,
                                                          float* __restrict__ dbn0, int B, int F, int NM) {
    const int q = NM >> 2;
    const long total = (long)B * F * q;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % q) << 2;
        const long row = i / q;
        const int f = (int)(row % F);
        const int b = (int)(row / F);
        const int bs = lam ? (b >> 1) : b;
        f32x4 g = *reinterpret_cast<const f32x4*>(dx0 + ((size_t)bs * F + f) * NM + c);
        if (lam) g = g * lam[b];
        const ClipMask m = clip_mask(stripes, nt, nf, b, f, c);
        float v[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (m.time || m.freq[j]) ? 0.0f : v[j];
        *reinterpret_cast<f32x4*>(dbn0 + (size_t)row * NM + c) = (f32x4){v[0], v[1], v[2], v[3]};
    }
}

int aug_blocks(long vec4s) { return (int)(vec4s / 256 + 1 < AUG_MAX_BLOCKS ? vec4s / 256 + 1 : AUG_MAX_BLOCKS); }

}  // namespace

extern "C" int tag_augment_forward(const float* lm, const float* scale, const float* shift, const int* stripes, int n_time,
                                   int n_freq, const float* lam, float* x0, int B, int F, int NM, void* stream) {
    TAG_CHECK_ARG(lm && x0 && B > 0 && F > 0 && NM >= 4 && NM % 4 == 0);
    TAG_CHECK_ARG((scale == nullptr) == (shift == nullptr));
    TAG_CHECK_ARG(n_time >= 0 && n_freq >= 0 && n_time <= AUG_MAX_STRIPES && n_freq <= AUG_MAX_STRIPES);
    TAG_CHECK_ARG(stripes != nullptr || (n_time == 0 && n_freq == 0));
    TAG_CHECK_ARG(lam == nullptr || B % 2 == 0);
    TAG_CHECK_ARG(x0 != lm);
    const int Bo = lam ? B / 2 : B;
    hipLaunchKernelGGL(augment_fwd_kernel, dim3(aug_blocks((long)Bo * F * (NM / 4))), dim3(256), 0, as_stream(stream), lm,
                       scale, shift, stripes, n_time, n_freq, lam, x0, Bo, F, NM);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_augment_backward(const float* dx0, const int* stripes, int n_time, int n_freq, const float* lam,
                                    float* dbn0, int B, int F, int NM, void* stream) {
    TAG_CHECK_ARG(dx0 && dbn0 && B > 0 && F > 0 && NM >= 4 && NM % 4 == 0);
    TAG_CHECK_ARG(n_time >= 0 && n_freq >= 0 && n_time <= AUG_MAX_STRIPES && n_freq <= AUG_MAX_STRIPES);
    TAG_CHECK_ARG(stripes != nullptr || (n_time == 0 && n_freq == 0));
    TAG_CHECK_ARG(lam == nullptr || B % 2 == 0);
    TAG_CHECK_ARG(dbn0 != dx0);
    hipLaunchKernelGGL(augment_bwd_kernel, dim3(aug_blocks((long)B * F * (NM / 4))), dim3(256), 0, as_stream(stream), dx0,
                       stripes, n_time, n_freq, lam, dbn0, B, F, NM);
    TAG_LAUNCH_CHECK();
    return 0;
}
