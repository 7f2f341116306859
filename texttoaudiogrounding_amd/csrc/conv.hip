// A1: 3x3 / stride 1 / pad 1 / no-bias convolution (models/panns.py:25-33,49-50), channels-last,
// forward + dgrad (one kernel, different weight pack) and wgrad, as implicit GEMMs on the exact-fp32
// MFMA v_mfma_f32_32x32x2_f32 (157 TFLOP/s peak on gfx950; bit-equal to an fmaf chain).
//
// forward / dgrad   M = B*H*W pixels, N = Cout, K = 9*Cin.  128 x {128,64} tile per 256-thread
//   workgroup (4 waves, each 64x64 or 64x32 of 32x32 MFMA tiles), K walked tap-major in chunks of
//   32 channels, operands staged through LDS k-major (As[k][m], Bs[k][n]) so that every MFMA
//   operand read is a conflict-free 32-lane row; double-buffered, one barrier per K chunk, the
//   global loads of chunk i+1 are in flight while chunk i is on the matrix pipe.  The producing
//   layer's BatchNorm + ReLU is applied to the A operand in registers on its way to LDS, so the
//   normalised activation never round-trips through HBM.
// wgrad             M = Cin, N = Cout, K = pixels (x9 taps), split over the pixel axis; partials
//   are reduced in a fixed order by a second kernel that also writes the reference's
//   (Cout,Cin,3,3) layout.
#include <stdlib.h>
#include "tag_common.h"

// TAG_ABLATE (tools/ablate_conv.py builds private copies with -DTAG_ABLATE=n; the product is built with 0):
//   1 no global loads after chunk 0 | 2 no LDS stores after chunk 0 | 4 no barrier | 8 no MFMA | 16 setprio(1) in the MFMA phase
//   32 odd workgroups run at priority 1 throughout
#ifndef TAG_ABLATE
#define TAG_ABLATE 0
#endif
// LDS chunk buffers of the MFMA conv kernels: 2 = double buffered (one barrier per chunk, 2 workgroups/CU),
// 1 = single buffered (two barriers per chunk, ~37 KB -> 3 workgroups/CU; the next chunk waits in registers).
// Measured on MI355X: 1 buffer + 3 workgroups/CU is 4-7 % faster (more waves to cover load latency).
#ifndef TAG_NBUF
#define TAG_NBUF 1
#endif

namespace {

constexpr int BM = 128;
constexpr int BK = 32;
constexpr int LDA = BM + 1;   // (4q+j)*LDA + p hits 32 distinct banks for the transposing A store

__device__ __forceinline__ f32x4 ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__device__ __forceinline__ f32x4 apply_prologue(f32x4 v, int mode, f32x4 s, f32x4 t) {
    if (mode == 1) {
        v.x = fmaxf(fmaf(v.x, s.x, t.x), 0.0f); v.y = fmaxf(fmaf(v.y, s.y, t.y), 0.0f);
        v.z = fmaxf(fmaf(v.z, s.z, t.z), 0.0f); v.w = fmaxf(fmaf(v.w, s.w, t.w), 0.0f);
    } else if (mode == 2) {
        v.x = fmaf(v.x > 0 ? v.x : 0.1f * v.x, s.x, t.x); v.y = fmaf(v.y > 0 ? v.y : 0.1f * v.y, s.y, t.y);
        v.z = fmaf(v.z > 0 ? v.z : 0.1f * v.z, s.z, t.z); v.w = fmaf(v.w > 0 ? v.w : 0.1f * v.w, s.w, t.w);
    } else if (mode == 3) {
        v.x = fmaf(v.x, s.x, t.x); v.y = fmaf(v.y, s.y, t.y); v.z = fmaf(v.z, s.z, t.z); v.w = fmaf(v.w, s.w, t.w);
    }
    return v;
}

// register image of one K chunk (32 channels of one tap) on its way from HBM to LDS
template <int B_LOADS>
struct FwdStage {
    f32x4 ra[4], rb[B_LOADS];
    unsigned ok;
    int c0;
};

template <int BN_, int PRO>
__global__ __launch_bounds__(256, TAG_NBUF == 2 ? 2 : 3) void conv3x3_fwd_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ wp,
                                                             const float* __restrict__ in_scale,
                                                             const float* __restrict__ in_shift,
                                                             float* __restrict__ y, int B, int H, int W, int Cin,
                                                             int Cout) {
    constexpr int TN = BN_ / 64;            // 32-wide n tiles per wave (waves 2 x 2, wave tile 64 x BN_/2)
    constexpr int B_LOADS = BN_ / 32;       // float4 per thread for the B chunk
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                        // [NBUF][BK][LDA]
    float* Bs = smem + TAG_NBUF * BK * LDA;  // [NBUF][BK][BN_]   (BK*LDA*4 bytes is a multiple of 16)
    float* Ss = Bs + TAG_NBUF * BK * BN_;    // [Cin] producer BN scale, then [Cin] shift (PRO != 0)

    const long M = (long)B * H * W;
    const int n_tiles = (Cout + BN_ - 1) / BN_;
    const int m_tiles = (int)((M + BM - 1) / BM);
    const int L = xcd_remap(blockIdx.x, m_tiles * n_tiles);
    const int n0 = (L % n_tiles) * BN_;
    const long m0 = (long)(L / n_tiles) * BM;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm0 = (wid >> 1) * 64, wn0 = (wid & 1) * (BN_ / 2);

    if (PRO != 0)
        for (int c = tid; c < Cin; c += 256) { Ss[c] = in_scale[c]; Ss[Cin + c] = in_shift[c]; }

    // ---- staging geometry, fixed for the whole tile: 4 pixels x one channel quad per thread (A), B_LOADS
    //      float4 of the weight chunk (B).  Per chunk only wave-uniform offsets change.  Byte offsets are
    //      32-bit (every tensor of the path is < 4 GiB; checked by the launcher).
    const int q = tid & 7;                   // channel quad within the 32-channel chunk
    unsigned aoffb[4];                       // byte offset of (pixel, channel quad) in x
    unsigned tapok[4];                       // bit t set <=> tap t of this pixel lies inside the image
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = (tid >> 3) + 32 * i;
        const long m = m0 + p;
        const bool v = m < M;
        const long mm = v ? m : 0;
        const int hw = (int)(mm % ((long)H * W));
        const int h = hw / W, w = hw % W;
        unsigned mask = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int hh = h + t / 3 - 1, ww = w + t % 3 - 1;
            mask |= (unsigned)(v & ((unsigned)hh < (unsigned)H) & ((unsigned)ww < (unsigned)W)) << t;
        }
        tapok[i] = mask;
        aoffb[i] = (unsigned)((mm * Cin + q * 4) * 4);
    }
    unsigned boffb[B_LOADS];
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
        const int idx = tid + 256 * i;
        const int k = idx / (BN_ / 4), n4 = idx % (BN_ / 4);
        int n = n0 + n4 * 4;
        n = n < Cout ? n : 0;                // (columns >= Cout are computed on garbage and never stored)
        boffb[i] = (unsigned)((k * Cout + n) * 4);
    }
    const int cchunks = Cin / BK;
    const int kiters = 9 * cchunks;

    // Loads are branch-free: an out-of-image tap reads the (valid) centre pixel instead and is zeroed when the
    // chunk is written to LDS; the producer's BN+ReLU prologue is applied there too, so the global loads of
    // chunk i+1 stay in flight across the whole MFMA phase of chunk i.
    auto issue_chunk = [&](FwdStage<B_LOADS>& st, int it) {
        const int tap = it / cchunks, c0 = (it - tap * cchunks) * BK;
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const int aoff = ((dy * W + dx) * Cin + c0) * 4;   // wave-uniform byte offsets
        const int coff = c0 * 4;
        st.ok = 0;
        st.c0 = c0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned ok = (tapok[i] >> tap) & 1u;
            st.ok |= ok << i;
            const unsigned off = aoffb[i] + (unsigned)(ok ? aoff : coff);   // 32-bit wrap-around sum (aoff < 0)
            st.ra[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(x) + off);
        }
        const float* wchunk = wp + ((size_t)tap * Cin + c0) * Cout;   // wave-uniform
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i)
            st.rb[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(wchunk) + boffb[i]);
    };
    auto store_chunk = [&](const FwdStage<B_LOADS>& st, int buf) {
        float* a = As + buf * BK * LDA;
        f32x4 rs = {1.0f, 1.0f, 1.0f, 1.0f}, rt = {0.0f, 0.0f, 0.0f, 0.0f};
        if (PRO != 0) {
            rs = *reinterpret_cast<const f32x4*>(Ss + st.c0 + q * 4);
            rt = *reinterpret_cast<const f32x4*>(Ss + Cin + st.c0 + q * 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = (tid >> 3) + 32 * i;
            f32x4 v = apply_prologue(st.ra[i], PRO, rs, rt);
            if (!((st.ok >> i) & 1u)) v = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            a[(q * 4 + 0) * LDA + p] = v.x;
            a[(q * 4 + 1) * LDA + p] = v.y;
            a[(q * 4 + 2) * LDA + p] = v.z;
            a[(q * 4 + 3) * LDA + p] = v.w;
        }
        float* b = Bs + buf * BK * BN_;
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            const int idx = tid + 256 * i;
            const int k = idx / (BN_ / 4), n4 = idx % (BN_ / 4);
            *reinterpret_cast<f32x4*>(b + k * BN_ + n4 * 4) = st.rb[i];
        }
    };

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int kl = lane >> 5, ml = lane & 31;
    // MFMA phase of one chunk; operand fragments are read PF k-steps ahead of their use
    auto mma_chunk = [&](int buf) {
        const float* a = As + buf * BK * LDA + kl * LDA + wm0 + ml;
        const float* b = Bs + buf * BK * BN_ + kl * BN_ + wn0 + ml;
        constexpr int PF = 2, NS = BK / 2;
        float af[PF + 1][2], bf[PF + 1][TN];
#pragma unroll
        for (int s0 = 0; s0 < PF; ++s0) {
#pragma unroll
            for (int i = 0; i < 2; ++i) af[s0][i] = a[(2 * s0) * LDA + i * 32];
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[s0][j] = b[(2 * s0) * BN_ + j * 32];
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
#pragma unroll
        for (int ks = 0; ks < NS; ++ks) {
            const int cur = ks % (PF + 1), nxt = (ks + PF) % (PF + 1);
            if (ks + PF < NS) {
#pragma unroll
                for (int i = 0; i < 2; ++i) af[nxt][i] = a[(2 * (ks + PF)) * LDA + i * 32];
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[nxt][j] = b[(2 * (ks + PF)) * BN_ + j * 32];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (TAG_ABLATE & 8) acc[i][j][0] += af[cur][i] * bf[cur][j];
                    else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);
                }
            // pin the software pipeline: the reads of step ks+PF issue ahead of the MFMAs of step ks
            if (ks + PF < NS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * TN, 0);
        }
    };

    FwdStage<B_LOADS> s0;
    issue_chunk(s0, 0);
    __syncthreads();                          // Ss (scale/shift table) visible
    store_chunk(s0, 0);
    __syncthreads();
    for (int it = 0; it < kiters; ++it) {
        const int buf = TAG_NBUF == 2 ? (it & 1) : 0;
        if (it + 1 < kiters && !(TAG_ABLATE & 1)) issue_chunk(s0, it + 1);
        __builtin_amdgcn_sched_barrier(0);
        mma_chunk(buf);
        // nothing that consumes the in-flight global loads may be hoisted into the MFMA phase
        __builtin_amdgcn_sched_barrier(0);
        if (TAG_NBUF == 1) __syncthreads();       // every wave is done reading the single buffer
        if (it + 1 < kiters && !(TAG_ABLATE & 2)) store_chunk(s0, TAG_NBUF == 2 ? (buf ^ 1) : 0);
        if (!(TAG_ABLATE & 4)) __syncthreads();
    }

    // ---- epilogue: C/D layout col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5) ----
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn0 + j * 32 + ml;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
                if (m < M && n < Cout) y[m * Cout + n] = acc[i][j][r];
            }
        }
}

// ------------------------------------------------------------------------------------------
// Halo-tile forward / dgrad kernel (images whose width is 8, 16, 32 or 64 -- every Cnn8Rnn / CrnnEncoder layer).
// The 128 output pixels of a workgroup form a TH x TW rectangle of ONE image (TW = W, or W / 2 for the 64-wide images); for each 32-channel chunk the
// (TH+2) x (TW+2) input patch is staged ONCE in LDS (BN+ReLU prologue and zero padding applied there) and all 9 taps
// read it at a shifted base -- 4-7x fewer global loads and LDS stores than the tap-by-tap kernel above, no per-tap masks.
//
// Round 4 form (tools/coissue_probe.hip, tools/run_halo_prof.sh):
//  * beside another wave's fp32 MFMA stream on the same SIMD a ds_write_b32 issues once per ~1250-5000 clocks (12-26 on an idle
//    SIMD) while ds_write_b64 / b128, every LDS read, VALU work and global loads are unaffected.  The patch used to be stored
//    k-major with 24 ds_write_b32 per thread and chunk (5800 clocks per chunk in the phase clocks): it is now PIXEL-major,
//    36 floats per patch pixel (row stride = 4 banks mod 32: the 16-byte pieces of 8 consecutive pixels cover the 32 banks),
//    written with 6 ds_write_b128 per thread.
//  * an A fragment is one ds_read_b128 per lane = 4 consecutive channels, i.e. the A operands of FOUR k-steps: k-step j of
//    channel group g (8 channels) multiplies channel 8g + 4 kl + j (kl = lane / 32), the B rows follow the same order.
//    MFMA row -> pixel goes through halo_row_to_pix so that the ds_read_b128 lane groups read 16 consecutive pixels.
//  * the 32 x BN_ weight chunk of a (chunk, tap) step is staged per HALF tap (16 channels) in two LDS buffers of half the size:
//    the half after the next one is requested from L2 at the start of a half, the next half is written to the other buffer in
//    the middle of the current half's MFMA stream, one barrier ends each half.  Same LDS and barrier count as the single
//    buffer (free / full) it replaces, but no store phase between two barriers in which the wave issues no MFMA
//    (127.7 -> 131.1 TFLOP/s forward, 131.2 -> 133.8 dgrad over the layer shapes at B = 64).
//  * scalar instructions (and dword stores) of a wave WITHOUT an MFMA stream of its own wait for the co-resident waves' fp32 MFMA
//    streams to pause (a new workgroup's set-up took 1.5 us on an idle chip, 9 us beside running ones: tools/halo_wg_timeline.py):
//    loop state is carried incrementally, the set-up uses host-made multiply-shift pairs and sign-bit validity arithmetic, the
//    output leaves as 16-byte stores after a 4 x 4 DPP transpose inside each lane quad.
//  * 64-wide images run as TWO tile columns of 4 x 32 pixels (204- instead of 264-pixel patch: four 64-cout workgroups per CU).
//  * measured and dropped on the way: weight operands straight from L2 into registers, whole-tap weight
//    stages at 2 workgroups per CU, 16-channel chunks with a double-buffered patch, a cout-major weight image read with
//    ds_read_b128, several tiles per workgroup (two forms), 256-pixel tiles for the 64-channel layers.
// ------------------------------------------------------------------------------------------
// -DTAG_HALO_PROF (tools/run_halo_prof.sh, never in the product build): s_memtime deltas of the phases of ONE workgroup's wave 0
#ifdef TAG_HALO_PROF
__device__ unsigned long long tag_halo_prof[8];
__device__ unsigned long long tag_halo_sub[4];        // (written by every workgroup: the last writer wins -- a sample)
__device__ unsigned long long tag_halo_wg[4 * 65536];   // [start of the pipeline | end | XCC/SE/CU id | first instruction] of every workgroup (s_memrealtime, 100 MHz)
#define HP_MARK(i) { const unsigned long long p1_ = __builtin_amdgcn_s_memtime(); hpc[i] += p1_ - hp0; hp0 = p1_; }
#else
#define HP_MARK(i)
#endif
// channels of a weight stage (one barrier per stage): 16 = half a tap (3 workgroups per CU), 32 = a whole tap in two 16 KB buffers
// (128 couts: 62 KB of LDS, 2 workgroups per CU, half the barriers).  The synthetic loop of tools/mfma_ubench.hip gains 2.5 % from
// the rarer barrier (147.8 vs 144.2 TFLOP/s); the kernel does not: 128.6 / 132.1 (32) vs 130.3 / 132.4 TFLOP/s (16), forward / dgrad
// over the seven layer shapes -- the third workgroup per CU is worth more.
#ifndef TAG_HALO_STAGE128
#define TAG_HALO_STAGE128 16
#endif
// -DTAG_HALO_VALU_PROBE=n (tools/run_valu_probe.sh, never in the product build): n dummy v_pk_fma_f32 per k-step beside the MFMAs --
// does packed-fp32 VALU work issue for free in the shadow of the fp32 MFMA stream of the REAL kernel (tools/dual_issue_probe.hip
// says the two pipes run concurrently on register operands)?
#ifndef TAG_HALO_VALU_PROBE
#define TAG_HALO_VALU_PROBE 0
#endif
template <int BN_> constexpr int halo_stage() { return 16; }
template <int TW>
struct HaloGeom {
    static constexpr int TH = 128 / TW, PW = TW + 2, PH = TH + 2, PP = PH * PW;
    static constexpr int AROW = 36;                               // floats per patch pixel in LDS (32 channels + 4 pad)
    static constexpr int ASZ = (PP + 1) * AROW;                   // + one scratch pixel: the staging items past the patch land there
    static constexpr int ITEMS = (PP * 8 + 255) / 256;            // float4 per thread per patch chunk
};
// n / d by the host's magic pair (mul, shift) of d (n < 2^31): three scalar instructions instead of a runtime division's ~25 --
// scalar instructions wait for gaps in the co-resident waves' MFMA streams, and a new workgroup's ~190 of them took ~9 us
__device__ __forceinline__ unsigned halo_fdiv(unsigned n, unsigned mul, unsigned shr) { return (__umulhi(n, mul) + n) >> shr; }
// MFMA row i (0..31) -> pixel inside the 32-pixel block: the ds_read_b128 lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31}
// read pixels 0..15 / 16..31 (quad map [0,4,5,1,6,2,3,7], the same as the bf16 kernels of conv_x3.hip)
__device__ __forceinline__ int halo_row_to_pix(int i) {
    return (int)((0xED6360u >> (3 * (i >> 2))) & 7u) * 4 + (i & 3);
}

// Epilogue operands of the dgrad launches (EPI == 1): the tensor whose BatchNorm+ReLU the gradient flows into next.
struct BnBwdEpi {
    const float* yref;      // (B,H,W,Cout) raw conv output saved by the forward pass (= BatchNorm input)
    const float* scale;     // gamma * invstd
    const float* shift;     // beta - mean * gamma * invstd
    const float* mean;
    const float* invstd;
    // EPI == 2 only: the gradient flows into relu(bn(yref)) -> ph x 2 pool -> dropout; yref is the UNPOOLED (B,Hf,Wf,Cout) tensor
    int Hf, Wf, ph;
    float wavg, wmax;       // pool_type: 'avg+max' (1/(ph*2), 1) | 'avg' (1/(ph*2), 0) | 'max' (0, 1)
    float drop_p;
    unsigned long long seed;
    int kind;               // 1 | 2 | 3 = the EPI instance to launch (host side only)
};
// EPI == 4 (the early-fusion CrossCDur, models/audio_text_model.py:461-479): y = conv(prologue(x)) + bias[img, cout] -- the text
// enters on the RAW conv output, so it is one add on the quad-transposed registers in front of the store and no pass of its own.
// `yref` carries the (B, Cout) bias table (the struct's other fields are unused); a workgroup's tile lies inside ONE image, so the
// table row is wave-uniform.  Forward launches only (launch_halo_bias), no statistics.

template <int BN_, int PRO, int TW, int EPI = 0>
__global__ __launch_bounds__(256, BN_ == 64 ? 4 : (BN_ == 256 ? 2 : 3)) void conv3x3_halo_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                              const float* __restrict__ in_scale,
                                                              const float* __restrict__ in_shift, float* __restrict__ y,
                                                              float* __restrict__ stats, BnBwdEpi epi, int B, int H, int W,
                                                              int Cin, int Cout, unsigned nt_mul, unsigned nt_shr,
                                                              unsigned rt_mul, unsigned rt_shr, int col_tiles) {
#ifdef TAG_HALO_PROF
    const unsigned long long hrt_first = __builtin_amdgcn_s_memrealtime();
#endif
    using G = HaloGeom<TW>;
    constexpr int ST = halo_stage<BN_>(), NSTG = 32 / ST;       // channels per weight stage, stages per tap
    constexpr int TN = BN_ / 64, BH_LOADS = ST * BN_ / 1024;     // float4 per thread per stage (ST x BN_ floats)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                          // [PP][AROW] patch, pixel-major
    float* Bs = smem + G::ASZ;                 // [2][ST][BN_] weight stages
    float* Ss = Bs + 2 * ST * BN_;             // [2][Cin] producer BN scale / shift

    const int n_tiles = (Cout + BN_ - 1) / BN_;
    // W == col_tiles * TW: one tile column, or two for the 64-wide images (a 4 x 32 rectangle has a 204-pixel patch where the
    // 2 x 64 one has 264: 38 instead of 47 KB of LDS, i.e. FOUR workgroups of the 64-cout tiles per CU)
    const int row_tiles = ((H + G::TH - 1) / G::TH) * col_tiles; // (row tile, column tile) pairs per image, column tiles fastest
    const int m_tiles = B * row_tiles;
    const int L = xcd_remap(blockIdx.x, m_tiles * n_tiles);
    const int mt = (int)halo_fdiv((unsigned)L, nt_mul, nt_shr);                  // L / n_tiles
    const int n0 = (L - mt * n_tiles) * BN_;
    const int img = (int)halo_fdiv((unsigned)mt, rt_mul, rt_shr);                // mt / row_tiles
    const int rc = mt - img * row_tiles;                         // col_tiles is 1 or 2
    const int h0 = (col_tiles == 2 ? rc >> 1 : rc) * G::TH, w0 = (col_tiles == 2 ? rc & 1 : 0) * TW;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm0 = (wid >> 1) * 64, wn0 = (wid & 1) * (BN_ / 2);
    const int kl = lane >> 5, ml = lane & 31;
    // 128-bit LDS writes: beside the fp32 MFMA streams of the two resident workgroups a ds_write_b32 waits 1250-5000 clocks for a gap
    // (tools/coissue_probe.hip); the one-float-per-thread form of this table fill held every new workgroup for ~8.7 us (halo_wg_timeline)
    if (PRO != 0 && tid < Cin / 4) {                             // Cin <= 512 (host check): one item per thread
        *reinterpret_cast<f32x4*>(Ss + 4 * tid) = ldg4(in_scale + 4 * tid);
        *reinterpret_cast<f32x4*>(Ss + Cin + 4 * tid) = ldg4(in_shift + 4 * tid);
    }

    // ---- patch staging geometry (loop invariant): item = (patch pixel, channel quad) ----
    const int q = tid & 7;
    unsigned poff[G::ITEMS];                   // byte offset of the item in x (clamped to a valid pixel)
    unsigned pvalid = 0;                       // bit i: the pixel lies inside the image
    // (sign-bit arithmetic instead of comparisons: vector compares and their && are combined in SCALAR mask registers)
#pragma unroll
    for (int i = 0; i < G::ITEMS; ++i) {
        const int idx = tid + 256 * i;
        const int pp = idx >> 3;
        const int pr = pp / G::PW, pc = pp - pr * G::PW;
        const unsigned uh = (unsigned)(h0 - 1 + pr), uw = (unsigned)(w0 + pc - 1);
        const unsigned okh = ((uh - (unsigned)H) >> 31) & (~uh >> 31);          // 0 <= h < H
        const unsigned okw = ((uw - (unsigned)W) >> 31) & (~uw >> 31);
        const unsigned ok = okh & okw & ((unsigned)(pp - G::PP) >> 31);         // ... and the item exists (pp < PP)
        pvalid |= ok << i;
        const unsigned pix = (uh * (unsigned)W + uw) & (0u - ok);               // inside the image: 32-bit byte offsets hold any batch
        poff[i] = (pix * (unsigned)Cin + (unsigned)(q * 4)) * 4u;
    }
    const char* ximg = reinterpret_cast<const char*>(x) + (size_t)img * H * W * Cin * 4;      // wave-uniform 64-bit image base
    // pixel of the tile behind result register r of row tile i (C/D layout: col = lane & 31, row = (r&3) + 8 (r>>2) + 4 kl)
    auto tile_m = [&](int i, int r) { return wm0 + i * 32 + halo_row_to_pix((r & 3) + 8 * (r >> 2) + 4 * kl); };
    // per-lane patch position of the two 32-pixel MFMA row tiles (tap (0,0) = +1,+1 inside the patch)
    int pbase[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = wm0 + i * 32 + halo_row_to_pix(ml);
        pbase[i] = (m / TW + 1) * G::PW + (m % TW) + 1;
    }

    const int cchunks = Cin / BK;
    const int total = cchunks * 9;
    f32x4 ra[G::ITEMS];
    auto issue_patch = [&](int cc) {
        const unsigned coff = (unsigned)(cc * BK * 4);
#pragma unroll
        for (int i = 0; i < G::ITEMS; ++i)
            ra[i] = *reinterpret_cast<const f32x4*>(ximg + (poff[i] + coff));
    };
    auto store_patch = [&](int cc) {
        f32x4 rs = {1.0f, 1.0f, 1.0f, 1.0f}, rt = {0.0f, 0.0f, 0.0f, 0.0f};
        if (PRO != 0) {
            rs = *reinterpret_cast<const f32x4*>(Ss + cc * BK + q * 4);
            rt = *reinterpret_cast<const f32x4*>(Ss + Cin + cc * BK + q * 4);
        }
#pragma unroll
        for (int i = 0; i < G::ITEMS; ++i) {
            int pp = (tid + 256 * i) >> 3;
            pp = pp < G::PP ? pp : G::PP;                      // items past the patch: the scratch pixel (no exec-mask branch)
            f32x4 v = apply_prologue(ra[i], PRO, rs, rt);
            if (!((pvalid >> i) & 1u)) v = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<f32x4*>(As + pp * G::AROW + q * 4) = v;
        }
    };
    // ---- weight staging per stage (ST k rows x BN_ couts) ----
    unsigned bhoff[BH_LOADS];
#pragma unroll
    for (int i = 0; i < BH_LOADS; ++i) {
        const int idx = tid + 256 * i;
        const int k = idx / (BN_ / 4), n4 = idx % (BN_ / 4);
        int n = n0 + n4 * 4;
        n = n < Cout ? n : 0;
        bhoff[i] = (unsigned)((k * Cout + n) * 4);
    }
    f32x4 rh[2][BH_LOADS];
    auto issue_bh = [&](const char* wchunk, f32x4 (&r)[BH_LOADS]) {        // ST weight rows x BN_ couts from wchunk (wave-uniform)
#pragma unroll
        for (int i = 0; i < BH_LOADS; ++i) r[i] = *reinterpret_cast<const f32x4*>(wchunk + bhoff[i]);
    };
    auto store_bh = [&](int buf, const f32x4 (&r)[BH_LOADS]) {
        float* b = Bs + buf * ST * BN_;
#pragma unroll
        for (int i = 0; i < BH_LOADS; ++i) {
            const int idx = tid + 256 * i;
            const int k = idx / (BN_ / 4), n4 = idx % (BN_ / 4);
            *reinterpret_cast<f32x4*>(b + k * BN_ + n4 * 4) = r[i];
        }
    };

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // The ST / 2 k-steps of one stage (channels ST h .. ST h + ST - 1 of the chunk, one tap) from weight buffer buf; mid() runs in the
    // middle.  k-step ks = 4 g + j multiplies channel 8 g + 4 kl + j of the stage: A = element j of the lane's float4 of channel
    // group g, B = that row of the buffer.
#if TAG_HALO_VALU_PROBE > 0
    typedef float probe_f2 __attribute__((ext_vector_type(2)));
    probe_f2 pacc[4] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#endif
    auto mma_stage = [&](int buf, int shift, int h, auto&& mid) {      // shift = (ky - 1) * PW + (kx - 1) of the tap
        const float* a0 = As + (pbase[0] + shift) * G::AROW + h * ST + kl * 4;
        const float* a1 = As + (pbase[1] + shift) * G::AROW + h * ST + kl * 4;
        const float* b = Bs + buf * ST * BN_ + (kl * 4) * BN_ + wn0 + ml;
        constexpr int PF = 2, NS = ST / 2, NG = NS / 4;
        f32x4 af[NG][2];                                        // [channel group][row tile]
        af[0][0] = *reinterpret_cast<const f32x4*>(a0);
        af[0][1] = *reinterpret_cast<const f32x4*>(a1);
        float bf[PF + 1][TN];
#pragma unroll
        for (int s0 = 0; s0 < PF; ++s0)
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[s0][j] = b[((s0 >> 2) * 8 + (s0 & 3)) * BN_ + j * 32];
        af[1][0] = *reinterpret_cast<const f32x4*>(a0 + 8);
        af[1][1] = *reinterpret_cast<const f32x4*>(a1 + 8);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < NS; ++ks) {
            const int cur = ks % (PF + 1), nxt = (ks + PF) % (PF + 1);
            if (ks + PF < NS) {
                const int kn = ks + PF;
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[nxt][j] = b[((kn >> 2) * 8 + (kn & 3)) * BN_ + j * 32];
            }
            if ((ks & 3) == 1 && (ks >> 2) + 2 < NG) {          // channel group g + 2 while group g is being multiplied
                af[(ks >> 2) + 2][0] = *reinterpret_cast<const f32x4*>(a0 + ((ks >> 2) + 2) * 8);
                af[(ks >> 2) + 2][1] = *reinterpret_cast<const f32x4*>(a1 + ((ks >> 2) + 2) * 8);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[ks >> 2][i][ks & 3], bf[cur][j], acc[i][j], 0, 0, 0);
#if TAG_HALO_VALU_PROBE > 0
            {
                const probe_f2 pa = {af[ks >> 2][0][ks & 3], af[ks >> 2][1][ks & 3]}, pb = {bf[cur][0], bf[cur][TN - 1]};
#pragma unroll
                for (int u = 0; u < TAG_HALO_VALU_PROBE; ++u)
                    asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(pacc[u & 3]) : "v"(pa), "v"(pb));
            }
#endif
            __builtin_amdgcn_sched_barrier(0);                  // keeps the operand reads of k-step ks + 2 ahead of their use
            if (ks == NS / 2 - 1) { mid(); __builtin_amdgcn_sched_barrier(0); }
        }
    };

#ifdef TAG_HALO_PROF   // 0 prologue, 1 MFMA taps, 2 barrier, 3 patch stores, 4 barrier (+ wait for the patch loads), 5 output stores, 6 statistics
    const unsigned long long hrt0 = __builtin_amdgcn_s_memrealtime();      // 100 MHz: shader clock = sum(hpc) / realtime
    unsigned long long hpc[7] = {0, 0, 0, 0, 0, 0, 0}, hp0 = __builtin_amdgcn_s_memtime();
#endif
    // Loop state is carried incrementally (tap / chunk counters, the tap's patch shift, the weight pointer one tap ahead): SALU
    // instructions wait for gaps in the co-resident waves' MFMA streams (tools/coissue_probe.hip: ~300 clocks each beside a dense
    // fp32 stream, 4.6 alone), and the divisions and 64-bit multiplies of the per-stage index form were ~90 of them per tap.
    static_assert(NSTG == 2, "two 16-channel stages per tap");
    const char* const wbase = reinterpret_cast<const char*>(wp);
    const size_t tap_stride = (size_t)Cin * Cout * 4;           // bytes from tap to tap in the (9, Cin, Cout) pack
    const unsigned half_stride = (unsigned)(ST * Cout * 4);     // from the first to the second 16 channels of a chunk
    issue_patch(0);
    issue_bh(wbase, rh[0]);
    issue_bh(wbase + half_stride, rh[1]);
#ifdef TAG_HALO_PROF
    { const unsigned long long p1_ = __builtin_amdgcn_s_memtime(); tag_halo_sub[0] = p1_ - hp0; }
#endif
    __syncthreads();                           // Ss visible
#ifdef TAG_HALO_PROF
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    { const unsigned long long p1_ = __builtin_amdgcn_s_memtime(); tag_halo_sub[1] = p1_ - hp0; }
#endif
    store_patch(0);
    store_bh(0, rh[0]);
#ifdef TAG_HALO_PROF
    { const unsigned long long p1_ = __builtin_amdgcn_s_memtime(); tag_halo_sub[2] = p1_ - hp0; }
#endif
    __syncthreads();
    HP_MARK(0)
    // Per tap two stages (weight buffers 0 / 1): at the start of a stage the weights of the stage after the next one are requested
    // into the register set this stage's weights left; in mid-stream the next stage's weights (requested one stage ago) go to the
    // other buffer; one barrier ends the stage.
    int tap = 0, cc = 0, kx = 0, shift = -G::PW - 1;            // current tap: (chunk cc, tap), its patch shift
    int p_tap = 1, p_cc = 0;                                    // the tap whose weights are requested during this one (= the next)
    const char* pw = wbase + tap_stride;
    if (total == 1) pw = wbase;
    for (int it = 0; it < total; ++it) {
        const bool newpatch = tap == 8 && cc + 1 < cchunks;
        if (newpatch) issue_patch(cc + 1);
        issue_bh(pw, rh[0]);                                   // (next tap, channels 0..15)
        __builtin_amdgcn_sched_barrier(0);
        mma_stage(0, shift, 0, [&] { store_bh(1, rh[1]); });   // (this tap, channels 16..31) -> buffer 1, read after the barrier
        HP_MARK(1)
        __syncthreads();
        HP_MARK(2)
        issue_bh(pw + half_stride, rh[1]);                     // (next tap, channels 16..31)
        __builtin_amdgcn_sched_barrier(0);
        mma_stage(1, shift, 1, [&] { store_bh(0, rh[0]); });   // (next tap, channels 0..15) -> buffer 0
        HP_MARK(1)
        __syncthreads();
        HP_MARK(2)
        if (newpatch) {                                        // every wave has read the last tap of the old patch
#ifdef TAG_HALO_PROF
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            HP_MARK(4)
#endif
            store_patch(cc + 1);
            HP_MARK(3)
            __syncthreads();
            HP_MARK(4)
        }
        // advance (tap, cc, shift) and the prefetch position by one tap
        if (tap == 8) { tap = 0; ++cc; kx = 0; shift = -G::PW - 1; }
        else { ++tap; if (kx == 2) { kx = 0; shift += G::PW - 2; } else { ++kx; ++shift; } }
        if (p_tap == 8) {
            p_tap = 0; ++p_cc;
            pw += (size_t)BK * Cout * 4;
            pw -= 8 * tap_stride;
            if (p_cc == cchunks) { p_cc = 0; pw = wbase; }      // past the end: the first tap again (stored, never used)
        } else { ++p_tap; pw += tap_stride; }
    }

    // ---- epilogue: C/D layout col = lane&31 (cout), row = (r&3) + 8*(r>>2) + 4*(lane>>5) -> pixel tile_m(i, r).  Registers 4 rq .. 4 rq + 3
    // of a lane quad (4 consecutive couts) are 4 consecutive pixels x 4 couts: transposed inside the quad (two DPP exchange rounds,
    // 16 VALU per block) each lane owns ONE pixel's 4 couts = one 16-byte store.  A global_store_dword is one of the instruction
    // forms that wait for the co-resident waves' MFMA streams to pause (tools/coissue_probe.hip; 32-64 of them held a finished tile
    // for 3-7 us), a dwordx4 store is not. ----
    {
        const int c4 = lane & 3;                                // position inside the lane quad = cout offset before, pixel offset after
        const bool odd = c4 & 1, hi = c4 & 2;
        // ---- EPI == 2 (the dgrad launch of the first conv of block i+1, whose output is the gradient of block i's POOLED output):
        // the reduction half of the backward of relu(bn(yref)) -> avg/max pool (ph x 2) -> dropout that this gradient flows into
        // next (models/panns.py:51-60 backward; what pool_bwd_reduce_kernel of bn_pool.hip computes in a pass of its own over the
        // largest tensors of the step).  Per 32-cout column block j the quad-transposed output tile (128 pixels x 64 couts of the four
        // waves, fp32) is ALSO parked in LDS -- the patch and weight buffers are free by now --, which ends the life of the
        // accumulators; then a thread takes (pooled pixel, channel quad) pieces of the tile -- its quad is FIXED, so 4 + 4 running sums
        // stay in registers --, undoes the dropout (the forward's counter-based mask is one hash per 4 consecutive channels = one per
        // piece), loads the ph x 2 window of yref as 16-byte pieces, recomputes a = bn(yref), the ReLU mask and the arg-max (first
        // maximum in scan order, as ATen's max_pool2d), forms dz = [a > 0] * g * (wavg + [arg-max] * wmax) and accumulates sum(dz),
        // sum(dz * xhat); the 16 threads of a quad are folded through LDS in a fixed order.  One partial row per workgroup m-tile
        // (row 2 mt of the [P][2][Cout] layout of EPI == 1, row 2 mt + 1 zero); tag_bn_grad_from_partials folds the rows;
        // pool_bwd_apply_kernel stays as the one pass that writes dy.  (The first form kept the sums in the store loop below, on the
        // live accumulators: the compiler spilled 280-560 B per lane -- 1.3 GB of scratch traffic per step -- and serialised the
        // window loads behind the spills.) ----
        float* const Ts = smem;                                 // [128 pixels][64 couts] fp32 tile of column block j (32 KB)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nq = n0 + wn0 + j * 32 + (ml & ~3);       // first of the quad's 4 couts
            f32x4 bq = {0.0f, 0.0f, 0.0f, 0.0f};
            if (EPI == 4) bq = ldg4(epi.yref + (size_t)img * Cout + (nq < Cout ? nq : 0));    // the clip's bias of these 4 couts
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    float x0 = acc[i][j][4 * rq], x1 = acc[i][j][4 * rq + 1], x2 = acc[i][j][4 * rq + 2], x3 = acc[i][j][4 * rq + 3];
                    // round 1: exchange with lane c4 ^ 1 (quad_perm [1,0,3,2]): even lanes send x1 / x3, odd lanes x0 / x2
                    const float s01 = odd ? x0 : x1, s23 = odd ? x2 : x3;
                    const float r01 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s01), 0xB1, 0xF, 0xF, true));
                    const float r23 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s23), 0xB1, 0xF, 0xF, true));
                    if (odd) { x0 = r01; x2 = r23; } else { x1 = r01; x3 = r23; }
                    // round 2: exchange with lane c4 ^ 2 (quad_perm [2,3,0,1]): low lanes send x2 / x3, high lanes x0 / x1
                    const float s02 = hi ? x0 : x2, s13 = hi ? x1 : x3;
                    const float r02 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s02), 0x4E, 0xF, 0xF, true));
                    const float r13 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s13), 0x4E, 0xF, 0xF, true));
                    if (hi) { x0 = r02; x1 = r13; } else { x2 = r02; x3 = r13; }
                    // now x_t = cout nq + t of the pixel behind register 4 rq + c4
                    if (EPI == 4) { x0 += bq[0]; x1 += bq[1]; x2 += bq[2]; x3 += bq[3]; }
                    const int m = wm0 + i * 32 + halo_row_to_pix(c4 + 8 * rq + 4 * kl);
                    const int h = h0 + m / TW, w = w0 + m % TW;
                    if (EPI != 3 && h < H && nq < Cout)         // (EPI == 3 writes the POOLED tensor only, below)
                        *reinterpret_cast<f32x4*>(y + (((size_t)img * H + h) * W + w) * Cout + nq) = (f32x4){x0, x1, x2, x3};
                    if (EPI == 2 || EPI == 3)                   // tile column = 32 (wid & 1) + (ml & ~3): the two 32-cout blocks side by side
                        *reinterpret_cast<f32x4*>(Ts + m * 64 + (wid & 1) * 32 + (ml & ~3)) = (f32x4){x0, x1, x2, x3};
                }
            // ---- EPI == 3 (inference: BatchNorm in eval mode, nothing saved for backward): relu(bn(.)) -> avg/max pool (ph x 2, floor)
            // of models/panns.py:50-60 straight from the parked tile -- the raw conv output, the largest tensor of the block (3.15 GB per
            // 64 clips of 30 s in block 1), is neither written nor read back by a pool pass.  Same expression and summation order as
            // bnact_pool_fwd_kernel: the result is bit-identical to the two-pass form. ----
            if (EPI == 3) {
                __syncthreads();                                // the tile of column block j is complete
                constexpr int THt = 128 / TW;
                const int pph = epi.ph, PWt = TW / 2, npool = (THt / pph) * PWt;
                const int qd = tid & 15;
                const int nt = n0 + (qd >> 3) * (BN_ / 2) + j * 32 + (qd & 7) * 4;
                const int ntc = nt < Cout ? nt : 0;
                const f32x4 bsc = ldg4(epi.scale + ntc), bsh = ldg4(epi.shift + ntc);
                const int Hp = H / pph, Wp = W >> 1;
                for (int pp = tid >> 4; pp < npool; pp += 16) {
                    const int py = pp / PWt, px = pp - py * PWt;
                    const int hp = h0 / pph + py, wp = (w0 >> 1) + px;
                    f32x4 sum = {0.0f, 0.0f, 0.0f, 0.0f}, mx = {0.0f, 0.0f, 0.0f, 0.0f};
                    for (int dh = 0; dh < pph; ++dh)
#pragma unroll
                        for (int dw = 0; dw < 2; ++dw) {
                            const f32x4 v = *reinterpret_cast<const f32x4*>(Ts + ((py * pph + dh) * TW + 2 * px + dw) * 64 + qd * 4);
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                const float a = fmaxf(fmaf(v[t], bsc[t], bsh[t]), 0.0f);
                                sum[t] += a;
                                mx[t] = (dh == 0 && dw == 0) ? a : fmaxf(mx[t], a);
                            }
                        }
                    f32x4 o;
#pragma unroll
                    for (int t = 0; t < 4; ++t) o[t] = sum[t] * epi.wavg + mx[t] * epi.wmax;
                    if (hp < Hp && nt < Cout)
                        *reinterpret_cast<f32x4*>(y + (((size_t)img * Hp + hp) * Wp + wp) * Cout + nt) = o;
                }
                if (j + 1 < TN) __syncthreads();                // the tile is rewritten by column block j + 1
            }
            if (EPI == 2) {
                __syncthreads();                                // the tile of column block j is complete
                const int qd = tid & 15, sub = tid >> 4;        // channel quad of the tile (fixed per thread), first pixel
                const int nt = n0 + (qd >> 3) * (BN_ / 2) + j * 32 + (qd & 7) * 4;        // global cout of the quad
                const int ntc = nt < Cout ? nt : 0;
                const f32x4 bsc = ldg4(epi.scale + ntc), bsh = ldg4(epi.shift + ntc), bmu = ldg4(epi.mean + ntc),
                            bis = ldg4(epi.invstd + ntc);
                const unsigned rowfb = (unsigned)epi.Wf * (unsigned)Cout * 4u, coutb = (unsigned)Cout * 4u;   // bytes: yref row, pixel
                const char* yimg = reinterpret_cast<const char*>(epi.yref) + (size_t)img * epi.Hf * rowfb;   // wave-uniform base
                const int pph = epi.ph;
                const bool pdrop = epi.drop_p > 0.0f;
                const float keep_scale = pdrop ? 1.0f / (1.0f - epi.drop_p) : 1.0f;
                const unsigned keep_thr = tag_keep4_threshold(epi.drop_p);
                float s1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
                for (int k2 = 0; k2 < 8; k2 += 2) {             // 8 pieces per thread, two at a time: 8 window loads in flight
                    f32x4 g2[2], vw[2][4];
                    int hh[2], ww[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int m = sub + 16 * (k2 + u);
                        hh[u] = h0 + m / TW; ww[u] = w0 + m % TW;
                        g2[u] = *reinterpret_cast<const f32x4*>(Ts + m * 64 + qd * 4);
                        if (hh[u] >= H) g2[u] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                        const int hc = hh[u] < H ? hh[u] : H - 1;
                        const unsigned off = (unsigned)(hc * pph) * rowfb + (unsigned)(2 * ww[u]) * coutb + (unsigned)ntc * 4u;
                        vw[u][0] = *reinterpret_cast<const f32x4*>(yimg + off);
                        vw[u][1] = *reinterpret_cast<const f32x4*>(yimg + (off + coutb));
                        if (pph == 2) {
                            vw[u][2] = *reinterpret_cast<const f32x4*>(yimg + (off + rowfb));
                            vw[u][3] = *reinterpret_cast<const f32x4*>(yimg + (off + rowfb + coutb));
                        } else { vw[u][2] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f}; vw[u][3] = vw[u][2]; }
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        f32x4 g = g2[u];
                        if (pdrop) {
                            const uint64_t grp = ((uint64_t)((unsigned)img * (unsigned)H + (unsigned)hh[u]) * (unsigned)W + (unsigned)ww[u])
                                                 * (unsigned)(Cout >> 2) + (unsigned)(ntc >> 2);     // flat index of the pooled element / 4
                            const uint64_t bits = tag_keep4_bits(epi.seed, grp);
#pragma unroll
                            for (int t = 0; t < 4; ++t) g[t] = tag_keep4(bits, t, keep_thr) ? g[t] * keep_scale : 0.0f;
                        }
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            float a[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) a[k] = fmaf(vw[u][k][t], bsc[t], bsh[t]);
                            if (pph != 2) { a[2] = -INFINITY; a[3] = -INFINITY; }
                            const float mx = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
                            const float gw = g[t] * epi.wavg, gwm = g[t] * (epi.wavg + epi.wmax);
                            bool found = false;
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const bool eq = a[k] == mx;
                                const bool hit = eq && !found;
                                found = found || eq;
                                const float dz = a[k] > 0.0f ? (hit ? gwm : gw) : 0.0f;
                                s1[t] += dz;
                                s2[t] = fmaf(dz, (vw[u][k][t] - bmu[t]) * bis[t], s2[t]);
                            }
                        }
                    }
                }
                __syncthreads();                                // every thread is done reading the tile
                *reinterpret_cast<f32x4*>(Ts + tid * 8) = (f32x4){s1[0], s1[1], s1[2], s1[3]};
                *reinterpret_cast<f32x4*>(Ts + tid * 8 + 4) = (f32x4){s2[0], s2[1], s2[2], s2[3]};
                __syncthreads();
                if (tid < 64) {                                 // tile column tid: quad tid / 4, element tid % 4; fold the 16 threads of the quad
                    const int q = tid >> 2, e = tid & 3;
                    float a = 0.0f, b = 0.0f;
                    for (int r = 0; r < 16; ++r) { a += Ts[(r * 16 + q) * 8 + e]; b += Ts[(r * 16 + q) * 8 + 4 + e]; }
                    const int n = n0 + (q >> 3) * (BN_ / 2) + j * 32 + (q & 7) * 4 + e;
                    if (n < Cout) {
                        float* ps = stats + (size_t)(mt * 2) * 2 * Cout;
                        ps[n] = a; ps[Cout + n] = b;
                        ps[2 * Cout + n] = 0.0f; ps[3 * Cout + n] = 0.0f;     // row 2 mt + 1 of the EPI == 1 layout stays empty
                    }
                }
                if (j + 1 < TN) __syncthreads();                // the tile is rewritten by column block j + 1
            }
        }
    }
#if TAG_HALO_VALU_PROBE > 0
    if (pacc[0][0] + pacc[1][0] + pacc[2][1] + pacc[3][1] == 12345.678f) y[0] = pacc[0][0];
#endif
    HP_MARK(5)
    // ---- fused BatchNorm statistics of the output (training): per (64-pixel wave tile, channel) a pivot mu (the tile
    // mean as rounded in fp32), r = sum(y - mu) and q = sum((y - mu)^2): the tile's sum is n*mu + r EXACTLY up to the
    // rounding of the small deviations, so channels whose |mean| >> std keep their variance;
    // tag_bn_stats_from_partials merges the tiles in fp64 ----
    // ---- EPI == 1 (dgrad launches): the reduction half of the BatchNorm+ReLU backward this gradient flows into.  The
    // accumulators hold da = dL/d relu(bn(yref)); with g = da * [bn(yref) > 0] and xhat = (yref - mean) * invstd the
    // BatchNorm backward needs sum(g) (= dbeta) and sum(g * xhat) (= dgamma) per channel BEFORE any dy can be formed.
    // Each wave folds them over its 64 pixels here -- yref is read once, by a kernel that is MFMA-bound and leaves the
    // HBM pipe idle -- instead of a separate 2-tensor pass (reduce2_kernel<BnReluBwdFn>).  Row layout [prow][2][Cout];
    // tag_bn_grad_from_partials merges the rows in fp64 in a fixed order. ----
    if (EPI == 1) {
        const int prow = mt * 2 + (wid >> 1);
        float* ps = stats + (size_t)prow * 2 * Cout;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn0 + j * 32 + ml;
            const int nc = n < Cout ? n : 0;
            const float sc = epi.scale[nc], sh = epi.shift[nc], mu = epi.mean[nc], is = epi.invstd[nc];
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float yv[16];                                // 16 loads in flight, then their arithmetic
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = tile_m(i, r);
                    const int h = h0 + m / TW, w = w0 + m % TW;
                    const int hc = h < H ? h : H - 1;
                    yv[r] = epi.yref[(((size_t)img * H + hc) * W + w) * Cout + nc];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = (h0 + tile_m(i, r) / TW) < H;
                    const float g = (ok && fmaf(yv[r], sc, sh) > 0.0f) ? acc[i][j][r] : 0.0f;
                    s1 += g;
                    s2 = fmaf(g, (yv[r] - mu) * is, s2);
                }
            }
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (kl == 0 && n < Cout) { ps[n] = s1; ps[Cout + n] = s2; }
        }
    }
    if (EPI == 0 && stats) {
        const int prow = mt * 2 + (wid >> 1);                        // partial row of this wave
        float* ps = stats + (size_t)prow * 3 * Cout;
        float cnt = 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) cnt += (h0 + tile_m(i, r) / TW) < H ? 1.0f : 0.0f;
        cnt += __shfl_xor(cnt, 32, 64);
        const float rc = 1.0f / fmaxf(cnt, 1.0f);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float s1 = 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = (h0 + tile_m(i, r) / TW) < H;
                    s1 += ok ? acc[i][j][r] : 0.0f;
                }
            s1 += __shfl_xor(s1, 32, 64);
            const float mu = s1 * rc;
            float r1 = 0.0f, q = 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = (h0 + tile_m(i, r) / TW) < H;
                    const float d = ok ? acc[i][j][r] - mu : 0.0f;
                    r1 += d;
                    q = fmaf(d, d, q);
                }
            r1 += __shfl_xor(r1, 32, 64);
            q += __shfl_xor(q, 32, 64);
            const int n = n0 + wn0 + j * 32 + ml;
            if (kl == 0 && n < Cout) { ps[n] = mu; ps[Cout + n] = r1; ps[2 * Cout + n] = q; }
        }
        if (n0 == 0 && wn0 == 0 && lane == 0) stats[(size_t)m_tiles * 2 * 3 * Cout + prow] = cnt;
    }
#ifdef TAG_HALO_PROF
    HP_MARK(6)
#ifndef TAG_HALO_PROF_BLOCK
#define TAG_HALO_PROF_BLOCK 1500                                  // the sampled workgroup (a late one + TAG_PROF_REPS launches: steady clocks)
#endif
    if (tid == 0 && blockIdx.x < 65536) {
        const unsigned hw = (unsigned)__builtin_amdgcn_s_getreg((15 << 11) | (0 << 6) | 4);            // HW_ID bits 0..15
        const unsigned xcc = (unsigned)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15u;     // XCC_ID
        tag_halo_wg[blockIdx.x] = hrt0;
        tag_halo_wg[65536 + blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        tag_halo_wg[2 * 65536 + blockIdx.x] = (xcc << 16) | (hw & 0xffffu);
        tag_halo_wg[3 * 65536 + blockIdx.x] = hrt_first;
    }
    if (blockIdx.x == TAG_HALO_PROF_BLOCK && tid == 0) {
        for (int i = 0; i < 7; ++i) tag_halo_prof[i] = hpc[i];
        tag_halo_sub[3] = __builtin_amdgcn_s_memrealtime() - hrt0;
    }
#endif
}

// ------------------------------------------------------------------------------------------
// wgrad: partial[split][tap][ci][co] = sum_{m in split} prologue(x)[m + shift(tap)][ci] * dy[m][co]
// ------------------------------------------------------------------------------------------
template <int TC, int PRO>   // TC x TC output tile (64 or 128)
__global__ __launch_bounds__(256, TAG_NBUF == 2 ? 2 : 3) void conv3x3_wgrad_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ in_scale,
                                                               const float* __restrict__ in_shift,
                                                               const float* __restrict__ dy,
                                                               float* __restrict__ partial, int B, int H, int W,
                                                               int Cin, int Cout, int splits, long chunk) {
    constexpr int TT = TC / 64;              // 32x32 tiles per wave per dim (waves 2 x 2)
    constexpr int LOADS = TC / 32;           // float4 per thread per operand per chunk (32 pixels x TC)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                        // [NBUF][BK][TC]  (pixel-major, ci contiguous)
    float* Bs = smem + TAG_NBUF * BK * TC;   // [NBUF][BK][TC]

    const long M = (long)B * H * W;
    const int ci_tiles = (Cin + TC - 1) / TC, co_tiles = (Cout + TC - 1) / TC;
    int L = xcd_remap(blockIdx.x, 9 * ci_tiles * co_tiles * splits);
    const int tap = L % 9; L /= 9;
    const int cot = L % co_tiles; L /= co_tiles;
    const int cit = L % ci_tiles; L /= ci_tiles;
    const int split = L;
    const int ci0 = cit * TC, co0 = cot * TC;
    const int dyy = tap / 3 - 1, dxx = tap % 3 - 1;
    const long kbeg = (long)split * chunk;
    long kend = kbeg + chunk;
    if (kend > M) kend = M;
    const int kiters = kbeg < kend ? (int)((kend - kbeg + BK - 1) / BK) : 0;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm0 = (wid >> 1) * (TC / 2), wn0 = (wid & 1) * (TC / 2);

    // branch-free loads (clamped addresses); zero-fill and the BN+ReLU prologue happen at the LDS store
    f32x4 ra[LOADS], rb[LOADS], rs[LOADS], rt[LOADS];
    unsigned amask = 0, bmask = 0;
    const int iHW = H * W;
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
        const int c4 = ((tid + 256 * i) % (TC / 4)) * 4;
        if (PRO != 0) {
            const int cc = ci0 + c4 < Cin ? ci0 + c4 : 0;
            rs[i] = ldg4(in_scale + cc);
            rt[i] = ldg4(in_shift + cc);
        } else {
            rs[i] = (f32x4){1.0f, 1.0f, 1.0f, 1.0f};
            rt[i] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
    // per-thread constants of the staging pattern; per chunk only the (wave-uniform) pixel origin changes
    int pixi[LOADS];
    unsigned cab[LOADS], cbb[LOADS];          // byte offsets of the channel quads (clamped: masked columns are never stored)
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
        const int idx = tid + 256 * i;
        const int c4 = (idx % (TC / 4)) * 4;
        pixi[i] = idx / (TC / 4);
        cab[i] = (unsigned)((ci0 + c4 < Cin ? ci0 + c4 : 0) * 4);
        cbb[i] = (unsigned)((co0 + c4 < Cout ? co0 + c4 : 0) * 4);
    }
    const unsigned rW = (65536u + (unsigned)W - 1u) / (unsigned)W;   // t / W == (t * rW) >> 16 for t < 64 + W <= 2^7
    const int tapoff = dyy * W + dxx;
    auto load_chunk = [&](int it) {
        const unsigned kb = (unsigned)(kbeg + (long)it * BK);         // M < 2^31 (checked by the launcher)
        const unsigned hw0 = kb % (unsigned)iHW;                     // wave-uniform: scalar ALU
        const int h0 = (int)(hw0 / (unsigned)W), w0 = (int)(hw0 - (unsigned)h0 * (unsigned)W);
        amask = bmask = 0;
#pragma unroll
        for (int i = 0; i < LOADS; ++i) {
            unsigned m = kb + (unsigned)pixi[i];
            const bool in_range = (long)m < kend;
            m = in_range ? m : (unsigned)(kend - 1);
            const int t = w0 + pixi[i];                               // < W + 32
            const int dh = W >= 32 ? (t >= W ? 1 : 0) : (int)(((unsigned)t * rW) >> 16);
            // A chunk may run into the next image -- and, when W < 32 and H W < 32 + W, across SEVERAL image boundaries (3 x 5
            // images: 32 pixels touch three of them), so the row wraps by a true modulo: h0 + dh < H + 33.  Where one subtraction
            // was enough (h0 + dh < 2 H: every W >= 32, every image of 32 + W pixels or more) the modulo gives the same row, so
            // masks, addresses and therefore every result bit are unchanged there.
            int hh = (int)((unsigned)(h0 + dh) % (unsigned)H);
            hh += dyy;
            const int ww = t - dh * W + dxx;
            const unsigned aok = (unsigned)in_range & (unsigned)((unsigned)hh < (unsigned)H) &
                                 (unsigned)((unsigned)ww < (unsigned)W);
            amask |= aok << i;
            bmask |= (unsigned)in_range << i;
            const unsigned ma = m + (unsigned)(aok ? tapoff : 0);
            ra[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(x) + (ma * (unsigned)Cin * 4u + cab[i]));
            rb[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(dy) + (m * (unsigned)Cout * 4u + cbb[i]));
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < LOADS; ++i) {
            const int idx = tid + 256 * i;
            const int pix = idx / (TC / 4), c4 = (idx % (TC / 4)) * 4;
            f32x4 va = apply_prologue(ra[i], PRO, rs[i], rt[i]);
            if (!((amask >> i) & 1u)) va = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            f32x4 vb = rb[i];
            if (!((bmask >> i) & 1u)) vb = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<f32x4*>(As + (buf * BK + pix) * TC + c4) = va;
            *reinterpret_cast<f32x4*>(Bs + (buf * BK + pix) * TC + c4) = vb;
        }
    };

    f32x16 acc[TT][TT];
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int kl = lane >> 5, ml = lane & 31;
    if (kiters > 0) {
        load_chunk(0);
        store_chunk(0);
    }
    __syncthreads();
    for (int it = 0; it < kiters; ++it) {
        const int buf = TAG_NBUF == 2 ? (it & 1) : 0;
        if (it + 1 < kiters) load_chunk(it + 1);
        __builtin_amdgcn_sched_barrier(0);
        const float* a = As + (buf * BK + kl) * TC + wm0 + ml;
        const float* b = Bs + (buf * BK + kl) * TC + wn0 + ml;
        float af[2][TT], bf[2][TT];
#pragma unroll
        for (int i = 0; i < TT; ++i) af[0][i] = a[i * 32];
#pragma unroll
        for (int j = 0; j < TT; ++j) bf[0][j] = b[j * 32];
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            const int cur = ks & 1, nxt = cur ^ 1;
            if (ks + 1 < BK / 2) {
#pragma unroll
                for (int i = 0; i < TT; ++i) af[nxt][i] = a[(2 * ks + 2) * TC + i * 32];
#pragma unroll
                for (int j = 0; j < TT; ++j) bf[nxt][j] = b[(2 * ks + 2) * TC + j * 32];
            }
#pragma unroll
            for (int i = 0; i < TT; ++i)
#pragma unroll
                for (int j = 0; j < TT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);
            if (ks + 1 < BK / 2) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, TT * TT, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (TAG_NBUF == 1) __syncthreads();       // every wave is done reading the single buffer
        if (it + 1 < kiters) store_chunk(TAG_NBUF == 2 ? (buf ^ 1) : 0);
        __syncthreads();
    }
    float* out = partial + ((size_t)split * 9 + tap) * Cin * Cout;
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            const int co = co0 + wn0 + j * 32 + ml;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ci0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
                if (ci < Cin && co < Cout) out[(size_t)ci * Cout + co] = acc[i][j][r];
            }
        }
}

// ------------------------------------------------------------------------------------------
// All-taps wgrad (image widths 8/16/32/64): a workgroup owns a 64(ci) x 64(co) block of ALL nine taps
// (9 x 16 accumulator registers per wave) and walks its share of the pixels in chunks of 32 output pixels
// (a CH x CW rectangle).  Per chunk the (CH+2) x (CW+2) x 64ci input patch and the 32 x 64co dy tile are staged
// ONCE in LDS (pixel-major = their HBM layout, straight float4 copies; producer BN+ReLU and zero padding applied
// at the store) and feed 9 x 16 MFMAs per wave: 9x fewer operand loads per FLOP than the per-tap kernel above.
// ------------------------------------------------------------------------------------------
template <int TW>
struct WgGeom {
    static constexpr int CW = TW >= 32 ? 32 : TW, CH = 32 / CW, PW = CW + 2, PH = CH + 2, PP = PH * PW;
    static constexpr int XITEMS = (PP * 16 + 255) / 256;          // float4 per thread for the 64-channel patch
};

template <int TW, int PRO>
__global__ __launch_bounds__(256, 2) void conv3x3_wgrad_alltaps_kernel(const float* __restrict__ x,
                                                                       const float* __restrict__ in_scale,
                                                                       const float* __restrict__ in_shift,
                                                                       const float* __restrict__ dy,
                                                                       float* __restrict__ partial, int B, int H, int W,
                                                                       int Cin, int Cout, int splits, int chunks_per_split) {
    using G = WgGeom<TW>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // two operand buffers: buffer b = [PP][64] input patch (pixel-major) followed by [32][64] dy chunk.  The next chunk is written
    // to the other buffer IN THE MIDDLE of the current chunk's MFMA stream (its loads were issued one chunk earlier) and one
    // barrier ends each chunk: no store phase between two barriers in which the wave issues no MFMA (round 4, as in the halo conv)
    constexpr int BUFSZ = (G::PP + 1) * 64 + 32 * 64;           // + one scratch pixel for the staging items past the patch

    const int ci_tiles = (Cin + 63) / 64, co_tiles = (Cout + 63) / 64;
    int L = xcd_remap(blockIdx.x, ci_tiles * co_tiles * splits);
    const int cot = L % co_tiles; L /= co_tiles;
    const int cit = L % ci_tiles; L /= ci_tiles;
    const int split = L;
    const int ci0 = cit * 64, co0 = cot * 64;
    const int rb_per_img = (H + G::CH - 1) / G::CH, cb_per_row = TW / G::CW;
    const int chunks_total = B * rb_per_img * cb_per_row;
    const int cbeg = split * chunks_per_split;
    int cend = cbeg + chunks_per_split;
    if (cend > chunks_total) cend = chunks_total;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wci = (wid >> 1) * 32, wco = (wid & 1) * 32;
    const int kl = lane >> 5, ml = lane & 31;

    // staging geometry (loop invariant): patch item = (patch pixel, channel quad), dy item = (pixel, channel quad).  Scalar
    // instructions wait for gaps in the co-resident workgroup's MFMA stream (tools/coissue_probe.hip), so the per-chunk part is kept
    // free of divisions, 64-bit multiplies, vector compares and exec-mask branches: the chunk origin is carried incrementally,
    // validity is sign-bit arithmetic, offsets are 32-bit inside the image, items past the patch go to a scratch pixel.
    int xpr[G::XITEMS], xpc[G::XITEMS], xpp[G::XITEMS];
    const int c4 = (tid & 15) * 4;
    const int ca = ci0 + c4 < Cin ? ci0 + c4 : 0, cb = co0 + c4 < Cout ? co0 + c4 : 0;
#pragma unroll
    for (int i = 0; i < G::XITEMS; ++i) {
        const int pp = (tid + 256 * i) >> 4;
        xpr[i] = pp / G::PW;
        xpc[i] = pp - xpr[i] * G::PW;
        xpp[i] = pp < G::PP ? pp : G::PP;
    }
    f32x4 rs = {1.0f, 1.0f, 1.0f, 1.0f}, rt = {0.0f, 0.0f, 0.0f, 0.0f};
    if (PRO != 0) { rs = ldg4(in_scale + ca); rt = ldg4(in_shift + ca); }

    f32x4 rx[G::XITEMS], rd[2];
    unsigned xok = 0, dok = 0;
    // origin of the NEXT chunk to be requested (chunks are requested in increasing order, column blocks fastest)
    int o_img, o_h0, o_w0;
    {
        const int cbk = cbeg % cb_per_row; const int r = cbeg / cb_per_row;
        o_img = r / rb_per_img; o_h0 = (r - o_img * rb_per_img) * G::CH; o_w0 = cbk * G::CW;
    }
    const size_t img_x = (size_t)H * W * Cin * 4, img_d = (size_t)H * W * Cout * 4;       // bytes per image
    const char* xi = reinterpret_cast<const char*>(x) + (size_t)o_img * img_x;
    const char* di = reinterpret_cast<const char*>(dy) + (size_t)o_img * img_d;
    auto issue_chunk = [&](int) {
        const int h0 = o_h0, w0 = o_w0;
        xok = dok = 0;
#pragma unroll
        for (int i = 0; i < G::XITEMS; ++i) {
            const unsigned uh = (unsigned)(h0 - 1 + xpr[i]), uw = (unsigned)(w0 - 1 + xpc[i]);
            const unsigned ok = ((uh - (unsigned)H) >> 31) & (~uh >> 31) & ((uw - (unsigned)W) >> 31) & (~uw >> 31);
            xok |= ok << i;
            const unsigned pix = (uh * (unsigned)W + uw) & (0u - ok);
            rx[i] = *reinterpret_cast<const f32x4*>(xi + (pix * (unsigned)Cin + (unsigned)ca) * 4u);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = (tid + 256 * i) >> 4;                     // pixel of the chunk, row-major in the rectangle
            const unsigned uh = (unsigned)(h0 + k / G::CW), uw = (unsigned)(w0 + k % G::CW);
            const unsigned ok = (uh - (unsigned)H) >> 31;
            dok |= ok << i;
            const unsigned pix = (uh * (unsigned)W + uw) & (0u - ok);
            rd[i] = *reinterpret_cast<const f32x4*>(di + (pix * (unsigned)Cout + (unsigned)cb) * 4u);
        }
        // advance the origin by one chunk
        o_w0 += G::CW;
        if (o_w0 >= TW) {
            o_w0 = 0; o_h0 += G::CH;
            if (o_h0 >= rb_per_img * G::CH) { o_h0 = 0; ++o_img; xi += img_x; di += img_d; }
        }
    };
    auto store_chunk = [&](int buf) {
        float* As = smem + buf * BUFSZ;
        float* Bs = As + (G::PP + 1) * 64;
#pragma unroll
        for (int i = 0; i < G::XITEMS; ++i) {
            f32x4 v = apply_prologue(rx[i], PRO, rs, rt);
            if (!((xok >> i) & 1u)) v = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<f32x4*>(As + xpp[i] * 64 + c4) = v;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = (tid + 256 * i) >> 4;
            f32x4 v = rd[i];
            if (!((dok >> i) & 1u)) v = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<f32x4*>(Bs + k * 64 + c4) = v;
        }
    };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    if (cbeg < cend) {
        issue_chunk(cbeg);
        store_chunk(0);
        if (cbeg + 1 < cend) issue_chunk(cbeg + 1);
    }
    __syncthreads();
    for (int c = cbeg; c < cend; ++c) {
        const int buf = (c - cbeg) & 1;
        __builtin_amdgcn_sched_barrier(0);
        const float* a = smem + buf * BUFSZ + kl * 64 + wci + ml;
        const float* b = smem + buf * BUFSZ + (G::PP + 1) * 64 + kl * 64 + wco + ml;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            if (ks == 8) {                                 // chunk c + 1 (loaded during chunk c - 1 .. c) -> the other buffer
                __builtin_amdgcn_sched_barrier(0);
                if (c + 1 < cend) store_chunk(buf ^ 1);
                if (c + 2 < cend) issue_chunk(c + 2);
                __builtin_amdgcn_sched_barrier(0);
            }
            // pixel pair (2ks, 2ks+1) of the chunk rectangle -> patch position of tap (0,0)
            constexpr int dummy = 0; (void)dummy;
            const int pr = (2 * ks) / G::CW, pc = (2 * ks) % G::CW;
            const int pbase = (pr + 1) * G::PW + pc + 1;
            const float bf = b[(2 * ks) * 64];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int shift = (t / 3 - 1) * G::PW + (t % 3 - 1);
                const float af = a[(pbase + shift) * 64];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc[t], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();                                   // chunk c + 1 is complete in LDS; every wave is done reading chunk c
    }
    // partial[split][tap][ci][co]
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        float* out = partial + ((size_t)split * 9 + t) * Cin * Cout;
        const int co = co0 + wco + ml;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = ci0 + wci + (r & 3) + 8 * (r >> 2) + 4 * kl;
            if (ci < Cin && co < Cout) out[(size_t)ci * Cout + co] = acc[t][r];
        }
    }
}

// ------------------------------------------------------------------------------------------
// All-taps wgrad for the 32- and 64-wide images (round 4): the same decomposition (64 ci x 64 co x 9 taps per workgroup, 32-pixel
// chunks = one image row of a 32-wide column strip), but a workgroup walks DOWN its strip and the input rows live in a RING of four
// row slots: a chunk stages only its one new row (34 pixels) instead of the whole 3 x 34 patch -- the full-patch form staged every
// input row three times, 7 + 2 float4 per thread and chunk against 4 + 2 on the narrow images, and ran at 0.85 MFMA busy against
// 0.90 there.  New row and dy tile are written in the middle of the chunk's MFMA stream; one barrier per chunk; a new strip (once
// per H chunks) rebuilds the ring synchronously.  Chunk order: (image, strip, row), rows fastest.
// ------------------------------------------------------------------------------------------
template <int TW, int PRO>
__global__ __launch_bounds__(256, 2) void conv3x3_wgrad_rowring_kernel(const float* __restrict__ x,
                                                                       const float* __restrict__ in_scale,
                                                                       const float* __restrict__ in_shift,
                                                                       const float* __restrict__ dy,
                                                                       float* __restrict__ partial, int B, int H, int W,
                                                                       int Cin, int Cout, int splits, int chunks_per_split) {
    // chunk = CH rows x CW columns = 32 pixels of one column strip; ring of R row slots: the CH + 2 rows a chunk reads and the CH
    // new rows of the next chunk
    constexpr int CW = TW >= 32 ? 32 : TW, CH = 32 / CW, PW = CW + 2, R = 2 * CH + 2, ROWF = PW * 64;
    constexpr int XI = (CH * PW * 16 + 255) / 256;               // float4 per thread per group of CH input rows (3)
    constexpr int NPRIME = (CH + 2 + CH - 1) / CH;               // row groups that rebuild the ring at a strip's first chunk
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Xr = smem;                                            // [R][PW][64] + one scratch pixel
    float* Ys = smem + R * ROWF + 64;                            // [2][32][64]

    const int ci_tiles = (Cin + 63) / 64, co_tiles = (Cout + 63) / 64;
    int L = xcd_remap(blockIdx.x, ci_tiles * co_tiles * splits);
    const int cot = L % co_tiles; L /= co_tiles;
    const int cit = L % ci_tiles; L /= ci_tiles;
    const int split = L;
    const int ci0 = cit * 64, co0 = cot * 64;
    constexpr int strips = TW / CW;
    const int rb = (H + CH - 1) / CH;                            // row blocks (chunks) per strip
    const int chunks_total = B * strips * rb;
    const int cbeg = split * chunks_per_split;
    int cend = cbeg + chunks_per_split;
    if (cend > chunks_total) cend = chunks_total;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wci = (wid >> 1) * 32, wco = (wid & 1) * 32;
    const int kl = lane >> 5, ml = lane & 31;
    const int c4 = (tid & 15) * 4;
    const int ca = ci0 + c4 < Cin ? ci0 + c4 : 0, cb = co0 + c4 < Cout ? co0 + c4 : 0;
    f32x4 rs = {1.0f, 1.0f, 1.0f, 1.0f}, rt = {0.0f, 0.0f, 0.0f, 0.0f};
    if (PRO != 0) { rs = ldg4(in_scale + ca); rt = ldg4(in_shift + ca); }

    // position of the current chunk: image, strip origin column, first row h0, ring slot of row h0 - 1 (division once per workgroup)
    int img, w0, h0, s0;
    {
        const int t = cbeg / rb;
        h0 = (cbeg - t * rb) * CH;
        img = t / strips;
        w0 = (t - img * strips) * CW;
        s0 = (h0 + R - 1) % R;
    }
    const size_t img_x = (size_t)H * W * Cin * 4, img_d = (size_t)H * W * Cout * 4;
    const char* xi = reinterpret_cast<const char*>(x) + (size_t)img * img_x;
    const char* di = reinterpret_cast<const char*>(dy) + (size_t)img * img_d;

    // staging geometry of a row group (loop invariant): item = (row pr of the group, patch column pc, channel quad)
    int xpr[XI], xpc[XI];
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        const int pp = (tid + 256 * i) >> 4;
        xpr[i] = pp / PW;                                        // >= CH: past the group -> scratch pixel
        xpc[i] = pp - xpr[i] * PW;
    }
    f32x4 rx[XI], rd[2];
    unsigned xok = 0, dok = 0;
    auto load_rows = [&](int first) {                            // input rows first .. first + CH - 1 of the strip (zeros outside the image)
        xok = 0;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const unsigned ur = (unsigned)(first + xpr[i]), uw = (unsigned)(w0 - 1 + xpc[i]);
            const unsigned ok = ((ur - (unsigned)H) >> 31) & (~ur >> 31) & ((uw - (unsigned)W) >> 31) & (~uw >> 31) &
                                ((unsigned)(xpr[i] - CH) >> 31);
            xok |= ok << i;
            const unsigned pix = (ur * (unsigned)W + uw) & (0u - ok);
            rx[i] = *reinterpret_cast<const f32x4*>(xi + (pix * (unsigned)Cin + (unsigned)ca) * 4u);
        }
    };
    auto store_rows = [&](int slot_first) {                      // -> ring slots slot_first .. (mod R)
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            f32x4 v = apply_prologue(rx[i], PRO, rs, rt);
            if (!((xok >> i) & 1u)) v = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            int sl = slot_first + xpr[i];
            sl = sl >= R ? sl - R : sl;
            float* d = xpr[i] < CH ? Xr + sl * ROWF + xpc[i] * 64 + c4 : Xr + R * ROWF + c4;
            *reinterpret_cast<f32x4*>(d) = v;
        }
    };
    auto load_dy = [&](int first) {                              // dy rows first .. first + CH - 1, columns w0 .. w0 + CW - 1
        dok = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = (tid + 256 * i) >> 4;
            const unsigned ur = (unsigned)(first + k / CW), uw = (unsigned)(w0 + k % CW);
            const unsigned ok = (ur - (unsigned)H) >> 31;
            dok |= ok << i;
            const unsigned pix = (ur * (unsigned)W + uw) & (0u - ok);
            rd[i] = *reinterpret_cast<const f32x4*>(di + (pix * (unsigned)Cout + (unsigned)cb) * 4u);
        }
    };
    auto store_dy = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = (tid + 256 * i) >> 4;
            f32x4 v = rd[i];
            if (!((dok >> i) & 1u)) v = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<f32x4*>(Ys + buf * 2048 + k * 64 + c4) = v;
        }
    };
    auto wrap = [](int sl) { return sl >= R ? sl - R : sl; };
    // rows h0 - 1 .. h0 + CH (and up to CH - 2 rows beyond) and dy of a strip's first chunk in this workgroup, synchronously
    auto prime = [&](int buf) {
        int sl = s0;
#pragma unroll
        for (int g = 0; g < NPRIME; ++g) {
            load_rows(h0 - 1 + g * CH);
            store_rows(sl);
            sl = wrap(sl + CH);
        }
        load_dy(h0);
        store_dy(buf);
    };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    bool have_next_regs = false;                                 // rx / rd hold the next chunk's new rows / dy tile
    if (cbeg < cend) {
        prime(0);
        if (cbeg + 1 < cend && h0 + CH < H) { load_rows(h0 + CH + 1); load_dy(h0 + CH); have_next_regs = true; }
    }
    __syncthreads();
    for (int c = cbeg; c < cend; ++c) {
        const int buf = (c - cbeg) & 1;
        const bool next = c + 1 < cend, next_same = next && h0 + CH < H;
        __builtin_amdgcn_sched_barrier(0);
        const float* ar[CH + 2];                                 // rows h0 - 1 .. h0 + CH
#pragma unroll
        for (int j = 0; j < CH + 2; ++j) {
            int sl = s0 + j;
            sl = sl >= R ? sl - R : sl;
            ar[j] = Xr + sl * ROWF + kl * 64 + wci + ml;
        }
        const float* b = Ys + buf * 2048 + kl * 64 + wco + ml;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            if (ks == 8) {                                 // the next chunk's new rows and dy tile (requested a chunk ago) -> LDS
                __builtin_amdgcn_sched_barrier(0);
                if (next_same && have_next_regs) {
                    store_rows(wrap(wrap(s0 + CH) + 2));   // slots of rows h0 + CH + 1 ..
                    store_dy(buf ^ 1);
                    have_next_regs = false;
                    if (c + 2 < cend && h0 + 2 * CH < H) { load_rows(h0 + 2 * CH + 1); load_dy(h0 + 2 * CH); have_next_regs = true; }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            const int pr = (2 * ks) / CW, pc = (2 * ks) % CW;   // pixel pair (2 ks, 2 ks + 1) of the chunk rectangle
            const float bf = b[(2 * ks) * 64];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float af = ar[pr + t / 3][(pc + t % 3) * 64];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc[t], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();                                   // the next chunk is complete in LDS; every wave is done reading this one
        // advance to the next chunk
        h0 += CH;
        s0 = wrap(s0 + CH);
        if (h0 >= H) {
            h0 = 0; s0 = R - 1; w0 += CW;
            if (w0 >= TW) { w0 = 0; ++img; xi += img_x; di += img_d; }
            if (next) {                                    // new strip: rebuild the ring
                prime(buf ^ 1);
                have_next_regs = false;
                if (c + 2 < cend && h0 + CH < H) { load_rows(h0 + CH + 1); load_dy(h0 + CH); have_next_regs = true; }
                __syncthreads();
            }
        }
    }
    // partial[split][tap][ci][co]
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        float* out = partial + ((size_t)split * 9 + t) * Cin * Cout;
        const int co = co0 + wco + ml;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = ci0 + wci + (r & 3) + 8 * (r >> 2) + 4 * kl;
            if (ci < Cin && co < Cout) out[(size_t)ci * Cout + co] = acc[t][r];
        }
    }
}

// dw[co][ci][tap] = sum_split partial[split][tap][ci][co]
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, int splits, int Cin,
                                                           int Cout, float* __restrict__ dw) {
    // 64 consecutive elements (16 lanes x float4) x 16 interleaved split groups per block, folded through LDS in a fixed
    // order; up to four splits of a group are in flight at a time.  The partials of a layer are ~150 MB (1024 workgroup
    // tiles of the all-taps kernel): 16-byte loads and n / 64 blocks (>= 576 even for the 64 x 64 layer) read them at the HBM
    // rate where one float per lane and 4 groups managed 2.7 TB/s.  Summation order (fixed): split group g = sp mod 16 in
    // increasing sp, then a balanced tree over the 16 groups.
    __shared__ f32x4 sh[16][16];
    const long n = (long)9 * Cin * Cout;          // multiple of 4 (Cin, Cout multiples of 32)
    const int e = threadIdx.x & 15, g = threadIdx.x >> 4;
    for (long base = (long)blockIdx.x * 64; base < n; base += (long)gridDim.x * 64) {
        const long i = base + 4 * e;              // indexes partial layout [tap][ci][co] (coalesced reads)
        f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i < n) {
            const float* p = partial + i;
            int sp = g;
            for (; sp + 48 < splits; sp += 64) {
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(p + (size_t)sp * n);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(p + (size_t)(sp + 16) * n);
                const f32x4 v2 = *reinterpret_cast<const f32x4*>(p + (size_t)(sp + 32) * n);
                const f32x4 v3 = *reinterpret_cast<const f32x4*>(p + (size_t)(sp + 48) * n);
                s += v0; s += v1; s += v2; s += v3;
            }
            for (; sp < splits; sp += 16) s += *reinterpret_cast<const f32x4*>(p + (size_t)sp * n);
        }
        sh[g][e] = s;
        __syncthreads();
        if (g == 0 && i < n) {
            f32x4 t[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = sh[2 * q][e] + sh[2 * q + 1][e];
            const f32x4 r4 = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long iq = i + q;
                const int co = (int)(iq % Cout);
                const long r = iq / Cout;
                const int ci = (int)(r % Cin), tap = (int)(r / Cin);
                dw[((size_t)co * Cin + ci) * 9 + tap] = r4[q];
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void pack_weight_kernel(const float* __restrict__ w, float* __restrict__ wf,
                                                          float* __restrict__ wd, int Cin, int Cout) {
    const long n = (long)9 * Cin * Cout;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        // i indexes wf layout [tap][ci][co]
        const int co = (int)(i % Cout);
        const long r = i / Cout;
        const int ci = (int)(r % Cin), tap = (int)(r / Cin);
        const float v = w[((size_t)co * Cin + ci) * 9 + tap];
        wf[i] = v;
        if (wd) wd[((size_t)(8 - tap) * Cout + co) * Cin + ci] = v;   // flipped taps, (co,ci) swapped
    }
}

int wgrad_splits(long M, int Cin, int Cout, int TC) {
    // two full residency rounds of 768 workgroup slots (3 per CU): floor, so the last round is not a stub
    const int tiles = 9 * ((Cin + TC - 1) / TC) * ((Cout + TC - 1) / TC);
    long s = 1536 / tiles;
    const long maxs = (M + 32 * 16 - 1) / (32 * 16);   // at least 16 K-chunks per split
    if (s > maxs) s = maxs;
    if (s < 1) s = 1;
    return (int)s;
}
int wgrad_tile(int Cin, int Cout) { return (Cin >= 128 && Cout >= 128) ? 128 : 64; }

}  // namespace

// option conv_impl (read once): 0 = auto (halo-tile kernel when the width allows), 1 = tap-by-tap kernel
static int conv_impl() {
    static int v = -1;
    if (v < 0) v = tag_option("conv_impl");
    return v;
}



extern "C" int tag_pack_conv_weight(const float* w, float* wfwd, float* wdgrad, int Cin, int Cout, void* stream) {
    TAG_CHECK_ARG(w && wfwd && Cin > 0 && Cout > 0);
    const long n = (long)9 * Cin * Cout;
    hipLaunchKernelGGL(pack_weight_kernel, dim3(cdiv(n, 256) > 2048 ? 2048 : cdiv(n, 256)), dim3(256), 0,
                       as_stream(stream), w, wfwd, wdgrad, Cin, Cout);
    TAG_LAUNCH_CHECK();
    return 0;
}

template <int BN_>
static int launch_fwd(const float* x, const float* wp, int pro, const float* s, const float* t, float* y, int B, int H,
                      int W, int Cin, int Cout, hipStream_t st) {
    const long M = (long)B * H * W;
    const int grid = (int)((M + BM - 1) / BM) * ((Cout + BN_ - 1) / BN_);
    const size_t lds = (size_t)(TAG_NBUF * (BK * LDA + BK * BN_) + 2 * 512) * sizeof(float);   // + scale/shift table
#define LAUNCH_PRO(P)                                                                                            \
    {                                                                                                            \
        static bool attr_set = false;                                                                            \
        if (!attr_set) {                                                                                         \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_fwd_kernel<BN_, P>),                      \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                           \
            attr_set = true;                                                                                     \
        }                                                                                                        \
        hipLaunchKernelGGL((conv3x3_fwd_kernel<BN_, P>), dim3(grid), dim3(256), lds, st, x, wp, s, t, y, B, H, W, \
                           Cin, Cout);                                                                           \
    }
    switch (pro) {
        case 0: LAUNCH_PRO(0) break;
        case 1: LAUNCH_PRO(1) break;
        case 2: LAUNCH_PRO(2) break;
        default: LAUNCH_PRO(3) break;
    }
#undef LAUNCH_PRO
    return 0;
}

template <int BN_, int TW>
static void launch_halo(const float* x, const float* wp, int pro, const float* s, const float* t, float* y, float* stats,
                        const BnBwdEpi* epi, int B, int H, int W, int Cin, int Cout, hipStream_t st) {
    using G = HaloGeom<TW>;
    const int col_tiles = W / TW;                                          // 1, or 2 for the 64-wide images on 32-wide tiles
    const int row_tiles = ((H + G::TH - 1) / G::TH) * col_tiles, n_tiles = (Cout + BN_ - 1) / BN_;
    const int grid = B * row_tiles * n_tiles;
    auto magic = [](unsigned d, unsigned* mul, unsigned* shr) {            // n / d = (mulhi(n, mul) + n) >> shr for n < 2^31
        unsigned l = 0;
        while ((1u << l) < d) ++l;
        *shr = l;
        *mul = (unsigned)((((unsigned long long)1 << 32) * ((1ull << l) - d)) / d + 1);
    };
    unsigned nt_mul, nt_shr, rt_mul, rt_shr;
    magic((unsigned)n_tiles, &nt_mul, &nt_shr);
    magic((unsigned)row_tiles, &rt_mul, &rt_shr);
    // patch + weight buffer(s) + the producer BatchNorm table [2][Cin] (sized by Cin: at 64 cout with two weight buffers the
    // third workgroup of a CU fits only without the unused part of a 512-channel table)
    // TAG_HALO_LDS_PAD (environment, experiments only: tools/hybrid_probe.py): extra dynamic LDS per workgroup, i.e. FEWER workgroups
    // per CU, to leave registers for waves of another kernel
    static int lds_pad = -1;
    if (lds_pad < 0) lds_pad = tag_option("halo_lds_pad");
    const size_t lds = (size_t)(G::ASZ + 2 * halo_stage<BN_>() * BN_ + 2 * ((Cin + 3) / 4 * 4)) * sizeof(float) + (size_t)lds_pad;
#define LAUNCH_EPI(P, E)                                                                                          \
    {                                                                                                             \
        static bool attr_set = false;                                                                             \
        if (!attr_set) {                                                                                          \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_halo_kernel<BN_, P, TW, E>),         \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                      \
            attr_set = true;                                                                                      \
        }                                                                                                         \
        hipLaunchKernelGGL((conv3x3_halo_kernel<BN_, P, TW, E>), dim3(grid), dim3(256), lds, st, x, wp, s, t, y, stats, *epi, \
                           B, H, W, Cin, Cout, nt_mul, nt_shr, rt_mul, rt_shr, col_tiles);                        \
    }
    if (epi && epi->kind == 3) {   // inference forward: BatchNorm(eval) + ReLU + pool from the parked tile (producer prologue 0 | 1)
        if (pro == 1) LAUNCH_EPI(1, 3) else LAUNCH_EPI(0, 3)
        return;
    }
    if (epi && epi->kind == 2) {   // dgrad + the sums of the BatchNorm+ReLU+pool backward below it: no producer prologue on this path
        LAUNCH_EPI(0, 2)
        return;
    }
    if (epi) {                     // dgrad + BatchNorm-backward sums: no producer prologue on this path
        LAUNCH_EPI(0, 1)
        return;
    }
#undef LAUNCH_EPI
    const BnBwdEpi none{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0ull, 0};
#define LAUNCH_PRO(P)                                                                                             \
    {                                                                                                             \
        static bool attr_set = false;                                                                             \
        if (!attr_set) {                                                                                          \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_halo_kernel<BN_, P, TW>),            \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                      \
            attr_set = true;                                                                                      \
        }                                                                                                         \
        hipLaunchKernelGGL((conv3x3_halo_kernel<BN_, P, TW>), dim3(grid), dim3(256), lds, st, x, wp, s, t, y, stats, \
                           none, B, H, W, Cin, Cout, nt_mul, nt_shr, rt_mul, rt_shr, col_tiles);                             \
    }
    switch (pro) {
        case 0: LAUNCH_PRO(0) break;
        case 1: LAUNCH_PRO(1) break;
        case 2: LAUNCH_PRO(2) break;
        default: LAUNCH_PRO(3) break;
    }
#undef LAUNCH_PRO
}

// 256-cout workgroups (2 per CU, 252 VGPRs) for the narrow deep layers (W <= 16, Cout a multiple of 256): the same rate as the
// 128-cout tile at 3 per CU (tools/conv_bench.py: 135.1 vs 135.0, 135.7 vs 135.9 TFLOP/s) with HALF the patch re-reads and weight
// passes through L2 -- in the TRAINING step, where the time is level (53.22 / 53.32 vs 53.27 / 53.34 ms).  The forward-only 30 s
// inference pass is 1.3 % slower with them (216 vs 213 ms per 256 clips), so launches that neither write BatchNorm statistics nor carry
// a backward epilogue keep the 128-cout tiles.  TAG_HALO_BN256=0: 128-cout tiles everywhere, =2: 256-cout tiles everywhere (A/B).
static bool halo_bn256(int W, int Cout, bool training_launch) {
    static int on = -1;
    if (on < 0) on = tag_option("halo_bn256");
    return (on == 2 || (on == 1 && training_launch)) && W <= 16 && Cout % 256 == 0;
}

// rows of BatchNorm partial statistics the forward kernel writes when asked to (one per 64-pixel wave tile);
// 0 = this shape is served by a kernel without the fused statistics
extern "C" int tag_conv3x3_stats_rows(int B, int H, int W, int Cout) {
    (void)Cout;
    if (!(conv_impl() == 0 && (W == 4 || W == 8 || W == 16 || W == 32 || W == 64))) return 0;
    const int tw = W == 64 ? 32 : W, th = 128 / tw;             // 64-wide images: two 4 x 32 tile columns
    return B * ((H + th - 1) / th) * (W / tw) * 2;
}

extern "C" int tag_conv3x3_forward(const float* x, const float* wpack, int prologue, const float* in_scale,
                                   const float* in_shift, float* y, float* stats, int B, int H, int W, int Cin,
                                   int Cout, void* stream) {
    TAG_CHECK_ARG(x && wpack && y && B > 0 && H > 0 && W > 0);
    TAG_CHECK_ARG(Cin % 32 == 0 && Cout % 4 == 0 && Cin <= 512);
    TAG_CHECK_ARG(prologue >= 0 && prologue <= 3);
    TAG_CHECK_ARG(prologue == 0 || (in_scale && in_shift));
    hipStream_t st = as_stream(stream);
    // (W == 4: the last two layers of CrnnEncoder, 125 x 4 images as 32 x 4 tiles -- round 5; the epilogue entry points below keep W >= 8)
    const bool halo = conv_impl() == 0 && (W == 4 || W == 8 || W == 16 || W == 32 || W == 64);
    // 32-bit byte offsets: inside ONE image for the halo-tile kernel (64-bit image base), over the whole batch for the fallback
    TAG_CHECK_ARG((long)B * H * W < (1L << 31) && (long)H * W * Cin * 4 < (1L << 32));
    TAG_CHECK_ARG(halo || (long)B * H * W * Cin * 4 < (1L << 32));
    TAG_CHECK_ARG(stats == nullptr || halo);
#define EPI_PTR nullptr
#define HALO_BY_W(BN_)                                                                                          \
    if (W == 4) launch_halo<BN_, 4>(x, wpack, prologue, in_scale, in_shift, y, stats, EPI_PTR, B, H, W, Cin, Cout, st);        \
    else if (W == 8) launch_halo<BN_, 8>(x, wpack, prologue, in_scale, in_shift, y, stats, EPI_PTR, B, H, W, Cin, Cout, st);   \
    else if (W == 16) launch_halo<BN_, 16>(x, wpack, prologue, in_scale, in_shift, y, stats, EPI_PTR, B, H, W, Cin, Cout, st); \
    else if (W == 32) launch_halo<BN_, 32>(x, wpack, prologue, in_scale, in_shift, y, stats, EPI_PTR, B, H, W, Cin, Cout, st); \
    else launch_halo<BN_, 32>(x, wpack, prologue, in_scale, in_shift, y, stats, EPI_PTR, B, H, W, Cin, Cout, st);   /* W == 64: two tile columns */
    if (halo) {
        if (halo_bn256(W, Cout, stats != nullptr)) { HALO_BY_W(256) } else if (Cout >= 128) { HALO_BY_W(128) } else { HALO_BY_W(64) }
    } else if (Cout >= 128) {
        launch_fwd<128>(x, wpack, prologue, in_scale, in_shift, y, B, H, W, Cin, Cout, st);
    } else {
        launch_fwd<64>(x, wpack, prologue, in_scale, in_shift, y, B, H, W, Cin, Cout, st);
    }
#undef EPI_PTR
    TAG_LAUNCH_CHECK();
    return 0;
}

// Launch of the EPI == 4 instances: the 128-cout tile of tag_conv3x3_forward's statistics-free launch (same geometry, LDS size and
// summation order, so an all-zero bias gives that entry's output bit for bit), prologues 2 and 3.
template <int TW>
static void launch_halo_bias(const float* x, const float* wp, int pro, const float* s, const float* t, const float* bias, float* y,
                             int B, int H, int W, int Cin, int Cout, hipStream_t st) {
    constexpr int BN_ = 128;
    using G = HaloGeom<TW>;
    const int col_tiles = W / TW;
    const int row_tiles = ((H + G::TH - 1) / G::TH) * col_tiles, n_tiles = (Cout + BN_ - 1) / BN_;
    const int grid = B * row_tiles * n_tiles;
    auto magic = [](unsigned d, unsigned* mul, unsigned* shr) {            // n / d = (mulhi(n, mul) + n) >> shr for n < 2^31
        unsigned l = 0;
        while ((1u << l) < d) ++l;
        *shr = l;
        *mul = (unsigned)((((unsigned long long)1 << 32) * ((1ull << l) - d)) / d + 1);
    };
    unsigned nt_mul, nt_shr, rt_mul, rt_shr;
    magic((unsigned)n_tiles, &nt_mul, &nt_shr);
    magic((unsigned)row_tiles, &rt_mul, &rt_shr);
    const size_t lds = (size_t)(G::ASZ + 2 * halo_stage<BN_>() * BN_ + 2 * ((Cin + 3) / 4 * 4)) * sizeof(float);
    const BnBwdEpi epi{bias, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0ull, 4};
#define LAUNCH_BIAS(P)                                                                                            \
    {                                                                                                             \
        static bool attr_set = false;                                                                             \
        if (!attr_set) {                                                                                          \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_halo_kernel<BN_, P, TW, 4>),         \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                      \
            attr_set = true;                                                                                      \
        }                                                                                                         \
        hipLaunchKernelGGL((conv3x3_halo_kernel<BN_, P, TW, 4>), dim3(grid), dim3(256), lds, st, x, wp, s, t, y,  \
                           (float*)nullptr, epi, B, H, W, Cin, Cout, nt_mul, nt_shr, rt_mul, rt_shr, col_tiles);  \
    }
    if (pro == 2) LAUNCH_BIAS(2) else LAUNCH_BIAS(3)
#undef LAUNCH_BIAS
}

// y = conv(prologue(x)) + bias[b, cout], bias (B, Cout): the conv of a CDurTextBlock (models/audio_text_model.py:461-479), the
// text added in the kernel's epilogue.  Served: the halo-tile kernel at W = 16 or 4, Cin 32 or 128, Cout 128, prologue 2
// (BatchNorm after LeakyReLU) or 3 (BatchNorm alone); anything else is TAG_EINVAL.  No BatchNorm statistics.
extern "C" int tag_conv3x3_forward_bias(const float* x, const float* wpack, int prologue, const float* in_scale,
                                        const float* in_shift, const float* bias, float* y, int B, int H, int W, int Cin,
                                        int Cout, void* stream) {
    TAG_CHECK_ARG(x && wpack && bias && y && in_scale && in_shift && B > 0 && H > 0);
    if (!(conv_impl() == 0 && (W == 16 || W == 4) && (Cin == 32 || Cin == 128) && Cout == 128 && (prologue == 2 || prologue == 3))) {
        tag_set_error("%s", "tag_conv3x3_forward_bias: unserved shape (W 16 | 4, Cin 32 | 128, Cout 128, prologue 2 | 3, halo-tile kernel)");
        return TAG_EINVAL;
    }
    TAG_CHECK_ARG((long)B * H * W < (1L << 31) && (long)H * W * Cin * 4 < (1L << 32));
    hipStream_t st = as_stream(stream);
    if (W == 4) launch_halo_bias<4>(x, wpack, prologue, in_scale, in_shift, bias, y, B, H, W, Cin, Cout, st);
    else launch_halo_bias<16>(x, wpack, prologue, in_scale, in_shift, bias, y, B, H, W, Cin, Cout, st);
    TAG_LAUNCH_CHECK();
    return 0;
}

// dgrad convolution + the reduction half of the BatchNorm+ReLU backward its output flows into (see the EPI == 1 epilogue).
// Only the halo-tile kernel has it: widths 8/16/32/64 (tag_conv3x3_stats_rows > 0); other shapes use tag_conv3x3_forward +
// tag_bnrelu_backward.
extern "C" int tag_conv3x3_dgrad_bnsums(const float* dy, const float* wpack, float* da, const float* yref,
                                        const float* bn_scale, const float* bn_shift, const float* bn_mean,
                                        const float* bn_invstd, float* bnpart, int B, int H, int W, int Cin, int Cout,
                                        void* stream) {
    TAG_CHECK_ARG(dy && wpack && da && yref && bn_scale && bn_shift && bn_mean && bn_invstd && bnpart);
    TAG_CHECK_ARG(B > 0 && H > 0 && Cin % 32 == 0 && Cout % 4 == 0 && Cin <= 512);
    TAG_CHECK_ARG((long)B * H * W < (1L << 31) && (long)H * W * Cin * 4 < (1L << 32));
    TAG_CHECK_ARG(conv_impl() == 0 && (W == 8 || W == 16 || W == 32 || W == 64));
    hipStream_t st = as_stream(stream);
    const BnBwdEpi epi{yref, bn_scale, bn_shift, bn_mean, bn_invstd, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0ull, 1};
    const float* x = dy;
    float* y = da;
    float* stats = bnpart;
    const int prologue = 0;
    const float *in_scale = nullptr, *in_shift = nullptr;
#define EPI_PTR (&epi)
    if (halo_bn256(W, Cout, true)) { HALO_BY_W(256) } else if (Cout >= 128) { HALO_BY_W(128) } else { HALO_BY_W(64) }
#undef EPI_PTR
    TAG_LAUNCH_CHECK();
    return 0;
}

// dgrad convolution of a block's FIRST conv + the reduction half of the backward of the block BELOW it: the conv's output dx
// (B,H,W,Cout) is the gradient of relu(bn(yref)) -> pool(ph x pw, floor) -> dropout(drop_p, seed) with yref (B,Hf,Wf,Cout),
// H = Hf / ph, W = Wf / pw (see the EPI == 2 epilogue).  bnpart: tag_conv3x3_stats_rows(B,H,W,Cout) rows of [2][Cout]
// (sum dz | sum dz * xhat) for tag_bn_grad_from_partials; tag_bnrelu_pool_backward_apply then writes dy from dx and the sums.
// Windows ph x 2 with ph = 1 or 2 (the Cnn8Rnn pools); other windows keep the separate reduction (tag_bnrelu_pool_backward).
extern "C" int tag_conv3x3_dgrad_poolsums(const float* dy, const float* wpack, float* dx, const float* yref,
                                          const float* bn_scale, const float* bn_shift, const float* bn_mean,
                                          const float* bn_invstd, float* bnpart, int B, int H, int W, int Cin, int Cout, int Hf,
                                          int Wf, int ph, int pw, int pool, float drop_p, uint64_t seed, void* stream) {
    TAG_CHECK_ARG(dy && wpack && dx && yref && bn_scale && bn_shift && bn_mean && bn_invstd && bnpart);
    TAG_CHECK_ARG(B > 0 && H > 0 && Cin % 32 == 0 && Cout % 4 == 0 && Cin <= 512);
    TAG_CHECK_ARG((long)B * H * W < (1L << 31) && (long)H * W * Cin * 4 < (1L << 32) && (long)B * Hf * Wf < (1L << 31));
    TAG_CHECK_ARG(conv_impl() == 0 && (W == 8 || W == 16 || W == 32 || W == 64));
    TAG_CHECK_ARG(pw == 2 && (ph == 1 || ph == 2) && H == Hf / ph && W == Wf / pw);
    TAG_CHECK_ARG((pool == 0 || pool == 2 || pool == 3) && drop_p >= 0.0f && drop_p < 1.0f);
    hipStream_t st = as_stream(stream);
    const float wavg = pool == 3 ? 0.0f : 1.0f / (float)(ph * pw), wmax = pool == 2 ? 0.0f : 1.0f;
    const BnBwdEpi epi{yref, bn_scale, bn_shift, bn_mean, bn_invstd, Hf, Wf, ph, wavg, wmax, drop_p, (unsigned long long)seed, 2};
    const float* x = dy;
    float* y = dx;
    float* stats = bnpart;
    const int prologue = 0;
    const float *in_scale = nullptr, *in_shift = nullptr;
#define EPI_PTR (&epi)
    if (halo_bn256(W, Cout, true)) { HALO_BY_W(256) } else if (Cout >= 128) { HALO_BY_W(128) } else { HALO_BY_W(64) }
#undef EPI_PTR
    TAG_LAUNCH_CHECK();
    return 0;
}

// Inference forward of a conv + the rest of its ConvBlock stage (models/panns.py:49-60 with BatchNorm in eval mode):
// out (B, H/ph, W/pw, Cout) = pool(relu(conv(prologue(x)) * bn_scale + bn_shift)), window ph x 2 (ph 1 | 2), floor; the raw conv output
// is never materialised (EPI == 3).  Bit-identical to tag_conv3x3_forward + tag_bnact_pool_forward(act 1, no dropout).
extern "C" int tag_conv3x3_forward_bnrelu_pool_eval(const float* x, const float* wpack, int prologue, const float* in_scale,
                                                    const float* in_shift, float* out, const float* bn_scale,
                                                    const float* bn_shift, int B, int H, int W, int Cin, int Cout, int ph, int pw,
                                                    int pool, void* stream) {
    TAG_CHECK_ARG(x && wpack && out && bn_scale && bn_shift && B > 0 && H > 0);
    TAG_CHECK_ARG(Cin % 32 == 0 && Cout % 4 == 0 && Cin <= 512 && (prologue == 0 || prologue == 1));
    TAG_CHECK_ARG(prologue == 0 || (in_scale && in_shift));
    TAG_CHECK_ARG((long)B * H * W < (1L << 31) && (long)H * W * Cin * 4 < (1L << 32));
    TAG_CHECK_ARG(conv_impl() == 0 && (W == 8 || W == 16 || W == 32 || W == 64));
    TAG_CHECK_ARG(pw == 2 && (ph == 1 || ph == 2) && H / ph > 0 && (pool == 0 || pool == 2 || pool == 3));
    hipStream_t st = as_stream(stream);
    const float wavg = pool == 3 ? 0.0f : 1.0f / (float)(ph * pw), wmax = pool == 2 ? 0.0f : 1.0f;
    const BnBwdEpi epi{nullptr, bn_scale, bn_shift, nullptr, nullptr, 0, 0, ph, wavg, wmax, 0.0f, 0ull, 3};
    float* y = out;
    float* stats = nullptr;
#define EPI_PTR (&epi)
    if (halo_bn256(W, Cout, false)) { HALO_BY_W(256) } else if (Cout >= 128) { HALO_BY_W(128) } else { HALO_BY_W(64) }
#undef EPI_PTR
#undef HALO_BY_W
    TAG_LAUNCH_CHECK();
    return 0;
}

static bool wgrad_alltaps_ok(int W) { return conv_impl() == 0 && (W == 4 || W == 8 || W == 16 || W == 32 || W == 64); }
// all-taps kernel: K slices (in chunks of 32 pixels) so that ~512 workgroups (ONE round of 2 per CU) are launched: against
// two rounds the fp32 kernels are level (16.00 -> 15.88 ms per step), the bf16 kernels gain 6 % (2.55 -> 2.41 ms) and the
// fp32 partials every layer writes and the reduction re-reads halve (151 -> 75 MB per layer, 2.1 -> 1.05 GB per step)
static int alltaps_splits(int B, int H, int W, int Cin, int Cout, int* chunks_per_split, int chunk_px = 32) {
    const int cw = W >= 32 ? 32 : W, ch = chunk_px / cw;
    const int chunks = B * ((H + ch - 1) / ch) * (W / cw);
    const int tiles = ((Cin + 63) / 64) * ((Cout + 63) / 64);
    static int target = 0;                                      // TAG_WGRAD_WGS (environment): workgroups per launch, A/B timing
    if (target == 0) { target = tag_option("wgrad_wgs"); if (target < 64) target = 512; }
    int s = target / tiles;
    if (s > chunks / 8) s = chunks / 8;
    if (s < 1) s = 1;
    *chunks_per_split = (chunks + s - 1) / s;
    return (chunks + *chunks_per_split - 1) / *chunks_per_split;
}

// shared with conv_x3.hip (same K split and the same deterministic reduction)
int tag_wgrad_alltaps_splits(int B, int H, int W, int Cin, int Cout, int* chunks_per_split, int chunk_px) {
    return alltaps_splits(B, H, W, Cin, Cout, chunks_per_split, chunk_px);
}
int tag_launch_wgrad_reduce(const float* partial, int splits, int Cin, int Cout, float* dw, hipStream_t st) {
    const long nred = (long)9 * Cin * Cout;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(nred, 64) > 8192 ? 8192 : cdiv(nred, 64)), dim3(256), 0, st,
                       partial, splits, Cin, Cout, dw);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t tag_conv3x3_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout) {
    const long M = (long)B * H * W;
    if (wgrad_alltaps_ok(W)) {
        int cps;
        return (size_t)alltaps_splits(B, H, W, Cin, Cout, &cps) * 9 * Cin * Cout * sizeof(float);
    }
    const int TC = wgrad_tile(Cin, Cout);
    return (size_t)wgrad_splits(M, Cin, Cout, TC) * 9 * Cin * Cout * sizeof(float);
}

// narrowest image width that takes the row-ring kernel.  Measured over the layer shapes: W = 32 / 64 gain 4-5 % (one new row of 34
// pixels instead of a 3 x 34 patch per chunk), W = 16 0.6 %, W = 8 LOSES 1.5 % (4 new rows of 10 pixels against a 6 x 10 patch:
// the ring's per-item slot arithmetic costs more than the 20 pixels it saves)
#ifndef TAG_WGRAD_RING_MINW
#define TAG_WGRAD_RING_MINW 16
#endif
template <int TW>
static void launch_wgrad_alltaps(const float* x, int pro, const float* s, const float* t, const float* dy, float* partial,
                                 int B, int H, int W, int Cin, int Cout, int splits, int cps, hipStream_t st) {
    using G = WgGeom<TW>;
    const int grid = ((Cin + 63) / 64) * ((Cout + 63) / 64) * splits;
    constexpr bool RING = TW >= TAG_WGRAD_RING_MINW;                       // row-ring kernel; the full-patch form below that width
    constexpr int RCW = TW >= 32 ? 32 : TW, RCH = 32 / RCW;
    const size_t lds = RING ? (size_t)((2 * RCH + 2) * (RCW + 2) * 64 + 64 + 2 * 32 * 64) * sizeof(float)
                            : (size_t)2 * ((G::PP + 1) * 64 + 32 * 64) * sizeof(float);
#define LAUNCH_PRO(P)                                                                                               \
    {                                                                                                               \
        static bool attr_set = false;                                                                               \
        if (!attr_set) {                                                                                            \
            if (RING) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_wgrad_rowring_kernel<TW, P>), \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                        \
            else (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_wgrad_alltaps_kernel<TW, P>),     \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                        \
            attr_set = true;                                                                                        \
        }                                                                                                           \
        if (RING) hipLaunchKernelGGL((conv3x3_wgrad_rowring_kernel<TW, P>), dim3(grid), dim3(256), lds, st, x, s, t, \
                           dy, partial, B, H, W, Cin, Cout, splits, cps);                                           \
        else hipLaunchKernelGGL((conv3x3_wgrad_alltaps_kernel<TW, P>), dim3(grid), dim3(256), lds, st, x, s, t, dy, partial, \
                           B, H, W, Cin, Cout, splits, cps);                                                        \
    }
    switch (pro) {
        case 0: LAUNCH_PRO(0) break;
        case 1: LAUNCH_PRO(1) break;
        case 2: LAUNCH_PRO(2) break;
        default: LAUNCH_PRO(3) break;
    }
#undef LAUNCH_PRO
}

template <int TC>
static void launch_wgrad(const float* x, int pro, const float* s, const float* t, const float* dy, float* partial,
                         int B, int H, int W, int Cin, int Cout, int splits, long chunk, hipStream_t st) {
    const int grid = 9 * ((Cin + TC - 1) / TC) * ((Cout + TC - 1) / TC) * splits;
    const size_t lds = (size_t)(TAG_NBUF * 2 * BK * TC) * sizeof(float);
#define LAUNCH_PRO(P)                                                                                              \
    {                                                                                                              \
        static bool attr_set = false;                                                                              \
        if (!attr_set) {                                                                                           \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_wgrad_kernel<TC, P>),                       \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                             \
            attr_set = true;                                                                                       \
        }                                                                                                          \
        hipLaunchKernelGGL((conv3x3_wgrad_kernel<TC, P>), dim3(grid), dim3(256), lds, st, x, s, t, dy, partial, B, \
                           H, W, Cin, Cout, splits, chunk);                                                        \
    }
    switch (pro) {
        case 0: LAUNCH_PRO(0) break;
        case 1: LAUNCH_PRO(1) break;
        case 2: LAUNCH_PRO(2) break;
        default: LAUNCH_PRO(3) break;
    }
#undef LAUNCH_PRO
}

extern "C" int tag_conv3x3_wgrad(const float* x, int prologue, const float* in_scale, const float* in_shift,
                                 const float* dy, float* dw, int B, int H, int W, int Cin, int Cout, void* ws,
                                 void* stream) {
    TAG_CHECK_ARG(x && dy && dw && ws && B > 0 && H > 0 && W > 0);
    TAG_CHECK_ARG(Cin % 4 == 0 && Cout % 4 == 0 && prologue >= 0 && prologue <= 3);
    TAG_CHECK_ARG(prologue == 0 || (in_scale && in_shift));
    const long M = (long)B * H * W;
    // the all-taps kernel keeps a 64-bit image base and 32-bit byte offsets inside ONE image; the per-tap fallback keeps 32-bit
    // byte offsets over the batch
    TAG_CHECK_ARG(M < (1L << 31) && W <= 64);
    TAG_CHECK_ARG((long)H * W * Cin * 4 < (1L << 32) && (long)H * W * Cout * 4 < (1L << 32));
    TAG_CHECK_ARG(wgrad_alltaps_ok(W) || (M * Cin * 4 < (1L << 32) && M * Cout * 4 < (1L << 32)));
    float* partial = static_cast<float*>(ws);
    hipStream_t st = as_stream(stream);
    const long nred = (long)9 * Cin * Cout;
    if (wgrad_alltaps_ok(W)) {
        int cps;
        const int sp = alltaps_splits(B, H, W, Cin, Cout, &cps);
        if (W == 4) launch_wgrad_alltaps<4>(x, prologue, in_scale, in_shift, dy, partial, B, H, W, Cin, Cout, sp, cps, st);
        else if (W == 8) launch_wgrad_alltaps<8>(x, prologue, in_scale, in_shift, dy, partial, B, H, W, Cin, Cout, sp, cps, st);
        else if (W == 16) launch_wgrad_alltaps<16>(x, prologue, in_scale, in_shift, dy, partial, B, H, W, Cin, Cout, sp, cps, st);
        else if (W == 32) launch_wgrad_alltaps<32>(x, prologue, in_scale, in_shift, dy, partial, B, H, W, Cin, Cout, sp, cps, st);
        else launch_wgrad_alltaps<64>(x, prologue, in_scale, in_shift, dy, partial, B, H, W, Cin, Cout, sp, cps, st);
        TAG_LAUNCH_CHECK();
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(nred, 64) > 8192 ? 8192 : cdiv(nred, 64)), dim3(256), 0, st,
                           partial, sp, Cin, Cout, dw);
        TAG_LAUNCH_CHECK();
        return 0;
    }
    const int TC = wgrad_tile(Cin, Cout);
    const int splits = wgrad_splits(M, Cin, Cout, TC);
    long chunk = (M + splits - 1) / splits;
    chunk = (chunk + BK - 1) / BK * BK;
    if (TC == 128)
        launch_wgrad<128>(x, prologue, in_scale, in_shift, dy, partial, B, H, W, Cin, Cout, splits, chunk,
                          as_stream(stream));
    else
        launch_wgrad<64>(x, prologue, in_scale, in_shift, dy, partial, B, H, W, Cin, Cout, splits, chunk,
                         as_stream(stream));
    TAG_LAUNCH_CHECK();
    const long n = (long)9 * Cin * Cout;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(n, 64) > 8192 ? 8192 : cdiv(n, 64)), dim3(256), 0,
                       as_stream(stream), partial, splits, Cin, Cout, dw);
    TAG_LAUNCH_CHECK();
    return 0;
}

#ifdef TAG_HALO_PROF
extern "C" int tag_debug_get_halo_prof(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(tag_halo_prof), 56) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out + 7, HIP_SYMBOL(tag_halo_sub), 32) == hipSuccess ? 0 : -1;
}
extern "C" int tag_debug_get_halo_wg(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(tag_halo_wg), sizeof(unsigned long long) * 4 * 65536) == hipSuccess ? 0 : -1;
}
#endif
