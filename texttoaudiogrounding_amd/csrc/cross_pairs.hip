// AudioTextCrossAlignByPhrase (models/audio_text_model.py:979-1073 in the reference): every clip of the batch cross-encoded
// against every phrase of the batch -- CrossAttentionGating (models/cross_encoder.py:5-79) + match.DotProduct(text_level="token")
// over ALL (clip i, phrase p) pairs, forward and backward, without ever forming a (B,P,T,D) tensor.
//
// The host projects once with tag_gemm: aq = a Wq^T (B,T,D), ak = w Wk^T + b_h (P,L,D), gu = sigmoid(a Wu^T + b_u) (B,T,D) and
// ws = w Ws^T (P,L,D) -- the attention weights sum to 1, so fc_s(attn @ tok) = attn @ (tok Ws^T) + b_s.  What is left per
// row r = (clip i, phrase p, frame t) is local to that row:
//     s_l = v . tanh(aq[i,t] + ak[p,l])   (-1e10 where t >= alen[i] or l >= wlen[p]),   alpha = softmax_l(s),
//     c = sum_l alpha_l w[p,l],   z = sum_l alpha_l ws[p,l] + b_s,   u = a[i,t] * sigmoid(z),   s = c * gu[i,t],
//     sim = clamp(sigmoid(u . s [/ sqrt D]), 1e-7, 1).
// Forward: one wave per row, D over the lanes; it keeps alpha (B,P,T,L) and the row's d sim / d (u.s) factor (B,P,T).
// Backward, in three steps that all work on the compact (B,P,T) row order:
//   1. dscore (B,P,T,L): one wave per row -- the softmax backward needs L dot products over D per row (no tanh);
//   2. frame side: one wave per (i,t) walks ALL phrases in index order and leaves daq, da (through u) and dgu final;
//   3. token side: one thread per (phrase, d) holds ak, w, ws of its phrase in registers, walks a chunk of the B*T frames and
//      leaves per-chunk partials of dak, dw (through c), dws, dv, db_s, which fold kernels add in chunk order.
// Steps 2 and 3 each recompute the tanh (a saved tanh would be a (B,P,T,L,D) tensor); dscore is saved between them because
// it is the only part of the backward that needs a reduction over D.  No atomics: every sum has one fixed order.
// The (B,P,T) rows are moved to / from the (B,B,N,T) matrix by one strided copy per text clip j (its pnum[j] phrases are
// contiguous in both layouts); pnum is read on the host, so the kernels never index by it.
#include "tag_common.h"

namespace {

constexpr int MAXL = 32;            // tokens per phrase
constexpr int MAXD = 1024;
constexpr int TOK_CHUNKS = 8;       // token side: at most this many chunks of frames per phrase ...
constexpr int TOK_CHUNK_MIN = 64;   // ... of at least this many frames each
constexpr float FILL = -1e10f;

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// backward of u = a * g, s = c * gu, y = u . s through one element d, given dy = d loss / d (u . s)
struct GateGrad {
    float dc, dz, da, dgu;
};
__device__ __forceinline__ GateGrad gate_grad(float a, float gu, float c, float z, float dy) {
    const float g = sigm(z), u = a * g, s = c * gu;
    GateGrad r;
    r.dc = dy * u * gu;                       // through s = c * gu
    r.dz = dy * s * a * g * (1.0f - g);       // through u = a * sigmoid(z)
    r.da = dy * s * g;
    r.dgu = dy * u * c;
    return r;
}

struct Row {
    int i, p, t;
    long frame;      // i * T + t
};
__device__ __forceinline__ Row split_row(long row, int P, int T) {
    Row r;
    r.i = (int)(row / ((long)P * T));
    const long rem = row % ((long)P * T);
    r.p = (int)(rem / T);
    r.t = (int)(rem % T);
    r.frame = (long)r.i * T + r.t;
    return r;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// lane k's value, as a wave-uniform scalar
__device__ __forceinline__ float lane_value(float v, int k) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(__shfl(v, k, 64))));
}

// One wave per row (i,p,t); lane l < L holds score / alpha l.  64 * ND bounds D.
template <int ND>
__global__ __launch_bounds__(256) void cp_fwd_kernel(const float* __restrict__ a, const float* __restrict__ aq,
                                                     const float* __restrict__ gu, const float* __restrict__ w,
                                                     const float* __restrict__ ak, const float* __restrict__ wst,
                                                     const float* __restrict__ v, const float* __restrict__ bs,
                                                     const long* __restrict__ alen, const long* __restrict__ wlen,
                                                     float* __restrict__ simp, float* __restrict__ alpha,
                                                     float* __restrict__ dyfac, int B, int T, int P, int L, int D,
                                                     float scale) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)B * P * T) return;
    const Row r = split_row(row, P, T);
    const bool qok = r.t < alen[r.i];
    const long kl = wlen[r.p];
    const float* akp = ak + (size_t)r.p * L * D;
    const float* wp = w + (size_t)r.p * L * D;
    const float* wsp = wst + (size_t)r.p * L * D;
    float score = FILL;
    if (qok) {
        float aqv[ND], vv[ND];
#pragma unroll
        for (int n = 0; n < ND; ++n) {
            const int d = lane + 64 * n;
            aqv[n] = d < D ? aq[r.frame * D + d] : 0.0f;
            vv[n] = d < D ? v[d] : 0.0f;
        }
        for (int k = 0; k < L && k < kl; ++k) {
            float s = 0.0f;
#pragma unroll
            for (int n = 0; n < ND; ++n) {
                const int d = lane + 64 * n;
                if (d < D) s = fmaf(vv[n], tanhf(aqv[n] + akp[(size_t)k * D + d]), s);
            }
            s = wave_sum(s);
            if (lane == k) score = s;
        }
    }
    const bool act = lane < L;
    const float mx = wave_max(act ? score : -3.0e38f);
    const float ex = act ? expf(score - mx) : 0.0f;
    const float al_l = ex * (1.0f / wave_sum(ex));
    if (act) alpha[row * L + lane] = al_l;
    float c[ND], z[ND];
#pragma unroll
    for (int n = 0; n < ND; ++n) c[n] = z[n] = 0.0f;
    for (int k = 0; k < L; ++k) {
        const float al = lane_value(al_l, k);
        if (al == 0.0f) continue;
#pragma unroll
        for (int n = 0; n < ND; ++n) {
            const int d = lane + 64 * n;
            if (d < D) {
                c[n] = fmaf(al, wp[(size_t)k * D + d], c[n]);
                z[n] = fmaf(al, wsp[(size_t)k * D + d], z[n]);
            }
        }
    }
    float dot = 0.0f;
#pragma unroll
    for (int n = 0; n < ND; ++n) {
        const int d = lane + 64 * n;
        if (d < D) {
            const float u = a[r.frame * D + d] * sigm(z[n] + bs[d]);
            dot = fmaf(u, c[n] * gu[r.frame * D + d], dot);
        }
    }
    dot = wave_sum(dot) * scale;
    const float p = sigm(dot);
    if (lane == 0) {
        simp[row] = fminf(fmaxf(p, 1e-7f), 1.0f);
        const float pass = (p >= 1e-7f && p <= 1.0f) ? 1.0f : 0.0f;          // clamp backward
        dyfac[row] = pass * p * (1.0f - p) * scale;
    }
}

// dscore[row, l] = alpha_l (dalpha_l - sum_m alpha_m dalpha_m), 0 at the filled scores; one wave per row, lane l holds token l
template <int ND>
__global__ __launch_bounds__(256) void cp_dscore_kernel(const float* __restrict__ a, const float* __restrict__ gu,
                                                        const float* __restrict__ w, const float* __restrict__ wst,
                                                        const float* __restrict__ bs, const long* __restrict__ alen,
                                                        const long* __restrict__ wlen, const float* __restrict__ alpha,
                                                        const float* __restrict__ dyfac, const float* __restrict__ dsimp,
                                                        float* __restrict__ dscore, int B, int T, int P, int L, int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)B * P * T) return;
    const Row r = split_row(row, P, T);
    const bool qok = r.t < alen[r.i];
    const long kl = wlen[r.p];
    const float dy = dsimp[row] * dyfac[row];
    if (!qok || kl <= 0 || dy == 0.0f) {           // a fully filled row passes no score gradient
        if (lane < L) dscore[row * L + lane] = 0.0f;
        return;
    }
    const float* wp = w + (size_t)r.p * L * D;
    const float* wsp = wst + (size_t)r.p * L * D;
    const float al_l = lane < L ? alpha[row * L + lane] : 0.0f;
    float dc[ND], dz[ND];
#pragma unroll
    for (int n = 0; n < ND; ++n) dc[n] = dz[n] = 0.0f;       // c, z first
    for (int k = 0; k < L; ++k) {
        const float al = lane_value(al_l, k);
        if (al == 0.0f) continue;
#pragma unroll
        for (int n = 0; n < ND; ++n) {
            const int d = lane + 64 * n;
            if (d < D) {
                dc[n] = fmaf(al, wp[(size_t)k * D + d], dc[n]);
                dz[n] = fmaf(al, wsp[(size_t)k * D + d], dz[n]);
            }
        }
    }
#pragma unroll
    for (int n = 0; n < ND; ++n) {
        const int d = lane + 64 * n;
        if (d < D) {
            const GateGrad g = gate_grad(a[r.frame * D + d], gu[r.frame * D + d], dc[n], dz[n] + bs[d], dy);
            dc[n] = g.dc;
            dz[n] = g.dz;
        }
    }
    float dal_l = 0.0f;
    for (int k = 0; k < L; ++k) {
        float s = 0.0f;
#pragma unroll
        for (int n = 0; n < ND; ++n) {
            const int d = lane + 64 * n;
            if (d < D) {
                s = fmaf(dc[n], wp[(size_t)k * D + d], s);
                s = fmaf(dz[n], wsp[(size_t)k * D + d], s);
            }
        }
        s = wave_sum(s);
        if (lane == k) dal_l = s;
    }
    const float dot_all = wave_sum(al_l * dal_l);
    if (lane < L) dscore[row * L + lane] = lane < kl ? al_l * (dal_l - dot_all) : 0.0f;
}

// Frame side: one wave per (i,t) walks the phrases p = 0 .. P-1 in order; daq, da (through u), dgu (B,T,D) are final
template <int ND>
__global__ __launch_bounds__(256) void cp_frame_bwd_kernel(const float* __restrict__ a, const float* __restrict__ aq,
                                                           const float* __restrict__ gu, const float* __restrict__ w,
                                                           const float* __restrict__ ak, const float* __restrict__ wst,
                                                           const float* __restrict__ v, const float* __restrict__ bs,
                                                           const long* __restrict__ alen, const long* __restrict__ wlen,
                                                           const float* __restrict__ alpha, const float* __restrict__ dyfac,
                                                           const float* __restrict__ dsimp, const float* __restrict__ dscore,
                                                           float* __restrict__ daq, float* __restrict__ da,
                                                           float* __restrict__ dgu, int B, int T, int P, int L, int D) {
    const int lane = threadIdx.x & 63;
    const long frame = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (frame >= (long)B * T) return;
    const int i = (int)(frame / T), t = (int)(frame % T);
    const bool qok = t < alen[i];
    float av[ND], aqv[ND], guv[ND], vv[ND], bsv[ND], acc_q[ND], acc_a[ND], acc_g[ND];
#pragma unroll
    for (int n = 0; n < ND; ++n) {
        const int d = lane + 64 * n;
        const bool ok = d < D;
        av[n] = ok ? a[frame * D + d] : 0.0f;
        aqv[n] = ok ? aq[frame * D + d] : 0.0f;
        guv[n] = ok ? gu[frame * D + d] : 0.0f;
        vv[n] = ok ? v[d] : 0.0f;
        bsv[n] = ok ? bs[d] : 0.0f;
        acc_q[n] = acc_a[n] = acc_g[n] = 0.0f;
    }
    for (int p = 0; p < P; ++p) {
        const long row = ((long)i * P + p) * T + t;
        const float dy = dsimp[row] * dyfac[row];
        if (dy == 0.0f) continue;                 // then dscore of the row is 0 too
        const float* wp = w + (size_t)p * L * D;
        const float* wsp = wst + (size_t)p * L * D;
        const float* akp = ak + (size_t)p * L * D;
        float c[ND], z[ND];
#pragma unroll
        for (int n = 0; n < ND; ++n) c[n] = z[n] = 0.0f;
        for (int k = 0; k < L; ++k) {
            const float al = alpha[row * L + k];
            if (al == 0.0f) continue;
#pragma unroll
            for (int n = 0; n < ND; ++n) {
                const int d = lane + 64 * n;
                if (d < D) {
                    c[n] = fmaf(al, wp[(size_t)k * D + d], c[n]);
                    z[n] = fmaf(al, wsp[(size_t)k * D + d], z[n]);
                }
            }
        }
#pragma unroll
        for (int n = 0; n < ND; ++n) {
            const GateGrad g = gate_grad(av[n], guv[n], c[n], z[n] + bsv[n], dy);
            acc_a[n] += g.da;
            acc_g[n] += g.dgu;
        }
        if (!qok) continue;
        const long kl = wlen[p];
        for (int k = 0; k < L && k < kl; ++k) {
            const float ds = dscore[row * L + k];
            if (ds == 0.0f) continue;
#pragma unroll
            for (int n = 0; n < ND; ++n) {
                const int d = lane + 64 * n;
                if (d < D) {
                    const float th = tanhf(aqv[n] + akp[(size_t)k * D + d]);
                    acc_q[n] = fmaf(ds * vv[n], 1.0f - th * th, acc_q[n]);
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < ND; ++n) {
        const int d = lane + 64 * n;
        if (d < D) {
            daq[frame * D + d] = acc_q[n];
            da[frame * D + d] = acc_a[n];
            dgu[frame * D + d] = acc_g[n];
        }
    }
}

// Token side: thread = one d of phrase blockIdx.z, frames [chunk * CH, (chunk + 1) * CH) of the B*T; partials
// dak_p, dw_p, dws_p (P,NCH,L,D) and dv_p, dbs_p (P,NCH,D)
template <int LM>
__global__ __launch_bounds__(256) void cp_token_bwd_kernel(const float* __restrict__ a, const float* __restrict__ aq,
                                                           const float* __restrict__ gu, const float* __restrict__ w,
                                                           const float* __restrict__ ak, const float* __restrict__ wst,
                                                           const float* __restrict__ v, const float* __restrict__ bs,
                                                           const long* __restrict__ alen, const long* __restrict__ wlen,
                                                           const float* __restrict__ alpha, const float* __restrict__ dyfac,
                                                           const float* __restrict__ dsimp, const float* __restrict__ dscore,
                                                           float* __restrict__ dak_p, float* __restrict__ dw_p,
                                                           float* __restrict__ dws_p, float* __restrict__ dv_p,
                                                           float* __restrict__ dbs_p, int B, int T, int P, int L, int D, int CH,
                                                           int NCH) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const int chunk = blockIdx.y, p = blockIdx.z;
    const long f0 = (long)chunk * CH, f1 = min((long)B * T, f0 + CH);
    const long kl = wlen[p];
    float akv[LM], wv[LM], wsv[LM], dak[LM], dw[LM], dws[LM];
#pragma unroll
    for (int k = 0; k < LM; ++k) {
        const size_t e = ((size_t)p * L + k) * D + d;
        akv[k] = k < L ? ak[e] : 0.0f;
        wv[k] = k < L ? w[e] : 0.0f;
        wsv[k] = k < L ? wst[e] : 0.0f;
        dak[k] = dw[k] = dws[k] = 0.0f;
    }
    const float vd = v[d], bsd = bs[d];
    float dv = 0.0f, dbs = 0.0f;
    for (long frame = f0; frame < f1; ++frame) {
        const int i = (int)(frame / T), t = (int)(frame % T);
        const long row = ((long)i * P + p) * T + t;
        const float dy = dsimp[row] * dyfac[row];
        if (dy == 0.0f) continue;
        float al[LM];
        float c = 0.0f, z = 0.0f;
#pragma unroll
        for (int k = 0; k < LM; ++k) {
            al[k] = k < L ? alpha[row * L + k] : 0.0f;
            c = fmaf(al[k], wv[k], c);
            z = fmaf(al[k], wsv[k], z);
        }
        const GateGrad g = gate_grad(a[frame * D + d], gu[frame * D + d], c, z + bsd, dy);
        dbs += g.dz;
#pragma unroll
        for (int k = 0; k < LM; ++k) {
            dw[k] = fmaf(al[k], g.dc, dw[k]);
            dws[k] = fmaf(al[k], g.dz, dws[k]);
        }
        if (t >= alen[i]) continue;
        const float aqd = aq[frame * D + d];
#pragma unroll
        for (int k = 0; k < LM; ++k)
            if (k < L && k < kl) {
                const float ds = dscore[row * L + k];
                if (ds != 0.0f) {
                    const float th = tanhf(aqd + akv[k]);
                    dak[k] = fmaf(ds * vd, 1.0f - th * th, dak[k]);
                    dv = fmaf(ds, th, dv);
                }
            }
    }
    const size_t slab = (size_t)p * NCH + chunk;
#pragma unroll
    for (int k = 0; k < LM; ++k)
        if (k < L) {
            const size_t e = (slab * L + k) * D + d;
            dak_p[e] = dak[k];
            dw_p[e] = dw[k];
            dws_p[e] = dws[k];
        }
    dv_p[slab * D + d] = dv;
    dbs_p[slab * D + d] = dbs;
}

// out[o][e] = sum_{c < NCH} part[o][c][e], chunk order
__global__ __launch_bounds__(256) void cp_fold_chunks_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                             long outer, int NCH, long inner) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < outer * inner; e += (long)gridDim.x * 256) {
        const long o = e / inner, i = e % inner;
        float s = 0.0f;
        for (int c = 0; c < NCH; ++c) s += part[(o * NCH + c) * inner + i];
        out[e] = s;
    }
}
// out[d] = sum over the n rows of part (n, D): 16 row groups in fp64, each in row order, then the groups in order
__global__ __launch_bounds__(256) void cp_fold_cols_kernel(const float* __restrict__ part, float* __restrict__ out, long n,
                                                           int D) {
    __shared__ double sh[16][17];
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4, d = blockIdx.x * 16 + c;
    double s = 0.0;
    if (d < D)
        for (long r = g; r < n; r += 16) s += (double)part[r * D + d];
    sh[g][c] = s;
    __syncthreads();
    if (g == 0 && d < D) {
        double t = 0.0;
        for (int q = 0; q < 16; ++q) t += sh[q][c];
        out[d] = (float)t;
    }
}

// dst[r * dpitch + c] = src[r * spitch + c], r < rows, c < width
__global__ __launch_bounds__(256) void cp_copy_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, long rows,
                                                           long width, long spitch, long dpitch) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < rows * width; e += (long)gridDim.x * 256) {
        const long r = e / width, c = e % width;
        dst[r * dpitch + c] = src[r * spitch + c];
    }
}

__global__ __launch_bounds__(256) void cp_sigmoid_bwd_kernel(const float* dg, const float* __restrict__ g, float* dz, long n) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const float gv = g[e];
        dz[e] = dg[e] * gv * (1.0f - gv);
    }
}

int grid_for(long n) { return (int)(cdiv(n, 256) > 4096 ? 4096 : cdiv(n, 256)); }

bool shape_ok(int B, int T, int P, int L, int D) {
    if (B <= 0 || T <= 0 || P <= 0 || L <= 0 || D <= 0) {
        tag_set_error("crosspairs: B, T, P, L, D must be positive (got %d, %d, %d, %d, %d)", B, T, P, L, D);
        return false;
    }
    if (L > MAXL) {
        tag_set_error("crosspairs: L = %d tokens per phrase, at most %d are served", L, MAXL);
        return false;
    }
    if (D % 32 != 0 || D > MAXD) {
        tag_set_error("crosspairs: D = %d is not served (multiples of 32 up to %d are)", D, MAXD);
        return false;
    }
    if ((long)B * P * T > (1L << 31) - 8 || (long)B * P * T * L > (1L << 40)) {
        tag_set_error("crosspairs: B * P * T = %ld rows exceed the launch grid", (long)B * P * T);
        return false;
    }
    return true;
}

// phrase counts: host array, every entry >= 0, sum = P, max <= N
bool pnum_ok(const long* pnum, int B, int P, int N) {
    long sum = 0;
    for (int j = 0; j < B; ++j) {
        if (pnum[j] < 0 || pnum[j] > N) {
            tag_set_error("crosspairs: pnum[%d] = %ld outside [0, N = %d]", j, pnum[j], N);
            return false;
        }
        sum += pnum[j];
    }
    if (sum != P) {
        tag_set_error("crosspairs: the phrase counts sum to %ld, the token tensor holds P = %d phrases", sum, P);
        return false;
    }
    return true;
}

int tok_chunk(int B, int T) {
    const int ch = cdiv((long)B * T, TOK_CHUNKS);
    return ch < TOK_CHUNK_MIN ? TOK_CHUNK_MIN : ch;
}

size_t rows_of(int B, int T, int P) { return (size_t)B * P * T; }

}  // namespace

extern "C" size_t tag_crosspairs_backward_ws_bytes(int B, int T, int P, int L, int D) {
    if (!shape_ok(B, T, P, L, D)) return 0;
    const size_t nch = (size_t)cdiv((long)B * T, tok_chunk(B, T));
    // dsimp (B,P,T), dscore (B,P,T,L), the token side's partials
    return (rows_of(B, T, P) * (1 + (size_t)L) + (size_t)P * nch * (3 * (size_t)L + 2) * D) * sizeof(float);
}

extern "C" size_t tag_crosspairs_ws_bytes(int B, int T, int P, int L, int D) {
    if (!shape_ok(B, T, P, L, D)) return 0;
    // saved by the forward: aq, gu (B,T,D), ak, ws (P,L,D), alpha (B,P,T,L), dyfac (B,P,T); its scratch: simp (B,P,T)
    const size_t fwd = (2 * (size_t)B * T * D + 2 * (size_t)P * L * D + rows_of(B, T, P) * ((size_t)L + 2)) * sizeof(float);
    return fwd + tag_crosspairs_backward_ws_bytes(B, T, P, L, D);
}

#define CP_DISPATCH_ND(D, CALL)                                                           \
    do {                                                                                 \
        if ((D) <= 128) { CALL(2) } else if ((D) <= 512) { CALL(8) } else { CALL(16) }   \
    } while (0)

extern "C" int tag_crosspairs_forward(const float* a, const float* aq, const float* gu, const float* w, const float* ak,
                                      const float* ws_tok, const float* v, const float* b_s, const long* alen,
                                      const long* wlen, const long* pnum_host, float* sim, float* alpha, float* dyfac,
                                      float* simp, int B, int T, int P, int L, int D, int N, int scale, void* stream) {
    TAG_CHECK_ARG(a && aq && gu && w && ak && ws_tok && v && b_s && alen && wlen && pnum_host && sim && alpha && dyfac && simp);
    if (!shape_ok(B, T, P, L, D)) return TAG_EINVAL;
    TAG_CHECK_ARG(N > 0);
    if (!pnum_ok(pnum_host, B, P, N)) return TAG_EINVAL;
    hipStream_t st = as_stream(stream);
    const long rows = (long)B * P * T;
    const float sc = scale ? 1.0f / sqrtf((float)D) : 1.0f;
#define CALL(ND)                                                                                                       \
    hipLaunchKernelGGL((cp_fwd_kernel<ND>), dim3(cdiv(rows, 4)), dim3(256), 0, st, a, aq, gu, w, ak, ws_tok, v, b_s, alen, \
                       wlen, simp, alpha, dyfac, B, T, P, L, D, sc);
    CP_DISPATCH_ND(D, CALL);
#undef CALL
    TAG_LAUNCH_CHECK();
    // sim (B,B,N,T): zero where n >= pnum[j]; clip j's phrases are one contiguous run of pnum[j] * T in both layouts
    hipError_t e = hipMemsetAsync(sim, 0, (size_t)B * B * N * T * sizeof(float), st);
    if (e != hipSuccess) {
        tag_set_error("crosspairs: hipMemsetAsync failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    long off = 0;
    for (int j = 0; j < B; ++j) {
        const long width = pnum_host[j] * T;
        if (width > 0)
            hipLaunchKernelGGL(cp_copy_rows_kernel, dim3(grid_for((long)B * width)), dim3(256), 0, st, simp + off * T,
                               sim + (size_t)j * N * T, (long)B, width, (long)P * T, (long)B * N * T);
        off += pnum_host[j];
    }
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_crosspairs_backward(const float* a, const float* aq, const float* gu, const float* w, const float* ak,
                                       const float* ws_tok, const float* v, const float* b_s, const long* alen,
                                       const long* wlen, const long* pnum_host, const float* alpha, const float* dyfac,
                                       const float* dsim, float* daq, float* da, float* dgu, float* dak, float* dw,
                                       float* dws, float* dv, float* db_s, int B, int T, int P, int L, int D, int N,
                                       void* ws, void* stream) {
    TAG_CHECK_ARG(a && aq && gu && w && ak && ws_tok && v && b_s && alen && wlen && pnum_host && alpha && dyfac && dsim);
    TAG_CHECK_ARG(daq && da && dgu && dak && dw && dws && dv && db_s && ws);
    if (!shape_ok(B, T, P, L, D)) return TAG_EINVAL;
    TAG_CHECK_ARG(N > 0);
    if (!pnum_ok(pnum_host, B, P, N)) return TAG_EINVAL;
    hipStream_t st = as_stream(stream);
    const long rows = (long)B * P * T;
    const int CH = tok_chunk(B, T), NCH = cdiv((long)B * T, CH);
    float* dsimp = static_cast<float*>(ws);
    float* dscore = dsimp + rows;
    float* dak_p = dscore + rows * L;
    const size_t slab = (size_t)P * NCH * L * D;
    float* dw_p = dak_p + slab;
    float* dws_p = dw_p + slab;
    float* dv_p = dws_p + slab;
    float* dbs_p = dv_p + (size_t)P * NCH * D;
    long off = 0;
    for (int j = 0; j < B; ++j) {
        const long width = pnum_host[j] * T;
        if (width > 0)
            hipLaunchKernelGGL(cp_copy_rows_kernel, dim3(grid_for((long)B * width)), dim3(256), 0, st,
                               dsim + (size_t)j * N * T, dsimp + off * T, (long)B, width, (long)B * N * T, (long)P * T);
        off += pnum_host[j];
    }
    TAG_LAUNCH_CHECK();
#define CALL(ND)                                                                                                       \
    hipLaunchKernelGGL((cp_dscore_kernel<ND>), dim3(cdiv(rows, 4)), dim3(256), 0, st, a, gu, w, ws_tok, b_s, alen, wlen, \
                       alpha, dyfac, dsimp, dscore, B, T, P, L, D);
    CP_DISPATCH_ND(D, CALL);
#undef CALL
    TAG_LAUNCH_CHECK();
#define CALL(ND)                                                                                                          \
    hipLaunchKernelGGL((cp_frame_bwd_kernel<ND>), dim3(cdiv((long)B * T, 4)), dim3(256), 0, st, a, aq, gu, w, ak, ws_tok, v, \
                       b_s, alen, wlen, alpha, dyfac, dsimp, dscore, daq, da, dgu, B, T, P, L, D);
    CP_DISPATCH_ND(D, CALL);
#undef CALL
    TAG_LAUNCH_CHECK();
    const int tpb = D < 256 ? 64 * cdiv(D, 64) : 256;
#define CALL(LM)                                                                                                          \
    hipLaunchKernelGGL((cp_token_bwd_kernel<LM>), dim3(cdiv(D, tpb), NCH, P), dim3(tpb), 0, st, a, aq, gu, w, ak, ws_tok, v,  \
                       b_s, alen, wlen, alpha, dyfac, dsimp, dscore, dak_p, dw_p, dws_p, dv_p, dbs_p, B, T, P, L, D, CH, NCH);
    if (L <= 4) { CALL(4) } else if (L <= 8) { CALL(8) } else if (L <= 16) { CALL(16) } else { CALL(32) }
#undef CALL
    TAG_LAUNCH_CHECK();
    const long inner = (long)L * D;
    hipLaunchKernelGGL(cp_fold_chunks_kernel, dim3(grid_for(P * inner)), dim3(256), 0, st, dak_p, dak, (long)P, NCH, inner);
    hipLaunchKernelGGL(cp_fold_chunks_kernel, dim3(grid_for(P * inner)), dim3(256), 0, st, dw_p, dw, (long)P, NCH, inner);
    hipLaunchKernelGGL(cp_fold_chunks_kernel, dim3(grid_for(P * inner)), dim3(256), 0, st, dws_p, dws, (long)P, NCH, inner);
    hipLaunchKernelGGL(cp_fold_cols_kernel, dim3(cdiv(D, 16)), dim3(256), 0, st, dv_p, dv, (long)P * NCH, D);
    hipLaunchKernelGGL(cp_fold_cols_kernel, dim3(cdiv(D, 16)), dim3(256), 0, st, dbs_p, db_s, (long)P * NCH, D);
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_sigmoid_backward(const float* dg, const float* g, float* dz, long n, void* stream) {
    TAG_CHECK_ARG(dg && g && dz && n > 0);
    hipLaunchKernelGGL(cp_sigmoid_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), dg, g, dz, n);
    TAG_LAUNCH_CHECK();
    return 0;
}
