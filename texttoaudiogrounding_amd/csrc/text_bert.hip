// T7: what a BERT encoder (Hugging Face BertModel; models/text_encoder.py:271-308 Bert / SentenceBert) needs beside the
// post-LayerNorm stack it shares with the LAION-CLAP tower (tag_gemm, tag_text_selfattn_*, the row kernels of text_clap.hip):
//   tag_text_bert_embed_*   word + token-type + ABSOLUTE position embeddings + LayerNorm   (BertEmbeddings), and its backward
//   tag_text_bert_pool_*    the sentence poolings ([CLS], masked mean) with the two normalisations, and their backward
// Row kernels in the layout of text_rows.h: one wave per row of D <= 1024, 16-byte accesses when D % 4 == 0 and the bases are
// aligned and 4-byte accesses of the same channels otherwise (same bits); row sums through wave_sum, sums over rows as
// fixed-stride partial rows folded by tag_colsum; no atomics, two runs are bit-identical.
#include "text_rows.h"

namespace {

constexpr int TB_MAX_T = 16;                     // token-type vocabulary (BERT: 2); bounds the partial rows of dtype

// BertEmbeddings: the position of a token is its column l, pads included.  type_ids: null = all zeros; a type id outside [0, T)
// is clamped (tag_embed_check_ids raises the flag), a token id outside [0, V) reads nothing.
template <int NQ, bool VEC>
__global__ __launch_bounds__(256) void tb_embed_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ type_ids,
                                                           const float* __restrict__ word, const float* __restrict__ type,
                                                           const float* __restrict__ pos, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float* __restrict__ h,
                                                           float* __restrict__ xhat, float* __restrict__ rstd, long rows, int L, int D,
                                                           int V, int T) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                  // whole waves leave
    const int l = (int)(row % L);
    const int64_t id = ids[row];
    const bool in_table = id >= 0 && id < V;
    int64_t t = type_ids ? type_ids[row] : 0;
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);
    f32x4 v[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int c = 256 * i + 4 * lane;
        v[i] = in_table ? tc_ld4<VEC>(word + id * D, c, D) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        v[i] += tc_ld4<VEC>(type + t * D, c, D);
        v[i] += tc_ld4<VEC>(pos + (long)l * D, c, D);
    }
    tc_ln_row<NQ, VEC>(v, D, lane, gamma, beta, eps, h + row * D, xhat ? xhat + row * D : nullptr, rstd ? rstd + row : nullptr);
}

// dtype: wave (gw, t = blockIdx.y) sums the rows gw, gw + nw, ... whose (clamped) type id is t into part[gw][t][:]; the fold over
// gw is ONE tag_colsum over (nw, T * D).  Every wave writes its row (zeros when no row of its stride has type t).
template <int NQ, bool VEC>
__global__ __launch_bounds__(256) void tb_type_part_kernel(const float* __restrict__ ds, const int64_t* __restrict__ type_ids,
                                                           float* __restrict__ part, long rows, int D, int T) {
    const int lane = threadIdx.x & 63, t = blockIdx.y;
    const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
    f32x4 acc[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc[i] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (long row = gw; row < rows; row += nw) {
        int64_t tt = type_ids ? type_ids[row] : 0;
        tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
        if (tt != t) continue;                                // uniform over the wave
#pragma unroll
        for (int i = 0; i < NQ; ++i) acc[i] += tc_ld4<VEC>(ds + row * D, 256 * i + 4 * lane, D);
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) tc_st4<VEC>(part + (gw * T + t) * D, 256 * i + 4 * lane, D, acc[i]);
}

// One wave per phrase r.  mode 0: x = h[r, 0]; mode 1: x = sum_{l < klen} h[r, l] / max(klen, 1e-9) (l ascending).
// norm 0: out = x; 1: x / max(|x|, 1e-12); 2: clip(x / (|x| + 1e-7), +-1e3).  raw (nullable) receives x.
template <int NQ, bool VEC>
__global__ __launch_bounds__(256) void tb_pool_fwd_kernel(const float* __restrict__ h, const int64_t* __restrict__ klen, int mode,
                                                          int norm, float* __restrict__ raw, float* __restrict__ out, long R, int L,
                                                          int D) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* hr = h + r * L * D;
    f32x4 v[NQ];
    if (mode == 0) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) v[i] = tc_ld4<VEC>(hr, 256 * i + 4 * lane, D);
    } else {
        int64_t k = klen[r];
        k = k < 0 ? 0 : (k > L ? L : k);
#pragma unroll
        for (int i = 0; i < NQ; ++i) v[i] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        for (int l = 0; l < (int)k; ++l) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) v[i] += tc_ld4<VEC>(hr + (long)l * D, 256 * i + 4 * lane, D);
        }
        const float den = fmaxf((float)k, 1e-9f);
#pragma unroll
        for (int i = 0; i < NQ; ++i) v[i] /= den;
    }
    if (raw) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) tc_st4<VEC>(raw + r * D, 256 * i + 4 * lane, D, v[i]);
    }
    if (norm != 0) {
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) q = fmaf(v[i][j], v[i][j], q);          // channels beyond D are zeros
        }
        const float n = sqrtf(wave_sum(q));
        const float den = norm == 1 ? fmaxf(n, 1e-12f) : n + 1e-7f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float y = v[i][j] / den;
                if (norm == 2) y = fminf(fmaxf(y, -1e3f), 1e3f);
                v[i][j] = y;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) tc_st4<VEC>(out + r * D, 256 * i + 4 * lane, D, v[i]);
}

// One wave per row (r, l) of dh.  A row the pooling read (l == 0, or l < klen) receives w * g with g = dseq[r] (norm 0) or the
// F.normalize gradient (d - x (x . d) / n^2) / n, n = max(|x|, 1e-12), x = raw[r] (d / 1e-12 where |x| <= 1e-12), and w = 1 or
// 1 / klen; every row starts from dtok (or zero).  dh must not alias an input.
template <int NQ, bool VEC>
__global__ __launch_bounds__(256) void tb_pool_bwd_kernel(const float* __restrict__ dseq, const float* dtok,
                                                          const float* __restrict__ raw, const int64_t* __restrict__ klen, int mode,
                                                          int norm, float* dh, long R, int L, int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R * L) return;
    const long r = row / L;
    const int l = (int)(row - r * L);
    f32x4 o[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i)
        o[i] = dtok ? tc_ld4<VEC>(dtok + row * D, 256 * i + 4 * lane, D) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    float w = 0.0f;
    if (dseq) {
        if (mode == 0) {
            w = l == 0 ? 1.0f : 0.0f;
        } else {
            int64_t k = klen[r];
            k = k < 0 ? 0 : (k > L ? L : k);
            w = l < (int)k ? 1.0f / fmaxf((float)k, 1e-9f) : 0.0f;
        }
    }
    if (w != 0.0f) {                                          // uniform over the wave
        f32x4 d[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) d[i] = tc_ld4<VEC>(dseq + r * D, 256 * i + 4 * lane, D);
        if (norm == 1) {
            f32x4 x[NQ];
            float q = 0.0f, s = 0.0f;
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                x[i] = tc_ld4<VEC>(raw + r * D, 256 * i + 4 * lane, D);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    q = fmaf(x[i][j], x[i][j], q);
                    s = fmaf(x[i][j], d[i][j], s);
                }
            }
            const float n = sqrtf(wave_sum(q));
            const float dot = wave_sum(s);
            if (n > 1e-12f) {
                const float c = dot / (n * n);
#pragma unroll
                for (int i = 0; i < NQ; ++i) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) d[i][j] = (d[i][j] - x[i][j] * c) / n;
                }
            } else {
#pragma unroll
                for (int i = 0; i < NQ; ++i) d[i] /= 1e-12f;
            }
        }
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[i][j] = fmaf(w, d[i][j], o[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) tc_st4<VEC>(dh + row * D, 256 * i + 4 * lane, D, o[i]);
}

size_t tb_type_floats(long rows, int D, int T) { return (size_t)tc_part_blocks(rows) * 4 * T * D; }

size_t tb_even(size_t n) { return n + (n & 1); }

}  // namespace

extern "C" int tag_text_bert_embed_forward(const int64_t* ids, const int64_t* type_ids, const float* word, const float* type,
                                           const float* pos, const float* gamma, const float* beta, float eps, float* h, float* xhat,
                                           float* rstd, int B, int L, int D, int V, int T, int P, void* stream) {
    TAG_CHECK_ARG(ids && word && type && pos && gamma && beta && h);
    TAG_CHECK_ARG((xhat == nullptr) == (rstd == nullptr));
    TAG_CHECK_ARG(B >= 1 && L >= 1 && D >= 1 && D <= TC_MAX_D && V >= 1 && T >= 1 && eps >= 0.0f);
    TAG_CHECK_ARG(L <= P);                                              // the largest position is L - 1
    const long rows = (long)B * L;
    const bool vec = D % 4 == 0 && aligned16(word) && aligned16(type) && aligned16(pos) && aligned16(gamma) &&
                     aligned16(beta) && aligned16(h) && aligned16(xhat);
#define CALL(NQ, VV)                                                                                                            \
    hipLaunchKernelGGL((tb_embed_fwd_kernel<NQ, VV>), dim3(cdiv(rows, 4)), dim3(256), 0, as_stream(stream), ids, type_ids, word, \
                       type, pos, gamma, beta, eps, h, xhat, rstd, rows, L, D, V, T);
    TC_BY_NQ(D, vec, CALL)
#undef CALL
    TAG_LAUNCH_CHECK();
    return 0;
}

// ws: ds (M, D) | LayerNorm partial rows | dtype partial rows | the column sums' workspace
extern "C" size_t tag_text_bert_embed_backward_ws_bytes(int B, int L, int D, int T) {
    if (B < 1 || L < 1 || D < 1 || D > TC_MAX_D || T < 1 || T > TB_MAX_T) return 0;
    const long rows = (long)B * L, np = (long)tc_part_blocks(rows) * 4;
    const size_t cws = tc_max(tc_max(tag_colsum_ws_bytes(np, D), tag_colsum_ws_bytes(np, T * D)), tag_colsum_ws_bytes(B, L * D));
    return (tb_even((size_t)rows * D) + tb_even(tc_part_floats(rows, D)) + tb_even(tb_type_floats(rows, D, T))) * sizeof(float) + cws;
}

extern "C" int tag_text_bert_embed_backward(const float* dh, const float* xhat, const float* rstd, const float* gamma,
                                            const int64_t* ids, const int64_t* type_ids, float* dword, float* dtype, float* dpos,
                                            float* dgamma, float* dbeta, int B, int L, int D, int V, int T, int P, int pad_id,
                                            void* ws, void* stream) {
    TAG_CHECK_ARG(dh && xhat && rstd && gamma && ids && ws);
    TAG_CHECK_ARG(dword || dtype || dpos || dgamma || dbeta);
    TAG_CHECK_ARG(B >= 1 && L >= 1 && D >= 1 && D <= TC_MAX_D && V >= 1 && T >= 1 && T <= TB_MAX_T && L <= P);
    const long rows = (long)B * L;
    TAG_CHECK_ARG(rows <= 0x7fffffffL);                                  // one workgroup per row in the table gather
    float* ds = static_cast<float*>(ws);
    float* part = ds + tb_even((size_t)rows * D);                        // even numbers of floats in front: 8-byte alignment
    float* tpart = part + tb_even(tc_part_floats(rows, D));
    void* cws = tpart + tb_even(tb_type_floats(rows, D, T));
    const long np = (long)tc_part_blocks(rows) * 4;
    const bool sums = dgamma || dbeta;
    int rc = tc_launch_ln_bwd(dh, xhat, rstd, gamma, ds, sums ? part : nullptr, rows, D, stream);
    if (rc) return rc;
    if (sums && (rc = tc_fold_parts(part, np, D, dgamma, dbeta, cws, stream))) return rc;
    if (dtype) {
        const bool vec = D % 4 == 0 && aligned16(ds) && aligned16(tpart);
#define CALL(NQ, VV)                                                                                                              \
    hipLaunchKernelGGL((tb_type_part_kernel<NQ, VV>), dim3(tc_part_blocks(rows), T), dim3(256), 0, as_stream(stream), ds, type_ids, \
                       tpart, rows, D, T);
        TC_BY_NQ(D, vec, CALL)
#undef CALL
        TAG_LAUNCH_CHECK();
        if ((rc = tag_colsum(tpart, T * D, np, T * D, dtype, cws, stream))) return rc;
    }
    // dpos[l] = sum_b ds[b, l]: the column sum of ds as (B, L * D); the rows >= L are not touched
    if (dpos && (rc = tag_colsum(ds, L * D, B, L * D, dpos, cws, stream))) return rc;
    // nn.Embedding(padding_idx = pad_id): pad tokens are skipped, row pad_id is not touched (pad_id < 0: no padding index)
    if (dword) {
        hipLaunchKernelGGL(tc_scatter_rows_kernel, dim3((unsigned)rows), dim3(256), 0, as_stream(stream), ds, ids, dword, (int)rows, D,
                           V, pad_id);
        TAG_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int tag_text_bert_pool_forward(const float* h, const int64_t* klen, int mode, int norm, float* raw, float* out, long R,
                                          int L, int D, void* stream) {
    TAG_CHECK_ARG(h && out && (mode == 0 || (mode == 1 && klen)) && norm >= 0 && norm <= 2);
    TAG_CHECK_ARG(R >= 1 && R <= (1L << 31) && L >= 1 && D >= 1 && D <= TC_MAX_D);
    const bool vec = D % 4 == 0 && aligned16(h) && aligned16(raw) && aligned16(out);
#define CALL(NQ, VV)                                                                                                        \
    hipLaunchKernelGGL((tb_pool_fwd_kernel<NQ, VV>), dim3(cdiv(R, 4)), dim3(256), 0, as_stream(stream), h, klen, mode, norm, \
                       raw, out, R, L, D);
    TC_BY_NQ(D, vec, CALL)
#undef CALL
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" int tag_text_bert_pool_backward(const float* dseq, const float* dtok, const float* raw, const int64_t* klen, int mode,
                                           int norm, float* dh, long R, int L, int D, void* stream) {
    TAG_CHECK_ARG(dh && (dseq || dtok) && (mode == 0 || (mode == 1 && klen)) && (norm == 0 || (norm == 1 && raw)));
    TAG_CHECK_ARG(R >= 1 && L >= 1 && R * (long)L <= (1L << 31) && D >= 1 && D <= TC_MAX_D);
    const bool vec = D % 4 == 0 && aligned16(dseq) && aligned16(dtok) && aligned16(raw) && aligned16(dh);
#define CALL(NQ, VV)                                                                                                         \
    hipLaunchKernelGGL((tb_pool_bwd_kernel<NQ, VV>), dim3(cdiv(R * (long)L, 4)), dim3(256), 0, as_stream(stream), dseq, dtok, \
                       raw, klen, mode, norm, dh, R, L, D);
    TC_BY_NQ(D, vec, CALL)
#undef CALL
    TAG_LAUNCH_CHECK();
    return 0;
}
