// T6: the TRAINING path of the LAION-CLAP text tower (models/text_encoder.py:311-327 LaionClapEncoder = Hugging Face
// ClapTextModel + ClapProjectionLayer, transformers models/clap/modeling_clap.py: a RoBERTa-style post-LayerNorm encoder).
// The dense layers are tag_gemm calls and the attention core is tag_text_selfattn_* (text_attn.hip); this file holds the row
// kernels in between, each with its backward:
//   tag_text_clap_resln_*      y = LayerNorm(x + res) * gamma + beta   (ClapTextSelfOutput / ClapTextOutput: LayerNorm(dense + input))
//   tag_text_clap_embed_*      position ids + word + type + position embeddings + LayerNorm   (ClapTextEmbeddings)
//   tag_text_clap_gelu_*       erf-GELU on a saved pre-activation   (ClapTextIntermediate: ACT2FN["gelu"])
//   tag_text_clap_tanh_backward   (ClapTextPooler: tanh(dense(h[:, 0])))
// text_tower.hip keeps the forward-only kernels of the inference wrapper; the arithmetic of the forward passes is the same.
//
// The row layout (one wave per row of D <= 1024), the LayerNorm row forward / backward and the deterministic table gather live in
// text_rows.h, shared with text_bert.hip: no atomics, two runs are bit-identical.
#include "text_rows.h"

namespace {

template <int NQ, bool VEC>
__global__ __launch_bounds__(256) void tc_resln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, float* __restrict__ y, float* __restrict__ xhat,
                                                           float* __restrict__ rstd, long rows, int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                  // whole waves leave
    f32x4 v[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int c = 256 * i + 4 * lane;
        v[i] = tc_ld4<VEC>(x + row * D, c, D);
        if (res) v[i] += tc_ld4<VEC>(res + row * D, c, D);
    }
    tc_ln_row<NQ, VEC>(v, D, lane, gamma, beta, eps, y + row * D, xhat ? xhat + row * D : nullptr, rstd ? rstd + row : nullptr);
}

// ClapTextEmbeddings: position id = (number of non-pad tokens in ids[b][0..l]) + pad_id for a non-pad token, pad_id for a pad token
template <int NQ, bool VEC>
__global__ __launch_bounds__(256) void tc_embed_fwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ word,
                                                           const float* __restrict__ type0, const float* __restrict__ pos,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, float* __restrict__ h, int64_t* __restrict__ pos_ids,
                                                           float* __restrict__ xhat, float* __restrict__ rstd, int B, int L, int D,
                                                           int V, int pad_id) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)B * L) return;
    const int b = (int)(row / L), l = (int)(row - (long)b * L);
    int cnt = 0;
    for (int i0 = 0; i0 <= l; i0 += 64) {
        const int i = i0 + lane;
        const bool np = i <= l && ids[(long)b * L + i] != pad_id;
        cnt += __popcll(__ballot(np));
    }
    const int64_t id = ids[row];
    const int p = id != pad_id ? cnt + pad_id : pad_id;       // <= L + pad_id < P (checked by the launcher)
    const bool in_table = id >= 0 && id < V;                  // an id outside the table reads nothing (tag_embed_check_ids raises)
    if (pos_ids && lane == 0) pos_ids[row] = p;
    f32x4 v[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int c = 256 * i + 4 * lane;
        v[i] = in_table ? tc_ld4<VEC>(word + id * D, c, D) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        v[i] += tc_ld4<VEC>(type0, c, D);
        v[i] += tc_ld4<VEC>(pos + (long)p * D, c, D);
    }
    tc_ln_row<NQ, VEC>(v, D, lane, gamma, beta, eps, h + row * D, xhat ? xhat + row * D : nullptr, rstd ? rstd + row : nullptr);
}

// ---- element-wise: 0 gelu forward (a = u), 1 gelu backward (a = u, b = df), 2 tanh backward (a = y, b = dy) ----
template <int OP>
__device__ __forceinline__ float tc_map(float a, float b) {
    if constexpr (OP == 0) {
        return 0.5f * a * (1.0f + erff(a * 0.70710678118654752f));
    } else if constexpr (OP == 1) {
        const float cdf = 0.5f * (1.0f + erff(a * 0.70710678118654752f));
        const float pdf = expf(-0.5f * a * a) * 0.39894228040143268f;
        return b * (cdf + a * pdf);
    } else {
        return b * (1.0f - a * a);
    }
}

// vec: a, b, out 16-byte aligned -> the first n / 4 * 4 elements in groups of 4, the tail one by one
template <int OP>
__global__ __launch_bounds__(256) void tc_map_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     float* __restrict__ out, long n, int vec) {
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nt = (long)gridDim.x * 256;
    long done = 0;
    if (vec) {
        const long n4 = n >> 2;
        for (long i = tid; i < n4; i += nt) {
            const f32x4 x = reinterpret_cast<const f32x4*>(a)[i];
            const f32x4 y = OP == 0 ? x : reinterpret_cast<const f32x4*>(b)[i];
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = tc_map<OP>(x[j], y[j]);
            reinterpret_cast<f32x4*>(out)[i] = o;
        }
        done = n4 << 2;
    }
    for (long i = done + tid; i < n; i += nt) out[i] = tc_map<OP>(a[i], OP == 0 ? 0.0f : b[i]);
}

template <int OP>
int tc_launch_map(const float* a, const float* b, float* out, long n, void* stream) {
    const int vec = aligned16(a) && aligned16(out) && (OP == 0 || aligned16(b));
    const long work = vec ? (n + 3) / 4 : n;
    long nb = (work + 255) / 256;
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(tc_map_kernel<OP>, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), a, b, out, n, vec);
    TAG_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int tag_text_clap_resln_forward(const float* x, const float* res, const float* gamma, const float* beta, float eps,
                                           float* y, float* xhat, float* rstd, long rows, int D, void* stream) {
    TAG_CHECK_ARG(x && gamma && beta && y);
    TAG_CHECK_ARG((xhat == nullptr) == (rstd == nullptr));
    TAG_CHECK_ARG(rows >= 1 && rows <= (1L << 31) && D >= 1 && D <= TC_MAX_D && eps >= 0.0f);
    const bool vec = D % 4 == 0 && aligned16(x) && aligned16(res) && aligned16(gamma) && aligned16(beta) &&
                     aligned16(y) && aligned16(xhat);
#define CALL(NQ, V)                                                                                                           \
    hipLaunchKernelGGL((tc_resln_fwd_kernel<NQ, V>), dim3(cdiv(rows, 4)), dim3(256), 0, as_stream(stream), x, res, gamma, beta, \
                       eps, y, xhat, rstd, rows, D);
    TC_BY_NQ(D, vec, CALL)
#undef CALL
    TAG_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t tag_text_clap_resln_backward_ws_bytes(long rows, int D) {
    if (rows < 1 || D < 1 || D > TC_MAX_D) return 0;
    return tc_part_floats(rows, D) * sizeof(float) + tag_colsum_ws_bytes((long)tc_part_blocks(rows) * 4, D);
}

extern "C" int tag_text_clap_resln_backward(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* ds,
                                            float* dgamma, float* dbeta, long rows, int D, void* ws, void* stream) {
    TAG_CHECK_ARG(dy && xhat && rstd && gamma && ds);
    TAG_CHECK_ARG(rows >= 1 && rows <= (1L << 31) && D >= 1 && D <= TC_MAX_D);
    const bool sums = dgamma || dbeta;
    TAG_CHECK_ARG(!sums || ws);
    float* part = sums ? static_cast<float*>(ws) : nullptr;
    const int rc = tc_launch_ln_bwd(dy, xhat, rstd, gamma, ds, part, rows, D, stream);
    if (rc) return rc;
    if (!sums) return 0;
    return tc_fold_parts(part, (long)tc_part_blocks(rows) * 4, D, dgamma, dbeta, part + tc_part_floats(rows, D), stream);
}

extern "C" int tag_text_clap_embed_forward(const int64_t* ids, const float* word, const float* type0, const float* pos,
                                           const float* gamma, const float* beta, float eps, float* h, int64_t* pos_ids,
                                           float* xhat, float* rstd, int B, int L, int D, int V, int P, int pad_id, void* stream) {
    TAG_CHECK_ARG(ids && word && type0 && pos && gamma && beta && h);
    TAG_CHECK_ARG((xhat == nullptr) == (rstd == nullptr));
    TAG_CHECK_ARG(B >= 1 && L >= 1 && D >= 1 && D <= TC_MAX_D && V >= 1 && eps >= 0.0f);
    TAG_CHECK_ARG(pad_id >= 0 && (long)L + pad_id < (long)P);          // the largest position id is L + pad_id
    const long rows = (long)B * L;
    const bool vec = D % 4 == 0 && aligned16(word) && aligned16(type0) && aligned16(pos) && aligned16(gamma) &&
                     aligned16(beta) && aligned16(h) && aligned16(xhat);
#define CALL(NQ, VV)                                                                                                         \
    hipLaunchKernelGGL((tc_embed_fwd_kernel<NQ, VV>), dim3(cdiv(rows, 4)), dim3(256), 0, as_stream(stream), ids, word, type0, \
                       pos, gamma, beta, eps, h, pos_ids, xhat, rstd, B, L, D, V, pad_id);
    TC_BY_NQ(D, vec, CALL)
#undef CALL
    TAG_LAUNCH_CHECK();
    return 0;
}

// ws: ds (M, D) | partial rows | the column sums' workspace
extern "C" size_t tag_text_clap_embed_backward_ws_bytes(int B, int L, int D) {
    if (B < 1 || L < 1 || D < 1 || D > TC_MAX_D) return 0;
    const long rows = (long)B * L;
    return ((size_t)(rows + (rows & 1)) * D + tc_part_floats(rows, D)) * sizeof(float) +
           tc_max(tag_colsum_ws_bytes(rows, D), tag_colsum_ws_bytes((long)tc_part_blocks(rows) * 4, D));
}

extern "C" int tag_text_clap_embed_backward(const float* dh, const float* xhat, const float* rstd, const float* gamma,
                                            const int64_t* ids, const int64_t* pos_ids, float* dword, float* dpos, float* dtype0,
                                            float* dgamma, float* dbeta, int B, int L, int D, int V, int P, int pad_id, void* ws,
                                            void* stream) {
    TAG_CHECK_ARG(dh && xhat && rstd && gamma && ids && pos_ids && ws);
    TAG_CHECK_ARG(dword || dpos || dtype0 || dgamma || dbeta);
    TAG_CHECK_ARG(B >= 1 && L >= 1 && D >= 1 && D <= TC_MAX_D && V >= 1);
    TAG_CHECK_ARG(pad_id >= 0 && (long)L + pad_id < (long)P);
    const long rows = (long)B * L;
    TAG_CHECK_ARG(rows <= 0x7fffffffL);                                  // one workgroup per row in the table gathers
    float* ds = static_cast<float*>(ws);
    float* part = ds + (size_t)(rows + (rows & 1)) * D;                  // an even number of floats in front: 8-byte alignment
    void* cws = part + tc_part_floats(rows, D);
    const bool sums = dgamma || dbeta;
    int rc = tc_launch_ln_bwd(dh, xhat, rstd, gamma, ds, sums ? part : nullptr, rows, D, stream);
    if (rc) return rc;
    if (sums && (rc = tc_fold_parts(part, (long)tc_part_blocks(rows) * 4, D, dgamma, dbeta, cws, stream))) return rc;
    if (dtype0 && (rc = tag_colsum(ds, D, rows, D, dtype0, cws, stream))) return rc;        // token_type_ids are all 0
    // nn.Embedding(padding_idx = pad_id) on both tables: pad tokens (position id pad_id) are skipped, row pad_id is not touched
    if (dword) {
        hipLaunchKernelGGL(tc_scatter_rows_kernel, dim3((unsigned)rows), dim3(256), 0, as_stream(stream), ds, ids, dword, (int)rows, D,
                           V, pad_id);
        TAG_LAUNCH_CHECK();
    }
    if (dpos) {
        hipLaunchKernelGGL(tc_scatter_rows_kernel, dim3((unsigned)rows), dim3(256), 0, as_stream(stream), ds, pos_ids, dpos, (int)rows,
                           D, P, pad_id);
        TAG_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int tag_text_clap_gelu_forward(const float* u, float* f, long n, void* stream) {
    TAG_CHECK_ARG(u && f && n >= 1);
    return tc_launch_map<0>(u, nullptr, f, n, stream);
}

extern "C" int tag_text_clap_gelu_backward(const float* u, const float* df, float* du, long n, void* stream) {
    TAG_CHECK_ARG(u && df && du && n >= 1);
    return tc_launch_map<1>(u, df, du, n, stream);
}

extern "C" int tag_text_clap_tanh_backward(const float* y, const float* dy, float* dx, long n, void* stream) {
    TAG_CHECK_ARG(y && dy && dx && n >= 1);
    return tc_launch_map<2>(y, dy, dx, n, stream);
}
