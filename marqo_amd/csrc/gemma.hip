// EmbeddingGemma text embedders (transformers Gemma3TextModel with use_bidirectional_attention: google/embeddinggemma-300m and its fine-tunes) on one HIP
// stream, no allocation, no sync: the row kernels this family adds (post-norm + residual add + next pre-norm in one pass; the tanh-GELU gated product; the
// token gather scaled by sqrt(width)) and the host-side orchestration of the tower on kernels that live in the sibling units — the bf16 GEMMs,
// mq_rmsnorm and mq_qk_norm_rope (qwen.hip), the 256-wide grouped-query band attention (attention_gqa256.hip), pooling.
//
// Per block, on the fp32 residual stream x [rows, W] (no Linear has a bias; every norm is an RMSNorm whose weight arrives as 1 + w, folded at load):
//   h = rmsnorm(x, input_layernorm)                                  (layer 0: mq_rmsnorm; later layers: the tail of the previous block's add_norm)
//   qkv = h Wqkv^T ; qk_norm_rope(qkv, the layer kind's inv_freq) ; a = attention_gqa_band(qkv, the layer kind's half_window, attn_scale)
//   o = a Wo^T (bf16) ; x += rmsnorm(o, post_attention_layernorm) ; h = rmsnorm(x, pre_feedforward_layernorm)          (one pass: mq_rmsnorm_add_norm)
//   (up | gate) = h Wug^T ; p = up * gelu_tanh(gate) ; o = p Wdown^T (bf16)
//   x += rmsnorm(o, post_feedforward_layernorm) ; h = rmsnorm(x, the next block's input_layernorm)                     (one pass; none after the last)
// then the final RMSNorm and the pooling (+ L2).
//
// The checks in front of the first launch and the workspace arithmetic are the packed-token scaffold of packed_text.h.
#include "packed_text.h"

static_assert(sizeof(mq_gemma_layer) == 88 && sizeof(mq_gemma_weights) == 40 && sizeof(mq_gemma_cfg) == 48, "Gemma layouts (marqo_amd/_lib.py)");

namespace {

__device__ __forceinline__ f32x4 bf16x4_to_f32(uint2 q) {
    return f32x4{__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u), __uint_as_float(q.y << 16), __uint_as_float(q.y & 0xffff0000u)};
}

// ---- x += rmsnorm(o; g_post) ; h = rmsnorm(x; g_next).  One wave64 per row, CH float4 chunks per lane: the row of o (bf16) and of x (fp32) stay in
// registers from the first load to the last store.  Statistics in fp32, each in mq_rmsnorm's order: per lane ((a^2 + b^2) + (c^2 + d^2)) summed over its
// chunks, the butterfly over the wave, / W + eps, rsqrtf; every product (v * rstd) * g.  h is written only when g_next is given.
template <int CH>
__global__ __launch_bounds__(256) void rmsnorm_add_norm_kernel(float* __restrict__ x, const bf16_t* __restrict__ o, const float* __restrict__ g_post,
                                                               const float* __restrict__ g_next, bf16_t* __restrict__ h, int64_t rows, int W, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nch = W >> 2;
    f32x4 v[CH], xv[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        v[i] = c < nch ? bf16x4_to_f32(*(const uint2*)(o + row * W + c * 4)) : f32x4{0.f, 0.f, 0.f, 0.f};
        xv[i] = c < nch ? *(const f32x4*)(x + row * W + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) ss += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
    const float rstd = rsqrtf(wave_sum(ss) / (float)W + eps);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        if (c >= nch) continue;
        xv[i] += (v[i] * rstd) * *(const f32x4*)(g_post + c * 4);
        *(f32x4*)(x + row * W + c * 4) = xv[i];
    }
    if (!g_next) return;
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) s2 += (xv[i][0] * xv[i][0] + xv[i][1] * xv[i][1]) + (xv[i][2] * xv[i][2] + xv[i][3] * xv[i][3]);
    const float rstd2 = rsqrtf(wave_sum(s2) / (float)W + eps);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        if (c >= nch) continue;
        const f32x4 y = (xv[i] * rstd2) * *(const f32x4*)(g_next + c * 4);
        uint2 p;
        p.x = pack_bf16x2(y[0], y[1]);
        p.y = pack_bf16x2(y[2], y[3]);
        *(uint2*)(h + row * W + c * 4) = p;
    }
}

// ---- tanh-GELU (transformers' gelu_pytorch_tanh), not the erf form: gelu_tanh(x) = x / 2 * (1 + tanh(u)) = x / (1 + exp(-2u)),
// u = sqrt(2 / pi) * (x + 0.044715 x^3).  Accurate expf and a true division; exp(-2u) = inf for very negative x gives x / inf = -0.
__device__ __forceinline__ float gelu_tanh(float x) {
    const float u = 0.7978845608028654f * (x * (1.0f + 0.044715f * (x * x)));
    return x / (1.0f + expf(-2.0f * u));
}

// buf [rows, 2F] = (up | gate) from the fc1 GEMM -> buf[:, :F] = up * gelu_tanh(gate), in place (row stride stays 2F): mq_glu's layout
__global__ __launch_bounds__(256) void glu_tanh_kernel(bf16_t* __restrict__ buf, int64_t rows, int F) {
    const int chunks = F >> 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows * chunks; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / chunks;
        const int c = (int)(i - r * chunks);
        bf16_t* p = buf + r * (2 * (int64_t)F) + c * 8;
        uint4 up = *(const uint4*)p;
        const uint4 gt = *(const uint4*)(p + F);
        uint32_t* a = (uint32_t*)&up;
        const uint32_t* g = (const uint32_t*)&gt;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float u0 = bf16_to_f32((bf16_t)(a[e] & 0xffff)), u1 = bf16_to_f32((bf16_t)(a[e] >> 16));
            const float g0 = bf16_to_f32((bf16_t)(g[e] & 0xffff)), g1 = bf16_to_f32((bf16_t)(g[e] >> 16));
            a[e] = pack_bf16x2(u0 * gelu_tanh(g0), u1 * gelu_tanh(g1));
        }
        *(uint4*)p = up;
    }
}

// ---- embed_tokens: x[row] = tok[id] * sqrt(W), the product in fp32 (Gemma3TextScaledWordEmbedding).  One wave per row; ids are clamped to the table.
__global__ __launch_bounds__(256) void embed_scaled_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok, float* __restrict__ x, int64_t rows,
                                                           int W, int vocab, float scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const float* tr = tok + (int64_t)id * W;
    for (int c = lane; c < (W >> 2); c += 64) *(f32x4*)(x + row * W + c * 4) = *(const f32x4*)(tr + c * 4) * scale;
}

struct Plan { size_t off_x, off_h, off_a, off_o, off_big, total; };
Plan plan(const mq_gemma_cfg* c, int64_t rows) {
    Plan p;
    Off ws;
    const size_t aw = (size_t)c->q_heads * c->head_dim, qkvw = (size_t)(c->q_heads + 2 * c->kv_heads) * c->head_dim;
    const size_t big = qkvw > 2 * (size_t)c->mlp_dim ? qkvw : 2 * (size_t)c->mlp_dim;
    p.off_x = ws.take((size_t)rows * c->width * 4);     // residual stream, fp32
    p.off_h = ws.take((size_t)rows * c->width * 2);     // normalised rows, bf16
    p.off_a = ws.take((size_t)rows * aw * 2);           // attention output, bf16
    p.off_o = ws.take((size_t)rows * c->width * 2);     // a sub-layer's output in front of its post-norm, bf16
    p.off_big = ws.take((size_t)rows * big * 2);        // qkv, then (up | gate)
    p.total = ws.end();
    return p;
}
int check_cfg(const mq_gemma_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_gemma: null cfg");
    MQ_CHECK_ARG(c->head_dim == 256, "mq_encode_gemma: head_dim %d unsupported (256)", c->head_dim);
    MQ_TRY(check_gqa_shape("mq_encode_gemma", c->q_heads, c->kv_heads, c->width));
    MQ_CHECK_ARG(c->width <= 2048, "mq_encode_gemma: width %d > 2048", c->width);
    MQ_TRY(check_tower_sizes("mq_encode_gemma", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->half_window >= 0, "mq_encode_gemma: half_window %d < 0", c->half_window);
    MQ_CHECK_ARG(c->attn_scale > 0.f && c->attn_scale <= 1e6f, "mq_encode_gemma: attn_scale %g must be positive and finite", (double)c->attn_scale);
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_CLS, "mq_encode_gemma: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_CLS)", c->pool);
    return MQ_OK;
}
}  // namespace

extern "C" int mq_rmsnorm_add_norm(float* d_x, const void* d_o, const float* d_g_post, const float* d_g_next, void* d_h, int64_t rows, int32_t W, float eps,
                                   void* stream) {
    MQ_CHECK_ARG(d_x && d_o && d_g_post, "mq_rmsnorm_add_norm: null pointer");
    MQ_CHECK_ARG((d_g_next == nullptr) == (d_h == nullptr), "mq_rmsnorm_add_norm: the second norm's weight and output come together or not at all");
    MQ_CHECK_ARG(W >= 4 && W % 4 == 0 && W <= 2048, "mq_rmsnorm_add_norm: W=%d unsupported (multiple of 4, <= 2048)", W);
    if (rows <= 0) return MQ_OK;
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(1, s);
    MQ_DISPATCH_CH(W, hipLaunchKernelGGL((rmsnorm_add_norm_kernel<CH>), dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, d_x, (const bf16_t*)d_o, d_g_post,
                                         d_g_next, (bf16_t*)d_h, rows, (int)W, eps));
    MQ_CHECK_LAUNCH("mq_rmsnorm_add_norm");
    return MQ_OK;
}

extern "C" int mq_glu_tanh(void* d_buf, int64_t rows, int32_t F, void* stream) {
    MQ_CHECK_ARG(d_buf, "mq_glu_tanh: null pointer");
    MQ_CHECK_ARG(F >= 8 && F % 8 == 0, "mq_glu_tanh: F=%d must be a multiple of 8", F);
    if (rows <= 0) return MQ_OK;
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(3, s);
    const int64_t blocks = cdiv64(rows * (F >> 3), 256);
    hipLaunchKernelGGL(glu_tanh_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, s, (bf16_t*)d_buf, rows, (int)F);
    MQ_CHECK_LAUNCH("mq_glu_tanh");
    return MQ_OK;
}

extern "C" size_t mq_gemma_workspace_bytes(const mq_gemma_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return plan(cfg, rows).total;
}

extern "C" int mq_encode_gemma(const mq_gemma_cfg* cfg, const mq_gemma_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens,
                               int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_gemma: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->final_norm_g && w->d_inv_freq_global && w->d_inv_freq_local && w->layers, "mq_encode_gemma: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_gemma_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.input_norm_g && b.qkv_w && b.q_norm_g && b.k_norm_g && b.out_w && b.post_attn_norm_g && b.pre_ffn_norm_g && b.ug_w && b.down_w &&
                         b.post_ffn_norm_g, "mq_encode_gemma: layer %d has null weights", l);
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_gemma", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const Plan p = plan(cfg, rows);
    MQ_TRY(packed_workspace("mq_encode_gemma", workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* o = base + p.off_o;
    void* big = base + p.off_big;
    const int W = cfg->width, F = cfg->mlp_dim, Q = cfg->q_heads, KV = cfg->kv_heads, hd = cfg->head_dim;
    const int AW = Q * hd, QKVW = (Q + 2 * KV) * hd;

    {   // embed_tokens * sqrt(W): a gather, no positions, no norm
        MqProfScope prof(3, s);
        hipLaunchKernelGGL(embed_scaled_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, d_ids, w->tok_emb, x, rows, W, cfg->vocab, sqrtf((float)W));
        MQ_CHECK_LAUNCH("mq_encode_gemma: embed");
    }
    MQ_TRY(mq_rmsnorm(x, nullptr, w->layers[0].input_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_gemma_layer& b = w->layers[l];
        const bool last = l == cfg->layers - 1;
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, nullptr, nullptr, big, QKVW, rows, QKVW, W, 0, s));
        MQ_TRY(mq_qk_norm_rope(big, d_cu_seqlens, nseq, 0, Q, KV, hd, b.q_norm_g, b.k_norm_g, cfg->rms_eps, b.sliding ? w->d_inv_freq_local : w->d_inv_freq_global, s));
        MQ_TRY(mq_attention_gqa_band(big, a, d_cu_seqlens, nseq, 0, maxl, Q, KV, hd, b.sliding ? cfg->half_window : 0, cfg->attn_scale, s));
        MQ_TRY(mq_gemm_bf16(a, AW, b.out_w, AW, nullptr, nullptr, o, W, rows, W, AW, 0, s));
        MQ_TRY(mq_rmsnorm_add_norm(x, o, b.post_attn_norm_g, b.pre_ffn_norm_g, h, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.ug_w, W, nullptr, nullptr, big, 2 * F, rows, 2 * F, W, 0, s));
        MQ_TRY(mq_glu_tanh(big, rows, F, s));
        MQ_TRY(mq_gemm_bf16(big, 2 * F, b.down_w, F, nullptr, nullptr, o, W, rows, W, F, 0, s));
        MQ_TRY(mq_rmsnorm_add_norm(x, o, b.post_ffn_norm_g, last ? nullptr : w->layers[l + 1].input_norm_g, last ? nullptr : h, rows, W, cfg->rms_eps, s));
    }
    MQ_TRY(mq_rmsnorm(x, nullptr, w->final_norm_g, nullptr, x, rows, W, cfg->rms_eps, s));   // (in place: a wave holds its whole row before it stores)
    MQ_TRY(mq_pool(x, d_cu_seqlens, nseq, d_out, W, cfg->pool, normalize, s));
    return MQ_OK;
}
