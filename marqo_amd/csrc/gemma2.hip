// Gemma2 text embedders (transformers Gemma2Model: BAAI/bge-multilingual-gemma2 and the Gemma-2-2B-shaped fine-tunes) on one HIP stream, no allocation, no
// sync: the post-norm + residual add + next pre-norm row kernel for rows up to 4096 wide, and the host-side orchestration of the tower.  The block is
// gemma.hip's — an RMSNorm in front of and behind each sub-layer, a gated tanh-GELU MLP, the token table scaled by sqrt(width) — without q / k norm, with
// one rotary base, under a causal mask, with soft-capped attention logits and a causal sliding window on the layers the config names
// (attention_gqa256_softcap.hip).  Everything else is the sibling units': the bf16 GEMMs, mq_rmsnorm_wide / mq_embed_tokens_wide / mq_pool_wide
// (llama.hip), mq_qk_norm_rope with null gains (qwen.hip), mq_glu_tanh (gemma.hip), mq_last_rows and mq_l2_normalize.
//
// Per block, on the fp32 residual stream x [rows, W] (no Linear has a bias; every norm weight arrives as 1 + w, folded at load):
//   h = rmsnorm(x, input_layernorm)                                  (layer 0: mq_rmsnorm_wide; later layers: the tail of the previous block's add_norm)
//   qkv = h Wqkv^T ; rope(qkv) ; a = attention_gqa256_softcap(qkv, window on sliding layers, softcap, attn_scale)
//   o = a Wo^T (bf16) ; x += rmsnorm(o, post_attention_layernorm) ; h = rmsnorm(x, pre_feedforward_layernorm)          (one pass: mq_rmsnorm_add_norm_wide)
//   (up | gate) = h Wug^T ; p = up * gelu_tanh(gate) ; o = p Wdown^T (bf16)
//   x += rmsnorm(o, post_feedforward_layernorm) ; h = rmsnorm(x, the next block's input_layernorm)                     (one pass; none after the last)
// then the final RMSNorm and the pooling (+ L2) as llama.hip does them: the last token's row alone, or every row and the mean.
//
// Why mq_rmsnorm_add_norm_wide and not a lifted bound: mq_rmsnorm_add_norm refuses W > 2048, and callers and tests rely on that refusal.  The wide entry
// point hands W <= 2048 to it (the same bits) and runs the kernel below above it: gemma.hip's rmsnorm_add_norm_kernel at up to 16 float4 chunks per lane
// — one wave64 per row, the whole row of o (bf16) and of x (fp32) in registers from the first load to the last store (2 x 64 VGPRs at 16 chunks), both
// statistics in mq_rmsnorm's order, the gains read at the stores as rmsnorm_wide_kernel reads them.  Compiler report at 16 chunks: 166 VGPRs, 3 waves / SIMD, no scratch.
//
// The checks in front of the first launch and the workspace arithmetic are the packed-token scaffold of packed_text.h.
#include "packed_text.h"

static_assert(sizeof(mq_gemma2_cfg) == 56, "Gemma2 layout (marqo_amd/_lib.py)");

namespace {

constexpr int WIDE_MAX_W = 4096;   // 16 float4 chunks per lane of a wave64

__device__ __forceinline__ f32x4 bf16x4_to_f32(uint2 q) {
    return f32x4{__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u), __uint_as_float(q.y << 16), __uint_as_float(q.y & 0xffff0000u)};
}

// x += rmsnorm(o; g_post) ; h = rmsnorm(x; g_next).  Per lane ((a^2 + b^2) + (c^2 + d^2)) summed over its chunks, the butterfly over the wave, / W + eps,
// rsqrtf; every product (v * rstd) * g.  h is written only when g_next is given.
template <int CH>
__global__ __launch_bounds__(256) void rmsnorm_add_norm_wide_kernel(float* __restrict__ x, const bf16_t* __restrict__ o, const float* __restrict__ g_post,
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
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        if (c < nch) {
            xv[i] += (v[i] * rstd) * *(const f32x4*)(g_post + c * 4);
            *(f32x4*)(x + row * W + c * 4) = xv[i];
        }
        s2 += (xv[i][0] * xv[i][0] + xv[i][1] * xv[i][1]) + (xv[i][2] * xv[i][2] + xv[i][3] * xv[i][3]);
    }
    if (!g_next) return;
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

struct Plan { size_t off_x, off_h, off_a, off_o, off_big, off_rows, total; };
Plan plan(const mq_gemma2_cfg* c, int64_t rows, int64_t nseq) {
    Plan p;
    Off ws;
    const size_t aw = (size_t)c->q_heads * c->head_dim, qkvw = (size_t)(c->q_heads + 2 * c->kv_heads) * c->head_dim;
    const size_t big = qkvw > 2 * (size_t)c->mlp_dim ? qkvw : 2 * (size_t)c->mlp_dim;
    p.off_x = ws.take((size_t)rows * c->width * 4);     // residual stream, fp32
    p.off_h = ws.take((size_t)rows * c->width * 2);     // normalised rows, bf16
    p.off_a = ws.take((size_t)rows * aw * 2);           // attention output, bf16
    p.off_o = ws.take((size_t)rows * c->width * 2);     // a sub-layer's output in front of its post-norm, bf16
    p.off_big = ws.take((size_t)rows * big * 2);        // qkv, then (up | gate)
    p.off_rows = ws.take((size_t)nseq * 4);             // the pooled (last) row of every sequence
    p.total = ws.end();
    return p;
}
int check_cfg(const mq_gemma2_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_gemma2: null cfg");
    MQ_CHECK_ARG(c->head_dim == 256, "mq_encode_gemma2: head_dim %d unsupported (256)", c->head_dim);
    MQ_TRY(check_gqa_shape("mq_encode_gemma2", c->q_heads, c->kv_heads, c->width));
    MQ_CHECK_ARG(c->width <= WIDE_MAX_W, "mq_encode_gemma2: width %d > %d (larger models are not served)", c->width, WIDE_MAX_W);
    MQ_TRY(check_tower_sizes("mq_encode_gemma2", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->window >= 0, "mq_encode_gemma2: window %d must be at least 1, or 0 for none", c->window);
    MQ_CHECK_ARG(c->softcap > 0.f && c->softcap <= 64.f, "mq_encode_gemma2: softcap %g unsupported (0 < softcap <= 64)", (double)c->softcap);
    MQ_CHECK_ARG(c->attn_scale > 0.f && c->attn_scale <= 1e6f, "mq_encode_gemma2: attn_scale %g must be positive and finite", (double)c->attn_scale);
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_LAST, "mq_encode_gemma2: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_LAST)", c->pool);
    return MQ_OK;
}
}  // namespace

extern "C" int mq_rmsnorm_add_norm_wide(float* d_x, const void* d_o, const float* d_g_post, const float* d_g_next, void* d_h, int64_t rows, int32_t W,
                                        float eps, void* stream) {
    MQ_CHECK_ARG(d_x && d_o && d_g_post, "mq_rmsnorm_add_norm_wide: null pointer");
    MQ_CHECK_ARG((d_g_next == nullptr) == (d_h == nullptr), "mq_rmsnorm_add_norm_wide: the second norm's weight and output come together or not at all");
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= WIDE_MAX_W, "mq_rmsnorm_add_norm_wide: W=%d unsupported (a multiple of 64, <= %d)", W, WIDE_MAX_W);
    if (W <= 2048) return mq_rmsnorm_add_norm(d_x, d_o, d_g_post, d_g_next, d_h, rows, W, eps, stream);
    if (rows <= 0) return MQ_OK;
    MQ_CHECK_ARG(cdiv64(rows, 4) < (1LL << 31), "mq_rmsnorm_add_norm_wide: grid too large (rows=%lld)", (long long)rows);
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(1, s);
    const dim3 grid((unsigned)cdiv64(rows, 4)), block(256);
    const int ch = (W / 4 + 63) / 64;   // 9 .. 16
#define MQ_ADD_NORM_WIDE(C) \
    hipLaunchKernelGGL((rmsnorm_add_norm_wide_kernel<C>), grid, block, 0, s, d_x, (const bf16_t*)d_o, d_g_post, d_g_next, (bf16_t*)d_h, rows, (int)W, eps)
    if (ch <= 10) MQ_ADD_NORM_WIDE(10); else if (ch <= 12) MQ_ADD_NORM_WIDE(12); else if (ch <= 14) MQ_ADD_NORM_WIDE(14); else MQ_ADD_NORM_WIDE(16);
#undef MQ_ADD_NORM_WIDE
    MQ_CHECK_LAUNCH("mq_rmsnorm_add_norm_wide");
    return MQ_OK;
}

extern "C" size_t mq_gemma2_workspace_bytes(const mq_gemma2_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return plan(cfg, rows, nseq).total;
}

extern "C" int mq_encode_gemma2(const mq_gemma2_cfg* cfg, const mq_gemma_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                                const int32_t* h_cu_seqlens, int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_gemma2: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->final_norm_g && w->d_inv_freq_global && w->layers, "mq_encode_gemma2: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_gemma_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.input_norm_g && b.qkv_w && b.out_w && b.post_attn_norm_g && b.pre_ffn_norm_g && b.ug_w && b.down_w && b.post_ffn_norm_g,
                     "mq_encode_gemma2: layer %d has null weights", l);
        MQ_CHECK_ARG(!b.q_norm_g && !b.k_norm_g, "mq_encode_gemma2: layer %d carries q / k norm weights (this block has none)", l);
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_gemma2", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const Plan p = plan(cfg, rows, nseq);
    MQ_TRY(packed_workspace("mq_encode_gemma2", workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* o = base + p.off_o;
    void* big = base + p.off_big;
    int32_t* last = (int32_t*)(base + p.off_rows);
    const int W = cfg->width, F = cfg->mlp_dim, Q = cfg->q_heads, KV = cfg->kv_heads, hd = cfg->head_dim;
    const int AW = Q * hd, QKVW = (Q + 2 * KV) * hd;

    MQ_TRY(mq_embed_tokens_wide(d_ids, d_cu_seqlens, nseq, w->tok_emb, x, W, cfg->vocab, s));   // (the table arrives times sqrtf(W))
    MQ_TRY(mq_rmsnorm_wide(x, nullptr, w->layers[0].input_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_gemma_layer& b = w->layers[l];
        const bool tail = l == cfg->layers - 1;
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, nullptr, nullptr, big, QKVW, rows, QKVW, W, 0, s));
        MQ_TRY(mq_qk_norm_rope(big, d_cu_seqlens, nseq, 0, Q, KV, hd, nullptr, nullptr, cfg->rms_eps, w->d_inv_freq_global, s));
        MQ_TRY(mq_attention_gqa256_softcap(big, a, d_cu_seqlens, nseq, 0, maxl, Q, KV, hd, b.sliding ? cfg->window : 0, cfg->softcap, cfg->attn_scale, s));
        MQ_TRY(mq_gemm_bf16(a, AW, b.out_w, AW, nullptr, nullptr, o, W, rows, W, AW, 0, s));
        MQ_TRY(mq_rmsnorm_add_norm_wide(x, o, b.post_attn_norm_g, b.pre_ffn_norm_g, h, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.ug_w, W, nullptr, nullptr, big, 2 * F, rows, 2 * F, W, 0, s));
        MQ_TRY(mq_glu_tanh(big, rows, F, s));
        MQ_TRY(mq_gemm_bf16(big, 2 * F, b.down_w, F, nullptr, nullptr, o, W, rows, W, F, 0, s));
        MQ_TRY(mq_rmsnorm_add_norm_wide(x, o, b.post_ffn_norm_g, tail ? nullptr : w->layers[l + 1].input_norm_g, tail ? nullptr : h, rows, W, cfg->rms_eps, s));
    }
    if (cfg->pool == MQ_POOL_LAST) {   // the final norm is per row: only the pooled rows take it
        MQ_TRY(mq_last_rows(d_cu_seqlens, last, nseq, s));
        MQ_TRY(mq_rmsnorm_wide(x, last, w->final_norm_g, nullptr, d_out, nseq, W, cfg->rms_eps, s));
        if (normalize) MQ_TRY(mq_l2_normalize(d_out, d_out, nseq, W, s));
    } else {
        MQ_TRY(mq_rmsnorm_wide(x, nullptr, w->final_norm_g, nullptr, x, rows, W, cfg->rms_eps, s));   // (in place: a wave holds its whole row before it stores)
        MQ_TRY(mq_pool_wide(x, d_cu_seqlens, nseq, d_out, W, normalize, s));
    }
    return MQ_OK;
}
