// Mistral / Llama text embedders (transformers MistralModel / LlamaModel: e5-mistral-7b-instruct, SFR-Embedding-Mistral, Linq-Embed-Mistral, Llama-2-shaped
// fine-tunes) on one HIP stream, no allocation, no sync: the row kernels this family adds — RMSNorm, the token gather and mean pooling for rows up to 4096
// wide — and the host-side orchestration of the tower.  The block is qwen.hip's without q / k norm and without a QKV bias; the GEMMs, the rotary step
// (mq_qk_norm_rope with null gains), the gated-SiLU product and causal grouped-query attention are the sibling units', and the sliding window is
// attention_gqa.hip's mq_attention_gqa_window.
//
// Why new entry points and not a lifted bound: mq_rmsnorm, mq_embed_tokens and mq_pool refuse W > 2048, and callers and tests rely on those refusals.  The
// wide entry points hand W <= 2048 to them (the same bits) and run the kernels below above it.
//
// The wide RMSNorm keeps the form of rmsnorm_kernel — one wave64 per row, the whole row in registers (up to 16 float4 chunks per lane = 64 VGPRs), fp32
// statistics in one pass, one rounding to bf16 — so it may run in place.  A workgroup per row with an LDS reduction buys nothing at 16 KiB per row: one
// wave issues its sixteen 1-KiB loads back to back.  The gain is read at the store, not ahead of the reduction as rmsnorm_kernel reads it (the W floats
// every wave shares come from the cache); the compiler reports 110 VGPRs at 16 chunks, 4 waves / SIMD, no scratch.
//
// The checks in front of the first launch and the workspace arithmetic are the packed-token scaffold of packed_text.h.
#include "packed_text.h"

static_assert(sizeof(mq_llama_cfg) == 48, "Llama layout (marqo_amd/_lib.py)");

namespace {

constexpr int WIDE_MAX_W = 4096;   // 16 float4 chunks per lane of a wave64

template <int CH>
__global__ __launch_bounds__(256) void rmsnorm_wide_kernel(const float* x /* may alias out_f32 */, const int32_t* __restrict__ row_idx, const float* __restrict__ gam,
                                                           bf16_t* out_bf16, float* out_f32, int64_t rows, int W, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nch = W >> 2;
    const int64_t src = row_idx ? (int64_t)row_idx[row] : row;
    f32x4 v[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        v[i] = c < nch ? *(const f32x4*)(x + src * W + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) ss += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
    const float rstd = rsqrtf(wave_sum(ss) / (float)W + eps);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        if (c >= nch) continue;
        const f32x4 y = (v[i] * rstd) * *(const f32x4*)(gam + c * 4);
        if (out_f32) *(f32x4*)(out_f32 + row * W + c * 4) = y;
        if (out_bf16) {
            uint2 p;
            p.x = pack_bf16x2(y[0], y[1]);
            p.y = pack_bf16x2(y[2], y[3]);
            *(uint2*)(out_bf16 + row * W + c * 4) = p;
        }
    }
}

// token gather: grid = sequences, the 4 waves of a block walk the sequence's rows, a lane copies float4 chunks lane, lane + 64, ...
__global__ __launch_bounds__(256) void embed_tokens_wide_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ cu, const float* __restrict__ tok,
                                                                float* __restrict__ x, int W, int vocab) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = cu[blockIdx.x], len = cu[blockIdx.x + 1] - row0;
    const int nch = W >> 2;
    for (int t = wave; t < len; t += 4) {
        const int64_t row = row0 + t;
        int id = ids[row];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        const float* tr = tok + (int64_t)id * W;
        for (int c = lane; c < nch; c += 64) *(f32x4*)(x + row * W + c * 4) = *(const f32x4*)(tr + c * 4);
    }
}

// mean pooling over packed sequences (+ L2): pool_kernel's arithmetic in its order (a column's rows summed first to last, one division by the length;
// F.normalize's x / max(||x||, 1e-12)) with 16 columns per thread.  grid = sequences.
__global__ __launch_bounds__(256) void pool_wide_kernel(const float* __restrict__ x, const int32_t* __restrict__ cu, float* __restrict__ out, int W, int normalize) {
    __shared__ float red[4];
    const int row0 = cu[blockIdx.x], len = cu[blockIdx.x + 1] - row0;
    float acc[16];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        acc[i] = 0.f;
        const int c = threadIdx.x + i * 256;
        if (c < W) {
            float s = 0.f;
            for (int t = 0; t < len; ++t) s += x[(int64_t)(row0 + t) * W + c];
            acc[i] = s / (float)len;
            ss += acc[i] * acc[i];
        }
    }
    float inv = 1.f;
    if (normalize) {
        ss = wave_sum(ss);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
        __syncthreads();
        const float tot = red[0] + red[1] + red[2] + red[3];
        inv = 1.0f / fmaxf(sqrtf(tot), 1e-12f);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = threadIdx.x + i * 256;
        if (c < W) out[(int64_t)blockIdx.x * W + c] = acc[i] * inv;
    }
}

int check_wide_w(const char* fn, int W) {
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= WIDE_MAX_W, "%s: W=%d unsupported (a multiple of 64, <= %d)", fn, W, WIDE_MAX_W);
    return MQ_OK;
}

struct Plan { size_t off_x, off_h, off_a, off_big, off_rows, total; };
Plan plan(const mq_llama_cfg* c, int64_t rows, int64_t nseq) {
    Plan p;
    Off ws;
    const size_t aw = (size_t)c->q_heads * c->head_dim, qkvw = (size_t)(c->q_heads + 2 * c->kv_heads) * c->head_dim;
    const size_t big = qkvw > 2 * (size_t)c->mlp_dim ? qkvw : 2 * (size_t)c->mlp_dim;
    p.off_x = ws.take((size_t)rows * c->width * 4);     // residual stream, fp32
    p.off_h = ws.take((size_t)rows * c->width * 2);     // normalised rows, bf16
    p.off_a = ws.take((size_t)rows * aw * 2);           // attention output, bf16
    p.off_big = ws.take((size_t)rows * big * 2);        // qkv, then (up | gate)
    p.off_rows = ws.take((size_t)nseq * 4);             // the pooled (last) row of every sequence
    p.total = ws.end();
    return p;
}
int check_cfg(const mq_llama_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_llama: null cfg");
    MQ_CHECK_ARG(c->head_dim == 64 || c->head_dim == 128, "mq_encode_llama: head_dim %d unsupported (64 or 128)", c->head_dim);
    MQ_TRY(check_gqa_shape("mq_encode_llama", c->q_heads, c->kv_heads, c->width));
    MQ_CHECK_ARG(c->width <= WIDE_MAX_W, "mq_encode_llama: width %d > %d (larger models are not served)", c->width, WIDE_MAX_W);
    MQ_TRY(check_tower_sizes("mq_encode_llama", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_LAST, "mq_encode_llama: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_LAST)", c->pool);
    MQ_CHECK_ARG(c->window >= 0, "mq_encode_llama: window %d must be at least 1, or 0 for none", c->window);
    return MQ_OK;
}
}  // namespace

extern "C" int mq_rmsnorm_wide(const float* d_x, const int32_t* d_row_idx, const float* d_g, void* d_out_bf16, float* d_out_f32, int64_t rows, int32_t W,
                               float eps, void* stream) {
    MQ_CHECK_ARG(d_x && d_g && (d_out_bf16 || d_out_f32), "mq_rmsnorm_wide: null pointer");
    MQ_TRY(check_wide_w("mq_rmsnorm_wide", W));
    if (W <= 2048) return mq_rmsnorm(d_x, d_row_idx, d_g, d_out_bf16, d_out_f32, rows, W, eps, stream);
    if (rows <= 0) return MQ_OK;
    MQ_CHECK_ARG(cdiv64(rows, 4) < (1LL << 31), "mq_rmsnorm_wide: grid too large (rows=%lld)", (long long)rows);
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(1, s);
    const dim3 grid((unsigned)cdiv64(rows, 4)), block(256);
    const int ch = (W / 4 + 63) / 64;   // 9 .. 16
#define MQ_RMS_WIDE(C) hipLaunchKernelGGL((rmsnorm_wide_kernel<C>), grid, block, 0, s, d_x, d_row_idx, d_g, (bf16_t*)d_out_bf16, d_out_f32, rows, (int)W, eps)
    if (ch <= 10) MQ_RMS_WIDE(10); else if (ch <= 12) MQ_RMS_WIDE(12); else MQ_RMS_WIDE(16);
#undef MQ_RMS_WIDE
    MQ_CHECK_LAUNCH("mq_rmsnorm_wide");
    return MQ_OK;
}

extern "C" int mq_embed_tokens_wide(const int32_t* d_ids, const int32_t* d_cu, int64_t nseq, const float* tok, float* d_x, int32_t W, int32_t vocab,
                                    void* stream) {
    MQ_CHECK_ARG(d_ids && d_cu && tok && d_x, "mq_embed_tokens_wide: null pointer");
    MQ_TRY(check_wide_w("mq_embed_tokens_wide", W));
    MQ_CHECK_ARG(vocab >= 1, "mq_embed_tokens_wide: vocab %d", vocab);
    if (W <= 2048) return mq_embed_tokens(d_ids, d_cu, nseq, tok, nullptr, nullptr, nullptr, nullptr, d_x, nullptr, W, vocab, 0.f, 0, stream);
    if (nseq <= 0) return MQ_OK;
    MQ_CHECK_ARG(nseq < (1LL << 31), "mq_embed_tokens_wide: grid too large");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(3, s);
    hipLaunchKernelGGL(embed_tokens_wide_kernel, dim3((unsigned)nseq), dim3(256), 0, s, d_ids, d_cu, tok, d_x, (int)W, (int)vocab);
    MQ_CHECK_LAUNCH("mq_embed_tokens_wide");
    return MQ_OK;
}

extern "C" int mq_pool_wide(const float* d_x, const int32_t* d_cu, int64_t nseq, float* d_out, int32_t W, int32_t normalize, void* stream) {
    MQ_CHECK_ARG(d_x && d_cu && d_out, "mq_pool_wide: null pointer");
    MQ_TRY(check_wide_w("mq_pool_wide", W));
    if (W <= 2048) return mq_pool(d_x, d_cu, nseq, d_out, W, MQ_POOL_MEAN, normalize, stream);
    if (nseq <= 0) return MQ_OK;
    MQ_CHECK_ARG(nseq < (1LL << 31), "mq_pool_wide: grid too large");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(4, s);
    hipLaunchKernelGGL(pool_wide_kernel, dim3((unsigned)nseq), dim3(256), 0, s, d_x, d_cu, d_out, (int)W, (int)normalize);
    MQ_CHECK_LAUNCH("mq_pool_wide");
    return MQ_OK;
}

extern "C" size_t mq_llama_workspace_bytes(const mq_llama_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return plan(cfg, rows, nseq).total;
}

extern "C" int mq_encode_llama(const mq_llama_cfg* cfg, const mq_qwen_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens,
                               int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_llama: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->final_norm_g && w->zeros && w->d_inv_freq && w->layers, "mq_encode_llama: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_qwen_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.input_norm_g && b.qkv_w && b.out_w && b.post_norm_g && b.ug_w && b.down_w, "mq_encode_llama: layer %d has null weights", l);
        MQ_CHECK_ARG(!b.qkv_b && !b.q_norm_g && !b.k_norm_g, "mq_encode_llama: layer %d carries a QKV bias or q / k norm weights (this block has neither)", l);
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_llama", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const Plan p = plan(cfg, rows, nseq);
    MQ_TRY(packed_workspace("mq_encode_llama", workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* big = base + p.off_big;
    int32_t* last = (int32_t*)(base + p.off_rows);
    const int W = cfg->width, F = cfg->mlp_dim, Q = cfg->q_heads, KV = cfg->kv_heads, hd = cfg->head_dim;
    const int AW = Q * hd, QKVW = (Q + 2 * KV) * hd;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;   // (the bias is w->zeros)
    const bool windowed = cfg->window > 0 && cfg->window < maxl;            // (a window no sequence of the call reaches cuts nothing)

    MQ_TRY(mq_embed_tokens_wide(d_ids, d_cu_seqlens, nseq, w->tok_emb, x, W, cfg->vocab, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_qwen_layer& b = w->layers[l];
        MQ_TRY(mq_rmsnorm_wide(x, nullptr, b.input_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, nullptr, nullptr, big, QKVW, rows, QKVW, W, 0, s));
        MQ_TRY(mq_qk_norm_rope(big, d_cu_seqlens, nseq, 0, Q, KV, hd, nullptr, nullptr, cfg->rms_eps, w->d_inv_freq, s));
        if (windowed) MQ_TRY(mq_attention_gqa_window(big, a, d_cu_seqlens, nseq, 0, maxl, Q, KV, hd, cfg->window, s));
        else MQ_TRY(mq_attention_gqa(big, a, d_cu_seqlens, nseq, 0, maxl, Q, KV, hd, MQ_MASK_CAUSAL, s));
        MQ_TRY(mq_gemm_bf16(a, AW, b.out_w, AW, w->zeros, x, x, W, rows, W, AW, res_flags, s));
        MQ_TRY(mq_rmsnorm_wide(x, nullptr, b.post_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.ug_w, W, nullptr, nullptr, big, 2 * F, rows, 2 * F, W, 0, s));
        MQ_TRY(mq_glu(big, rows, F, MQ_ACT_SILU, 0, s));
        MQ_TRY(mq_gemm_bf16(big, 2 * F, b.down_w, F, w->zeros, x, x, W, rows, W, F, res_flags, s));
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
