// ModernBERT text tower (transformers ModernBertModel) on one HIP stream, no allocation, no sync: host-side orchestration of kernels that live in the
// sibling units — token embedding + LayerNorm (embed.hip), LayerNorm (rowops.hip), the bf16 GEMMs, rotary positions and the gated-GELU product
// (embed.hip: mq_rope, mq_glu), full attention (attention.hip) and the band kernel of the sliding layers (attention_window.hip), pooling.
//
// Per block, on the fp32 residual stream x [rows, W] (pre-LN; no Linear and no LayerNorm has a bias):
//   h = attn_norm(x)                       (layer 0: h = bf16(x), the embedding LayerNorm's output is used as it is)
//   qkv = h Wqkv^T ; rope(q, k) with the layer kind's inverse frequencies ; a = attention(qkv) — a band of half_window keys on a sliding layer
//   x += a Wo^T
//   (up | gate) = mlp_norm(x) Wi'^T  (Wi' = mlp.Wi with its halves swapped at load) ; p = up * gelu(gate) ; x += p mlp.Wo^T
// then final_norm over every row and the loaders' mean / CLS pooling (+ L2).
//
// The checks in front of the first launch and the workspace arithmetic are the packed-token scaffold of packed_text.h.
#include "packed_text.h"

int mq_cast_bf16(const float* d_x, void* d_out, int64_t n, hipStream_t s);   // rowops.hip

static_assert(sizeof(mq_modernbert_layer) == 56 && sizeof(mq_modernbert_weights) == 56 && sizeof(mq_modernbert_cfg) == 40, "ModernBERT layouts (marqo_amd/_lib.py)");

namespace {
struct Plan { size_t off_x, off_h, off_a, off_big, total; };
Plan plan(const mq_modernbert_cfg* c, int64_t rows) {
    Plan p;
    Off ws;
    const size_t big = (size_t)(3 * c->width > 2 * c->mlp_dim ? 3 * c->width : 2 * c->mlp_dim);
    p.off_x = ws.take((size_t)rows * c->width * 4);     // residual stream, fp32
    p.off_h = ws.take((size_t)rows * c->width * 2);     // normalised rows, bf16
    p.off_a = ws.take((size_t)rows * c->width * 2);     // attention output, bf16
    p.off_big = ws.take((size_t)rows * big * 2);        // qkv, then (up | gate)
    p.total = ws.end();
    return p;
}
int check_cfg(const mq_modernbert_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_modernbert: null cfg");
    MQ_CHECK_ARG(c->heads >= 1 && c->width == c->heads * 64, "mq_encode_modernbert: 64-wide heads only (width %d, heads %d)", c->width, c->heads);
    MQ_CHECK_ARG(c->width <= 2048, "mq_encode_modernbert: width %d > 2048", c->width);
    MQ_TRY(check_tower_sizes("mq_encode_modernbert", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->half_window >= 0, "mq_encode_modernbert: half_window %d < 0", c->half_window);
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_CLS, "mq_encode_modernbert: bad pooling %d", c->pool);
    return MQ_OK;
}
}  // namespace

extern "C" size_t mq_modernbert_workspace_bytes(const mq_modernbert_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return plan(cfg, rows).total;
}

extern "C" int mq_encode_modernbert(const mq_modernbert_cfg* cfg, const mq_modernbert_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                                    const int32_t* h_cu_seqlens, int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes,
                                    void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_modernbert: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->emb_ln_g && w->final_ln_g && w->zeros && w->d_inv_freq_global && w->d_inv_freq_local && w->layers,
                 "mq_encode_modernbert: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_modernbert_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.qkv_w && b.out_w && b.mlp_norm_g && b.wi_w && b.wo_w && (l == 0 || b.attn_norm_g), "mq_encode_modernbert: layer %d has null weights", l);
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_modernbert", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const Plan p = plan(cfg, rows);
    MQ_TRY(packed_workspace("mq_encode_modernbert", workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* big = base + p.off_big;
    const int W = cfg->width, F = cfg->mlp_dim;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;   // (the bias is w->zeros)

    // tok_embeddings -> LayerNorm: fp32 into the stream, bf16 into h (layer 0's GEMM operand)
    MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq, w->tok_emb, nullptr, nullptr, w->emb_ln_g, w->zeros, x, h, W, cfg->vocab, cfg->ln_eps, 0, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_modernbert_layer& b = w->layers[l];
        if (b.attn_norm_g) MQ_TRY(mq_layernorm(x, nullptr, b.attn_norm_g, w->zeros, h, nullptr, rows, W, cfg->ln_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, nullptr, nullptr, big, 3 * W, rows, 3 * W, W, 0, s));
        MQ_TRY(mq_rope(big, d_cu_seqlens, nseq, 0, W, cfg->heads, b.sliding ? w->d_inv_freq_local : w->d_inv_freq_global, s));
        if (b.sliding) MQ_TRY(mq_attention_window(big, a, d_cu_seqlens, nseq, 0, maxl, W, cfg->heads, cfg->half_window, s));
        else MQ_TRY(mq_attention(big, a, d_cu_seqlens, nseq, 0, maxl, W, cfg->heads, MQ_MASK_NONE, s));
        MQ_TRY(mq_gemm_bf16(a, W, b.out_w, W, w->zeros, x, x, W, rows, W, W, res_flags, s));
        MQ_TRY(mq_layernorm(x, nullptr, b.mlp_norm_g, w->zeros, h, nullptr, rows, W, cfg->ln_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.wi_w, W, nullptr, nullptr, big, 2 * F, rows, 2 * F, W, 0, s));
        MQ_TRY(mq_glu(big, rows, F, MQ_ACT_GELU, 0, s));
        MQ_TRY(mq_gemm_bf16(big, 2 * F, b.wo_w, F, w->zeros, x, x, W, rows, W, F, res_flags, s));
    }
    MQ_TRY(mq_layernorm(x, nullptr, w->final_ln_g, w->zeros, nullptr, x, rows, W, cfg->ln_eps, s));
    MQ_TRY(mq_pool(x, d_cu_seqlens, nseq, d_out, W, cfg->pool, normalize, s));
    return MQ_OK;
}
