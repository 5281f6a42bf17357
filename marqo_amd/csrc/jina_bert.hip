// JinaBERT text tower (jina-embeddings-v2-small-en / -base-en and their fine-tunes, MosaicBERT-style ALiBi encoders with the same block) on one HIP
// stream, no allocation, no sync: host-side orchestration of kernels that live in the sibling units — token gather + type row + LayerNorm (embed.hip),
// LayerNorm (rowops.hip), the bf16 GEMMs with their bias / residual epilogues, the erf-GELU gated product (embed.hip: mq_glu), the ALiBi attention
// (attention_alibi.hip), pooling.  The block semantics restate the published architecture; they are not pinned to a run of the original modelling code.
//
// Post-LN blocks on the fp32 residual stream x [rows, W], with a bf16 copy h of it for the GEMMs:
//   x, h = LN_emb(tok[ids] + type_emb[0])                          (no position table)
//   qkv = h Wqkv^T + bqkv                                          (rows query | key | value, fused at load)
//   a = attention_alibi(qkv, slopes, 1 / sqrt(head_dim))
//   x, h = LN_attn(a Wo^T + bo + x)
//   (up | gate) = h Wg'^T                                          (no bias; Wg' = mlp.gated_layers with its halves swapped at load)
//   p = up * gelu_erf(gate)
//   x, h = LN_mlp(p Wwo^T + bwo + x)
// then mean / CLS pooling over x (+ L2).  No final norm.
//
// The checks in front of the first launch and the workspace arithmetic are the packed-token scaffold of packed_text.h.
#include "packed_text.h"

static_assert(sizeof(mq_jina_bert_layer) == 88 && sizeof(mq_jina_bert_weights) == 48 && sizeof(mq_jina_bert_cfg) == 40, "JinaBERT layouts (marqo_amd/_lib.py)");

namespace {
struct Plan { size_t off_x, off_h, off_a, off_big, total; };
Plan plan(const mq_jina_bert_cfg* c, int64_t rows) {
    Plan p;
    Off ws;
    const size_t big = (size_t)(3 * c->width > 2 * c->mlp_dim ? 3 * c->width : 2 * c->mlp_dim);
    p.off_x = ws.take((size_t)rows * c->width * 4);     // residual stream, fp32
    p.off_h = ws.take((size_t)rows * c->width * 2);     // the same rows, bf16
    p.off_a = ws.take((size_t)rows * c->width * 2);     // attention output, bf16
    p.off_big = ws.take((size_t)rows * big * 2);        // qkv, then (up | gate)
    p.total = ws.end();
    return p;
}
int check_cfg(const mq_jina_bert_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_jina_bert: null cfg");
    MQ_CHECK_ARG(c->head_dim == 64, "mq_encode_jina_bert: head_dim %d unsupported (64)", c->head_dim);
    MQ_CHECK_ARG(c->width >= 64 && c->width % 64 == 0 && c->width <= 2048, "mq_encode_jina_bert: width %d must be a multiple of 64, at most 2048", c->width);
    MQ_CHECK_ARG(c->heads >= 1 && c->heads * 64 == c->width, "mq_encode_jina_bert: heads %d x 64 is not the width %d", c->heads, c->width);
    MQ_TRY(check_tower_sizes("mq_encode_jina_bert", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_CLS, "mq_encode_jina_bert: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_CLS)", c->pool);
    return MQ_OK;
}
}  // namespace

extern "C" size_t mq_jina_bert_workspace_bytes(const mq_jina_bert_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return plan(cfg, rows).total;
}

extern "C" int mq_encode_jina_bert(const mq_jina_bert_cfg* cfg, const mq_jina_bert_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                                   const int32_t* h_cu_seqlens, int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes,
                                   void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_jina_bert: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->type0 && w->emb_ln_g && w->emb_ln_b && w->d_slopes && w->layers, "mq_encode_jina_bert: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_jina_bert_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.qkv_w && b.qkv_b && b.out_w && b.out_b && b.attn_ln_g && b.attn_ln_b && b.wg_w && b.wo_w && b.wo_b && b.mlp_ln_g && b.mlp_ln_b,
                     "mq_encode_jina_bert: layer %d has null weights", l);
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_jina_bert", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const Plan p = plan(cfg, rows);
    MQ_TRY(packed_workspace("mq_encode_jina_bert", workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* big = base + p.off_big;
    const int W = cfg->width, F = cfg->mlp_dim, H = cfg->heads, hd = cfg->head_dim;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;
    const float scale = 1.0f / sqrtf((float)hd);

    // word_embeddings + token_type_embeddings[0] -> LayerNorm: fp32 into the stream, bf16 into h; no position table
    MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq, w->tok_emb, nullptr, w->type0, w->emb_ln_g, w->emb_ln_b, x, h, W, cfg->vocab, cfg->ln_eps, 0, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_jina_bert_layer& b = w->layers[l];
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, b.qkv_b, nullptr, big, 3 * W, rows, 3 * W, W, MQ_EPI_BIAS, s));
        MQ_TRY(mq_attention_alibi(big, a, d_cu_seqlens, nseq, 0, maxl, H, hd, w->d_slopes, scale, s));
        MQ_TRY(mq_gemm_bf16(a, W, b.out_w, W, b.out_b, x, x, W, rows, W, W, res_flags, s));
        MQ_TRY(mq_layernorm(x, nullptr, b.attn_ln_g, b.attn_ln_b, h, x, rows, W, cfg->ln_eps, s));   // (in place: a wave holds its whole row before it stores)
        MQ_TRY(mq_gemm_bf16(h, W, b.wg_w, W, nullptr, nullptr, big, 2 * F, rows, 2 * F, W, 0, s));
        MQ_TRY(mq_glu(big, rows, F, MQ_ACT_GELU, 0, s));
        MQ_TRY(mq_gemm_bf16(big, 2 * F, b.wo_w, F, b.wo_b, x, x, W, rows, W, F, res_flags, s));
        MQ_TRY(mq_layernorm(x, nullptr, b.mlp_ln_g, b.mlp_ln_b, h, x, rows, W, cfg->ln_eps, s));
    }
    MQ_TRY(mq_pool(x, d_cu_seqlens, nseq, d_out, W, cfg->pool, normalize, s));
    return MQ_OK;
}
