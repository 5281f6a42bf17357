// NomicBERT text tower (nomic-embed-text-v1 / -v1.5 / -v1-unsupervised, their fine-tunes, snowflake-arctic-embed-m-long; transformers NomicBertModel) on
// one HIP stream, no allocation, no sync: host-side orchestration of kernels that live in the sibling units — token gather + type row + LayerNorm
// (embed.hip), LayerNorm (rowops.hip), the bf16 GEMMs with their residual epilogue, rotary positions and the gated-SiLU product (embed.hip: mq_rope,
// mq_glu), the sliced full attention (attention_full.hip), pooling.
//
// Post-LN blocks on the fp32 residual stream x [rows, W], with a bf16 copy h of it for the GEMMs; no Linear has a bias, every LayerNorm has one:
//   x, h = LN_emb(tok[ids] + type_emb[0])                          (no position table)
//   qkv = h Wqkv^T                                                 (rows q | k | v, fused at load)
//   rope(q, k)                                                     (mq_rope: packed positions 0 .. len - 1, inv_freq = theta ^ -(2 i / 64))
//   a = attention_full(qkv, 1 / sqrt(64))
//   x, h = LN_attn(a Wo^T + x)
//   (up | gate) = h Wug^T                                          (up_proj | gate_proj stacked at load, the order mq_glu reads)
//   p = up * silu(gate)
//   x, h = LN_mlp(p Wdown^T + x)
// then mean / CLS pooling over x (+ L2).  No final norm; the pooler is not run.
//
// Rotary convention, checked against transformers' modeling_nomic_bert.py: apply_rotary_pos_emb forms x cos + rotate_half(x) sin with
// rotate_half(x) = (-x2, x1) over the halves of the whole head and cos / sin of cat(freqs, freqs), freqs = position * inv_freq — dims d and d + 32 share
// the angle t * inv_freq[d]: y1 = x1 cos - x2 sin, y2 = x2 cos + x1 sin.  That is rope_kernel's arithmetic (embed.hip), the convention the NewModel /
// stella path already runs, so mq_rope is used as it is and the arch lays inv_freq out in the plain order i = 0 .. 31.
//
// The checks in front of the first launch and the workspace arithmetic are the packed-token scaffold of packed_text.h.
#include "packed_text.h"

static_assert(sizeof(mq_nomic_bert_layer) == 64 && sizeof(mq_nomic_bert_weights) == 56 && sizeof(mq_nomic_bert_cfg) == 40, "NomicBERT layouts (marqo_amd/_lib.py)");

namespace {
struct Plan { size_t off_x, off_h, off_a, off_big, total; };
Plan plan(const mq_nomic_bert_cfg* c, int64_t rows) {
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
int check_cfg(const mq_nomic_bert_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_nomic_bert: null cfg");
    MQ_CHECK_ARG(c->head_dim == 64, "mq_encode_nomic_bert: head_dim %d unsupported (64)", c->head_dim);
    MQ_CHECK_ARG(c->width >= 64 && c->width % 64 == 0 && c->width <= 2048, "mq_encode_nomic_bert: width %d must be a multiple of 64, at most 2048", c->width);
    MQ_CHECK_ARG(c->heads >= 1 && c->heads * 64 == c->width, "mq_encode_nomic_bert: heads %d x 64 is not the width %d", c->heads, c->width);
    MQ_TRY(check_tower_sizes("mq_encode_nomic_bert", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_CLS, "mq_encode_nomic_bert: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_CLS)", c->pool);
    return MQ_OK;
}
}  // namespace

extern "C" size_t mq_nomic_bert_workspace_bytes(const mq_nomic_bert_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return plan(cfg, rows).total;
}

extern "C" int mq_encode_nomic_bert(const mq_nomic_bert_cfg* cfg, const mq_nomic_bert_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                                    const int32_t* h_cu_seqlens, int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes,
                                    void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_nomic_bert: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->type0 && w->emb_ln_g && w->emb_ln_b && w->zeros && w->d_inv_freq && w->layers, "mq_encode_nomic_bert: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_nomic_bert_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.qkv_w && b.out_w && b.attn_ln_g && b.attn_ln_b && b.ug_w && b.down_w && b.mlp_ln_g && b.mlp_ln_b,
                     "mq_encode_nomic_bert: layer %d has null weights", l);
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_nomic_bert", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const Plan p = plan(cfg, rows);
    MQ_TRY(packed_workspace("mq_encode_nomic_bert", workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* big = base + p.off_big;
    const int W = cfg->width, F = cfg->mlp_dim, H = cfg->heads, hd = cfg->head_dim;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;   // (the bias is w->zeros)
    const float scale = 1.0f / sqrtf((float)hd);

    // word_embeddings + token_type_embeddings[0] -> LayerNorm: fp32 into the stream, bf16 into h; no position table
    MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq, w->tok_emb, nullptr, w->type0, w->emb_ln_g, w->emb_ln_b, x, h, W, cfg->vocab, cfg->ln_eps, 0, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_nomic_bert_layer& b = w->layers[l];
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, nullptr, nullptr, big, 3 * W, rows, 3 * W, W, 0, s));
        MQ_TRY(mq_rope(big, d_cu_seqlens, nseq, 0, W, H, w->d_inv_freq, s));
        MQ_TRY(mq_attention_full(big, a, d_cu_seqlens, nseq, 0, maxl, H, hd, scale, s));
        MQ_TRY(mq_gemm_bf16(a, W, b.out_w, W, w->zeros, x, x, W, rows, W, W, res_flags, s));
        MQ_TRY(mq_layernorm(x, nullptr, b.attn_ln_g, b.attn_ln_b, h, x, rows, W, cfg->ln_eps, s));   // (in place: a wave holds its whole row before it stores)
        MQ_TRY(mq_gemm_bf16(h, W, b.ug_w, W, nullptr, nullptr, big, 2 * F, rows, 2 * F, W, 0, s));
        MQ_TRY(mq_glu(big, rows, F, MQ_ACT_SILU, 0, s));
        MQ_TRY(mq_gemm_bf16(big, 2 * F, b.down_w, F, w->zeros, x, x, W, rows, W, F, res_flags, s));
        MQ_TRY(mq_layernorm(x, nullptr, b.mlp_ln_g, b.mlp_ln_b, h, x, rows, W, cfg->ln_eps, s));
    }
    MQ_TRY(mq_pool(x, d_cu_seqlens, nseq, d_out, W, cfg->pool, normalize, s));
    return MQ_OK;
}
