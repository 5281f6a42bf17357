// T5 encoder text tower (transformers T5EncoderModel: sentence-t5, gtr-t5, flan-t5 / T5 v1.1 encoder fine-tunes) on one HIP stream, no allocation, no
// sync: host-side orchestration of kernels that live in the sibling units — the token gather (embed.hip), mq_rmsnorm (qwen.hip: T5LayerNorm is an
// RMSNorm), the bf16 GEMMs (no Linear has a bias; the ReLU epilogue is the NLLB one), the tanh-GELU gated product (gemma.hip: T5 v1.1's gated gelu_new),
// the clamped relative-bias attention (attention_relbias.hip), pooling.
//
// Per block, on the fp32 residual stream x [rows, W] (W = d_model; A = heads * d_kv need not be W):
//   x = tok[ids]                                        (no scaling, no position table)
//   h = bf16(rms(x) * g_attn)
//   qkv = h Wqkv^T                                      (rows q | k | v, [3 A, W])
//   a = attention_relbias(qkv, the ONE bias table of block 0, scale 1.0)        (T5 applies no 1 / sqrt(d_kv))
//   x += a Wo^T
//   h = bf16(rms(x) * g_ff)
//   relu:        x += relu(h Wi^T) Wo_ff^T
//   gated-gelu:  (up | gate) = h Wi'^T (rows wi_1 | wi_0) ; x += (up * gelu_new(gate)) Wo_ff^T
// then the final RMSNorm over every row and mean / CLS pooling (+ L2).
//
// The checks in front of the first launch and the workspace arithmetic are the packed-token scaffold of packed_text.h.
#include "packed_text.h"

static_assert(sizeof(mq_t5_layer) == 48 && sizeof(mq_t5_weights) == 40 && sizeof(mq_t5_cfg) == 48, "T5 layouts (marqo_amd/_lib.py)");

namespace {
struct Plan { size_t off_x, off_h, off_a, off_big, total; };
Plan plan(const mq_t5_cfg* c, int64_t rows) {
    Plan p;
    Off ws;
    const size_t A = (size_t)c->heads * c->head_dim;
    const size_t ff = (size_t)(c->gated ? 2 : 1) * c->mlp_dim;
    const size_t big = 3 * A > ff ? 3 * A : ff;
    p.off_x = ws.take((size_t)rows * c->width * 4);     // residual stream, fp32
    p.off_h = ws.take((size_t)rows * c->width * 2);     // normalised rows, bf16
    p.off_a = ws.take((size_t)rows * A * 2);            // attention output, bf16
    p.off_big = ws.take((size_t)rows * big * 2);        // qkv, then the MLP's hidden rows
    p.total = ws.end();
    return p;
}
int check_cfg(const mq_t5_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_t5: null cfg");
    MQ_CHECK_ARG(c->head_dim == 64 || c->head_dim == 128, "mq_encode_t5: head_dim (d_kv) %d unsupported (64 or 128)", c->head_dim);
    MQ_CHECK_ARG(c->width >= 64 && c->width % 64 == 0 && c->width <= 2048, "mq_encode_t5: width (d_model) %d must be a multiple of 64, at most 2048", c->width);
    MQ_CHECK_ARG(c->heads >= 1 && (int64_t)c->heads * c->head_dim <= 4096, "mq_encode_t5: inner width heads %d x head_dim %d outside [1, 4096]", c->heads,
                 c->head_dim);
    MQ_TRY(check_tower_sizes("mq_encode_t5", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_CLS, "mq_encode_t5: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_CLS)", c->pool);
    MQ_CHECK_ARG(c->max_distance >= 1 && c->max_distance <= 1024, "mq_encode_t5: max_distance %d outside [1, 1024]", c->max_distance);
    MQ_CHECK_ARG(c->gated == 0 || c->gated == 1, "mq_encode_t5: gated %d must be 0 (relu) or 1 (gated gelu_new)", c->gated);
    return MQ_OK;
}
}  // namespace

extern "C" size_t mq_t5_workspace_bytes(const mq_t5_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return plan(cfg, rows).total;
}

extern "C" int mq_encode_t5(const mq_t5_cfg* cfg, const mq_t5_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens,
                            int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_t5: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->final_norm_g && w->zeros && w->d_rel_bias && w->layers, "mq_encode_t5: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_t5_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.attn_norm_g && b.qkv_w && b.out_w && b.ff_norm_g && b.wi_w && b.wo_w, "mq_encode_t5: layer %d has null weights", l);
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_t5", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const Plan p = plan(cfg, rows);
    MQ_TRY(packed_workspace("mq_encode_t5", workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* big = base + p.off_big;
    const int W = cfg->width, F = cfg->mlp_dim, H = cfg->heads, hd = cfg->head_dim, A = H * hd;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;   // (the bias is w->zeros)

    // shared embedding: a gather, no scaling, no positions, no norm
    MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq, w->tok_emb, nullptr, nullptr, nullptr, nullptr, x, nullptr, W, cfg->vocab, cfg->rms_eps, 0, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_t5_layer& b = w->layers[l];
        MQ_TRY(mq_rmsnorm(x, nullptr, b.attn_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, nullptr, nullptr, big, 3 * A, rows, 3 * A, W, 0, s));
        MQ_TRY(mq_attention_relbias(big, a, d_cu_seqlens, nseq, 0, maxl, H, hd, w->d_rel_bias, cfg->max_distance, 1.0f, s));   // block 0's table, every block
        MQ_TRY(mq_gemm_bf16(a, A, b.out_w, A, w->zeros, x, x, W, rows, W, A, res_flags, s));
        MQ_TRY(mq_rmsnorm(x, nullptr, b.ff_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
        if (cfg->gated) {
            MQ_TRY(mq_gemm_bf16(h, W, b.wi_w, W, nullptr, nullptr, big, 2 * F, rows, 2 * F, W, 0, s));
            MQ_TRY(mq_glu_tanh(big, rows, F, s));
            MQ_TRY(mq_gemm_bf16(big, 2 * F, b.wo_w, F, w->zeros, x, x, W, rows, W, F, res_flags, s));
        } else {
            MQ_TRY(mq_gemm_bf16(h, W, b.wi_w, W, w->zeros, nullptr, big, F, rows, F, W, MQ_EPI_BIAS | MQ_EPI_RELU, s));   // (w->zeros: the ReLU epilogue comes with a bias)
            MQ_TRY(mq_gemm_bf16(big, F, b.wo_w, F, w->zeros, x, x, W, rows, W, F, res_flags, s));
        }
    }
    MQ_TRY(mq_rmsnorm(x, nullptr, w->final_norm_g, nullptr, x, rows, W, cfg->rms_eps, s));   // (in place: a wave holds its whole row before it stores)
    MQ_TRY(mq_pool(x, d_cu_seqlens, nseq, d_out, W, cfg->pool, normalize, s));
    return MQ_OK;
}
