// Mixture-of-experts NomicBERT text tower (nomic-embed-text-v2-moe: model_type "nomic_bert" with moe_every_n_layers / num_experts / moe_top_k) on one HIP
// stream, no allocation, no sync: host-side orchestration of kernels that live in the sibling units — token gather + type row (embed.hip), LayerNorm
// (rowops.hip), the bf16 GEMMs with their bias / GELU / residual epilogues, rotary positions (embed.hip: mq_rope), the sliced full attention
// (attention_full.hip), the router, the plan, the grouped GEMM and the combine (moe.hip), pooling.
//
// The block is the Jina v3 base block (jina_v3.hip with lora == NULL): post-LN on the fp32 residual stream x [rows, W] with a bf16 copy h for the GEMMs,
// biases on Wqkv and out_proj.  A layer is routed when its router_w is set, dense otherwise (the loader decides from the checkpoint's tensors):
//   x, h = LN_emb(tok[ids] + type_emb[0])                          (no position table)
//   qkv = h Wqkv^T + b ; rope(q, k) ; a = attention_full(qkv, 1 / sqrt(64)) ; x, h = norm1(a Wo^T + b + x)
//   dense:   p = gelu(h W1^T + b1) ; x, h = norm2(p W2^T + b2 + x)
//   routed:  (e, w) = top-k softmax_fp32(x Wr^T)                   (mq_moe_route, on the FP32 stream)
//            plan: slots in expert-major order, the tile table     (mq_moe_plan; the segment sizes never reach the host)
//            P[slot] = bf16(gelu(h[row(slot)] W1[e]^T))            (mq_moe_gemm MQ_MOE_UP, rows gathered)
//            Y[slot] = w(slot) (P[slot] W2t[e]^T)                  (mq_moe_gemm MQ_MOE_DOWN)
//            x, h = norm2(((x + Y[slot(r, 0)]) + Y[slot(r, 1)]) + b_experts)      (mq_moe_combine_ln)
// then mean / CLS pooling over x (+ L2).  No final norm; the pooler is not run.  The tile height of the grouped GEMM is the host's choice from the row
// count (mq_moe_tile_rows).  The checks in front of the first launch and the workspace arithmetic are the scaffold of packed_text.h; P shares the slice
// of qkv / fc1's output (dead while a routed MLP runs).
#include "packed_text.h"

static_assert(sizeof(mq_nomic_moe_layer) == 128 && sizeof(mq_nomic_moe_weights) == 48 && sizeof(mq_nomic_moe_cfg) == 48, "MoE NomicBERT layouts (marqo_amd/_lib.py)");

namespace {
struct Plan { size_t off_x, off_h, off_a, off_big, off_y, off_top_e, off_top_w, off_expert_off, off_slot_row, off_slot_w, off_row_slot, off_tiles, total; };
Plan plan(const mq_nomic_moe_cfg* c, int64_t rows) {
    Plan p;
    Off ws;
    const size_t k = (size_t)c->top_k, slots = (size_t)rows * k;
    size_t big = (size_t)(3 * c->width > c->mlp_dim ? 3 * c->width : c->mlp_dim);
    if (k * c->mlp_dim > big) big = k * c->mlp_dim;
    p.off_x = ws.take((size_t)rows * c->width * 4);     // residual stream, fp32
    p.off_h = ws.take((size_t)rows * c->width * 2);     // the same rows, bf16
    p.off_a = ws.take((size_t)rows * c->width * 2);     // attention output, bf16
    p.off_big = ws.take((size_t)rows * big * 2);        // qkv, then fc1's output or P [k rows, F]
    p.off_y = ws.take(slots * c->width * 4);            // Y [k rows, W], fp32
    p.off_top_e = ws.take(slots * 4);
    p.off_top_w = ws.take(slots * 4);
    p.off_expert_off = ws.take((size_t)(c->experts + 1) * 4);
    p.off_slot_row = ws.take(slots * 4);
    p.off_slot_w = ws.take(slots * 4);
    p.off_row_slot = ws.take(slots * 4);
    p.off_tiles = ws.take((size_t)(1 + 2 * mq_moe_max_tiles(rows, c->experts, c->top_k, 32)) * 4);      // (sized for the shorter tile)
    p.total = ws.end();
    return p;
}
int check_cfg(const mq_nomic_moe_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_nomic_moe: null cfg");
    MQ_CHECK_ARG(c->head_dim == 64, "mq_encode_nomic_moe: head_dim %d unsupported (64)", c->head_dim);
    MQ_CHECK_ARG(c->width >= 64 && c->width % 64 == 0 && c->width <= 2048, "mq_encode_nomic_moe: width %d must be a multiple of 64, at most 2048", c->width);
    MQ_CHECK_ARG(c->heads >= 1 && c->heads * 64 == c->width, "mq_encode_nomic_moe: heads %d x 64 is not the width %d", c->heads, c->width);
    MQ_TRY(check_tower_sizes("mq_encode_nomic_moe", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_CLS, "mq_encode_nomic_moe: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_CLS)", c->pool);
    MQ_CHECK_ARG(c->experts >= 2 && c->experts <= 16, "mq_encode_nomic_moe: experts %d outside [2, 16]", c->experts);
    MQ_CHECK_ARG((c->top_k == 1 || c->top_k == 2) && c->top_k <= c->experts, "mq_encode_nomic_moe: top_k %d must be 1 or 2", c->top_k);
    return MQ_OK;
}
}  // namespace

extern "C" size_t mq_nomic_moe_workspace_bytes(const mq_nomic_moe_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0 || cfg->top_k < 1 || cfg->experts < 1) return 0;
    return plan(cfg, rows).total;
}

extern "C" int mq_encode_nomic_moe(const mq_nomic_moe_cfg* cfg, const mq_nomic_moe_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                                   const int32_t* h_cu_seqlens, int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes,
                                   void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_nomic_moe: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->type0 && w->emb_ln_g && w->emb_ln_b && w->d_inv_freq && w->layers, "mq_encode_nomic_moe: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_nomic_moe_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.qkv_w && b.qkv_b && b.out_w && b.out_b && b.attn_ln_g && b.attn_ln_b && b.mlp_ln_g && b.mlp_ln_b,
                     "mq_encode_nomic_moe: layer %d has null weights", l);
        if (b.router_w) MQ_CHECK_ARG(b.w1 && b.w2t && b.experts_b, "mq_encode_nomic_moe: routed layer %d has null expert tensors", l);
        else MQ_CHECK_ARG(b.fc1_w && b.fc1_b && b.fc2_w && b.fc2_b, "mq_encode_nomic_moe: dense layer %d has null MLP tensors", l);
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_nomic_moe", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const Plan p = plan(cfg, rows);
    MQ_TRY(packed_workspace("mq_encode_nomic_moe", workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* big = base + p.off_big;
    float* Y = (float*)(base + p.off_y);
    int32_t* top_e = (int32_t*)(base + p.off_top_e);
    float* top_w = (float*)(base + p.off_top_w);
    int32_t* expert_off = (int32_t*)(base + p.off_expert_off);
    int32_t* slot_row = (int32_t*)(base + p.off_slot_row);
    float* slot_w = (float*)(base + p.off_slot_w);
    int32_t* row_slot = (int32_t*)(base + p.off_row_slot);
    int32_t* tiles = (int32_t*)(base + p.off_tiles);
    const int W = cfg->width, F = cfg->mlp_dim, H = cfg->heads, hd = cfg->head_dim, E = cfg->experts, k = cfg->top_k;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;
    const float scale = 1.0f / sqrtf((float)hd);
    const int bm = mq_moe_tile_rows(rows, E, k);

    // word_embeddings + token_type_embeddings[0] -> LayerNorm: fp32 into the stream, bf16 into h; no position table
    MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq, w->tok_emb, nullptr, w->type0, w->emb_ln_g, w->emb_ln_b, x, h, W, cfg->vocab, cfg->ln_eps, 0, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_nomic_moe_layer& b = w->layers[l];
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, b.qkv_b, nullptr, big, 3 * W, rows, 3 * W, W, MQ_EPI_BIAS, s));
        MQ_TRY(mq_rope(big, d_cu_seqlens, nseq, 0, W, H, w->d_inv_freq, s));
        MQ_TRY(mq_attention_full(big, a, d_cu_seqlens, nseq, 0, maxl, H, hd, scale, s));
        MQ_TRY(mq_gemm_bf16(a, W, b.out_w, W, b.out_b, x, x, W, rows, W, W, res_flags, s));
        MQ_TRY(mq_layernorm(x, nullptr, b.attn_ln_g, b.attn_ln_b, h, x, rows, W, cfg->ln_eps, s));   // (in place: a wave holds its whole row before it stores)
        if (!b.router_w) {
            MQ_TRY(mq_gemm_bf16(h, W, b.fc1_w, W, b.fc1_b, nullptr, big, F, rows, F, W, MQ_EPI_BIAS | MQ_EPI_GELU, s));
            MQ_TRY(mq_gemm_bf16(big, F, b.fc2_w, F, b.fc2_b, x, x, W, rows, W, F, res_flags, s));
            MQ_TRY(mq_layernorm(x, nullptr, b.mlp_ln_g, b.mlp_ln_b, h, x, rows, W, cfg->ln_eps, s));
        } else {
            MQ_TRY(mq_moe_route(x, b.router_w, top_e, top_w, rows, W, E, k, s));
            MQ_TRY(mq_moe_plan(top_e, top_w, rows, E, k, bm, expert_off, slot_row, slot_w, row_slot, tiles, s));
            MQ_TRY(mq_moe_gemm(MQ_MOE_UP, h, b.w1, tiles, expert_off, slot_row, slot_w, big, rows, E, k, bm, F, W, s));
            MQ_TRY(mq_moe_gemm(MQ_MOE_DOWN, big, b.w2t, tiles, expert_off, slot_row, slot_w, Y, rows, E, k, bm, W, F, s));
            MQ_TRY(mq_moe_combine_ln(x, Y, row_slot, b.experts_b, b.mlp_ln_g, b.mlp_ln_b, h, rows, W, k, cfg->ln_eps, s));
        }
    }
    MQ_TRY(mq_pool(x, d_cu_seqlens, nseq, d_out, W, cfg->pool, normalize, s));
    return MQ_OK;
}
