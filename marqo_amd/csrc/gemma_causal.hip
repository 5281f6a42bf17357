// Gemma rerankers (transformers GemmaForCausalLM read as a judge — BAAI/bge-reranker-v2-gemma = Gemma-2B — or GemmaForSequenceClassification with one
// label): one query against n documents on one HIP stream, no allocation, no sync.  Host-side orchestration only: every kernel lives in a sibling unit —
// the token gather (embed.hip), mq_rmsnorm and the rotary step (qwen.hip), the bf16 GEMMs, the causal and prefix-sharing 256-wide grouped-query attention
// (attention_gqa256_causal.hip), the tanh-GELU gated product (gemma.hip), the one-row head (rerank.hip).
//
// Packed rows [prefix | seg_1 | ... | seg_n], mq_score_qwen_pairs' contract: the prefix ([bos] "A: " query — the same token row for every hit of a
// search, and under the causal mask independent of what follows it) is sequence 0 of the batch, cu_seqlens has nseq + 2 entries {0, P, P + d_1, ...};
// P = prefix_len may be 0 (no sharing: every segment is a whole pair).  Per block, on the fp32 residual stream x [rows, W] (no Linear has a bias; every
// norm is an RMSNorm whose weight arrives as 1 + w, folded at load; no q / k norm):
//   h = rmsnorm(x, input_layernorm)
//   qkv = h Wqkv^T                              Wqkv = cat(q_proj, k_proj, v_proj) at load: [(Q + 2 KV) hd, W]
//   rope(qkv): the prefix at offset 0, the segments at offset P
//   a = attention: mq_attention_gqa256_causal on the prefix, mq_attention_gqa256_prefix on the segments, scale = head_dim^-0.5
//   x += a Wo^T                                 (K of this GEMM is Q hd, which need not be W)
//   h = rmsnorm(x, post_attention_layernorm)
//   (up | gate) = h Wug^T ; p = up * gelu_tanh(gate) ; x += p Wdown^T
// The norms, the GEMMs, the gated product and the residuals are row-wise and run over all rows at once.  The final norm runs on every segment's last row
// only, and the logit is one fp32 dot product with the score row.  The token table arrives scaled by sqrt(W) (marqo_hip.h).
//
// The checks in front of the first launch and the workspace arithmetic are the packed-token scaffold of packed_text.h.
#include "packed_text.h"

static_assert(sizeof(mq_gemma_causal_layer) == 48 && sizeof(mq_gemma_causal_weights) == 40 && sizeof(mq_gemma_causal_cfg) == 40,
              "Gemma reranker layouts (marqo_amd/_lib.py)");

namespace {
struct Plan { size_t off_x, off_h, off_a, off_big, off_rows, off_pooled, total; };
Plan plan(const mq_gemma_causal_cfg* c, int64_t rows, int64_t nseq) {
    Plan p;
    Off ws;
    const size_t aw = (size_t)c->q_heads * c->head_dim, qkvw = (size_t)(c->q_heads + 2 * c->kv_heads) * c->head_dim;
    const size_t big = qkvw > 2 * (size_t)c->mlp_dim ? qkvw : 2 * (size_t)c->mlp_dim;
    p.off_x = ws.take((size_t)rows * c->width * 4);        // residual stream, fp32
    p.off_h = ws.take((size_t)rows * c->width * 2);        // normalised rows, bf16
    p.off_a = ws.take((size_t)rows * aw * 2);              // attention output, bf16
    p.off_big = ws.take((size_t)rows * big * 2);           // qkv, then (up | gate)
    p.off_rows = ws.take((size_t)nseq * 4);                // the last row of every segment
    p.off_pooled = ws.take((size_t)nseq * c->width * 4);   // its normalised copy, fp32
    p.total = ws.end();
    return p;
}
int check_cfg(const mq_gemma_causal_cfg* c) {
    MQ_CHECK_ARG(c, "mq_score_gemma_pairs: null cfg");
    MQ_CHECK_ARG(c->head_dim == 256, "mq_score_gemma_pairs: head_dim %d unsupported (256)", c->head_dim);
    MQ_TRY(check_gqa_shape("mq_score_gemma_pairs", c->q_heads, c->kv_heads, c->width));
    MQ_CHECK_ARG(c->width <= 2048, "mq_score_gemma_pairs: width %d > 2048 (the 7B size of this family is not served)", c->width);
    MQ_TRY(check_tower_sizes("mq_score_gemma_pairs", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->attn_scale > 0.f && c->attn_scale <= 1e6f, "mq_score_gemma_pairs: attn_scale %g must be positive and finite", (double)c->attn_scale);
    return MQ_OK;
}
}  // namespace

extern "C" size_t mq_score_gemma_pairs_workspace_bytes(const mq_gemma_causal_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return plan(cfg, rows, nseq).total;
}

extern "C" int mq_score_gemma_pairs(const mq_gemma_causal_cfg* cfg, const mq_gemma_causal_weights* w, const float* d_score_w, const int32_t* d_ids,
                                    const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq, int32_t prefix_len, float* d_logits,
                                    float* d_scores, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* what = "mq_score_gemma_pairs";
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_score_w && d_logits, "%s: null pointer", what);
    MQ_CHECK_ARG(w->tok_emb && w->final_norm_g && w->zeros && w->d_inv_freq && w->layers, "%s: null weight pointer", what);
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_gemma_causal_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.input_norm_g && b.qkv_w && b.out_w && b.post_norm_g && b.ug_w && b.down_w, "%s: layer %d has null weights", what, l);
    }
    MQ_CHECK_ARG(prefix_len >= 0 && prefix_len < cfg->max_pos, "%s: prefix_len %d outside [0, max_pos=%d)", what, prefix_len, cfg->max_pos);
    if (nseq <= 0) return MQ_OK;
    MQ_CHECK_ARG(nseq < (1ll << 31) - 1, "%s: nseq=%lld too large", what, (long long)nseq);
    MQ_CHECK_ARG(h_cu_seqlens && h_cu_seqlens[0] == 0 && h_cu_seqlens[1] == prefix_len, "%s: cu_seqlens must begin {0, prefix_len=%d}", what, prefix_len);
    const int P = prefix_len;
    int maxl = 0, maxseg = 0;
    int64_t rows = 0, seg_rows = 0;
    // every length in [1, max_pos]: the segments' always, the prefix's (sequence 0) when there is one
    MQ_TRY(packed_begin(what, d_ids, d_cu_seqlens, h_cu_seqlens + (P ? 0 : 1), nseq + (P ? 1 : 0), cfg->max_pos, d_workspace, &maxl, &rows));
    maxseg = max_seq_len(h_cu_seqlens + 1, nseq, &seg_rows);
    MQ_CHECK_ARG(maxseg >= 1 && P + maxseg <= cfg->max_pos, "%s: prefix_len %d + the longest segment %d exceeds max_pos=%d", what, P, maxseg, cfg->max_pos);
    const Plan p = plan(cfg, rows, nseq);
    MQ_TRY(packed_workspace(what, workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* big = base + p.off_big;
    int32_t* last = (int32_t*)(base + p.off_rows);
    float* pooled = (float*)(base + p.off_pooled);
    const int32_t* d_seg_cu = d_cu_seqlens + 1;     // {P, P + d_1, ...}: the segments, as mq_attention_gqa256_prefix reads them
    const int W = cfg->width, F = cfg->mlp_dim, Q = cfg->q_heads, KV = cfg->kv_heads, hd = cfg->head_dim;
    const int AW = Q * hd, QKVW = (Q + 2 * KV) * hd;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;   // (the bias is w->zeros)

    // embed_tokens (already scaled by sqrt(W)): a gather, no positions, no norm
    MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq + 1, w->tok_emb, nullptr, nullptr, nullptr, nullptr, x, nullptr, W, cfg->vocab, cfg->rms_eps, 0, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_gemma_causal_layer& b = w->layers[l];
        MQ_TRY(mq_rmsnorm(x, nullptr, b.input_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, nullptr, nullptr, big, QKVW, rows, QKVW, W, 0, s));
        if (P) {   // the prefix: one fixed-length causal sequence of P rows at positions 0 .. P - 1
            MQ_TRY(mq_qk_norm_rope(big, nullptr, 1, P, Q, KV, hd, nullptr, nullptr, cfg->rms_eps, w->d_inv_freq, s));
            MQ_TRY(mq_attention_gqa256_causal(big, a, nullptr, 1, P, P, Q, KV, hd, cfg->attn_scale, s));
        }
        MQ_TRY(mq_qk_norm_rope_at(big, d_seg_cu, nseq, 0, Q, KV, hd, nullptr, nullptr, cfg->rms_eps, w->d_inv_freq, P, s));
        MQ_TRY(mq_attention_gqa256_prefix(big, a, d_seg_cu, nseq, P, maxseg, Q, KV, hd, cfg->attn_scale, s));
        MQ_TRY(mq_gemm_bf16(a, AW, b.out_w, AW, w->zeros, x, x, W, rows, W, AW, res_flags, s));
        MQ_TRY(mq_rmsnorm(x, nullptr, b.post_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.ug_w, W, nullptr, nullptr, big, 2 * F, rows, 2 * F, W, 0, s));
        MQ_TRY(mq_glu_tanh(big, rows, F, s));
        MQ_TRY(mq_gemm_bf16(big, 2 * F, b.down_w, F, w->zeros, x, x, W, rows, W, F, res_flags, s));
    }
    MQ_TRY(mq_last_rows(d_seg_cu, last, nseq, s));
    MQ_TRY(mq_rmsnorm(x, last, w->final_norm_g, nullptr, pooled, nseq, W, cfg->rms_eps, s));
    return mq_score_dot(pooled, d_score_w, nseq, W, d_logits, d_scores, s);
}
