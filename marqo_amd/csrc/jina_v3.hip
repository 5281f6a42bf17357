// Jina v3 text tower (jina-embeddings-v3; transformers JinaEmbeddingsV3Model, model_type "jina_embeddings_v3") with its per-sequence task LoRA adapters,
// on one HIP stream, no allocation, no sync: host-side orchestration of kernels that live in the sibling units — token gather + type row (embed.hip),
// LayerNorm (rowops.hip), the bf16 GEMMs with their bias / GELU / residual epilogues, rotary positions (embed.hip: mq_rope), the sliced full attention
// (attention_full.hip), the LoRA corrections (lora.hip), pooling.
//
// The NomicBERT block (nomic_bert.hip) with biases on all four Linears and a plain fc1 -> erf-GELU -> fc2 MLP: post-LN on the fp32 residual stream x
// [rows, W], with a bf16 copy h of it for the GEMMs.  A sequence s runs adapter t = task[s] on every adapted Linear and on the token table, or none
// (task[s] < 0); the base GEMM runs once for all rows and the rank-r correction is added per row (lora.hip), so one batch mixes tasks:
//   e = tok[ids] + type_emb[0]                 (mq_embed_tokens without its LayerNorm; no position table)
//   e += scale_t A_emb_t[:, id]^T B_emb_t^T    (mq_lora_gather, then mq_lora_up MQ_LORA_ACCUM)
//   x, h = LN_emb(e)                           (mq_layernorm, in place)
//   qkv = h Wqkv^T + b                         (bf16, MQ_EPI_BIAS)
//   qkv = bf16(qkv + delta)                    (mq_lora_down on h with (A_q | A_k | A_v), mq_lora_up MQ_LORA_INPLACE: block b of q | k | v reads its own r of T)
//   rope(q, k) ; a = attention_full(qkv, 1 / sqrt(64))
//   x += delta_o(a)                            (mq_lora_down on a, mq_lora_up MQ_LORA_ACCUM — the out-projection's epilogue then adds the stream as before)
//   x, h = LN_attn(a Wo^T + b + x)
//   p = h W1^T + b                             (bf16, MQ_EPI_BIAS only: the epilogue's GELU sits in front of its residual operand)
//   p = bf16(gelu(p + delta))                  (mq_lora_down on h, mq_lora_up MQ_LORA_INPLACE with MQ_ACT_GELU: delta and activation in one in-place pass)
//   x += delta_fc2(p)                          (mq_lora_down on p, mq_lora_up MQ_LORA_ACCUM)
//   x, h = LN_mlp(p W2^T + b + x)
// then mean / CLS pooling over x (+ L2).  No final norm; the pooler is not run.
//
// QKV takes its delta in place and not as the GEMM's MQ_EPI_RESIDUAL operand: with bf16 output that epilogue reads its residual as bf16 in place
// (gemm_epilogue.h: RES_BF16), an fp32 delta buffer cannot be handed to it.
//
// A tower with adapters (lora != NULL) always runs the block in this form: with every task negative the down / up / gather launches are skipped except
// fc1's activation pass (mq_lora_up with no row to correct is then the plain GELU), so a sequence without adapter gets the same bits whatever else
// is in its batch.  lora == NULL: no kernel of lora.hip is launched and fc1 runs with MQ_EPI_BIAS | MQ_EPI_GELU in its epilogue.
//
// The rotary convention is NomicBERT's (rotate_half over the whole 64-wide head: mq_rope as it is, inv_freq = theta ^ -(2 i / 64)), checked against
// transformers' modeling_jina_embeddings_v3.py.  The checks in front of the first launch and the workspace arithmetic are the scaffold of packed_text.h.
#include "packed_text.h"

static_assert(sizeof(mq_jina_v3_layer) == 96 && sizeof(mq_jina_v3_weights) == 48 && sizeof(mq_jina_v3_cfg) == 40 && sizeof(mq_jina_v3_lora_layer) == 64 &&
              sizeof(mq_jina_v3_lora) == 40, "Jina v3 layouts (marqo_amd/_lib.py)");

namespace {
constexpr int T_COLS = 48;      // fp32 columns of the LoRA intermediate per row: q | k | v at the largest rank, 16
struct Plan { size_t off_x, off_h, off_a, off_big, off_t, total; };
Plan plan(const mq_jina_v3_cfg* c, int64_t rows) {
    Plan p;
    Off ws;
    const size_t big = (size_t)(3 * c->width > c->mlp_dim ? 3 * c->width : c->mlp_dim);
    p.off_x = ws.take((size_t)rows * c->width * 4);     // residual stream, fp32
    p.off_h = ws.take((size_t)rows * c->width * 2);     // the same rows, bf16
    p.off_a = ws.take((size_t)rows * c->width * 2);     // attention output, bf16
    p.off_big = ws.take((size_t)rows * big * 2);        // qkv, then fc1's output
    p.off_t = ws.take((size_t)rows * T_COLS * 4);       // T of mq_lora_down / mq_lora_gather
    p.total = ws.end();
    return p;
}
int check_cfg(const mq_jina_v3_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_jina_v3: null cfg");
    MQ_CHECK_ARG(c->head_dim == 64, "mq_encode_jina_v3: head_dim %d unsupported (64)", c->head_dim);
    MQ_CHECK_ARG(c->width >= 64 && c->width % 64 == 0 && c->width <= 2048, "mq_encode_jina_v3: width %d must be a multiple of 64, at most 2048", c->width);
    MQ_CHECK_ARG(c->heads >= 1 && c->heads * 64 == c->width, "mq_encode_jina_v3: heads %d x 64 is not the width %d", c->heads, c->width);
    MQ_TRY(check_tower_sizes("mq_encode_jina_v3", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_CLS, "mq_encode_jina_v3: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_CLS)", c->pool);
    return MQ_OK;
}
}  // namespace

extern "C" size_t mq_jina_v3_workspace_bytes(const mq_jina_v3_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return plan(cfg, rows).total;
}

extern "C" int mq_encode_jina_v3(const mq_jina_v3_cfg* cfg, const mq_jina_v3_weights* w, const mq_jina_v3_lora* lora, const int32_t* d_ids,
                                 const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, const int32_t* d_seq_task, const int32_t* h_seq_task, int64_t nseq,
                                 float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_jina_v3: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->type0 && w->emb_ln_g && w->emb_ln_b && w->d_inv_freq && w->layers, "mq_encode_jina_v3: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_jina_v3_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.qkv_w && b.qkv_b && b.out_w && b.out_b && b.attn_ln_g && b.attn_ln_b && b.fc1_w && b.fc1_b && b.fc2_w && b.fc2_b && b.mlp_ln_g &&
                     b.mlp_ln_b, "mq_encode_jina_v3: layer %d has null weights", l);
    }
    if (lora) {
        MQ_CHECK_ARG(lora->tasks >= 1 && lora->tasks <= 1024, "mq_encode_jina_v3: lora tasks %d outside [1, 1024]", lora->tasks);
        MQ_CHECK_ARG(lora->rank >= 4 && lora->rank <= 16 && lora->rank % 4 == 0, "mq_encode_jina_v3: lora rank %d must be 4, 8, 12 or 16", lora->rank);
        MQ_CHECK_ARG(lora->d_scale && lora->layers, "mq_encode_jina_v3: lora has null scale / layers");
        MQ_CHECK_ARG(!lora->emb_a == !lora->emb_b, "mq_encode_jina_v3: lora embedding adapter needs both emb_a and emb_b");
        for (int l = 0; l < cfg->layers; ++l) {
            const mq_jina_v3_lora_layer& a = lora->layers[l];
            MQ_CHECK_ARG(a.qkv_a && a.qkv_b && a.out_a && a.out_b && a.fc1_a && a.fc1_b && a.fc2_a && a.fc2_b,
                         "mq_encode_jina_v3: lora layer %d has null adapter tensors (a Linear no task adapts carries zeros)", l);
        }
        MQ_CHECK_ARG(d_seq_task && h_seq_task, "mq_encode_jina_v3: a tower with adapters needs the task list (device and host copies of int32 [nseq])");
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_jina_v3", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    bool any = false;       // some sequence of this batch has an adapter
    if (lora)
        for (int64_t s = 0; s < nseq; ++s) {
            MQ_CHECK_ARG(h_seq_task[s] < lora->tasks, "mq_encode_jina_v3: task id %d of sequence %lld is not below tasks %d", h_seq_task[s], (long long)s,
                         lora->tasks);
            any = any || h_seq_task[s] >= 0;
        }
    const Plan p = plan(cfg, rows);
    MQ_TRY(packed_workspace("mq_encode_jina_v3", workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* big = base + p.off_big;
    float* T = (float*)(base + p.off_t);
    const int W = cfg->width, F = cfg->mlp_dim, H = cfg->heads, hd = cfg->head_dim;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;
    const float scale = 1.0f / sqrtf((float)hd);
    const int tasks = lora ? lora->tasks : 0, r = lora ? lora->rank : 0;
    // one adapted Linear: T = scale_t (in A_t^T), then the up half in `mode` on `out`
    auto adapt = [&](const void* in, int64_t lda, int K, const void* A, const void* B, int nblocks, void* out, int64_t ldc, int N, int mode, int act) -> int {
        MQ_TRY(mq_lora_down(in, lda, A, lora->d_scale, d_seq_task, h_seq_task, d_cu_seqlens, nseq, 0, rows, tasks, nblocks * r, K, T, s));
        return mq_lora_up(T, nblocks * r, B, r, nblocks, d_seq_task, h_seq_task, d_cu_seqlens, nseq, 0, rows, tasks, out, ldc, N, mode, act, s);
    };

    // word_embeddings + token_type_embeddings[0] (+ the embedding adapter) -> LayerNorm: fp32 into the stream, bf16 into h; no position table
    MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq, w->tok_emb, nullptr, w->type0, nullptr, nullptr, x, nullptr, W, cfg->vocab, cfg->ln_eps, 0, s));
    if (any && lora->emb_a) {
        MQ_TRY(mq_lora_gather(d_ids, lora->emb_a, lora->d_scale, d_seq_task, h_seq_task, d_cu_seqlens, nseq, 0, rows, tasks, r, cfg->vocab, T, s));
        MQ_TRY(mq_lora_up(T, r, lora->emb_b, r, 1, d_seq_task, h_seq_task, d_cu_seqlens, nseq, 0, rows, tasks, x, W, W, MQ_LORA_ACCUM, 0, s));
    }
    MQ_TRY(mq_layernorm(x, nullptr, w->emb_ln_g, w->emb_ln_b, h, x, rows, W, cfg->ln_eps, s));   // (in place: a wave holds its whole row before it stores)
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_jina_v3_layer& b = w->layers[l];
        const mq_jina_v3_lora_layer* ad = lora ? &lora->layers[l] : nullptr;
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, b.qkv_b, nullptr, big, 3 * W, rows, 3 * W, W, MQ_EPI_BIAS, s));
        if (any) MQ_TRY(adapt(h, W, W, ad->qkv_a, ad->qkv_b, 3, big, 3 * W, 3 * W, MQ_LORA_INPLACE, 0));
        MQ_TRY(mq_rope(big, d_cu_seqlens, nseq, 0, W, H, w->d_inv_freq, s));
        MQ_TRY(mq_attention_full(big, a, d_cu_seqlens, nseq, 0, maxl, H, hd, scale, s));
        if (any) MQ_TRY(adapt(a, W, W, ad->out_a, ad->out_b, 1, x, W, W, MQ_LORA_ACCUM, 0));
        MQ_TRY(mq_gemm_bf16(a, W, b.out_w, W, b.out_b, x, x, W, rows, W, W, res_flags, s));
        MQ_TRY(mq_layernorm(x, nullptr, b.attn_ln_g, b.attn_ln_b, h, x, rows, W, cfg->ln_eps, s));
        if (!lora) {
            MQ_TRY(mq_gemm_bf16(h, W, b.fc1_w, W, b.fc1_b, nullptr, big, F, rows, F, W, MQ_EPI_BIAS | MQ_EPI_GELU, s));
        } else {
            MQ_TRY(mq_gemm_bf16(h, W, b.fc1_w, W, b.fc1_b, nullptr, big, F, rows, F, W, MQ_EPI_BIAS, s));
            // (no sequence with an adapter: mq_lora_down launches nothing, and the up half, which then corrects no row and reads no T, is the plain GELU pass)
            MQ_TRY(adapt(h, W, W, ad->fc1_a, ad->fc1_b, 1, big, F, F, MQ_LORA_INPLACE, MQ_ACT_GELU));
            if (any) MQ_TRY(adapt(big, F, F, ad->fc2_a, ad->fc2_b, 1, x, W, W, MQ_LORA_ACCUM, 0));
        }
        MQ_TRY(mq_gemm_bf16(big, F, b.fc2_w, F, b.fc2_b, x, x, W, rows, W, F, res_flags, s));
        MQ_TRY(mq_layernorm(x, nullptr, b.mlp_ln_g, b.mlp_ln_b, h, x, rows, W, cfg->ln_eps, s));
    }
    MQ_TRY(mq_pool(x, d_cu_seqlens, nseq, d_out, W, cfg->pool, normalize, s));
    return MQ_OK;
}
