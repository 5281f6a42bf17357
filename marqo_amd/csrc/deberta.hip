// DeBERTa-v2 / -v3 text tower (transformers DebertaV2Model as the one-label DebertaV2ForSequenceClassification rerankers configure it: relative_attention,
// pos_att_type c2p | p2c, position_biased_input false, type_vocab_size 0, norm_rel_ebd layer_norm, no convolution) on one HIP stream, no allocation, no
// sync: host-side orchestration of kernels that live in the sibling units — token gather + LayerNorm (embed.hip), LayerNorm (rowops.hip), the bf16 GEMMs
// with their bias / GELU / residual epilogues, the disentangled attention (attention_disentangled.hip), pooling.
//
// Post-LN BERT blocks on the fp32 residual stream x [rows, W], with a bf16 copy h of it for the GEMMs:
//   x, h = LN_emb(tok[ids])                                        (no position table, no type row)
//   qkv = h Wqkv^T + bqkv                                          (rows query | key | value, fused at load)
//   a = attention_disentangled(qkv, Kr_l, Qr_l, idx, 1 / sqrt(3 head_dim))
//   x, h = LN_attn(a Wo^T + bo + x)
//   f = gelu_erf(h W1^T + b1)
//   x, h = LN_mlp(f W2^T + b2 + x)
// then CLS / mean pooling over x (+ L2).  No final norm.  Kr_l / Qr_l = key_proj | pos_key_proj and query_proj | pos_query_proj of LayerNorm(rel_embeddings),
// split into heads: they depend on weights only and are computed once at load (engine/tower_weights.py::deberta_state_dict).  The bucket index table is
// built on the host from the model's own formula (engine/archs.py::DebertaArch.idx_table) and handed over twice: on the device for the kernel, on the
// host so that this file can read the bucket window of a call's longest sequence.
//
// The attention's strip buffer (fp32 [rows][heads][2][window], attention_disentangled.hip) is bounded: a block's attention runs over GROUPS of whole
// sequences whose strips stay under DEB_STRIP_CAP = 256 MiB — a constant nobody measured — or, for one sequence whose own strips are larger (16 heads,
// 256 buckets: from 4097 tokens on), under that sequence's.
//
// The checks in front of the first launch and the workspace arithmetic are the packed-token scaffold of packed_text.h.
#include "packed_text.h"

static_assert(sizeof(mq_deberta_layer) == 112 && sizeof(mq_deberta_weights) == 48 && sizeof(mq_deberta_cfg) == 48, "DeBERTa layouts (marqo_amd/_lib.py)");

namespace {
constexpr size_t DEB_STRIP_CAP = (size_t)256 << 20;

// strips of `rows` rows at the widest window a cfg allows (every bucket: 2 span)
size_t strip_bytes_worst(const mq_deberta_cfg* c, int64_t rows) { return mq_attention_disentangled_workspace_bytes(rows, c->heads, 0, 2 * c->span - 1); }

struct Plan { size_t off_x, off_h, off_a, off_big, off_strips, strip_bytes, total; };
Plan plan(const mq_deberta_cfg* c, int64_t rows) {
    Plan p;
    Off ws;
    const size_t big = (size_t)(3 * c->width > c->mlp_dim ? 3 * c->width : c->mlp_dim);
    p.off_x = ws.take((size_t)rows * c->width * 4);     // residual stream, fp32
    p.off_h = ws.take((size_t)rows * c->width * 2);     // the same rows, bf16
    p.off_a = ws.take((size_t)rows * c->width * 2);     // attention output, bf16
    p.off_big = ws.take((size_t)rows * big * 2);        // qkv, then the MLP's hidden rows
    // the strips of one group: everything when it is under the cap, else the cap — or the longest sequence the cfg serves, when that alone is above it
    const size_t all = strip_bytes_worst(c, rows);
    const size_t one = strip_bytes_worst(c, rows < c->max_pos ? rows : c->max_pos);
    p.strip_bytes = all <= DEB_STRIP_CAP ? all : (one > DEB_STRIP_CAP ? one : DEB_STRIP_CAP);
    p.off_strips = ws.take(p.strip_bytes);
    p.total = ws.end();
    return p;
}
int check_cfg(const mq_deberta_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_deberta: null cfg");
    MQ_CHECK_ARG(c->head_dim == 64, "mq_encode_deberta: head_dim %d unsupported (64)", c->head_dim);
    MQ_CHECK_ARG(c->width >= 64 && c->width % 64 == 0 && c->width <= 2048, "mq_encode_deberta: width %d must be a multiple of 64, at most 2048", c->width);
    MQ_CHECK_ARG(c->heads >= 1 && c->heads * 64 == c->width, "mq_encode_deberta: heads %d x 64 is not the width %d", c->heads, c->width);
    MQ_TRY(check_tower_sizes("mq_encode_deberta", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->span >= 1 && c->span <= 1024, "mq_encode_deberta: span %d outside [1, 1024]", c->span);
    MQ_CHECK_ARG(c->reach >= 0 && c->max_pos <= c->reach + 1, "mq_encode_deberta: max_pos %d is beyond the index table's reach + 1 = %d", c->max_pos, c->reach + 1);
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_CLS, "mq_encode_deberta: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_CLS)", c->pool);
    return MQ_OK;
}
}  // namespace

extern "C" size_t mq_deberta_workspace_bytes(const mq_deberta_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0 || cfg->heads <= 0 || cfg->span < 1 || cfg->span > 1024) return 0;
    return plan(cfg, rows).total;
}

extern "C" int mq_encode_deberta(const mq_deberta_cfg* cfg, const mq_deberta_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                                 const int32_t* h_cu_seqlens, int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes,
                                 void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_deberta: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->emb_ln_g && w->emb_ln_b && w->d_idx && w->h_idx && w->layers, "mq_encode_deberta: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_deberta_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.qkv_w && b.qkv_b && b.out_w && b.out_b && b.attn_ln_g && b.attn_ln_b && b.fc1_w && b.fc1_b && b.fc2_w && b.fc2_b && b.mlp_ln_g &&
                         b.mlp_ln_b && b.pos_key && b.pos_query,
                     "mq_encode_deberta: layer %d has null weights", l);
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_deberta", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const Plan p = plan(cfg, rows);
    MQ_TRY(packed_workspace("mq_encode_deberta", workspace_bytes, p.total));
    // the bucket window of the call's longest sequence, from the host copy of the table the kernel reads on the device
    const int S = cfg->span, reach = cfg->reach;
    const int lo = w->h_idx[reach - (maxl - 1)], hi = w->h_idx[reach + (maxl - 1)];
    MQ_CHECK_ARG(lo >= 0 && lo <= hi && hi <= 2 * S - 1, "mq_encode_deberta: the index table's window [%d, %d] of %d tokens lies outside [0, %d]", lo, hi, maxl,
                 2 * S - 1);
    const size_t per_row = mq_attention_disentangled_workspace_bytes(1, cfg->heads, lo, hi);
    const int64_t cap_rows = (int64_t)(p.strip_bytes / per_row);      // >= maxl: the plan holds the longest sequence at the widest window
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    char* a = base + p.off_a;
    void* big = base + p.off_big;
    void* strips = base + p.off_strips;
    const int W = cfg->width, F = cfg->mlp_dim, H = cfg->heads, hd = cfg->head_dim;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;
    const float scale = 1.0f / sqrtf(3.0f * (float)hd);      // scale_factor = 1 + |{c2p, p2c}|

    // LayerNorm(word_embeddings[ids]): fp32 into the stream, bf16 into h; no position table, no type row
    MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq, w->tok_emb, nullptr, nullptr, w->emb_ln_g, w->emb_ln_b, x, h, W, cfg->vocab, cfg->ln_eps, 0, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_deberta_layer& b = w->layers[l];
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, b.qkv_b, nullptr, big, 3 * W, rows, 3 * W, W, MQ_EPI_BIAS, s));
        // groups of whole sequences [s0, s1) whose strips fit the slot; cu_seqlens holds absolute rows, so a group is the same buffers behind a moved pointer
        for (int64_t s0 = 0; s0 < nseq;) {
            int64_t s1 = s0 + 1;
            while (s1 < nseq && h_cu_seqlens[s1 + 1] - h_cu_seqlens[s0] <= cap_rows) ++s1;
            MQ_TRY(mq_attention_disentangled(big, a, d_cu_seqlens + s0, s1 - s0, h_cu_seqlens[s1] - h_cu_seqlens[s0], 0, maxl, H, hd, b.pos_key, b.pos_query,
                                             w->d_idx, reach, S, lo, hi, scale, strips, p.strip_bytes, s));
            s0 = s1;
        }
        MQ_TRY(mq_gemm_bf16(a, W, b.out_w, W, b.out_b, x, x, W, rows, W, W, res_flags, s));
        MQ_TRY(mq_layernorm(x, nullptr, b.attn_ln_g, b.attn_ln_b, h, x, rows, W, cfg->ln_eps, s));   // (in place: a wave holds its whole row before it stores)
        MQ_TRY(mq_gemm_bf16(h, W, b.fc1_w, W, b.fc1_b, nullptr, big, F, rows, F, W, MQ_EPI_BIAS | MQ_EPI_GELU, s));
        MQ_TRY(mq_gemm_bf16(big, F, b.fc2_w, F, b.fc2_b, x, x, W, rows, W, F, res_flags, s));
        MQ_TRY(mq_layernorm(x, nullptr, b.mlp_ln_g, b.mlp_ln_b, h, x, rows, W, cfg->ln_eps, s));
    }
    MQ_TRY(mq_pool(x, d_cu_seqlens, nseq, d_out, W, cfg->pool, normalize, s));
    return MQ_OK;
}
