// Decoder-style text embedders (transformers Qwen3Model / Qwen2Model: Qwen3-Embedding-0.6B, gte-Qwen2-1.5B-instruct, Qwen2-0.5B fine-tunes) on one HIP
// stream, no allocation, no sync: the two row kernels this family adds (RMSNorm; per-head q/k RMSNorm + rotary positions) and the host-side orchestration
// of the tower on kernels that live in the sibling units — the token gather (embed.hip), the bf16 GEMMs, grouped-query causal attention
// (attention_gqa.hip), the gated-SiLU product (embed.hip: mq_glu), last-row / mean pooling.
//
// Per block, on the fp32 residual stream x [rows, W] (pre-norm; no Linear has a bias but Qwen2's q / k / v projections):
//   h = rmsnorm(x, input_layernorm)
//   qkv = h Wqkv^T (+ bqkv)                     Wqkv = cat(q_proj, k_proj, v_proj) at load: [(Q + 2 KV) hd, W]
//   qk_norm_rope(qkv) ; a = attention_gqa(qkv, causal)
//   x += a Wo^T                                 (K of this GEMM is Q hd, which need not be W)
//   h = rmsnorm(x, post_attention_layernorm)
//   (up | gate) = h Wug^T                       Wug = cat(up_proj, gate_proj) at load
//   p = up * silu(gate) ; x += p Wdown^T
// then the final RMSNorm — over the pooled last rows only under MQ_POOL_LAST — and the pooling (+ L2).
//
// The checks in front of the first launch and the workspace arithmetic are the packed-token scaffold of packed_text.h.
#include "packed_text.h"

static_assert(sizeof(mq_qwen_layer) == 72 && sizeof(mq_qwen_weights) == 40 && sizeof(mq_qwen_cfg) == 40, "Qwen layouts (marqo_amd/_lib.py)");

namespace {

// ---- RMSNorm: y = x * rsqrt(mean(x^2) + eps) * g.  One wave64 per row, CH float4 chunks per lane; fp32 statistics in one pass over the registers, one
// rounding to bf16.  Rows are gathered through row_idx when it is given (the pooled rows of the tail).
template <int CH>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* x /* may alias out_f32 */, const int32_t* __restrict__ row_idx, const float* __restrict__ gam,
                                                      bf16_t* out_bf16, float* out_f32, int64_t rows, int W, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nch = W >> 2;
    const int64_t src = row_idx ? (int64_t)row_idx[row] : row;
    f32x4 v[CH], gv[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        v[i] = c < nch ? *(const f32x4*)(x + src * W + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        gv[i] = c < nch ? *(const f32x4*)(gam + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) ss += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
    const float rstd = rsqrtf(wave_sum(ss) / (float)W + eps);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        if (c >= nch) continue;
        const f32x4 y = (v[i] * rstd) * gv[i];
        if (out_f32) *(f32x4*)(out_f32 + row * W + c * 4) = y;
        if (out_bf16) {
            uint2 p;
            p.x = pack_bf16x2(y[0], y[1]);
            p.y = pack_bf16x2(y[2], y[3]);
            *(uint2*)(out_bf16 + row * W + c * 4) = p;
        }
    }
}

// ---- per-head q / k RMSNorm (Qwen3's q_norm / k_norm; none for Qwen2) and rotary positions, in place on the q and k parts of the QKV buffer.
// grid = (sequences, row slabs).  HD / 4 lanes own one (row, head): lane j of them holds dims 2j, 2j + 1 of the first half and their rotate_half partners
// 2j + HD/2, 2j + 1 + HD/2 — two 4-byte loads, fp32 norm and rotation with accurate sincosf (angles reach 8191 rad), ONE rounding to bf16, two stores.
template <int HD, bool NORM>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(bf16_t* __restrict__ qkv, const int32_t* __restrict__ cu, int fixed_len, int q_heads, int kv_heads,
                                                           const float* __restrict__ q_g, const float* __restrict__ k_g, float eps,
                                                           const float* __restrict__ inv_freq, int offset) {
    constexpr int LPH = HD / 4;            // lanes per head (16, 32 or 64)
    constexpr int UPB = 256 / LPH;         // (row, head) units per block and step
    const int row0 = cu ? cu[blockIdx.x] : blockIdx.x * fixed_len;
    const int len = cu ? cu[blockIdx.x + 1] - row0 : fixed_len;
    const int nh = q_heads + kv_heads;
    const int ld = (q_heads + 2 * kv_heads) * HD;
    const int j = threadIdx.x % LPH;
    // this block's rows: blockIdx.y, blockIdx.y + gridDim.y, ...
    const int my_rows = len > (int)blockIdx.y ? (len - 1 - (int)blockIdx.y) / (int)gridDim.y + 1 : 0;
    const int total = my_rows * nh;
    const float f0 = inv_freq[2 * j], f1 = inv_freq[2 * j + 1];
    for (int base = 0; base < total; base += UPB) {          // (block-uniform bound: every lane reaches the shuffles)
        const int unit = base + threadIdx.x / LPH;
        const bool on = unit < total;
        const int u = on ? unit : total - 1;
        const int ri = u / nh, hh = u - ri * nh;
        const int t = (int)blockIdx.y + ri * (int)gridDim.y;   // the row's position in its sequence
        bf16_t* p = qkv + (int64_t)(row0 + t) * ld + hh * HD + 2 * j;
        const uint32_t lo = *(const uint32_t*)p, hi = *(const uint32_t*)(p + HD / 2);
        float x1[2] = {__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u)};
        float x2[2] = {__uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
        if (NORM) {
            float ss = (x1[0] * x1[0] + x1[1] * x1[1]) + (x2[0] * x2[0] + x2[1] * x2[1]);
#pragma unroll
            for (int o = LPH / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
            const float rstd = rsqrtf(ss / (float)HD + eps);
            const float* gam = (hh < q_heads ? q_g : k_g) + 2 * j;
            x1[0] = (x1[0] * rstd) * gam[0];
            x1[1] = (x1[1] * rstd) * gam[1];
            x2[0] = (x2[0] * rstd) * gam[HD / 2];
            x2[1] = (x2[1] * rstd) * gam[HD / 2 + 1];
        }
        float y1[2], y2[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float sn, cs;
            sincosf((float)(offset + t) * (k ? f1 : f0), &sn, &cs);   // (offset: the rows in front of the sequence, mq_qk_norm_rope_at; else 0)
            y1[k] = x1[k] * cs - x2[k] * sn;
            y2[k] = x2[k] * cs + x1[k] * sn;
        }
        if (on) {
            *(uint32_t*)p = pack_bf16x2(y1[0], y1[1]);
            *(uint32_t*)(p + HD / 2) = pack_bf16x2(y2[0], y2[1]);
        }
    }
}

struct Plan { size_t off_x, off_h, off_a, off_big, off_rows, total; };
Plan plan(const mq_qwen_cfg* c, int64_t rows, int64_t nseq) {
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
int check_cfg(const mq_qwen_cfg* c) {
    MQ_CHECK_ARG(c, "mq_encode_qwen: null cfg");
    MQ_CHECK_ARG(c->head_dim == 64 || c->head_dim == 128, "mq_encode_qwen: head_dim %d unsupported (64 or 128)", c->head_dim);
    MQ_TRY(check_gqa_shape("mq_encode_qwen", c->q_heads, c->kv_heads, c->width));
    MQ_CHECK_ARG(c->width <= 2048, "mq_encode_qwen: width %d > 2048 (the 4B / 8B sizes of this family are not served)", c->width);
    MQ_TRY(check_tower_sizes("mq_encode_qwen", c->mlp_dim, c->layers, c->vocab, c->max_pos));
    MQ_CHECK_ARG(c->pool == MQ_POOL_MEAN || c->pool == MQ_POOL_LAST, "mq_encode_qwen: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_LAST)", c->pool);
    return MQ_OK;
}
}  // namespace

extern "C" int mq_rmsnorm(const float* d_x, const int32_t* d_row_idx, const float* d_g, void* d_out_bf16, float* d_out_f32, int64_t rows, int32_t W,
                          float eps, void* stream) {
    MQ_CHECK_ARG(d_x && d_g && (d_out_bf16 || d_out_f32), "mq_rmsnorm: null pointer");
    MQ_CHECK_ARG(W >= 4 && W % 4 == 0 && W <= 2048, "mq_rmsnorm: W=%d unsupported (multiple of 4, <= 2048)", W);
    if (rows <= 0) return MQ_OK;
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(1, s);
    MQ_DISPATCH_CH(W, hipLaunchKernelGGL((rmsnorm_kernel<CH>), dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, d_x, d_row_idx, d_g, (bf16_t*)d_out_bf16,
                                         d_out_f32, rows, (int)W, eps));
    MQ_CHECK_LAUNCH("mq_rmsnorm");
    return MQ_OK;
}

namespace {
// mq_qk_norm_rope (offset 0) and mq_qk_norm_rope_at: the same checks under the entry point's name `fn`, the same launch
int qk_norm_rope(const char* fn, void* d_qkv, const int32_t* d_cu, int64_t nseq, int32_t fixed_len, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                 const float* d_q_g, const float* d_k_g, float eps, const float* d_inv_freq, int32_t offset, void* stream) {
    MQ_CHECK_ARG(d_qkv && d_inv_freq, "%s: null pointer", fn);
    MQ_CHECK_ARG(head_dim == 64 || head_dim == 128 || head_dim == 256, "%s: head_dim %d unsupported (64, 128 or 256)", fn, head_dim);
    MQ_CHECK_ARG(q_heads >= 1 && kv_heads >= 1 && q_heads <= 1024 && kv_heads <= q_heads, "%s: q_heads %d / kv_heads %d", fn, q_heads, kv_heads);
    MQ_CHECK_ARG((d_q_g == nullptr) == (d_k_g == nullptr), "%s: q and k norm weights come together or not at all", fn);
    MQ_CHECK_ARG(d_cu || fixed_len > 0, "%s: need fixed_len or cu_seqlens", fn);
    MQ_CHECK_ARG(offset >= 0 && offset <= 8192, "%s: offset %d outside [0, 8192]", fn, offset);
    if (nseq <= 0) return MQ_OK;
    MQ_CHECK_ARG(nseq < (1LL << 31), "%s: grid too large", fn);
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(3, s);
    const dim3 grid((unsigned)nseq, nseq >= 2048 ? 1 : 8), block(256);
    const int fl = d_cu ? 0 : fixed_len;
#define MQ_QK_ROPE(HD, NORM) \
    hipLaunchKernelGGL((qk_norm_rope_kernel<HD, NORM>), grid, block, 0, s, (bf16_t*)d_qkv, d_cu, fl, q_heads, kv_heads, d_q_g, d_k_g, eps, d_inv_freq, offset)
    if (head_dim == 64) {
        if (d_q_g) MQ_QK_ROPE(64, true); else MQ_QK_ROPE(64, false);
    } else if (head_dim == 256) {   // (EmbeddingGemma: one wave64 per (row, head))
        if (d_q_g) MQ_QK_ROPE(256, true); else MQ_QK_ROPE(256, false);
    } else {
        if (d_q_g) MQ_QK_ROPE(128, true); else MQ_QK_ROPE(128, false);
    }
#undef MQ_QK_ROPE
    MQ_CHECK_LAUNCH(fn);
    return MQ_OK;
}
}  // namespace

extern "C" int mq_qk_norm_rope(void* d_qkv, const int32_t* d_cu, int64_t nseq, int32_t fixed_len, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                               const float* d_q_g, const float* d_k_g, float eps, const float* d_inv_freq, void* stream) {
    return qk_norm_rope("mq_qk_norm_rope", d_qkv, d_cu, nseq, fixed_len, q_heads, kv_heads, head_dim, d_q_g, d_k_g, eps, d_inv_freq, 0, stream);
}

// mq_qk_norm_rope with a position offset: row t of a sequence rotates at position offset + t (the segments behind a shared prefix of `offset` rows)
extern "C" int mq_qk_norm_rope_at(void* d_qkv, const int32_t* d_cu, int64_t nseq, int32_t fixed_len, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                                  const float* d_q_g, const float* d_k_g, float eps, const float* d_inv_freq, int32_t offset, void* stream) {
    return qk_norm_rope("mq_qk_norm_rope_at", d_qkv, d_cu, nseq, fixed_len, q_heads, kv_heads, head_dim, d_q_g, d_k_g, eps, d_inv_freq, offset, stream);
}

extern "C" size_t mq_qwen_workspace_bytes(const mq_qwen_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return plan(cfg, rows, nseq).total;
}

extern "C" int mq_encode_qwen(const mq_qwen_cfg* cfg, const mq_qwen_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens,
                              int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream) {
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_out, "mq_encode_qwen: null pointer");
    MQ_CHECK_ARG(w->tok_emb && w->final_norm_g && w->zeros && w->d_inv_freq && w->layers, "mq_encode_qwen: null weight pointer");
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_qwen_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.input_norm_g && b.qkv_w && b.out_w && b.post_norm_g && b.ug_w && b.down_w, "mq_encode_qwen: layer %d has null weights", l);
        MQ_CHECK_ARG((b.q_norm_g == nullptr) == (b.k_norm_g == nullptr), "mq_encode_qwen: layer %d has one of q_norm / k_norm only", l);
    }
    if (nseq <= 0) return MQ_OK;
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin("mq_encode_qwen", d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const Plan p = plan(cfg, rows, nseq);
    MQ_TRY(packed_workspace("mq_encode_qwen", workspace_bytes, p.total));
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

    // embed_tokens: a gather, no positions, no norm
    MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq, w->tok_emb, nullptr, nullptr, nullptr, nullptr, x, nullptr, W, cfg->vocab, cfg->rms_eps, 0, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_qwen_layer& b = w->layers[l];
        MQ_TRY(mq_rmsnorm(x, nullptr, b.input_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, b.qkv_b, nullptr, big, QKVW, rows, QKVW, W, b.qkv_b ? MQ_EPI_BIAS : 0, s));
        MQ_TRY(mq_qk_norm_rope(big, d_cu_seqlens, nseq, 0, Q, KV, hd, b.q_norm_g, b.k_norm_g, cfg->rms_eps, w->d_inv_freq, s));
        MQ_TRY(mq_attention_gqa(big, a, d_cu_seqlens, nseq, 0, maxl, Q, KV, hd, MQ_MASK_CAUSAL, s));
        MQ_TRY(mq_gemm_bf16(a, AW, b.out_w, AW, w->zeros, x, x, W, rows, W, AW, res_flags, s));
        MQ_TRY(mq_rmsnorm(x, nullptr, b.post_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.ug_w, W, nullptr, nullptr, big, 2 * F, rows, 2 * F, W, 0, s));
        MQ_TRY(mq_glu(big, rows, F, MQ_ACT_SILU, 0, s));
        MQ_TRY(mq_gemm_bf16(big, 2 * F, b.down_w, F, w->zeros, x, x, W, rows, W, F, res_flags, s));
    }
    if (cfg->pool == MQ_POOL_LAST) {   // the final norm is per row: only the pooled rows take it
        MQ_TRY(mq_last_rows(d_cu_seqlens, last, nseq, s));
        MQ_TRY(mq_rmsnorm(x, last, w->final_norm_g, nullptr, d_out, nseq, W, cfg->rms_eps, s));
        if (normalize) MQ_TRY(mq_l2_normalize(d_out, d_out, nseq, W, s));
    } else {
        MQ_TRY(mq_rmsnorm(x, nullptr, w->final_norm_g, nullptr, x, rows, W, cfg->rms_eps, s));   // (in place: a wave holds its whole row before it stores)
        MQ_TRY(mq_pool(x, d_cu_seqlens, nseq, d_out, W, MQ_POOL_MEAN, normalize, s));
    }
    return MQ_OK;
}

// ---- Qwen3 rerankers: one query against n documents, the part every pair shares computed once ---------------------------------------------------------
// Packed rows [prefix | seg_1 | ... | seg_n]: the prefix (system prompt, instruction, query: identical for every hit of a search, and under the causal
// mask independent of what follows it) is sequence 0 of the batch, so cu_seqlens has nseq + 2 entries {0, P, P + d_1, ...}; P = prefix_len may be 0 (no
// sharing: every segment is a whole pair).  The token gather, the norms, the GEMMs, the gated product and the residuals are row-wise and run over all
// rows at once; the rotary step runs on the prefix at offset 0 and on the segments at offset P; attention is mq_attention_gqa (causal) on the prefix and
// mq_attention_gqa_prefix on the segments.  The final norm runs on every segment's last row only, and the logit is one fp32 dot product with the score row.
namespace {
struct PairsPlan { Plan tower; size_t off_pooled, total; };
PairsPlan pairs_plan(const mq_qwen_cfg* c, int64_t rows, int64_t nseq) {
    PairsPlan p;
    p.tower = plan(c, rows, nseq);
    Off ws;
    ws.take(p.tower.total);
    p.off_pooled = ws.take((size_t)nseq * c->width * 4);   // the normalised last row of every segment, fp32
    p.total = ws.end();
    return p;
}
}  // namespace

extern "C" size_t mq_score_qwen_pairs_workspace_bytes(const mq_qwen_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return pairs_plan(cfg, rows, nseq).total;
}

extern "C" int mq_score_qwen_pairs(const mq_qwen_cfg* cfg, const mq_qwen_weights* w, const float* d_score_w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                                   const int32_t* h_cu_seqlens, int64_t nseq, int32_t prefix_len, float* d_logits, float* d_scores, void* d_workspace,
                                   size_t workspace_bytes, void* stream) {
    const char* what = "mq_score_qwen_pairs";
    MQ_TRY(check_cfg(cfg));
    MQ_CHECK_ARG(w && d_score_w && d_logits, "%s: null pointer", what);
    MQ_CHECK_ARG(w->tok_emb && w->final_norm_g && w->zeros && w->d_inv_freq && w->layers, "%s: null weight pointer", what);
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_qwen_layer& b = w->layers[l];
        MQ_CHECK_ARG(b.input_norm_g && b.qkv_w && b.out_w && b.post_norm_g && b.ug_w && b.down_w, "%s: layer %d has null weights", what, l);
        MQ_CHECK_ARG((b.q_norm_g == nullptr) == (b.k_norm_g == nullptr), "%s: layer %d has one of q_norm / k_norm only", what, l);
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
    const PairsPlan pp = pairs_plan(cfg, rows, nseq);
    const Plan& p = pp.tower;
    MQ_TRY(packed_workspace(what, workspace_bytes, pp.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)(base + p.off_x);
    void* h = base + p.off_h;
    void* a = base + p.off_a;
    void* big = base + p.off_big;
    int32_t* last = (int32_t*)(base + p.off_rows);
    float* pooled = (float*)(base + pp.off_pooled);
    const int32_t* d_seg_cu = d_cu_seqlens + 1;     // {P, P + d_1, ...}: the segments, as mq_attention_gqa_prefix reads them
    const int W = cfg->width, F = cfg->mlp_dim, Q = cfg->q_heads, KV = cfg->kv_heads, hd = cfg->head_dim;
    const int AW = Q * hd, QKVW = (Q + 2 * KV) * hd;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;   // (the bias is w->zeros)

    MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq + 1, w->tok_emb, nullptr, nullptr, nullptr, nullptr, x, nullptr, W, cfg->vocab, cfg->rms_eps, 0, s));
    for (int l = 0; l < cfg->layers; ++l) {
        const mq_qwen_layer& b = w->layers[l];
        MQ_TRY(mq_rmsnorm(x, nullptr, b.input_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.qkv_w, W, b.qkv_b, nullptr, big, QKVW, rows, QKVW, W, b.qkv_b ? MQ_EPI_BIAS : 0, s));
        if (P) {   // the prefix: one fixed-length causal sequence of P rows at positions 0 .. P - 1
            MQ_TRY(mq_qk_norm_rope(big, nullptr, 1, P, Q, KV, hd, b.q_norm_g, b.k_norm_g, cfg->rms_eps, w->d_inv_freq, s));
            MQ_TRY(mq_attention_gqa(big, a, nullptr, 1, P, P, Q, KV, hd, MQ_MASK_CAUSAL, s));
        }
        MQ_TRY(mq_qk_norm_rope_at(big, d_seg_cu, nseq, 0, Q, KV, hd, b.q_norm_g, b.k_norm_g, cfg->rms_eps, w->d_inv_freq, P, s));
        MQ_TRY(mq_attention_gqa_prefix(big, a, d_seg_cu, nseq, P, maxseg, Q, KV, hd, s));
        MQ_TRY(mq_gemm_bf16(a, AW, b.out_w, AW, w->zeros, x, x, W, rows, W, AW, res_flags, s));
        MQ_TRY(mq_rmsnorm(x, nullptr, b.post_norm_g, h, nullptr, rows, W, cfg->rms_eps, s));
        MQ_TRY(mq_gemm_bf16(h, W, b.ug_w, W, nullptr, nullptr, big, 2 * F, rows, 2 * F, W, 0, s));
        MQ_TRY(mq_glu(big, rows, F, MQ_ACT_SILU, 0, s));
        MQ_TRY(mq_gemm_bf16(big, 2 * F, b.down_w, F, w->zeros, x, x, W, rows, W, F, res_flags, s));
    }
    MQ_TRY(mq_last_rows(d_seg_cu, last, nseq, s));
    MQ_TRY(mq_rmsnorm(x, last, w->final_norm_g, nullptr, pooled, nseq, W, cfg->rms_eps, s));
    return mq_score_dot(pooled, d_score_w, nseq, W, d_logits, d_scores, s);
}
