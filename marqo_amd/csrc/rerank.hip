// Text reranking: a cross-encoder (BertForSequenceClassification / XLMRobertaForSequenceClassification, one logit) on the BERT tower.
//   * pair_plan / pack_pairs: [CLS] q [SEP] d [SEP] for ONE query against n documents with the `tokenizers` library's LongestFirst
//     truncation, from the ids mq_tokenize_wordpiece left on the device.  pack_pairs_xlmr: <s> q </s> </s> d </s> (four specials, no
//     type ids) from the rows mq_tokenize_sentencepiece left there.
//   * embed_tokens_typed: embed.hip's embed_tokens with a token-type id per row.
//   * score_head: pooler (tanh(Linear), through mq_gemm_bf16) + the one-logit classifier (+ sigmoid).
//   * mq_score_pairs_bert: typed embedding -> encoder (the [CLS] row selection of mq_encode_bert) -> head.
//   * mq_score_pairs_xlmr: the same with mq_encode_bert's own embedding (one type row; the position table starts at the offset row).
//   * score_head_ln: ModernBERT's classification head: dense + erf-GELU (mq_gemm_bf16's epilogue), then LayerNorm and the one-logit classifier
//     fused in one wave64 per pair (+ sigmoid).  mq_score_pairs_modernbert: mq_encode_modernbert (normalize = 0) -> that head.
//   * mq_score_head_gelu: DeBERTa's ContextPooler head: dense -> erf GELU -> one-logit classifier (+ sigmoid); mq_score_head with the tail's activation
//     swapped (score_tail_kernel's template parameter).  mq_score_pairs_deberta: mq_encode_deberta (CLS rows, normalize = 0) -> that head.
// All of it is bandwidth-trivial next to the encoder: coalesced, bounds-guarded, untuned.
// WS_ALIGN and score_pairs' packed-sequence checks are packed_text.h's.
#include "packed_text.h"

int mq_cast_bf16(const float* d_x, void* d_out, int64_t n, hipStream_t s);   // rowops.hip

static_assert(sizeof(mq_score_head_weights) == 32, "mq_score_head_weights layout");   // (marqo_amd/_lib.py ScoreHeadWeights)
static_assert(sizeof(mq_score_head_ln_weights) == 48, "mq_score_head_ln_weights layout");   // (marqo_amd/_lib.py ScoreHeadLnWeights)

namespace {
constexpr int MAXC = 8;          // W <= 2048

// ---- LongestFirst truncation of a pair to B pieces ----------------------------------------------------------------------------------
// tokenizers' truncate_encodings: n1 = the shorter (the FIRST text on a tie), n2 = n1 when n1 > B else max(n1, B - n1); when that
// still exceeds B: n1 = B / 2, n2 = B - n1; the texts take them back in their own order.
__host__ __device__ inline void pair_keep(int la, int lb, int B, int* a, int* b) {
    if (la + lb <= B) { *a = la; *b = lb; return; }
    const bool swap = la > lb;
    int s = swap ? lb : la;
    int l = s > B ? s : (s > B - s ? s : B - s);
    if (s + l > B) { s = B / 2; l = B - s; }
    *a = swap ? l : s;
    *b = swap ? s : l;
}

__global__ __launch_bounds__(256) void pair_plan_kernel(int la, const int32_t* __restrict__ doc_len, int n, int ld, int B, int specials,
                                                        int32_t* __restrict__ keep_a, int32_t* __restrict__ keep_b, int32_t* __restrict__ total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int lb = doc_len[i] - 2;                      // [CLS] pieces [SEP] / <s> pieces </s>
    lb = lb < 0 ? 0 : (lb > ld - 2 ? ld - 2 : lb);
    int a, b;
    pair_keep(la, lb, B, &a, &b);
    keep_a[i] = a;
    keep_b[i] = b;
    total[i] = a + b + specials;
}

// grid = n blocks; the block's threads walk the sequence's rows.  Reads stay inside q [Lq] and row i of docs [n, ld], writes inside
// [cu[i], min(cu[i + 1], rows)), whatever the plan arrays hold.
__global__ __launch_bounds__(256) void pack_pairs_kernel(const int32_t* __restrict__ q, int Lq, const int32_t* __restrict__ docs, int ld,
                                                         const int32_t* __restrict__ keep_a, const int32_t* __restrict__ keep_b,
                                                         const int32_t* __restrict__ cu, int cls_id, int sep_id, int32_t* __restrict__ ids,
                                                         int32_t* __restrict__ types, int64_t rows) {
    const int i = blockIdx.x;
    int a = keep_a[i], b = keep_b[i];
    a = a < 0 ? 0 : (a > Lq ? Lq : a);
    b = b < 0 ? 0 : (b > ld - 2 ? ld - 2 : b);
    const int64_t row0 = cu[i];
    int len = cu[i + 1] - cu[i];
    if (len > a + b + 3) len = a + b + 3;
    if (row0 < 0) return;
    const int32_t* d = docs + (int64_t)i * ld + 1;
    for (int t = threadIdx.x; t < len && row0 + t < rows; t += 256) {
        int id, ty = 0;
        if (t == 0) id = cls_id;
        else if (t <= a) id = q[t - 1];
        else if (t == a + 1) id = sep_id;
        else if (t < a + 2 + b) { id = d[t - a - 2]; ty = 1; }
        else { id = sep_id; ty = 1; }
        ids[row0 + t] = id;
        types[row0 + t] = ty;
    }
}

// <s> q[:a] </s> </s> d[:b] </s>: the same walk with four specials and no type ids; the same clamps keep reads inside q [Lq] and the pieces
// of row i of docs [n, ld] (columns 1 .. ld - 2), writes inside [cu[i], min(cu[i + 1], rows)).
__global__ __launch_bounds__(256) void pack_pairs_xlmr_kernel(const int32_t* __restrict__ q, int Lq, const int32_t* __restrict__ docs, int ld,
                                                              const int32_t* __restrict__ keep_a, const int32_t* __restrict__ keep_b,
                                                              const int32_t* __restrict__ cu, int cls_id, int sep_id, int32_t* __restrict__ ids,
                                                              int64_t rows) {
    const int i = blockIdx.x;
    int a = keep_a[i], b = keep_b[i];
    a = a < 0 ? 0 : (a > Lq ? Lq : a);
    b = b < 0 ? 0 : (b > ld - 2 ? ld - 2 : b);
    const int64_t row0 = cu[i];
    int len = cu[i + 1] - cu[i];
    if (len > a + b + 4) len = a + b + 4;
    if (row0 < 0) return;
    const int32_t* d = docs + (int64_t)i * ld + 1;
    for (int t = threadIdx.x; t < len && row0 + t < rows; t += 256) {
        int id;
        if (t == 0) id = cls_id;
        else if (t <= a) id = q[t - 1];
        else if (t <= a + 2) id = sep_id;
        else if (t < a + 3 + b) id = d[t - a - 3];
        else id = sep_id;
        ids[row0 + t] = id;
    }
}

// ---- token + position + type[type id] embedding (+ LayerNorm): embed.hip's embed_tokens_kernel with the type row looked up per token -----
// (the same statements in the same order, so that all-zero type ids reproduce its bits)
template <bool LN, int CH>
__global__ __launch_bounds__(256, (CH <= 2 ? 8 : 4)) void embed_tokens_typed_kernel(
    const int32_t* __restrict__ ids, const int32_t* __restrict__ tids, const int32_t* __restrict__ cu, const float* __restrict__ tok,
    const float* __restrict__ pos, const float* __restrict__ type_emb, int type_vocab, const float* __restrict__ gam,
    const float* __restrict__ bet, float* __restrict__ x, bf16_t* __restrict__ xb, int W, int vocab, float eps, int last_pos) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = cu[blockIdx.x], len = cu[blockIdx.x + 1] - row0;
    const int nch = W >> 2;
    for (int t = wave; t < len; t += 4) {
        const int64_t row = row0 + t;
        int id = ids[row];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        int ty = tids[row];
        ty = ty < 0 ? 0 : (ty >= type_vocab ? type_vocab - 1 : ty);
        const float* tr = tok + (int64_t)id * W;
        const float* pr = pos ? pos + (int64_t)((last_pos > 0 && t == len - 1) ? last_pos : t) * W : nullptr;
        const float* yr = type_emb + (int64_t)ty * W;
        f32x4 v[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + i * 64;
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < nch) {
                v[i] = *(const f32x4*)(tr + c * 4);
                if (pr) v[i] += *(const f32x4*)(pr + c * 4);
                v[i] += *(const f32x4*)(yr + c * 4);
            }
        }
        if (LN) ln_normalize_row<CH>(v, lane, nch, W, eps);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + i * 64;
            if (c < nch) {
                f32x4 y = v[i];
                if (LN) {
                    const f32x4 gg = *(const f32x4*)(gam + c * 4);
                    const f32x4 bb = *(const f32x4*)(bet + c * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = v[i][e] * gg[e] + bb[e];
                }
                if (x) *(f32x4*)(x + row * W + c * 4) = y;
                if (xb) {
                    uint2 p;
                    p.x = pack_bf16x2(y[0], y[1]);
                    p.y = pack_bf16x2(y[2], y[3]);
                    *(uint2*)(xb + row * W + c * 4) = p;
                }
            }
        }
    }
}

// ---- classifier on the pooler's pre-activation: one wave64 per pair --------------------------------------------------------------------
// z = sum_j cls_w[j] act(p[j]) + cls_b: lane c takes columns c, c + 64, ... (fma chain), the xor butterfly adds the lanes.  GELU = false: act = tanhf
// (BERT's pooler, RoBERTa's classification head); GELU = true: the erf GELU 0.5 x (1 + erff(x / sqrt(2))) with libm's erff (DeBERTa's ContextPooler —
// n W values per call: the GEMM epilogues' polynomial, rounded to bf16 there, would be the largest error of a logit here)
template <bool GELU>
__global__ __launch_bounds__(256) void score_tail_kernel(const float* __restrict__ p, const float* __restrict__ cls_w, float cls_b, int64_t n,
                                                         int W, float* __restrict__ logits, float* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float* pr = p + r * W;
    float acc = 0.f;
    for (int j = lane; j < W; j += 64) {
        const float x = pr[j];
        acc = fmaf(cls_w[j], GELU ? 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)) : tanhf(x), acc);
    }
    const float z = wave_sum(acc) + cls_b;
    if (lane == 0) {
        logits[r] = z;
        if (scores) scores[r] = 1.0f / (1.0f + expf(-z));
    }
}

// ---- the head of the decoder rerankers (Qwen3-Reranker): z = x . w, one fp32 weight row, no dense layer and no bias: one wave64 per pair ------------
// (lane c takes columns c, c + 64, ... in an fma chain, the xor butterfly adds the lanes)
__global__ __launch_bounds__(256) void score_dot_kernel(const float* __restrict__ x, const float* __restrict__ w, int64_t n, int W,
                                                        float* __restrict__ logits, float* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float* xr = x + r * W;
    float acc = 0.f;
    for (int j = lane; j < W; j += 64) acc = fmaf(w[j], xr[j], acc);
    const float z = wave_sum(acc);
    if (lane == 0) {
        logits[r] = z;
        if (scores) scores[r] = 1.0f / (1.0f + expf(-z));
    }
}

// ---- LayerNorm + classifier on the dense layer's GELU output: one wave64 per pair --------------------------------------------------------
// z = sum_j ((a_j - mu) rstd g_j + b_j) c_j + c_b.  Lane c holds columns c, c + 64, ... of the row (W / 64 <= 32 registers, read once); the mean
// and the sum of squared deviations (two-pass, as ln_normalize_row) and the classifier's dot product each go through the xor butterfly.  The
// normalised row exists in registers only.  norm_b may be null (no LayerNorm bias).
constexpr int TAIL_LN_MAXJ = 4 * MAXC;     // columns per lane at W = 2048
__global__ __launch_bounds__(256) void score_tail_ln_kernel(const float* __restrict__ a, const float* __restrict__ norm_g, const float* __restrict__ norm_b,
                                                            const float* __restrict__ cls_w, float cls_b, float eps, int64_t n, int W,
                                                            float* __restrict__ logits, float* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;                    // (the whole wave leaves: r is wave-uniform)
    const float* ar = a + r * W;
    const int nc = W >> 6;
    float v[TAIL_LN_MAXJ];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < TAIL_LN_MAXJ; ++i) {
        v[i] = i < nc ? ar[lane + i * 64] : 0.f;
        s += v[i];
    }
    const float mean = wave_sum(s) / (float)W;
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < TAIL_LN_MAXJ; ++i)
        if (i < nc) { const float d = v[i] - mean; s2 = fmaf(d, d, s2); }
    const float rstd = rsqrtf(wave_sum(s2) / (float)W + eps);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < TAIL_LN_MAXJ; ++i)
        if (i < nc) {
            const int j = lane + i * 64;
            const float y = fmaf((v[i] - mean) * rstd, norm_g[j], norm_b ? norm_b[j] : 0.f);
            acc = fmaf(y, cls_w[j], acc);
        }
    const float z = wave_sum(acc) + cls_b;
    if (lane == 0) {
        logits[r] = z;
        if (scores) scores[r] = 1.0f / (1.0f + expf(-z));
    }
}

struct HeadLnPlan { size_t off_hb, off_a, off_zero, total; };
HeadLnPlan head_ln_plan(int64_t n, int W) {
    HeadLnPlan h;
    Off ws;
    h.off_hb = ws.take((size_t)n * W * 2);        // bf16 [n, W]: the pooled rows as the GEMM's operand
    h.off_a = ws.take((size_t)n * W * 4);         // fp32 [n, W]: gelu(dense_w h + dense_b)
    h.off_zero = ws.take((size_t)W * 4);          // fp32 [W] of zeros: the GEMM's bias when the head has none
    h.total = ws.end();
    return h;
}

struct HeadPlan { size_t off_hb, off_p, total; };
HeadPlan head_plan(int64_t n, int W) {
    HeadPlan h;
    h.off_hb = 0;                                                       // bf16 [n, W]: the rows as the GEMM's operand
    h.off_p = align_up((size_t)n * W * 2, WS_ALIGN);                    // fp32 [n, W]: pooler_w h + pooler_b
    h.total = h.off_p + align_up((size_t)n * W * 4, WS_ALIGN);
    return h;
}

struct PairsPlan { size_t off_enc, enc_bytes, off_cls, off_head, total; };
// [ mq_bert_workspace_bytes: x fp32 [rows, W] | encoder scratch ] [ CLS rows fp32 [nseq, W] ] [ head scratch ]
PairsPlan pairs_plan(const mq_bert_cfg* cfg, int64_t rows, int64_t nseq) {
    PairsPlan p;
    const size_t bert = align_up(mq_bert_workspace_bytes(cfg, rows, nseq), WS_ALIGN);
    p.off_enc = align_up((size_t)rows * cfg->enc.width * 4, WS_ALIGN);
    p.enc_bytes = bert - p.off_enc;
    p.off_cls = bert;
    p.off_head = p.off_cls + align_up((size_t)nseq * cfg->enc.width * 4, WS_ALIGN);
    p.total = p.off_head + head_plan(nseq, cfg->enc.width).total;
    return p;
}
}  // namespace

extern "C" int mq_pair_plan_n(int32_t Lq, const int32_t* d_doc_len, int64_t n, int32_t ld, int32_t max_length, int32_t specials,
                              int32_t* d_keep_a, int32_t* d_keep_b, int32_t* d_total, void* stream) {
    MQ_CHECK_ARG(specials >= 0 && specials <= 8, "mq_pair_plan: specials=%d must be in [0, 8]", specials);
    MQ_CHECK_ARG(max_length >= specials + 1, "mq_pair_plan: max_length=%d must be >= %d (%d special tokens and at least one piece)", max_length,
                 specials + 1, specials);
    MQ_CHECK_ARG(Lq >= 0 && ld >= 2 && n < (1ll << 31), "mq_pair_plan: bad shape Lq=%d ld=%d n=%lld", Lq, ld, (long long)n);
    if (n <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_doc_len && d_keep_a && d_keep_b && d_total, "mq_pair_plan: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(3, s);
    hipLaunchKernelGGL(pair_plan_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, Lq, d_doc_len, (int)n, ld, max_length - specials, specials,
                       d_keep_a, d_keep_b, d_total);
    MQ_CHECK_LAUNCH("mq_pair_plan");
    return MQ_OK;
}

// [CLS] a [SEP] b [SEP]: three specials
extern "C" int mq_pair_plan(int32_t Lq, const int32_t* d_doc_len, int64_t n, int32_t ld, int32_t max_length, int32_t* d_keep_a,
                            int32_t* d_keep_b, int32_t* d_total, void* stream) {
    return mq_pair_plan_n(Lq, d_doc_len, n, ld, max_length, 3, d_keep_a, d_keep_b, d_total, stream);
}

extern "C" int mq_pack_pairs(const int32_t* d_query, int32_t Lq, const int32_t* d_docs, int32_t ld, const int32_t* d_keep_a,
                             const int32_t* d_keep_b, const int32_t* d_cu, int64_t n, int32_t cls_id, int32_t sep_id, int32_t* d_ids,
                             int32_t* d_type_ids, int64_t rows, void* stream) {
    MQ_CHECK_ARG(Lq >= 0 && ld >= 2 && n < (1ll << 31) && rows >= 0, "mq_pack_pairs: bad shape Lq=%d ld=%d n=%lld rows=%lld", Lq, ld,
                 (long long)n, (long long)rows);
    if (n <= 0) return MQ_OK;
    MQ_CHECK_ARG((d_query || Lq == 0) && d_docs && d_keep_a && d_keep_b && d_cu && d_ids && d_type_ids, "mq_pack_pairs: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(3, s);
    hipLaunchKernelGGL(pack_pairs_kernel, dim3((unsigned)n), dim3(256), 0, s, d_query, Lq, d_docs, ld, d_keep_a, d_keep_b, d_cu, cls_id, sep_id,
                       d_ids, d_type_ids, rows);
    MQ_CHECK_LAUNCH("mq_pack_pairs");
    return MQ_OK;
}

extern "C" int mq_pack_pairs_xlmr(const int32_t* d_query, int32_t Lq, const int32_t* d_docs, int32_t ld, const int32_t* d_keep_a,
                                  const int32_t* d_keep_b, const int32_t* d_cu, int64_t n, int32_t cls_id, int32_t sep_id, int32_t* d_ids,
                                  int64_t rows, void* stream) {
    MQ_CHECK_ARG(Lq >= 0 && ld >= 2 && n < (1ll << 31) && rows >= 0, "mq_pack_pairs_xlmr: bad shape Lq=%d ld=%d n=%lld rows=%lld", Lq, ld,
                 (long long)n, (long long)rows);
    if (n <= 0) return MQ_OK;
    MQ_CHECK_ARG((d_query || Lq == 0) && d_docs && d_keep_a && d_keep_b && d_cu && d_ids, "mq_pack_pairs_xlmr: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(3, s);
    hipLaunchKernelGGL(pack_pairs_xlmr_kernel, dim3((unsigned)n), dim3(256), 0, s, d_query, Lq, d_docs, ld, d_keep_a, d_keep_b, d_cu, cls_id,
                       sep_id, d_ids, rows);
    MQ_CHECK_LAUNCH("mq_pack_pairs_xlmr");
    return MQ_OK;
}

extern "C" int mq_embed_tokens_typed(const int32_t* d_ids, const int32_t* d_type_ids, const int32_t* d_cu, int64_t nseq, const float* tok,
                                     const float* pos, const float* type_emb, int32_t type_vocab, const float* g, const float* b, float* d_x,
                                     void* d_xb, int32_t W, int32_t vocab, float eps, int32_t last_pos, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    MQ_CHECK_ARG(W >= 4 && W % 4 == 0 && W <= 64 * 4 * MAXC, "embed_tokens_typed: W=%d unsupported", W);
    MQ_CHECK_ARG(type_vocab >= 1 && vocab >= 1, "embed_tokens_typed: type_vocab=%d vocab=%d", type_vocab, vocab);
    if (nseq <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_ids && d_type_ids && d_cu && tok && type_emb && (!g || b) && (d_x || d_xb), "embed_tokens_typed: null pointer");
    MqProfScope prof(3, s);
    if (g)
        MQ_DISPATCH_CH(W, hipLaunchKernelGGL((embed_tokens_typed_kernel<true, CH>), dim3((unsigned)nseq), dim3(256), 0, s, d_ids, d_type_ids,
                                             d_cu, tok, pos, type_emb, type_vocab, g, b, d_x, (bf16_t*)d_xb, W, vocab, eps, last_pos));
    else
        MQ_DISPATCH_CH(W, hipLaunchKernelGGL((embed_tokens_typed_kernel<false, CH>), dim3((unsigned)nseq), dim3(256), 0, s, d_ids, d_type_ids,
                                             d_cu, tok, pos, type_emb, type_vocab, g, b, d_x, (bf16_t*)d_xb, W, vocab, eps, last_pos));
    MQ_CHECK_LAUNCH("embed_tokens_typed");
    return MQ_OK;
}

extern "C" size_t mq_score_head_workspace_bytes(int64_t n, int32_t W) {
    if (n <= 0 || W <= 0) return 0;
    return head_plan(n, W).total;
}

namespace {
// dense (mq_gemm_bf16, fp32 pre-activation) -> score_tail_kernel<GELU>; `what` (the entry point's name) opens every message
template <bool GELU>
int score_head(const char* what, const float* d_h, int64_t n, int32_t W, const mq_score_head_weights* head, float* d_logits, float* d_scores,
               void* d_workspace, size_t workspace_bytes, void* stream) {
    MQ_CHECK_ARG(head, "%s: null head", what);
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= 64 * 4 * MAXC, "%s: W=%d must be a multiple of 64, at most %d", what, W, 64 * 4 * MAXC);
    MQ_CHECK_ARG(head->pooler_w && head->pooler_b && head->cls_w, "%s: null weight pointer", what);
    MQ_CHECK_ARG(n < (1ll << 31), "%s: n=%lld too large", what, (long long)n);
    if (n <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_h && d_logits && d_workspace, "%s: null input / output / workspace", what);
    const HeadPlan hp = head_plan(n, W);
    if (workspace_bytes < hp.total) { mq_set_error("%s: workspace %zu < required %zu", what, workspace_bytes, hp.total); return MQ_ERR_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    void* hb = base + hp.off_hb;
    float* p = (float*)(base + hp.off_p);
    MQ_TRY(mq_cast_bf16(d_h, hb, n * W, s));
    MQ_TRY(mq_gemm_bf16(hb, W, head->pooler_w, W, head->pooler_b, nullptr, p, W, n, W, W, MQ_EPI_BIAS | MQ_EPI_OUT_F32, s));
    MqProfScope prof(4, s);
    hipLaunchKernelGGL(score_tail_kernel<GELU>, dim3((unsigned)cdiv64(n, 4)), dim3(256), 0, s, p, head->cls_w, head->cls_b, n, W, d_logits, d_scores);
    MQ_CHECK_LAUNCH(what);
    return MQ_OK;
}
}  // namespace

extern "C" int mq_score_head(const float* d_h, int64_t n, int32_t W, const mq_score_head_weights* head, float* d_logits, float* d_scores,
                             void* d_workspace, size_t workspace_bytes, void* stream) {
    return score_head<false>("mq_score_head", d_h, n, W, head, d_logits, d_scores, d_workspace, workspace_bytes, stream);
}

// DeBERTa's ContextPooler head: gelu(pooler_w bf16(h) + pooler_b) . cls_w + cls_b; the weights struct, the scratch (mq_score_head_workspace_bytes) and the
// checks are mq_score_head's, type_vocab is not read
extern "C" int mq_score_head_gelu(const float* d_h, int64_t n, int32_t W, const mq_score_head_weights* head, float* d_logits, float* d_scores,
                                  void* d_workspace, size_t workspace_bytes, void* stream) {
    return score_head<true>("mq_score_head_gelu", d_h, n, W, head, d_logits, d_scores, d_workspace, workspace_bytes, stream);
}

// The decoder rerankers' head: d_logits[i] = d_h[i] . d_w (fp32 [n, W] rows against one fp32 [W] row), d_scores (optional) its sigmoid
extern "C" int mq_score_dot(const float* d_h, const float* d_w, int64_t n, int32_t W, float* d_logits, float* d_scores, void* stream) {
    MQ_CHECK_ARG(W >= 1 && W <= 64 * 4 * MAXC, "mq_score_dot: W=%d must be in [1, %d]", W, 64 * 4 * MAXC);
    MQ_CHECK_ARG(n < (1ll << 31), "mq_score_dot: n=%lld too large", (long long)n);
    if (n <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_h && d_w && d_logits, "mq_score_dot: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(4, s);
    hipLaunchKernelGGL(score_dot_kernel, dim3((unsigned)cdiv64(n, 4)), dim3(256), 0, s, d_h, d_w, n, (int)W, d_logits, d_scores);
    MQ_CHECK_LAUNCH("mq_score_dot");
    return MQ_OK;
}

extern "C" size_t mq_score_pairs_workspace_bytes(const mq_bert_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0) return 0;
    return pairs_plan(cfg, rows, nseq).total;
}

namespace {
// typed = false: every token adds type row 0, through mq_embed_tokens as mq_encode_bert embeds (XLM-R: one type row).  The position of
// token t of a sequence is row t of w->pos_emb: for a checkpoint whose position ids start at padding_idx + 1 the host hands over the table
// from that row on (as for mq_encode_bert), so a packed pair runs offset, offset + 1, ... over the whole pair.
int score_pairs(const char* what, const mq_bert_cfg* cfg, const mq_bert_weights* w, const mq_score_head_weights* head, const int32_t* d_ids,
                const int32_t* d_type_ids, bool typed, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq, float* d_logits,
                float* d_scores, float* d_cls_rows, void* d_workspace, size_t workspace_bytes, void* stream) {
    MQ_CHECK_ARG(cfg && w && head && d_logits, "%s: null pointer", what);
    MQ_CHECK_ARG(cfg->enc.precision == MQ_PREC_BF16, "%s: bf16 encoders only (precision %d)", what, cfg->enc.precision);
    MQ_CHECK_ARG(cfg->enc.post_ln == 1 && cfg->enc.mask == MQ_MASK_NONE, "%s: BERT is post-LN with full attention", what);
    MQ_CHECK_ARG(!cfg->enc.d_rope_inv_freq && !cfg->enc.mlp_glu && !cfg->enc.d_rel_bias, "%s: plain BERT encoders only", what);
    MQ_CHECK_ARG(w->word_emb && w->pos_emb && w->type_emb && w->emb_ln_g && w->emb_ln_b, "%s: null weight pointer", what);
    MQ_CHECK_ARG(head->type_vocab >= 1, "%s: type_vocab=%d", what, head->type_vocab);
    const int W = cfg->enc.width;
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= 64 * 4 * MAXC, "%s: W=%d must be a multiple of 64, at most %d", what, W, 64 * 4 * MAXC);
    MQ_CHECK_ARG(nseq < (1ll << 31), "%s: nseq=%lld too large", what, (long long)nseq);
    if (nseq <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_type_ids || !typed, "%s: null input / workspace", what);
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin(what, d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const PairsPlan p = pairs_plan(cfg, rows, nseq);
    const size_t enc_need = mq_encoder_workspace_bytes(&cfg->enc, rows, nseq);
    MQ_TRY(packed_workspace(what, workspace_bytes, p.total));
    if (p.enc_bytes < enc_need) { mq_set_error("%s: encoder scratch %zu < required %zu", what, p.enc_bytes, enc_need); return MQ_ERR_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* x = (float*)base;
    float* cls = (float*)(base + p.off_cls);

    if (typed)
        MQ_TRY(mq_embed_tokens_typed(d_ids, d_type_ids, d_cu_seqlens, nseq, w->word_emb, w->pos_emb, w->type_emb, head->type_vocab, w->emb_ln_g,
                                     w->emb_ln_b, x, nullptr, W, cfg->vocab, cfg->enc.ln_eps, 0, s));
    else
        MQ_TRY(mq_embed_tokens(d_ids, d_cu_seqlens, nseq, w->word_emb, w->pos_emb, w->type_emb, w->emb_ln_g, w->emb_ln_b, x, nullptr, W, cfg->vocab,
                               cfg->enc.ln_eps, 0, s));
    // the final [CLS] row of sequence i is row d_cu_seqlens[i]: the last block may run on those rows only, as for MQ_POOL_CLS
    MQ_TRY(mq_encoder_forward_rows(&cfg->enc, w->blocks, x, rows, d_cu_seqlens, nseq, 0, maxl, d_cu_seqlens, nseq, base + p.off_enc, p.enc_bytes, s));
    MQ_TRY(mq_pool(x, d_cu_seqlens, nseq, cls, W, MQ_POOL_CLS, 0, s));
    if (d_cls_rows) MQ_CHECK_HIP(hipMemcpyAsync(d_cls_rows, cls, (size_t)nseq * W * 4, hipMemcpyDeviceToDevice, s));
    return mq_score_head(cls, nseq, W, head, d_logits, d_scores, base + p.off_head, workspace_bytes - p.off_head, s);
}
}  // namespace

extern "C" int mq_score_pairs_bert(const mq_bert_cfg* cfg, const mq_bert_weights* w, const mq_score_head_weights* head, const int32_t* d_ids,
                                   const int32_t* d_type_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq,
                                   float* d_logits, float* d_scores, float* d_cls_rows, void* d_workspace, size_t workspace_bytes,
                                   void* stream) {
    return score_pairs("mq_score_pairs_bert", cfg, w, head, d_ids, d_type_ids, true, d_cu_seqlens, h_cu_seqlens, nseq, d_logits, d_scores,
                       d_cls_rows, d_workspace, workspace_bytes, stream);
}

extern "C" int mq_score_pairs_xlmr(const mq_bert_cfg* cfg, const mq_bert_weights* w, const mq_score_head_weights* head, const int32_t* d_ids,
                                   const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq, float* d_logits, float* d_scores,
                                   float* d_cls_rows, void* d_workspace, size_t workspace_bytes, void* stream) {
    return score_pairs("mq_score_pairs_xlmr", cfg, w, head, d_ids, nullptr, false, d_cu_seqlens, h_cu_seqlens, nseq, d_logits, d_scores,
                       d_cls_rows, d_workspace, workspace_bytes, stream);
}

// ---- ModernBERT cross-encoders ------------------------------------------------------------------------------------------------------------
extern "C" size_t mq_score_head_ln_workspace_bytes(int64_t n, int32_t W) {
    if (n <= 0 || W <= 0) return 0;
    return head_ln_plan(n, W).total;
}

extern "C" int mq_score_head_ln(const float* d_h, int64_t n, int32_t W, const mq_score_head_ln_weights* head, float* d_logits, float* d_scores,
                                void* d_workspace, size_t workspace_bytes, void* stream) {
    MQ_CHECK_ARG(head, "mq_score_head_ln: null head");
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= 64 * TAIL_LN_MAXJ, "mq_score_head_ln: W=%d must be a multiple of 64, at most %d", W, 64 * TAIL_LN_MAXJ);
    MQ_CHECK_ARG(n >= 1 && n < (1ll << 31), "mq_score_head_ln: n=%lld must be in [1, 2^31)", (long long)n);
    MQ_CHECK_ARG(head->dense_w && head->norm_g && head->cls_w, "mq_score_head_ln: null weight pointer (dense_w / norm_g / cls_w)");
    MQ_CHECK_ARG(head->ln_eps >= 0.f, "mq_score_head_ln: ln_eps=%g must not be negative", (double)head->ln_eps);
    MQ_CHECK_ARG(d_h && d_logits && d_workspace, "mq_score_head_ln: null input / output / workspace");
    const HeadLnPlan hp = head_ln_plan(n, W);
    MQ_TRY(packed_workspace("mq_score_head_ln", workspace_bytes, hp.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    void* hb = base + hp.off_hb;
    float* a = (float*)(base + hp.off_a);
    const float* bias = head->dense_b;
    if (!bias) {   // (the GEMM family has one fp32-out GELU epilogue, the biased one: a head without a dense bias adds zeros)
        MQ_CHECK_HIP(hipMemsetAsync(base + hp.off_zero, 0, (size_t)W * 4, s));
        bias = (const float*)(base + hp.off_zero);
    }
    MQ_TRY(mq_cast_bf16(d_h, hb, n * W, s));
    MQ_TRY(mq_gemm_bf16(hb, W, head->dense_w, W, bias, nullptr, a, W, n, W, W, MQ_EPI_BIAS | MQ_EPI_GELU | MQ_EPI_OUT_F32, s));
    MqProfScope prof(4, s);
    hipLaunchKernelGGL(score_tail_ln_kernel, dim3((unsigned)cdiv64(n, 4)), dim3(256), 0, s, a, head->norm_g, head->norm_b, head->cls_w, head->cls_b,
                       head->ln_eps, n, W, d_logits, d_scores);
    MQ_CHECK_LAUNCH("mq_score_head_ln");
    return MQ_OK;
}

namespace {
struct PairsMbPlan { size_t off_enc, enc_bytes, off_pooled, off_head, total; };
// [ mq_modernbert_workspace_bytes: the encoder's own scratch ] [ pooled rows fp32 [nseq, W] ] [ head scratch ]
PairsMbPlan pairs_mb_plan(const mq_modernbert_cfg* cfg, int64_t rows, int64_t nseq) {
    PairsMbPlan p;
    Off ws;
    p.enc_bytes = mq_modernbert_workspace_bytes(cfg, rows, nseq);
    p.off_enc = ws.take(p.enc_bytes);
    p.off_pooled = ws.take((size_t)nseq * cfg->width * 4);
    p.off_head = ws.take(head_ln_plan(nseq, cfg->width).total);
    p.total = ws.end();
    return p;
}
}  // namespace

extern "C" size_t mq_score_pairs_modernbert_workspace_bytes(const mq_modernbert_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0 || cfg->width <= 0) return 0;
    return pairs_mb_plan(cfg, rows, nseq).total;
}

// The encoder IS mq_encode_modernbert (normalize = 0, the cfg's pooling) writing into this call's pooled slot: the pooled rows cannot differ from
// that entry point's.  What it refuses (cfg, weights, sequence lengths) it refuses here, under its own name; the checks below are this call's own.
extern "C" int mq_score_pairs_modernbert(const mq_modernbert_cfg* cfg, const mq_modernbert_weights* w, const mq_score_head_ln_weights* head,
                                         const int32_t* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq,
                                         float* d_logits, float* d_scores, float* d_pooled, void* d_workspace, size_t workspace_bytes,
                                         void* stream) {
    const char* what = "mq_score_pairs_modernbert";
    MQ_CHECK_ARG(cfg && w, "%s: null cfg / weights", what);
    MQ_CHECK_ARG(head, "%s: null head", what);
    MQ_CHECK_ARG(cfg->pool == MQ_POOL_MEAN || cfg->pool == MQ_POOL_CLS, "%s: bad pooling %d (MQ_POOL_MEAN or MQ_POOL_CLS)", what, cfg->pool);
    const int W = cfg->width;
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= 64 * TAIL_LN_MAXJ, "%s: W=%d must be a multiple of 64, at most %d", what, W, 64 * TAIL_LN_MAXJ);
    MQ_CHECK_ARG(head->dense_w && head->norm_g && head->cls_w, "%s: null weight pointer (dense_w / norm_g / cls_w)", what);
    MQ_CHECK_ARG(head->ln_eps >= 0.f, "%s: ln_eps=%g must not be negative", what, (double)head->ln_eps);
    MQ_CHECK_ARG(nseq >= 1 && nseq < (1ll << 31), "%s: nseq=%lld must be in [1, 2^31)", what, (long long)nseq);
    MQ_CHECK_ARG(d_logits, "%s: null output", what);
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin(what, d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const PairsMbPlan p = pairs_mb_plan(cfg, rows, nseq);
    MQ_TRY(packed_workspace(what, workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* pooled = (float*)(base + p.off_pooled);
    MQ_TRY(mq_encode_modernbert(cfg, w, d_ids, d_cu_seqlens, h_cu_seqlens, nseq, pooled, 0, base + p.off_enc, p.enc_bytes, stream));
    if (d_pooled) MQ_CHECK_HIP(hipMemcpyAsync(d_pooled, pooled, (size_t)nseq * W * 4, hipMemcpyDeviceToDevice, s));
    return mq_score_head_ln(pooled, nseq, W, head, d_logits, d_scores, base + p.off_head, workspace_bytes - p.off_head, stream);
}

// ---- DeBERTa-v2 / -v3 cross-encoders ---------------------------------------------------------------------------------------------------------
namespace {
struct PairsDebPlan { size_t off_enc, enc_bytes, off_pooled, off_head, total; };
// [ mq_deberta_workspace_bytes: the encoder's own scratch ] [ CLS rows fp32 [nseq, W] ] [ head scratch ]
PairsDebPlan pairs_deb_plan(const mq_deberta_cfg* cfg, int64_t rows, int64_t nseq) {
    PairsDebPlan p;
    Off ws;
    p.enc_bytes = mq_deberta_workspace_bytes(cfg, rows, nseq);
    p.off_enc = ws.take(p.enc_bytes);
    p.off_pooled = ws.take((size_t)nseq * cfg->width * 4);
    p.off_head = ws.take(head_plan(nseq, cfg->width).total);
    p.total = ws.end();
    return p;
}
}  // namespace

extern "C" size_t mq_score_pairs_deberta_workspace_bytes(const mq_deberta_cfg* cfg, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0 || cfg->width <= 0) return 0;
    return pairs_deb_plan(cfg, rows, nseq).total;
}

// The encoder IS mq_encode_deberta (normalize = 0, CLS pooling) writing into this call's pooled slot; what it refuses it refuses here, under its own name.
extern "C" int mq_score_pairs_deberta(const mq_deberta_cfg* cfg, const mq_deberta_weights* w, const mq_score_head_weights* head, const int32_t* d_ids,
                                      const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq, float* d_logits, float* d_scores,
                                      float* d_pooled, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* what = "mq_score_pairs_deberta";
    MQ_CHECK_ARG(cfg && w, "%s: null cfg / weights", what);
    MQ_CHECK_ARG(head, "%s: null head", what);
    MQ_CHECK_ARG(cfg->pool == MQ_POOL_CLS, "%s: bad pooling %d (MQ_POOL_CLS: the ContextPooler reads the first row)", what, cfg->pool);
    const int W = cfg->width;
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= 64 * 4 * MAXC, "%s: W=%d must be a multiple of 64, at most %d", what, W, 64 * 4 * MAXC);
    MQ_CHECK_ARG(head->pooler_w && head->pooler_b && head->cls_w, "%s: null weight pointer (pooler_w / pooler_b / cls_w)", what);
    MQ_CHECK_ARG(nseq >= 1 && nseq < (1ll << 31), "%s: nseq=%lld must be in [1, 2^31)", what, (long long)nseq);
    MQ_CHECK_ARG(d_logits, "%s: null output", what);
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin(what, d_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const PairsDebPlan p = pairs_deb_plan(cfg, rows, nseq);
    MQ_TRY(packed_workspace(what, workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* pooled = (float*)(base + p.off_pooled);
    MQ_TRY(mq_encode_deberta(cfg, w, d_ids, d_cu_seqlens, h_cu_seqlens, nseq, pooled, 0, base + p.off_enc, p.enc_bytes, stream));
    if (d_pooled) MQ_CHECK_HIP(hipMemcpyAsync(d_pooled, pooled, (size_t)nseq * W * 4, hipMemcpyDeviceToDevice, s));
    return mq_score_head_gelu(pooled, nseq, W, head, d_logits, d_scores, base + p.off_head, workspace_bytes - p.off_head, stream);
}
