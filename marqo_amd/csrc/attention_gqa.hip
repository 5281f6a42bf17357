// Grouped-query attention of the decoder-style embedders (Qwen3-Embedding, gte-Qwen2: transformers Qwen3Model / Qwen2Model): q_heads query heads read
// kv_heads K/V heads, query head h reads K/V head h / G with G = q_heads / kv_heads (transformers' repeat_kv: consecutive query heads share), causal or
// unmasked, bf16, 64- or 128-wide heads, packed or fixed-length sequences.
//
// The tile math is attention_core.h's (chunks swizzled by key & (NC - 1)), the work split attention_gqa_core.h's; this file's three kernels choose:
//
//   - A sequence's queries are split into SLICES of 128 (eight 16-query blocks).  One workgroup (8 wave64s) per (sequence, K/V head, slice): it stages
//     that head's K and V ONCE for all G query heads that read it — expanding K/V to q_heads and running mq_attention would stage them G times.
//   - The work items, G x 8 of them for a full slice, count their block from the slice's far end on odd heads so that under the causal mask no wave
//     keeps the longest blocks.
//   - MQ_MASK_CAUSAL: a 16-query block visits only the key tiles whose first key is <= its last query, and the slice stages only the keys up to its last
//     query — slice s of a long sequence stages 128 (s + 1) keys, not the sequence.
//   - What the slice needs goes through the LDS in pieces of kpad keys when it is more than the LDS holds (320 keys at 256-byte rows, 640 at 128-byte
//     rows), re-staged for every round of work items, as attention.hip does it.
//
// Compiler report for gfx950 (-Rpass-analysis=kernel-resource-usage), VGPRs / waves per SIMD, 0 AGPRs and no scratch throughout: plain causal 69 / 7
// (64-wide heads) and 106 / 4 (128), plain unmasked 67 / 7 and 106 / 4, prefix 79 / 6 and 112 / 4, window 78 / 6 and 120 / 4.  (As separate copies of
// the body, before attention_gqa_core.h: 75 / 6 and 118 / 4, 73 / 6 and 118 / 4, 90 / 5 and 124 / 4, 78 / 6 and 120 / 4.)
#include "attention_gqa_core.h"

namespace {

constexpr int GQA_NW = 8;        // wave64s per workgroup
constexpr int GQA_SLICE = 128;   // queries per workgroup: a multiple of 64, so a slice starts on a key-tile boundary
constexpr size_t GQA_LDS = 160 * 1024;   // the most dynamic LDS a kernel here asks for: 640 keys of K + V at 128-byte rows, 320 at 256-byte rows
using GqaSlice = AttnSliceFixed<GQA_SLICE, true>;

// Plain causal is NOT the prefix kernel at P = 0: the second staging source and mask form cost that kernel 10 registers and a wave per SIMD at 64-wide heads
// (79 / 6 against 69 / 7)
template <int MASK, int HD>
__global__ __launch_bounds__(GQA_NW * 64) void attention_gqa_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                    int fixed_len, int q_heads, int kv_heads, int nslices, int kpad, float scale_log2e) {
    attn_gqa_body<HD, HD / 8 - 1, GQA_NW>(qkv, out, cu, fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e,
                                          AttnGqaPolicy<GqaSlice, AttnKeysPlain<MASK>>{});
}

// ---- prefix-sharing causal form (the decoder rerankers: one system prompt + instruction + query in front of every document of a search) --------------
// Rows [0, P) of the buffer are the shared prefix, the segments follow (cu[0] = P).  The query at local position t of a segment sees the P prefix keys
// and its own segment's keys 0 .. t: the VIRTUAL key tiles of AttnKeysPrefix.  With P = 0 there is no prefix tile and every statement reduces to
// attention_gqa_kernel<MQ_MASK_CAUSAL>'s, in its order (bit-identical output).
template <int HD>
__global__ __launch_bounds__(GQA_NW * 64) void attention_gqa_prefix_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                           int fixed_len, int q_heads, int kv_heads, int nslices, int kpad, float scale_log2e,
                                                                           int P) {
    attn_gqa_body<HD, HD / 8 - 1, GQA_NW>(qkv, out, cu, fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e,
                                          AttnGqaPolicy<GqaSlice, AttnKeysPrefix>{{}, {P}});
}

// ---- causal sliding-window form (Mistral-7B-v0.1's sliding_window: transformers masking_utils, sliding_window_overlay AND causal_mask_function) -------
// The query at position i of a sequence sees the keys j with i - window < j <= i.  What differs from the causal form is the LOWER end of what a slice
// stages and a block walks (AttnKeysCausalWindow):
//
//   - the slice [q0, q_last] stages the key tiles [st0, skt): st0 = the tile of key max(0, q0 - window + 1), skt as under the causal mask — at most
//     2 + ceil((window - 1) / 64) tiles, which is what the entry point sizes kpad by, so a long sequence costs O(T window), not O(T^2);
//   - a 16-query block visits the tiles [kt_begin, kt_end): kt_begin = the tile of key max(0, qb0 - window + 1), kt_end as under the causal mask;
//   - the tiles that cut the band — above (the diagonal), below (the first tile or two of the block), the ragged last — are masked per key.
//
// The tiles of a block that lie below the band of its LATER queries give those queries no key: attn_softmax_step keeps m_run = -1e30 for them, their
// probabilities are exp2(-inf) = 0, and the first tile with a key rescales the empty accumulators by exp2(-huge) = 0.  With window >= len: st0 = 0 and
// kt_begin = 0, and every statement reduces to attention_gqa_kernel<MQ_MASK_CAUSAL>'s, in its order (bit-identical output).
template <int HD>
__global__ __launch_bounds__(GQA_NW * 64) void attention_gqa_window_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                           int fixed_len, int q_heads, int kv_heads, int nslices, int kpad, float scale_log2e,
                                                                           int window) {
    attn_gqa_body<HD, HD / 8 - 1, GQA_NW>(qkv, out, cu, fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e,
                                          AttnGqaPolicy<GqaSlice, AttnKeysCausalWindow>{{}, {window}});
}

}  // namespace

// d_qkv bf16 [rows, (q_heads + 2 kv_heads) head_dim] = (q | k | v), head h of each part at columns h head_dim ..; d_out bf16 [rows, q_heads head_dim];
// sequences packed (d_cu_seqlens int32 [nseq + 1]; max_len = the longest) or fixed_len > 0 (d_cu_seqlens NULL ok).
extern "C" int mq_attention_gqa(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len,
                                int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t mask, void* stream) {
    ATTN_ARG_PTRS("mq_attention_gqa", d_qkv, d_out);
    MQ_CHECK_ARG(head_dim == 64 || head_dim == 128, "mq_attention_gqa: head_dim %d unsupported (64 or 128)", head_dim);
    ATTN_ARG_GROUPS("mq_attention_gqa", q_heads, kv_heads);
    MQ_CHECK_ARG(mask == MQ_MASK_NONE || mask == MQ_MASK_CAUSAL, "mq_attention_gqa: mask %d unsupported (MQ_MASK_NONE or MQ_MASK_CAUSAL)", mask);
    ATTN_ARG_SEQS("mq_attention_gqa", fixed_len, d_cu_seqlens);
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    ATTN_ARG_MAXL("mq_attention_gqa", maxl);
    const int nslices = (maxl + GQA_SLICE - 1) / GQA_SLICE;
    ATTN_ARG_GRID("mq_attention_gqa", nseq * kv_heads * nslices);
    // K + V rows of head_dim bf16 each live in the CU's 160 KiB of LDS: 640 keys (head_dim 64) / 320 keys (128); what a slice needs beyond that streams
    const int kpad = attn_kpad(maxl, head_dim == 64 ? 640 : 320);
    const float scale_log2e = 1.44269504088896340736f / sqrtf((float)head_dim);   // 1 / sqrt(head dim) * log2(e)
    hipStream_t s = (hipStream_t)stream;
    if (head_dim == 64)
        return mask == MQ_MASK_CAUSAL ? attn_gqa_launch<attention_gqa_kernel<MQ_MASK_CAUSAL, 64>, 64, GQA_NW>("mq_attention_gqa", GQA_LDS, d_qkv, d_out, d_cu_seqlens, nseq,
                                                                                                              fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e, s)
                                      : attn_gqa_launch<attention_gqa_kernel<MQ_MASK_NONE, 64>, 64, GQA_NW>("mq_attention_gqa", GQA_LDS, d_qkv, d_out, d_cu_seqlens, nseq,
                                                                                                            fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e, s);
    return mask == MQ_MASK_CAUSAL ? attn_gqa_launch<attention_gqa_kernel<MQ_MASK_CAUSAL, 128>, 128, GQA_NW>("mq_attention_gqa", GQA_LDS, d_qkv, d_out, d_cu_seqlens, nseq,
                                                                                                            fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e, s)
                                  : attn_gqa_launch<attention_gqa_kernel<MQ_MASK_NONE, 128>, 128, GQA_NW>("mq_attention_gqa", GQA_LDS, d_qkv, d_out, d_cu_seqlens, nseq,
                                                                                                          fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e, s);
}

// The prefix-sharing causal form: rows [0, prefix_len) of d_qkv are the shared prefix, the nseq segments follow (d_cu_seqlens int32 [nseq + 1],
// d_cu_seqlens[0] = prefix_len; max_len = the longest segment).  Only the segments' rows of d_out are written.
extern "C" int mq_attention_gqa_prefix(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t prefix_len, int32_t max_len,
                                       int32_t q_heads, int32_t kv_heads, int32_t head_dim, void* stream) {
    ATTN_ARG_PTRS("mq_attention_gqa_prefix", d_qkv, d_out);
    MQ_CHECK_ARG(head_dim == 64 || head_dim == 128, "mq_attention_gqa_prefix: head_dim %d unsupported (64 or 128)", head_dim);
    ATTN_ARG_GROUPS("mq_attention_gqa_prefix", q_heads, kv_heads);
    MQ_CHECK_ARG(d_cu_seqlens, "mq_attention_gqa_prefix: need cu_seqlens (cu_seqlens[0] = prefix_len)");
    MQ_CHECK_ARG(prefix_len >= 0 && prefix_len < 8192, "mq_attention_gqa_prefix: prefix_len %d unsupported (0..8191)", prefix_len);
    if (nseq <= 0) return MQ_OK;
    ATTN_ARG_MAXL("mq_attention_gqa_prefix", max_len);
    MQ_CHECK_ARG(prefix_len + max_len <= 8192, "mq_attention_gqa_prefix: prefix_len %d + max segment length %d exceeds 8192", prefix_len, max_len);
    const int nslices = (max_len + GQA_SLICE - 1) / GQA_SLICE;
    ATTN_ARG_GRID("mq_attention_gqa_prefix", nseq * kv_heads * nslices);
    // the virtual key space: the prefix in whole tiles, then the longest segment in whole tiles (with prefix_len = 0: mq_attention_gqa's kpad)
    const int kpad = attn_kpad(((prefix_len + 63) / 64) * 64 + max_len, head_dim == 64 ? 640 : 320);
    const float scale_log2e = 1.44269504088896340736f / sqrtf((float)head_dim);
    hipStream_t s = (hipStream_t)stream;
    // (fixed_len 0: the segments are always packed)
    return head_dim == 64 ? attn_gqa_launch<attention_gqa_prefix_kernel<64>, 64, GQA_NW>("mq_attention_gqa_prefix", GQA_LDS, d_qkv, d_out, d_cu_seqlens, nseq, 0,
                                                                                          q_heads, kv_heads, nslices, kpad, scale_log2e, s, (int)prefix_len)
                          : attn_gqa_launch<attention_gqa_prefix_kernel<128>, 128, GQA_NW>("mq_attention_gqa_prefix", GQA_LDS, d_qkv, d_out, d_cu_seqlens, nseq, 0,
                                                                                            q_heads, kv_heads, nslices, kpad, scale_log2e, s, (int)prefix_len);
}

// The causal sliding-window form: mq_attention_gqa's layout and sequence arguments; query i of a sequence sees the keys j with i - window < j <= i.
// window >= the longest sequence: the bits of mq_attention_gqa with MQ_MASK_CAUSAL.
extern "C" int mq_attention_gqa_window(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len,
                                       int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t window, void* stream) {
    ATTN_ARG_PTRS("mq_attention_gqa_window", d_qkv, d_out);
    MQ_CHECK_ARG(head_dim == 64 || head_dim == 128, "mq_attention_gqa_window: head_dim %d unsupported (64 or 128)", head_dim);
    ATTN_ARG_GROUPS("mq_attention_gqa_window", q_heads, kv_heads);
    MQ_CHECK_ARG(window >= 1, "mq_attention_gqa_window: window %d must be at least 1 (a query sees itself)", window);
    ATTN_ARG_SEQS("mq_attention_gqa_window", fixed_len, d_cu_seqlens);
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    ATTN_ARG_MAXL("mq_attention_gqa_window", maxl);
    const int nslices = (maxl + GQA_SLICE - 1) / GQA_SLICE;
    ATTN_ARG_GRID("mq_attention_gqa_window", nseq * kv_heads * nslices);
    // (a window past the longest sequence cuts nothing: clamped, the kernel's position arithmetic stays far inside int32)
    const int w = window < maxl ? window : maxl;
    // a slice's band spans at most 2 + ceil((w - 1) / 64) key tiles (its own two and what the window reaches below them), never more than the sequence
    const int band = (2 + (w - 1 + 63) / 64) * 64;
    const int kpad = attn_kpad(band < maxl ? band : maxl, head_dim == 64 ? 640 : 320);
    const float scale_log2e = 1.44269504088896340736f / sqrtf((float)head_dim);
    hipStream_t s = (hipStream_t)stream;
    return head_dim == 64 ? attn_gqa_launch<attention_gqa_window_kernel<64>, 64, GQA_NW>("mq_attention_gqa_window", GQA_LDS, d_qkv, d_out, d_cu_seqlens, nseq,
                                                                                          fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e, s, w)
                          : attn_gqa_launch<attention_gqa_window_kernel<128>, 128, GQA_NW>("mq_attention_gqa_window", GQA_LDS, d_qkv, d_out, d_cu_seqlens, nseq,
                                                                                            fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e, s, w);
}
