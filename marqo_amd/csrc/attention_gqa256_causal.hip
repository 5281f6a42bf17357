// Grouped-query CAUSAL attention at 256-wide heads, plain and prefix-sharing (the Gemma-2B rerankers: transformers GemmaForCausalLM read as a judge,
// 8 query heads over ONE K/V head): q_heads query heads read kv_heads K/V heads, query head h reads K/V head h / G with G = q_heads / kv_heads; bf16;
// the softmax scale is an argument.  Two entry points on ONE kernel:
//
//   mq_attention_gqa256_causal   packed or fixed-length sequences; query i of a sequence sees keys 0 .. i of that sequence
//   mq_attention_gqa256_prefix   mq_attention_gqa_prefix's conventions: rows [0, P) of the buffer are a shared prefix, the segments follow (cu[0] = P);
//                                the query at local position t of a segment sees the P prefix keys and its own segment's keys 0 .. t
//
// The plain form is the prefix form with P = 0 (the kernel has no second code path for it), so the two give the same bits on the same packed batch.
//
// The tile math is attention_core.h's; the 512-byte row is attention_gqa256.hip's: 32 chunk slots, chunk c of key k in slot c ^ (k & 15) — the 16-slot
// swizzle that keeps the swizzled chunk offsets per-lane constants of the whole kernel (see that file's header: with k & 31 the compiler spilled).  A
// 64-key tile of K plus V is 64 KiB, the LDS holds two: a PIECE is at most 128 keys, and everything longer streams through the LDS in pieces.
//
// Key space.  A slice stages and a block walks VIRTUAL key tiles, as attention_gqa_prefix_kernel does (attention_gqa_core.h's AttnKeysPrefix):
//   tiles [0, npt), npt = ceil(P / 64)   the prefix keys (rows 0 .. P - 1); the last one is partial when P % 64 != 0: its keys >= P are masked
//   tiles npt ..                         the segment's own keys, own key j at virtual key 64 npt + j: a FRESH tile, no tile straddles the two ranges
// so P need not be a multiple of 64: the segment's first key tile starts on a tile boundary of the LDS image whatever P is, a virtual key and its LDS row
// agree modulo 64, and the swizzle holds unchanged.  The price is one more partly empty tile per block when P % 64 != 0.
//
// Work split (the body is attention_gqa_core.h's attn_gqa_body; this kernel's policy is AttnSliceBlocks{nb} and AttnKeysPrefix{P}):
//   - One workgroup of 8 wave64s per (sequence, K/V head, slice of nb 16-query blocks).  It stages that K/V head's tiles once per piece for ALL G query
//     heads that read it; K/V are never expanded to q_heads.
//   - It stages only the prefix tiles and the own tiles up to the slice's last query; a 16-query block visits only the prefix tiles and the own tiles
//     whose first key is <= its last query.
//   - Only the diagonal own tile (the one that reaches past the block's first query; the ragged last tile of a sequence is always some block's diagonal
//     tile) and the partial last prefix tile mask per key; every other tile takes the unmasked path (attn_mask_causal's wave-uniform test).
//   - The round structure.  The work items are the (query head of the group, block of the slice) pairs, G nb of them; wave w takes items w, w + 8, ...
//     A 64-query slice at G = 8 would be 32 items = four rounds, each re-staging every piece.  Instead the SLICE IS NARROWED until one round holds it:
//     nb = 8 / G blocks (G = 8: one 16-query block, the eight waves are its eight query heads; G = 3 or 4: two blocks; G = 2: four; G = 1: eight), so a
//     workgroup stages its pieces exactly once.  Per 64 queries that is the same staging volume as four rounds of a 64-query slice would be, but the eight
//     waves walk the SAME tiles in lockstep — under the causal mask no wave idles at a barrier while another works off a longer block —, a slice stages
//     only up to ITS last query, and a short document (the rerankers' segments are a few hundred tokens) becomes four times as many workgroups.  G > 8
//     (not a served shape) keeps nb = 1 and takes ceil(G / 8) rounds that re-stage, as the sibling kernels do.
//   - Slices are dealt longest first (blockIdx counts them from the sequence's end): the workgroups with the most tiles start first.
//   - Staging is synchronous (stage, wait, barrier, compute, barrier), as in the sibling files; the two tiles of LDS are one piece, not two buffers in
//     flight.  Overlapping the next piece with this one's MFMAs is left open.
//
// Registers per wave: 16 output tiles = 64 fp32 accumulators, 8 Q fragments = 32, one S^T tile = 16.  Compiler report for gfx950
// (-Rpass-analysis=kernel-resource-usage): 224 VGPRs, 0 AGPRs, 80 SGPRs, scratch 0 bytes / lane, no spill, no static LDS (dynamic: 64 KiB or 128 KiB
// per workgroup), 2 waves per SIMD — one 8-wave workgroup per CU, which is also what a two-tile piece of LDS admits.  (The two mask forms and the two
// staging sources cost 12 registers over the band kernel's 212; the unit is in _lib.NO_SCRATCH_UNITS, so a build that spills is refused.)
#include "attention_gqa_core.h"

namespace {

constexpr int C256_NW = 8;           // wave64s per workgroup
constexpr int C256_PIECE_KEYS = 128; // keys of K + V the LDS holds at 512-byte rows: 128 KiB of the 160 KiB
constexpr int C256_HD = 256;
constexpr int C256_SWZ = 15;         // chunk c of key k lives in slot c ^ (k & 15): the swizzle stays inside one 256-B half of the row

__global__ __launch_bounds__(C256_NW * 64) void attention_gqa256_causal_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                               const int32_t* __restrict__ cu, int fixed_len, int q_heads, int kv_heads,
                                                                               int nslices, int kpad, float scale_log2e, int nb, int P) {
    attn_gqa_body<C256_HD, C256_SWZ, C256_NW>(qkv, out, cu, fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e,
                                              AttnGqaPolicy<AttnSliceBlocks, AttnKeysPrefix>{{nb}, {P}});
}

// the checks both entry points make behind their own, and the launch.  maxl = the longest sequence / segment
int launch_gqa256_causal(const char* fn, const void* d_qkv, void* d_out, const int32_t* d_cu, int64_t nseq, int fixed_len, int P, int maxl, int q_heads,
                         int kv_heads, float scale, void* stream) {
    // blocks per slice: as many as one round of eight waves holds for this group size (the file header)
    const int G = q_heads / kv_heads;
    const int nb = G >= 8 ? 1 : 8 / G;
    const int nslices = (maxl + nb * 16 - 1) / (nb * 16);
    MQ_CHECK_ARG(nseq * kv_heads * nslices < (1LL << 31), "%s: grid too large", fn);
    // the virtual key space: the prefix in whole tiles, then the longest sequence in whole tiles; the LDS holds two tiles of it
    const int kpad = attn_kpad(((P + 63) / 64) * 64 + maxl, C256_PIECE_KEYS);
    return attn_gqa_launch<attention_gqa256_causal_kernel, C256_HD, C256_NW>(fn, (size_t)C256_PIECE_KEYS * C256_HD * 4, d_qkv, d_out, d_cu, nseq, fixed_len,
                                                                             q_heads, kv_heads, nslices, kpad, 1.44269504088896340736f * scale,
                                                                             (hipStream_t)stream, nb, P);
}

}  // namespace

// d_qkv bf16 [rows, (q_heads + 2 kv_heads) 256] = (q | k | v), head h of each part at columns 256 h ..; d_out bf16 [rows, 256 q_heads]; sequences packed
// (d_cu_seqlens int32 [nseq + 1]; max_len = the longest) or fixed_len > 0 (d_cu_seqlens NULL ok).  scale: the softmax scale, > 0.
extern "C" int mq_attention_gqa256_causal(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len,
                                          int32_t q_heads, int32_t kv_heads, int32_t head_dim, float scale, void* stream) {
    ATTN_ARG_PTRS("mq_attention_gqa256_causal", d_qkv, d_out);
    MQ_CHECK_ARG(head_dim == C256_HD, "mq_attention_gqa256_causal: head_dim %d unsupported (256; mq_attention_gqa serves 64 and 128)", head_dim);
    ATTN_ARG_GROUPS("mq_attention_gqa256_causal", q_heads, kv_heads);
    MQ_CHECK_ARG(scale > 0.f && scale <= 1e6f, "mq_attention_gqa256_causal: softmax scale %g must be positive and finite", (double)scale);
    ATTN_ARG_SEQS("mq_attention_gqa256_causal", fixed_len, d_cu_seqlens);
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    ATTN_ARG_MAXL("mq_attention_gqa256_causal", maxl);
    return launch_gqa256_causal("mq_attention_gqa256_causal", d_qkv, d_out, d_cu_seqlens, nseq, fixed_len > 0 ? fixed_len : 0, 0, maxl, q_heads, kv_heads,
                                scale, stream);
}

// The prefix-sharing form: rows [0, prefix_len) of d_qkv are the shared prefix, the nseq segments follow (d_cu_seqlens int32 [nseq + 1],
// d_cu_seqlens[0] = prefix_len; max_len = the longest segment).  Only the segments' rows of d_out are written.
extern "C" int mq_attention_gqa256_prefix(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t prefix_len, int32_t max_len,
                                          int32_t q_heads, int32_t kv_heads, int32_t head_dim, float scale, void* stream) {
    ATTN_ARG_PTRS("mq_attention_gqa256_prefix", d_qkv, d_out);
    MQ_CHECK_ARG(head_dim == C256_HD, "mq_attention_gqa256_prefix: head_dim %d unsupported (256; mq_attention_gqa_prefix serves 64 and 128)", head_dim);
    ATTN_ARG_GROUPS("mq_attention_gqa256_prefix", q_heads, kv_heads);
    MQ_CHECK_ARG(scale > 0.f && scale <= 1e6f, "mq_attention_gqa256_prefix: softmax scale %g must be positive and finite", (double)scale);
    MQ_CHECK_ARG(d_cu_seqlens, "mq_attention_gqa256_prefix: need cu_seqlens (cu_seqlens[0] = prefix_len)");
    MQ_CHECK_ARG(prefix_len >= 0 && prefix_len < 8192, "mq_attention_gqa256_prefix: prefix_len %d unsupported (0..8191)", prefix_len);
    if (nseq <= 0) return MQ_OK;
    ATTN_ARG_MAXL("mq_attention_gqa256_prefix", max_len);
    MQ_CHECK_ARG(prefix_len + max_len <= 8192, "mq_attention_gqa256_prefix: prefix_len %d + max segment length %d exceeds 8192", prefix_len, max_len);
    return launch_gqa256_causal("mq_attention_gqa256_prefix", d_qkv, d_out, d_cu_seqlens, nseq, 0, prefix_len, max_len, q_heads, kv_heads, scale, stream);
}
