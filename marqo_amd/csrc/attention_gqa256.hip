// Grouped-query BAND attention at 256-wide heads (EmbeddingGemma: transformers Gemma3TextModel with use_bidirectional_attention): q_heads query heads read
// kv_heads K/V heads, query head h reads K/V head h / G with G = q_heads / kv_heads; bidirectional, never causal; query i sees the keys j of its own
// sequence with |i - j| <= half_window (half_window == 0: every key); bf16; packed or fixed-length sequences; the softmax scale is an argument.
//
// The tile math is attention_core.h's.  What a 512-byte row changes:
//
//   - A row has 32 chunk slots (two 256-B bank rows).  Chunk c of key k lives in slot c ^ (k & 15) — the 16-slot swizzle of the 128-wide heads, which
//     leaves the row's half (slot bit 4) alone: the 16 keys of a K fragment read land on 16 different slots of the bank row, and because a fragment's
//     keys differ from the tile's first by a multiple of 16 plus the lane's own offset, the swizzled chunk offsets are 8 (K) + 16 (V) per-lane constants
//     of the whole kernel.  (With k & 31 they are 96, and the compiler spilled 63 of them to scratch.)  One LDS-DMA of 1 KiB carries 2 rows.
//   - A 64-key tile of K plus V is 64 KiB, so the 160 KiB of LDS hold two tiles: a PIECE is at most 128 keys (128 KiB).  A band of half_window 256
//     over a 64-query slice reaches nine tiles, so K and V always stream through the LDS in pieces, re-staged for every round of work items.
//
// Work split:
//   - A sequence's queries are split into SLICES of 64 (four 16-query blocks; a slice starts on a key-tile boundary).  One workgroup of 8 wave64s per
//     (sequence, K/V head, slice) stages that head's tiles ONCE per round for all G query heads that read it, and only the 64-key tiles the slice's band
//     reaches: tiles floor((q0 - hw) / 64) .. floor((q_last + hw) / 64), clipped to the sequence.
//   - The work items are the (query head of the group, 16-query block of the slice) pairs, 4 G for a full slice; wave w takes items w, w + 8, ...
//     (G = 3: 12 items, two rounds).  A block visits only the tiles that cut ITS band, floor((qb0 - hw) / 64) .. floor((qb0 + 15 + hw) / 64).
//   - A tile inside the band of all 16 queries and inside the sequence takes the unmasked path; a tile cut by the band's edge or by the end of the
//     sequence masks per key.
//
// Registers per wave: 16 output tiles = 64 fp32 accumulators, 8 Q fragments = 32, one S^T tile = 16.  Compiler report for gfx950
// (-Rpass-analysis=kernel-resource-usage): 212 VGPRs, 0 AGPRs, 68 SGPRs, scratch 0 bytes / lane, no spill, no static LDS (dynamic: 64 KiB or 128 KiB
// per workgroup), 2 waves per SIMD — one 8-wave workgroup per CU, which is also what a two-tile piece of LDS admits.  Four waves per workgroup would
// allow 512 registers but take three rounds (three re-stagings of the band) for the checkpoint's G = 3 where eight take two.
//
// This kernel KEEPS ITS OWN BODY of the work split that its four siblings share (attention_gqa_core.h's attn_gqa_body; it would be that body with
// 64-query slices dealt forward, no reversed block order and a band key space).  Tried: on the shared body the bits were the parent's and the compiler
// reported 212 VGPRs / 2 waves per SIMD again (254 until the block's end tile was clipped to the slice's per piece, as below), but a differently
// scheduled stream, and 16 sequences of 512 tokens at (3, 1) heads measured 85.7 µs [85.5 – 87.4] against 81.2 µs [80.8 – 84.9] here at half_window 256,
// 87.0 µs against 82.6 µs at 0 (MI355X, interleaved medians of 15 launches, 7 repeats): 5 % slower, outside the spread.
#include "attention_core.h"

namespace {

constexpr int G256_NW = 8;           // wave64s per workgroup
constexpr int G256_SLICE = 64;       // queries per workgroup: one 64-key tile's worth, so a slice starts on a tile boundary
constexpr int G256_PIECE_KEYS = 128; // keys of K + V the LDS holds at 512-byte rows: 128 KiB of the 160 KiB
constexpr int G256_HD = 256;

__global__ __launch_bounds__(G256_NW * 64) void attention_gqa256_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                        int fixed_len, int q_heads, int kv_heads, int nslices, int kpad, int hw,
                                                                        float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int HD = G256_HD;
    constexpr int RB = HD * 2;       // 512 bytes per K / V row in LDS
    constexpr int NC = HD / 8;       // 32 16-byte chunk slots per LDS row
    constexpr int NKK = HD / 32;     // 8 32-deep MFMA k-chunks of a Q.K dot product
    constexpr int NDT = HD / 16;     // 16 16-wide output-dim tiles
    constexpr int SWZ = 15;          // chunk c of key k lives in slot c ^ (k & 15): the swizzle stays inside one 256-B half of the row
    char* sK = smem;                      // [kpad][RB], 16-B chunks XOR-swizzled by (key & 15)
    char* sV = smem + (size_t)kpad * RB;  // [kpad][RB], same image

    const unsigned sk = blockIdx.x / (unsigned)nslices;
    const int slice = (int)(blockIdx.x - sk * (unsigned)nslices);
    const int seq = sk / kv_heads, kvh = sk - seq * kv_heads;
    int row0, len;
    if (fixed_len > 0) { row0 = seq * fixed_len; len = fixed_len; }
    else { row0 = cu[seq]; len = cu[seq + 1] - row0; }
    const int q0 = slice * G256_SLICE;
    if (len <= 0 || q0 >= len) return;     // (the whole workgroup: no barrier has been reached)
    const int G = q_heads / kv_heads;
    const int ld = (q_heads + 2 * kv_heads) * HD, ldo = q_heads * HD;
    const bf16_t* qrow = qkv + (int64_t)row0 * ld;
    const bf16_t* kb = qrow + (q_heads + kvh) * HD;
    const bf16_t* vb = kb + kv_heads * HD;
    const int nkt = (len + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // key tiles [kt_lo, kt_hi) the slice's band reaches (hw is >= len when there is no band); they pass through the LDS in nchunks pieces of tpc tiles
    const int q_last = q0 + G256_SLICE - 1 < len - 1 ? q0 + G256_SLICE - 1 : len - 1;
    const int nblk = ((q_last - q0) >> 4) + 1;
    const int kt_lo = (q0 - hw > 0 ? q0 - hw : 0) >> 6;
    const int kt_hi = (((q_last + hw) >> 6) < nkt - 1 ? ((q_last + hw) >> 6) : nkt - 1) + 1;
    const int tpc = kpad >> 6;
    const int nchunks = (kt_hi - kt_lo + tpc - 1) / tpc;
    const int nitems = G * nblk;
    const int nrounds = (nitems + G256_NW - 1) / G256_NW;
    auto stage = [&](int c) {
        const int tiles_here = kt_hi - (kt_lo + c * tpc) < tpc ? kt_hi - (kt_lo + c * tpc) : tpc;
        attn_stage_piece<RB, NC, SWZ, G256_NW>(sK, sV, kb, vb, ld, (kt_lo + c * tpc) << 6, tiles_here << 6, len, lane, wave);
    };
    if (nchunks == 1) {
        stage(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    const int l15 = lane & 15, g = lane >> 4;
    const int vkey = 4 * g + (l15 >> 2);     // per-lane constants of the V^T transpose reads
    const int vcol = (l15 & 3) >> 1, vhalf = (l15 & 1) << 3;

    for (int rnd = 0; rnd < nrounds; ++rnd) {
        const int item = rnd * G256_NW + wave;
        const bool active = item < nitems;       // wave-uniform; with nchunks > 1 an idle wave still stages and keeps the barriers
        if (nchunks == 1 && !active) break;
        const int gh = active ? item / nblk : 0;
        const int blk = active ? item - gh * nblk : 0;
        const int h = kvh * G + gh;              // repeat_kv: K/V head kvh serves query heads kvh G .. kvh G + G - 1
        const int qb0 = q0 + blk * 16;
        const int q = qb0 + l15;                 // this lane's query (B-operand column / output row)
        bf16x8 qf[NKK];
        {
            const int qr = q < len ? q : len - 1;
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) qf[kk] = *(const bf16x8*)(qrow + (int64_t)qr * ld + h * HD + 8 * g + 32 * kk);
        }
        // the block's own band, in tiles
        const int ql = qb0 + 15 < len - 1 ? qb0 + 15 : len - 1;
        const int bk_lo = (qb0 - hw > 0 ? qb0 - hw : 0) >> 6;
        const int bk_hi = (((ql + hw) >> 6) < nkt - 1 ? ((ql + hw) >> 6) : nkt - 1) + 1;

        float m_run = -1e30f, l_run = 0.f;
        f32x4 o[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int c = 0; c < nchunks; ++c) {
            if (nchunks > 1) {   // (re)fill the LDS with the next piece of the slice's band
                __syncthreads();
                stage(c);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
            const int ct0 = kt_lo + c * tpc;
            const int ct1 = ct0 + tpc < kt_hi ? ct0 + tpc : kt_hi;
            const int t0 = bk_lo > ct0 ? bk_lo : ct0;
            const int t1 = !active ? t0 : (bk_hi < ct1 ? bk_hi : ct1);
            const int cb = ct0 << 6;                         // LDS row of global key `key` is key - cb (cb is a multiple of 64)
            for (int kt = t0; kt < t1; ++kt) {
                f32x4 sc[4];
                attn_score_tile<RB, NKK, SWZ>(sK, kt, cb, l15, g, qf, sc);
                attn_mask_band(sc, kt, g, q, qb0, hw, len);
                attn_softmax_step<NDT>(sc, m_run, l_run, o, scale_log2e);
                attn_pv_tile<RB, NDT, SWZ>(sV, kt, cb, vkey, vcol, vhalf, sc, o);
            }
        }  // pieces
        if (!active) continue;
        const float inv = attn_inv_denominator(l_run);
        if (q < len) attn_store_bf16<NDT>(out + (int64_t)(row0 + q) * ldo + h * HD + 4 * g, o, inv);
    }
}

}  // namespace

// d_qkv bf16 [rows, (q_heads + 2 kv_heads) 256] = (q | k | v), head h of each part at columns 256 h ..; d_out bf16 [rows, 256 q_heads]; sequences packed
// (d_cu_seqlens int32 [nseq + 1]; max_len = the longest) or fixed_len > 0 (d_cu_seqlens NULL ok).  half_window == 0: every key of the sequence;
// half_window > 0: query i sees keys i - half_window .. i + half_window.  scale: the softmax scale (query_pre_attn_scalar ** -0.5), > 0.
extern "C" int mq_attention_gqa_band(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len,
                                     int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t half_window, float scale, void* stream) {
    ATTN_ARG_PTRS("mq_attention_gqa_band", d_qkv, d_out);
    MQ_CHECK_ARG(head_dim == G256_HD, "mq_attention_gqa_band: head_dim %d unsupported (256; mq_attention_gqa serves 64 and 128)", head_dim);
    ATTN_ARG_GROUPS("mq_attention_gqa_band", q_heads, kv_heads);
    MQ_CHECK_ARG(half_window >= 0, "mq_attention_gqa_band: half_window %d < 0", half_window);
    MQ_CHECK_ARG(scale > 0.f && scale <= 1e6f, "mq_attention_gqa_band: softmax scale %g must be positive and finite", (double)scale);
    ATTN_ARG_SEQS("mq_attention_gqa_band", fixed_len, d_cu_seqlens);
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    ATTN_ARG_MAXL("mq_attention_gqa_band", maxl);
    const int nslices = (maxl + G256_SLICE - 1) / G256_SLICE;
    ATTN_ARG_GRID("mq_attention_gqa_band", nseq * kv_heads * nslices);
    // no band, or one that covers every sequence whole: every key (the kernel's tile and mask arithmetic runs on hw >= the longest sequence; a slice then
    // reaches more tiles than any sequence has).  The LDS holds two tiles
    const int hw = (half_window == 0 || half_window >= maxl - 1) ? 16384 : half_window;
    const int kpad = attn_band_kpad(hw, maxl, G256_PIECE_KEYS);
    const size_t lds = (size_t)kpad * G256_HD * 4;
    hipStream_t s = (hipStream_t)stream;
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)attention_gqa256_kernel, lds, (size_t)G256_PIECE_KEYS * G256_HD * 4, done, "mq_attention_gqa_band");
    if (rc != MQ_OK) return rc;
    MqProfScope prof(2, s);
    const float scale_log2e = 1.44269504088896340736f * scale;
    hipLaunchKernelGGL(attention_gqa256_kernel, dim3((unsigned)(nseq * kv_heads * nslices)), dim3(G256_NW * 64), lds, s, (const bf16_t*)d_qkv,
                       (bf16_t*)d_out, d_cu_seqlens, (int)fixed_len, (int)q_heads, (int)kv_heads, nslices, kpad, hw, scale_log2e);
    MQ_CHECK_LAUNCH("mq_attention_gqa_band");
    return MQ_OK;
}
