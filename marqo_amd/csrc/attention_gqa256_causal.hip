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
// Key space.  A slice stages and a block walks VIRTUAL key tiles, as attention_gqa_prefix_kernel does:
//   tiles [0, npt), npt = ceil(P / 64)   the prefix keys (rows 0 .. P - 1); the last one is partial when P % 64 != 0: its keys >= P are masked
//   tiles npt ..                         the segment's own keys, own key j at virtual key 64 npt + j: a FRESH tile, no tile straddles the two ranges
// so P need not be a multiple of 64: the segment's first key tile starts on a tile boundary of the LDS image whatever P is, a virtual key and its LDS row
// agree modulo 64, and the swizzle holds unchanged.  The price is one more partly empty tile per block when P % 64 != 0.
//
// Work split:
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
// (-Rpass-analysis=kernel-resource-usage): 250 VGPRs, 0 AGPRs, 80 SGPRs, scratch 0 bytes / lane, no spill, no static LDS (dynamic: 64 KiB or 128 KiB
// per workgroup), 2 waves per SIMD — one 8-wave workgroup per CU, which is also what a two-tile piece of LDS admits.  (The two mask forms and the two
// staging sources cost 38 registers over the band kernel's 212; the unit is in _lib.NO_SCRATCH_UNITS, so a build that spills is refused.)
#include "attention_core.h"

namespace {

constexpr int C256_NW = 8;           // wave64s per workgroup
constexpr int C256_PIECE_KEYS = 128; // keys of K + V the LDS holds at 512-byte rows: 128 KiB of the 160 KiB
constexpr int C256_HD = 256;

__global__ __launch_bounds__(C256_NW * 64) void attention_gqa256_causal_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                               const int32_t* __restrict__ cu, int fixed_len, int P, int q_heads, int kv_heads,
                                                                               int nslices, int nb, int kpad, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int HD = C256_HD;
    constexpr int RB = HD * 2;       // 512 bytes per K / V row in LDS
    constexpr int NC = HD / 8;       // 32 16-byte chunk slots per LDS row
    constexpr int NKK = HD / 32;     // 8 32-deep MFMA k-chunks of a Q.K dot product
    constexpr int NDT = HD / 16;     // 16 16-wide output-dim tiles
    constexpr int SWZ = 15;          // chunk c of key k lives in slot c ^ (k & 15): the swizzle stays inside one 256-B half of the row
    char* sK = smem;                      // [kpad][RB]
    char* sV = smem + (size_t)kpad * RB;  // [kpad][RB], same image

    const unsigned sk = blockIdx.x / (unsigned)nslices;
    const int slice = nslices - 1 - (int)(blockIdx.x - sk * (unsigned)nslices);   // longest first
    const int seq = sk / kv_heads, kvh = sk - seq * kv_heads;
    int row0, len;
    if (fixed_len > 0) { row0 = seq * fixed_len; len = fixed_len; }
    else { row0 = cu[seq]; len = cu[seq + 1] - row0; }
    const int q0 = slice * nb * 16;
    if (len <= 0 || q0 >= len) return;     // (the whole workgroup: no barrier has been reached)
    const int G = q_heads / kv_heads;
    const int ld = (q_heads + 2 * kv_heads) * HD, ldo = q_heads * HD;
    const bf16_t* qrow = qkv + (int64_t)row0 * ld;
    const bf16_t* kb = qrow + (q_heads + kvh) * HD;      // the sequence's own keys / values
    const bf16_t* vb = kb + kv_heads * HD;
    const bf16_t* pkb = qkv + (q_heads + kvh) * HD;      // the prefix's: rows 0 .. P - 1 of the same buffer (never read when P = 0)
    const bf16_t* pvb = pkb + kv_heads * HD;
    const int npt = (P + 63) >> 6;
    const int nkt = (len + 63) >> 6;                     // own tiles of the sequence
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    const int q_last = q0 + nb * 16 - 1 < len - 1 ? q0 + nb * 16 - 1 : len - 1;
    const int nblk = ((q_last - q0) >> 4) + 1;
    const int skt = npt + (q_last >> 6) + 1;             // virtual tiles [0, skt) the slice stages
    const int tpc = kpad >> 6;
    const int nchunks = (skt + tpc - 1) / tpc;
    const int nitems = G * nblk;
    const int nrounds = (nitems + C256_NW - 1) / C256_NW;
    auto stage = [&](int c) {   // virtual tiles [t0, t1) -> LDS rows 0 ..: the prefix tiles among them, then the own tiles
        const int t0 = c * tpc, t1 = skt < t0 + tpc ? skt : t0 + tpc;
        const int pe = t1 < npt ? t1 : npt;              // one past the last prefix tile of the piece
        const int os = t0 > npt ? t0 : npt;              // its first own tile
        if (pe > t0) attn_stage_piece<RB, NC, SWZ, C256_NW>(sK, sV, pkb, pvb, ld, t0 << 6, (pe - t0) << 6, P, lane, wave);
        if (t1 > os) {
            const size_t off = (size_t)((os - t0) << 6) * RB;
            attn_stage_piece<RB, NC, SWZ, C256_NW>(sK + off, sV + off, kb, vb, ld, (os - npt) << 6, (t1 - os) << 6, len, lane, wave);
        }
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
        const int item = rnd * C256_NW + wave;
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

        float m_run = -1e30f, l_run = 0.f;
        f32x4 o[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

        const int last = npt + ((qb0 + 15) >> 6);        // the virtual tile of the block's last query: own tiles behind it start past every query
        const int kt_end = last + 1 < skt ? last + 1 : skt;
        for (int c = 0; c < nchunks; ++c) {
            if (nchunks > 1) {   // (re)fill the LDS with virtual tiles [c tpc, (c + 1) tpc) of the slice
                __syncthreads();
                stage(c);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
            const int kt0 = c * tpc;
            const int kt1 = !active ? kt0 : (kt_end < kt0 + tpc ? kt_end : kt0 + tpc);
            const int cb = kt0 << 6;                         // LDS row of virtual key `key` is key - cb (cb is a multiple of 64)
            for (int kt = kt0; kt < kt1; ++kt) {
                f32x4 sc[4];
                attn_score_tile<RB, NKK, SWZ>(sK, kt, cb, l15, g, qf, sc);
                if (kt < npt) attn_mask_causal<MQ_MASK_NONE>(sc, kt, npt, g, q, qb0, P);                     // prefix: only keys >= P of its partial last tile
                else attn_mask_causal<MQ_MASK_CAUSAL>(sc, kt - npt, nkt, g, q, qb0, len);                    // own: the diagonal tile, per key
                attn_softmax_step<NDT>(sc, m_run, l_run, o, scale_log2e);   // (first tile visited: prefix key 0 when P >= 1, else own key 0)
                attn_pv_tile<RB, NDT, SWZ>(sV, kt, cb, vkey, vcol, vhalf, sc, o);
            }
        }  // pieces
        if (!active) continue;
        const float inv = attn_inv_denominator(l_run);
        if (q < len) attn_store_bf16<NDT>(out + (int64_t)(row0 + q) * ldo + h * HD + 4 * g, o, inv);
    }
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
    const size_t lds = (size_t)kpad * C256_HD * 4;
    hipStream_t s = (hipStream_t)stream;
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)attention_gqa256_causal_kernel, lds, (size_t)C256_PIECE_KEYS * C256_HD * 4, done, fn);
    if (rc != MQ_OK) return rc;
    MqProfScope prof(2, s);
    const float scale_log2e = 1.44269504088896340736f * scale;
    hipLaunchKernelGGL(attention_gqa256_causal_kernel, dim3((unsigned)(nseq * kv_heads * nslices)), dim3(C256_NW * 64), lds, s, (const bf16_t*)d_qkv,
                       (bf16_t*)d_out, d_cu, fixed_len, P, q_heads, kv_heads, nslices, nb, kpad, scale_log2e);
    MQ_CHECK_LAUNCH(fn);
    return MQ_OK;
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
