// Grouped-query attention of the decoder-style embedders (Qwen3-Embedding, gte-Qwen2: transformers Qwen3Model / Qwen2Model): q_heads query heads read
// kv_heads K/V heads, query head h reads K/V head h / G with G = q_heads / kv_heads (transformers' repeat_kv: consecutive query heads share), causal or
// unmasked, bf16, 64- or 128-wide heads, packed or fixed-length sequences.
//
// The tile math is attention_core.h's (chunks swizzled by key & (NC - 1)); what is this file's own is the work split:
//
//   - A sequence's queries are split into SLICES of 128 (eight 16-query blocks).  One workgroup (8 wave64s) per (sequence, K/V head, slice): it stages
//     that head's K and V ONCE for all G query heads that read it — expanding K/V to q_heads and running mq_attention would stage them G times.
//   - The workgroup's work items are the (query head of the group, 16-query block of the slice) pairs, G x 8 of them for a full slice; wave w takes items
//     w, w + 8, ...  Item i is query head i / nblk and block i % nblk, counted from the slice's far end on odd heads so that under the causal mask no
//     wave keeps the longest blocks.
//   - MQ_MASK_CAUSAL: a 16-query block visits only the key tiles whose first key is <= its last query, and the slice stages only the keys up to its last
//     query — slice s of a long sequence stages 128 (s + 1) keys, not the sequence.
//   - What the slice needs goes through the LDS in pieces of kpad keys when it is more than the LDS holds (320 keys at 256-byte rows, 640 at 128-byte
//     rows), re-staged for every round of work items, as attention.hip does it.
#include "attention_core.h"

namespace {

constexpr int GQA_NW = 8;        // wave64s per workgroup
constexpr int GQA_SLICE = 128;   // queries per workgroup: a multiple of 64, so a slice starts on a key-tile boundary

template <int MASK, int HD>
__global__ __launch_bounds__(GQA_NW * 64) void attention_gqa_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                    int fixed_len, int q_heads, int kv_heads, int nslices, int kpad, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = HD * 2;       // bytes per K / V row in LDS (128 or 256)
    constexpr int NC = HD / 8;       // 16-byte chunk slots per LDS row (8 or 16)
    constexpr int NKK = HD / 32;     // 32-deep MFMA k-chunks of a Q.K dot product
    constexpr int NDT = HD / 16;     // 16-wide output-dim tiles
    char* sK = smem;                      // [kpad][RB], 16-B chunks XOR-swizzled by (key & (NC - 1))
    char* sV = smem + (size_t)kpad * RB;  // [kpad][RB], same image

    const unsigned sk = blockIdx.x / (unsigned)nslices;
    const int slice = (int)(blockIdx.x - sk * (unsigned)nslices);
    const int seq = sk / kv_heads, kvh = sk - seq * kv_heads;
    int row0, len;
    if (fixed_len > 0) { row0 = seq * fixed_len; len = fixed_len; }
    else { row0 = cu[seq]; len = cu[seq + 1] - row0; }
    const int q0 = slice * GQA_SLICE;
    if (len <= 0 || q0 >= len) return;     // (the whole workgroup: no barrier has been reached)
    const int G = q_heads / kv_heads;
    const int ld = (q_heads + 2 * kv_heads) * HD, ldo = q_heads * HD;
    const bf16_t* qrow = qkv + (int64_t)row0 * ld;
    const bf16_t* kb = qrow + (q_heads + kvh) * HD;
    const bf16_t* vb = kb + kv_heads * HD;
    const int nkt = (len + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // the slice: its 16-query blocks, the key tiles [0, skt) it stages (causal: up to its last query), the pieces they pass through the LDS in
    const int q_last = q0 + GQA_SLICE - 1 < len - 1 ? q0 + GQA_SLICE - 1 : len - 1;
    const int nblk = ((q_last - q0) >> 4) + 1;
    const int skt = MASK == MQ_MASK_CAUSAL ? (q_last >> 6) + 1 : nkt;
    const int tpc = kpad >> 6;
    const int nchunks = (skt + tpc - 1) / tpc;
    const int nitems = G * nblk;
    const int nrounds = (nitems + GQA_NW - 1) / GQA_NW;
    auto stage = [&](int c) {
        const int tiles_here = skt - c * tpc < tpc ? skt - c * tpc : tpc;
        attn_stage_piece<RB, NC, NC - 1, GQA_NW>(sK, sV, kb, vb, ld, (c * tpc) << 6, tiles_here << 6, len, lane, wave);
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
        const int item = rnd * GQA_NW + wave;
        const bool active = item < nitems;       // wave-uniform; with nchunks > 1 an idle wave still stages and keeps the barriers
        if (nchunks == 1 && !active) break;
        const int gh = active ? item / nblk : 0;
        int blk = active ? item - gh * nblk : 0;
        if (gh & 1) blk = nblk - 1 - blk;
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

        int kt_end = skt;                        // one past the last key tile this block visits
        if (MASK == MQ_MASK_CAUSAL) {
            const int last = (qb0 + 15) >> 6;    // the tile of the block's last query: tiles behind it start past every query of the block
            kt_end = last + 1 < skt ? last + 1 : skt;
        }
        for (int c = 0; c < nchunks; ++c) {
            if (nchunks > 1) {   // (re)fill the LDS with key tiles [c tpc, (c + 1) tpc) of the slice
                __syncthreads();
                stage(c);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
            const int kt0 = c * tpc;
            const int kt1 = !active ? kt0 : (kt_end < kt0 + tpc ? kt_end : kt0 + tpc);
            const int cb = kt0 << 6;                         // LDS row of global key `key` is key - cb (cb is a multiple of 64)
            for (int kt = kt0; kt < kt1; ++kt) {
                f32x4 sc[4];
                attn_score_tile<RB, NKK, NC - 1>(sK, kt, cb, l15, g, qf, sc);
                attn_mask_causal<MASK>(sc, kt, nkt, g, q, qb0, len);
                attn_softmax_step<NDT>(sc, m_run, l_run, o, scale_log2e);   // (every query sees at least key 0, in the first tile it visits)
                attn_pv_tile<RB, NDT, NC - 1>(sV, kt, cb, vkey, vcol, vhalf, sc, o);
            }
        }  // pieces
        if (!active) continue;
        const float inv = attn_inv_denominator(l_run);
        if (q < len) attn_store_bf16<NDT>(out + (int64_t)(row0 + q) * ldo + h * HD + 4 * g, o, inv);
    }
}

template <int MASK, int HD>
int launch_gqa(const void* d_qkv, void* d_out, const int32_t* d_cu, int64_t nseq, int fixed_len, int q_heads, int kv_heads, int nslices, int kpad,
               hipStream_t s) {
    const size_t lds = (size_t)kpad * HD * 4;
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)attention_gqa_kernel<MASK, HD>, lds, 160 * 1024, done, "mq_attention_gqa");
    if (rc != MQ_OK) return rc;
    const float scale_log2e = 1.44269504088896340736f / sqrtf((float)HD);   // 1 / sqrt(head dim) * log2(e)
    hipLaunchKernelGGL((attention_gqa_kernel<MASK, HD>), dim3((unsigned)(nseq * kv_heads * nslices)), dim3(GQA_NW * 64), lds, s, (const bf16_t*)d_qkv,
                       (bf16_t*)d_out, d_cu, fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e);
    return MQ_OK;
}

// ---- prefix-sharing causal form (the decoder rerankers: one system prompt + instruction + query in front of every document of a search) --------------
// Rows [0, P) of the buffer are the shared prefix, the segments follow (cu[0] = P).  The query at local position t of a segment sees the P prefix keys
// and its own segment's keys 0 .. t.  The work split is attention_gqa_kernel's; what differs is the key space a slice stages and a block walks — VIRTUAL
// key tiles:
//
//   tiles [0, npt), npt = ceil(P / 64)   the prefix keys (rows 0 .. P - 1); the last one is partial when P % 64 != 0: its keys >= P are masked
//   tiles npt ..                         the segment's own keys, own key j at virtual key 64 npt + j: a FRESH tile, no tile straddles the two ranges
//
// A virtual key and its LDS row agree modulo 64 (both ranges are staged from a tile boundary on), so the swizzle of attention_core.h holds unchanged.
// Prefix tiles come first: with P >= 1 the first tile a query visits holds prefix key 0, which it sees; with P = 0 there is no prefix tile and every
// statement below reduces to attention_gqa_kernel<MQ_MASK_CAUSAL>'s, in its order (bit-identical output).
template <int HD>
__global__ __launch_bounds__(GQA_NW * 64) void attention_gqa_prefix_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                           int P, int q_heads, int kv_heads, int nslices, int kpad, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = HD * 2;
    constexpr int NC = HD / 8;
    constexpr int NKK = HD / 32;
    constexpr int NDT = HD / 16;
    char* sK = smem;
    char* sV = smem + (size_t)kpad * RB;

    const unsigned sk = blockIdx.x / (unsigned)nslices;
    const int slice = (int)(blockIdx.x - sk * (unsigned)nslices);
    const int seq = sk / kv_heads, kvh = sk - seq * kv_heads;
    const int row0 = cu[seq], len = cu[seq + 1] - row0;
    const int q0 = slice * GQA_SLICE;
    if (len <= 0 || q0 >= len) return;     // (the whole workgroup: no barrier has been reached)
    const int G = q_heads / kv_heads;
    const int ld = (q_heads + 2 * kv_heads) * HD, ldo = q_heads * HD;
    const bf16_t* qrow = qkv + (int64_t)row0 * ld;
    const bf16_t* kb = qrow + (q_heads + kvh) * HD;      // the segment's own keys / values
    const bf16_t* vb = kb + kv_heads * HD;
    const bf16_t* pkb = qkv + (q_heads + kvh) * HD;      // the prefix's: rows 0 .. P - 1 of the same buffer
    const bf16_t* pvb = pkb + kv_heads * HD;
    const int npt = (P + 63) >> 6;
    const int nkt = (len + 63) >> 6;                     // own tiles of the segment
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    const int q_last = q0 + GQA_SLICE - 1 < len - 1 ? q0 + GQA_SLICE - 1 : len - 1;
    const int nblk = ((q_last - q0) >> 4) + 1;
    const int skt = npt + (q_last >> 6) + 1;             // virtual tiles [0, skt) the slice stages
    const int tpc = kpad >> 6;
    const int nchunks = (skt + tpc - 1) / tpc;
    const int nitems = G * nblk;
    const int nrounds = (nitems + GQA_NW - 1) / GQA_NW;
    auto stage = [&](int c) {   // virtual tiles [t0, t1) -> LDS rows 0 ..: the prefix tiles among them, then the own tiles
        const int t0 = c * tpc, t1 = skt < t0 + tpc ? skt : t0 + tpc;
        const int pe = t1 < npt ? t1 : npt;              // one past the last prefix tile of the piece
        const int os = t0 > npt ? t0 : npt;              // its first own tile
        if (pe > t0) attn_stage_piece<RB, NC, NC - 1, GQA_NW>(sK, sV, pkb, pvb, ld, t0 << 6, (pe - t0) << 6, P, lane, wave);
        if (t1 > os) {
            const size_t off = (size_t)((os - t0) << 6) * RB;
            attn_stage_piece<RB, NC, NC - 1, GQA_NW>(sK + off, sV + off, kb, vb, ld, (os - npt) << 6, (t1 - os) << 6, len, lane, wave);
        }
    };
    if (nchunks == 1) {
        stage(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    const int l15 = lane & 15, g = lane >> 4;
    const int vkey = 4 * g + (l15 >> 2);
    const int vcol = (l15 & 3) >> 1, vhalf = (l15 & 1) << 3;

    for (int rnd = 0; rnd < nrounds; ++rnd) {
        const int item = rnd * GQA_NW + wave;
        const bool active = item < nitems;       // wave-uniform; with nchunks > 1 an idle wave still stages and keeps the barriers
        if (nchunks == 1 && !active) break;
        const int gh = active ? item / nblk : 0;
        int blk = active ? item - gh * nblk : 0;
        if (gh & 1) blk = nblk - 1 - blk;
        const int h = kvh * G + gh;
        const int qb0 = q0 + blk * 16;
        const int q = qb0 + l15;
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

        const int last = npt + ((qb0 + 15) >> 6);        // the virtual tile of the block's last query
        const int kt_end = last + 1 < skt ? last + 1 : skt;
        for (int c = 0; c < nchunks; ++c) {
            if (nchunks > 1) {
                __syncthreads();
                stage(c);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
            const int kt0 = c * tpc;
            const int kt1 = !active ? kt0 : (kt_end < kt0 + tpc ? kt_end : kt0 + tpc);
            const int cb = kt0 << 6;
            for (int kt = kt0; kt < kt1; ++kt) {
                f32x4 sc[4];
                attn_score_tile<RB, NKK, NC - 1>(sK, kt, cb, l15, g, qf, sc);
                if (kt < npt) attn_mask_causal<MQ_MASK_NONE>(sc, kt, npt, g, q, qb0, P);                     // prefix: only keys >= P of its partial last tile
                else attn_mask_causal<MQ_MASK_CAUSAL>(sc, kt - npt, nkt, g, q, qb0, len);                    // own: the causal kernel's mask on own tile kt - npt
                attn_softmax_step<NDT>(sc, m_run, l_run, o, scale_log2e);   // (first tile visited: prefix key 0 when P >= 1, else own key 0)
                attn_pv_tile<RB, NDT, NC - 1>(sV, kt, cb, vkey, vcol, vhalf, sc, o);
            }
        }  // pieces
        if (!active) continue;
        const float inv = attn_inv_denominator(l_run);
        if (q < len) attn_store_bf16<NDT>(out + (int64_t)(row0 + q) * ldo + h * HD + 4 * g, o, inv);
    }
}

template <int HD>
int launch_gqa_prefix(const void* d_qkv, void* d_out, const int32_t* d_cu, int64_t nseq, int P, int q_heads, int kv_heads, int nslices, int kpad, hipStream_t s) {
    const size_t lds = (size_t)kpad * HD * 4;
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)attention_gqa_prefix_kernel<HD>, lds, 160 * 1024, done, "mq_attention_gqa_prefix");
    if (rc != MQ_OK) return rc;
    const float scale_log2e = 1.44269504088896340736f / sqrtf((float)HD);
    hipLaunchKernelGGL((attention_gqa_prefix_kernel<HD>), dim3((unsigned)(nseq * kv_heads * nslices)), dim3(GQA_NW * 64), lds, s, (const bf16_t*)d_qkv,
                       (bf16_t*)d_out, d_cu, P, q_heads, kv_heads, nslices, kpad, scale_log2e);
    return MQ_OK;
}

// ---- causal sliding-window form (Mistral-7B-v0.1's sliding_window: transformers masking_utils, sliding_window_overlay AND causal_mask_function) -------
// The query at position i of a sequence sees the keys j with i - window < j <= i.  The work split is attention_gqa_kernel's; what differs is the LOWER
// end of what a slice stages and a block walks:
//
//   - the slice [q0, q_last] stages the key tiles [st0, skt): st0 = the tile of key max(0, q0 - window + 1), skt as under the causal mask — at most
//     2 + ceil((window - 1) / 64) tiles, which is what the entry point sizes kpad by, so a long sequence costs O(T window), not O(T^2);
//   - a 16-query block visits the tiles [kt_begin, kt_end): kt_begin = the tile of key max(0, qb0 - window + 1), kt_end as under the causal mask;
//   - the tiles that cut the band — above (the diagonal), below (the first tile or two of the block), the ragged last — are masked per key.
//
// The tiles of a block that lie below the band of its LATER queries give those queries no key: attn_softmax_step keeps m_run = -1e30 for them, their
// probabilities are exp2(-inf) = 0, and the first tile with a key rescales the empty accumulators by exp2(-huge) = 0.  With window >= len: st0 = 0 and
// kt_begin = 0, and every statement below reduces to attention_gqa_kernel<MQ_MASK_CAUSAL>'s, in its order (bit-identical output).
template <int HD>
__global__ __launch_bounds__(GQA_NW * 64) void attention_gqa_window_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                           int fixed_len, int q_heads, int kv_heads, int nslices, int kpad, int window,
                                                                           float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = HD * 2;
    constexpr int NC = HD / 8;
    constexpr int NKK = HD / 32;
    constexpr int NDT = HD / 16;
    char* sK = smem;
    char* sV = smem + (size_t)kpad * RB;

    const unsigned sk = blockIdx.x / (unsigned)nslices;
    const int slice = (int)(blockIdx.x - sk * (unsigned)nslices);
    const int seq = sk / kv_heads, kvh = sk - seq * kv_heads;
    int row0, len;
    if (fixed_len > 0) { row0 = seq * fixed_len; len = fixed_len; }
    else { row0 = cu[seq]; len = cu[seq + 1] - row0; }
    const int q0 = slice * GQA_SLICE;
    if (len <= 0 || q0 >= len) return;     // (the whole workgroup: no barrier has been reached)
    const int G = q_heads / kv_heads;
    const int ld = (q_heads + 2 * kv_heads) * HD, ldo = q_heads * HD;
    const bf16_t* qrow = qkv + (int64_t)row0 * ld;
    const bf16_t* kb = qrow + (q_heads + kvh) * HD;
    const bf16_t* vb = kb + kv_heads * HD;
    const int nkt = (len + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // the slice: its 16-query blocks, the key tiles [st0, skt) it stages, the pieces they pass through the LDS in
    const int q_last = q0 + GQA_SLICE - 1 < len - 1 ? q0 + GQA_SLICE - 1 : len - 1;
    const int nblk = ((q_last - q0) >> 4) + 1;
    const int st0 = q0 - window + 1 > 0 ? (q0 - window + 1) >> 6 : 0;
    const int skt = (q_last >> 6) + 1;
    const int tpc = kpad >> 6;
    const int nchunks = (skt - st0 + tpc - 1) / tpc;
    const int nitems = G * nblk;
    const int nrounds = (nitems + GQA_NW - 1) / GQA_NW;
    auto stage = [&](int c) {
        const int t0 = st0 + c * tpc;
        const int tiles_here = skt - t0 < tpc ? skt - t0 : tpc;
        attn_stage_piece<RB, NC, NC - 1, GQA_NW>(sK, sV, kb, vb, ld, t0 << 6, tiles_here << 6, len, lane, wave);
    };
    if (nchunks == 1) {
        stage(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    const int l15 = lane & 15, g = lane >> 4;
    const int vkey = 4 * g + (l15 >> 2);
    const int vcol = (l15 & 3) >> 1, vhalf = (l15 & 1) << 3;

    for (int rnd = 0; rnd < nrounds; ++rnd) {
        const int item = rnd * GQA_NW + wave;
        const bool active = item < nitems;       // wave-uniform; with nchunks > 1 an idle wave still stages and keeps the barriers
        if (nchunks == 1 && !active) break;
        const int gh = active ? item / nblk : 0;
        int blk = active ? item - gh * nblk : 0;
        if (gh & 1) blk = nblk - 1 - blk;
        const int h = kvh * G + gh;
        const int qb0 = q0 + blk * 16;
        const int q = qb0 + l15;
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

        const int kt_begin = qb0 - window + 1 > 0 ? (qb0 - window + 1) >> 6 : 0;   // the tile of the lowest key the block's first query sees (>= st0)
        const int last = (qb0 + 15) >> 6;                                          // the tile of the block's last query
        const int kt_end = last + 1 < skt ? last + 1 : skt;
        for (int c = 0; c < nchunks; ++c) {
            if (nchunks > 1) {   // (re)fill the LDS with key tiles [st0 + c tpc, st0 + (c + 1) tpc) of the slice
                __syncthreads();
                stage(c);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
            const int kt0 = st0 + c * tpc;
            const int ks = kt_begin > kt0 ? kt_begin : kt0;
            const int ke = !active ? ks : (kt_end < kt0 + tpc ? kt_end : kt0 + tpc);
            const int cb = kt0 << 6;                         // LDS row of global key `key` is key - cb (cb is a multiple of 64)
            for (int kt = ks; kt < ke; ++kt) {
                f32x4 sc[4];
                attn_score_tile<RB, NKK, NC - 1>(sK, kt, cb, l15, g, qf, sc);
                attn_mask_causal_window(sc, kt, nkt, g, q, qb0, window, len);
                attn_softmax_step<NDT>(sc, m_run, l_run, o, scale_log2e);
                attn_pv_tile<RB, NDT, NC - 1>(sV, kt, cb, vkey, vcol, vhalf, sc, o);
            }
        }  // pieces
        if (!active) continue;
        const float inv = attn_inv_denominator(l_run);
        if (q < len) attn_store_bf16<NDT>(out + (int64_t)(row0 + q) * ldo + h * HD + 4 * g, o, inv);
    }
}

template <int HD>
int launch_gqa_window(const void* d_qkv, void* d_out, const int32_t* d_cu, int64_t nseq, int fixed_len, int q_heads, int kv_heads, int nslices, int kpad,
                      int window, hipStream_t s) {
    const size_t lds = (size_t)kpad * HD * 4;
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)attention_gqa_window_kernel<HD>, lds, 160 * 1024, done, "mq_attention_gqa_window");
    if (rc != MQ_OK) return rc;
    const float scale_log2e = 1.44269504088896340736f / sqrtf((float)HD);
    hipLaunchKernelGGL((attention_gqa_window_kernel<HD>), dim3((unsigned)(nseq * kv_heads * nslices)), dim3(GQA_NW * 64), lds, s, (const bf16_t*)d_qkv,
                       (bf16_t*)d_out, d_cu, fixed_len, q_heads, kv_heads, nslices, kpad, window, scale_log2e);
    return MQ_OK;
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
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(2, s);
    int rc;
    if (head_dim == 64)
        rc = mask == MQ_MASK_CAUSAL ? launch_gqa<MQ_MASK_CAUSAL, 64>(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, q_heads, kv_heads, nslices, kpad, s)
                                    : launch_gqa<MQ_MASK_NONE, 64>(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, q_heads, kv_heads, nslices, kpad, s);
    else
        rc = mask == MQ_MASK_CAUSAL ? launch_gqa<MQ_MASK_CAUSAL, 128>(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, q_heads, kv_heads, nslices, kpad, s)
                                    : launch_gqa<MQ_MASK_NONE, 128>(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, q_heads, kv_heads, nslices, kpad, s);
    if (rc != MQ_OK) return rc;
    MQ_CHECK_LAUNCH("mq_attention_gqa");
    return MQ_OK;
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
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(2, s);
    const int rc = head_dim == 64 ? launch_gqa_prefix<64>(d_qkv, d_out, d_cu_seqlens, nseq, prefix_len, q_heads, kv_heads, nslices, kpad, s)
                                  : launch_gqa_prefix<128>(d_qkv, d_out, d_cu_seqlens, nseq, prefix_len, q_heads, kv_heads, nslices, kpad, s);
    if (rc != MQ_OK) return rc;
    MQ_CHECK_LAUNCH("mq_attention_gqa_prefix");
    return MQ_OK;
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
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(2, s);
    const int rc = head_dim == 64 ? launch_gqa_window<64>(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, q_heads, kv_heads, nslices, kpad, w, s)
                                  : launch_gqa_window<128>(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, q_heads, kv_heads, nslices, kpad, w, s);
    if (rc != MQ_OK) return rc;
    MQ_CHECK_LAUNCH("mq_attention_gqa_window");
    return MQ_OK;
}
