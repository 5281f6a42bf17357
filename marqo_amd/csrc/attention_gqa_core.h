// The work split of the grouped-query attention kernels, above the tile math of attention_core.h: one body, attn_gqa_body, which the three __global__
// kernels of attention_gqa.hip and the one of attention_gqa256_causal.hip call with a POLICY that says what they differ in.  (attention_gqa256.hip's band
// kernel has the same work split in a body of its own: its header says why.)  No kernel and no entry point lives here.
//
//   - A sequence's queries are split into SLICES.  One workgroup of NW wave64s per (sequence, K/V head, slice), decoded from blockIdx.x: it stages that
//     head's K and V once for all G = q_heads / kv_heads query heads that read it (repeat_kv: K/V head kvh serves query heads kvh G .. kvh G + G - 1).
//   - The slice stages the key tiles [first_tile, end_tile) of its policy.  They pass through the LDS in PIECES of tpc = kpad / 64 tiles; LDS row 0 of
//     piece c is the first key of tile first_tile + c tpc, so a key and its LDS row agree modulo 64 and the swizzle of attention_core.h holds.
//   - The work ITEMS are the (query head of the group, 16-query block of the slice) pairs; wave w takes items w, w + NW, ... in ROUNDS.  Item i is
//     query head i / nblk and block i % nblk.  A block walks the tiles [block_first_tile, block_end_tile) of its policy, piece by piece:
//     score -> mask -> online-softmax step -> PV, in one loop body (the register allocation follows the shape of the source: attention_core.h).
//   - One piece: it is staged once, in front of the rounds, and a wave with no item left is done.  More than one: every round re-stages every piece
//     (barrier, stage, vmcnt(0), barrier), and a wave without an item in the last round STILL stages and keeps the barriers; it walks no tile and
//     stores nothing.  The only return is the whole workgroup's, before any barrier.
//
// A policy is a small struct, passed by value, of the kernel's own run-time scalars and inlined members.  AttnGqaPolicy<Slice, Keys> joins the two halves:
//
//   Slice   slice_queries()                  queries per slice, a multiple of 16; a slice starts on a key-tile boundary where the key space needs it
//           slice_of(dealt, nslices)         the slice of the dealt index blockIdx.x % nslices
//           REVERSE_ODD_HEADS                count the blocks of odd heads from the slice's far end
//   Keys    first_tile(q0) / end_tile(q_last, nkt)                  the tiles the slice stages
//           stage<RB, NC, SWZ, NW>(..., t0, tiles, ...)             `tiles` of them from t0 on -> LDS rows 0 ..
//           block_first_tile(qb0) / block_end_tile(qb0, skt)             the tiles a block visits, the end at most skt; CUTS_BELOW: the first may lie above
//                                                                   the slice's (without it the body does not clip below: a compare per piece less)
//           mask(sc, kt, nkt, g, q, qb0, len)                       attention_core.h's mask of tile kt, its wave-uniform test inside
//
// Why each kernel's policy is what it is stands in that kernel's file.
#pragma once
#include "attention_core.h"

// ---- slice geometry ----------------------------------------------------------------------------------------------------------------------------------
template <int QUERIES, bool REVERSE>
struct AttnSliceFixed {   // QUERIES per slice, dealt forward
    static constexpr bool REVERSE_ODD_HEADS = REVERSE;
    __device__ __forceinline__ int slice_queries() const { return QUERIES; }
    __device__ __forceinline__ int slice_of(int dealt, int) const { return dealt; }
};
struct AttnSliceBlocks {  // nb 16-query blocks per slice, dealt longest first (from the sequence's end)
    int nb;
    static constexpr bool REVERSE_ODD_HEADS = false;
    __device__ __forceinline__ int slice_queries() const { return nb * 16; }
    __device__ __forceinline__ int slice_of(int dealt, int nslices) const { return nslices - 1 - dealt; }
};

// ---- key spaces --------------------------------------------------------------------------------------------------------------------------------------
// One source: `tiles` tiles of the sequence's own keys, from tile t0 on
template <int RB, int NC, int SWZ, int NW>
__device__ __forceinline__ void attn_gqa_stage_own(char* sK, char* sV, const bf16_t* kb, const bf16_t* vb, int ld, int t0, int tiles, int len, int lane, int wave) {
    attn_stage_piece<RB, NC, SWZ, NW>(sK, sV, kb, vb, ld, t0 << 6, tiles << 6, len, lane, wave);
}

// Every key (MQ_MASK_NONE) or keys 0 .. q (MQ_MASK_CAUSAL): a causal slice stages only the tiles up to its last query, a causal block visits only
// the tiles whose first key is <= its last query
template <int MASK>
struct AttnKeysPlain {
    static constexpr bool CUTS_BELOW = false;
    __device__ __forceinline__ int first_tile(int) const { return 0; }
    __device__ __forceinline__ int end_tile(int q_last, int nkt) const { return MASK == MQ_MASK_CAUSAL ? (q_last >> 6) + 1 : nkt; }
    template <int RB, int NC, int SWZ, int NW>
    __device__ __forceinline__ void stage(char* sK, char* sV, const bf16_t* kb, const bf16_t* vb, const bf16_t*, const bf16_t*, int ld, int t0, int tiles, int len,
                                          int lane, int wave) const {
        attn_gqa_stage_own<RB, NC, SWZ, NW>(sK, sV, kb, vb, ld, t0, tiles, len, lane, wave);
    }
    __device__ __forceinline__ int block_first_tile(int) const { return 0; }
    __device__ __forceinline__ int block_end_tile(int qb0, int skt) const {
        if (MASK != MQ_MASK_CAUSAL) return skt;
        const int last = (qb0 + 15) >> 6;    // the tile of the block's last query: tiles behind it start past every query of the block
        return last + 1 < skt ? last + 1 : skt;
    }
    __device__ __forceinline__ void mask(f32x4 (&sc)[4], int kt, int nkt, int g, int q, int qb0, int len) const {
        attn_mask_causal<MASK>(sc, kt, nkt, g, q, qb0, len);   // (every query sees at least key 0, in the first tile it visits)
    }
};

// The P keys of a shared prefix (rows 0 .. P - 1 of the buffer), then keys 0 .. q of the query's own segment, as VIRTUAL tiles:
//   tiles [0, npt), npt = ceil(P / 64)   the prefix keys; the last one is partial when P % 64 != 0: its keys >= P are masked
//   tiles npt ..                         the segment's own keys, own key j at virtual key 64 npt + j: a FRESH tile, no tile straddles the two ranges
// Both ranges are staged from a tile boundary on, so a virtual key and its LDS row agree modulo 64.  Prefix tiles come first: with P >= 1 the first tile
// a query visits holds prefix key 0, which it sees; with P = 0 there is no prefix tile and every member reduces to AttnKeysPlain<MQ_MASK_CAUSAL>'s.
struct AttnKeysPrefix {
    int P;
    static constexpr bool CUTS_BELOW = false;
    __device__ __forceinline__ int npt() const { return (P + 63) >> 6; }
    __device__ __forceinline__ int first_tile(int) const { return 0; }
    __device__ __forceinline__ int end_tile(int q_last, int) const { return npt() + (q_last >> 6) + 1; }
    template <int RB, int NC, int SWZ, int NW>
    __device__ __forceinline__ void stage(char* sK, char* sV, const bf16_t* kb, const bf16_t* vb, const bf16_t* pkb, const bf16_t* pvb, int ld, int t0, int tiles,
                                          int len, int lane, int wave) const {   // the prefix tiles among [t0, t1), then the own tiles
        const int t1 = t0 + tiles;
        const int pe = t1 < npt() ? t1 : npt();          // one past the last prefix tile of the piece
        const int os = t0 > npt() ? t0 : npt();          // its first own tile
        if (pe > t0) attn_stage_piece<RB, NC, SWZ, NW>(sK, sV, pkb, pvb, ld, t0 << 6, (pe - t0) << 6, P, lane, wave);
        if (t1 > os) {
            const size_t off = (size_t)((os - t0) << 6) * RB;
            attn_stage_piece<RB, NC, SWZ, NW>(sK + off, sV + off, kb, vb, ld, (os - npt()) << 6, (t1 - os) << 6, len, lane, wave);
        }
    }
    __device__ __forceinline__ int block_first_tile(int) const { return 0; }
    __device__ __forceinline__ int block_end_tile(int qb0, int skt) const {
        const int last = npt() + ((qb0 + 15) >> 6);      // the virtual tile of the block's last query: own tiles behind it start past every query
        return last + 1 < skt ? last + 1 : skt;
    }
    __device__ __forceinline__ void mask(f32x4 (&sc)[4], int kt, int nkt, int g, int q, int qb0, int len) const {
        if (kt < npt()) attn_mask_causal<MQ_MASK_NONE>(sc, kt, npt(), g, q, qb0, P);             // prefix: only keys >= P of its partial last tile
        else attn_mask_causal<MQ_MASK_CAUSAL>(sc, kt - npt(), nkt, g, q, qb0, len);              // own: the causal mask on own tile kt - npt
    }
};

// Keys q - window < key <= q: what differs from the causal form is the LOWER end of what a slice stages and a block walks
struct AttnKeysCausalWindow {
    int window;
    static constexpr bool CUTS_BELOW = true;
    __device__ __forceinline__ int first_tile(int q0) const { return q0 - window + 1 > 0 ? (q0 - window + 1) >> 6 : 0; }
    __device__ __forceinline__ int end_tile(int q_last, int) const { return (q_last >> 6) + 1; }
    template <int RB, int NC, int SWZ, int NW>
    __device__ __forceinline__ void stage(char* sK, char* sV, const bf16_t* kb, const bf16_t* vb, const bf16_t*, const bf16_t*, int ld, int t0, int tiles, int len,
                                          int lane, int wave) const {
        attn_gqa_stage_own<RB, NC, SWZ, NW>(sK, sV, kb, vb, ld, t0, tiles, len, lane, wave);
    }
    __device__ __forceinline__ int block_first_tile(int qb0) const { return first_tile(qb0); }   // the tile of the lowest key the block's first query sees
    __device__ __forceinline__ int block_end_tile(int qb0, int skt) const {
        const int last = (qb0 + 15) >> 6;                // the tile of the block's last query
        return last + 1 < skt ? last + 1 : skt;
    }
    __device__ __forceinline__ void mask(f32x4 (&sc)[4], int kt, int nkt, int g, int q, int qb0, int len) const {
        attn_mask_causal_window(sc, kt, nkt, g, q, qb0, window, len);
    }
};

template <class Slice, class Keys>
struct AttnGqaPolicy : Slice, Keys {};

// ---- the body ----------------------------------------------------------------------------------------------------------------------------------------
// qkv bf16 [rows, (q_heads + 2 kv_heads) HD] = (q | k | v); sequences fixed-length (fixed_len > 0) or packed (cu).  Dynamic LDS: K then V, [kpad][2 HD]
// bytes each, 16-B chunks XOR-swizzled by (key & SWZ).
template <int HD, int SWZ, int NW, class Policy>
__device__ __forceinline__ void attn_gqa_body(const bf16_t* qkv, bf16_t* out, const int32_t* cu, int fixed_len,
                                              int q_heads, int kv_heads, int nslices, int kpad, float scale_log2e, const Policy pol) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = HD * 2;       // bytes per K / V row in LDS
    constexpr int NC = HD / 8;       // 16-byte chunk slots per LDS row
    constexpr int NKK = HD / 32;     // 32-deep MFMA k-chunks of a Q.K dot product
    constexpr int NDT = HD / 16;     // 16-wide output-dim tiles
    char* sK = smem;
    char* sV = smem + (size_t)kpad * RB;

    const unsigned sk = blockIdx.x / (unsigned)nslices;
    const int slice = pol.slice_of((int)(blockIdx.x - sk * (unsigned)nslices), nslices);
    const int seq = sk / kv_heads, kvh = sk - seq * kv_heads;
    int row0, len;
    if (fixed_len > 0) { row0 = seq * fixed_len; len = fixed_len; }
    else { row0 = cu[seq]; len = cu[seq + 1] - row0; }
    const int q0 = slice * pol.slice_queries();
    if (len <= 0 || q0 >= len) return;     // (the whole workgroup: no barrier has been reached)
    const int G = q_heads / kv_heads;
    const int ld = (q_heads + 2 * kv_heads) * HD, ldo = q_heads * HD;
    const bf16_t* qrow = qkv + (int64_t)row0 * ld;
    const bf16_t* kb = qrow + (q_heads + kvh) * HD;      // the sequence's own keys / values
    const bf16_t* vb = kb + kv_heads * HD;
    const bf16_t* pkb = qkv + (q_heads + kvh) * HD;      // the same columns from row 0 of the buffer on: a shared prefix's (read by AttnKeysPrefix alone)
    const bf16_t* pvb = pkb + kv_heads * HD;
    const int nkt = (len + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // the slice: its 16-query blocks, the key tiles [st0, skt) it stages, the pieces they pass through the LDS in
    const int q_last = q0 + pol.slice_queries() - 1 < len - 1 ? q0 + pol.slice_queries() - 1 : len - 1;
    const int nblk = ((q_last - q0) >> 4) + 1;
    const int st0 = pol.first_tile(q0), skt = pol.end_tile(q_last, nkt);
    const int tpc = kpad >> 6;
    const int nchunks = (skt - st0 + tpc - 1) / tpc;
    const int nitems = G * nblk;
    const int nrounds = (nitems + NW - 1) / NW;
    auto stage = [&](int c) {
        const int t0 = st0 + c * tpc;
        pol.template stage<RB, NC, SWZ, NW>(sK, sV, kb, vb, pkb, pvb, ld, t0, skt - t0 < tpc ? skt - t0 : tpc, len, lane, wave);
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
        const int item = rnd * NW + wave;
        const bool active = item < nitems;       // wave-uniform; with nchunks > 1 an idle wave still stages and keeps the barriers
        if (nchunks == 1 && !active) break;
        const int gh = active ? item / nblk : 0;
        int blk = active ? item - gh * nblk : 0;
        if (Policy::REVERSE_ODD_HEADS && (gh & 1)) blk = nblk - 1 - blk;
        const int h = kvh * G + gh;
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

        const int kt_begin = pol.block_first_tile(qb0), kt_end = pol.block_end_tile(qb0, skt);
        for (int c = 0; c < nchunks; ++c) {
            if (nchunks > 1) {   // (re)fill the LDS with key tiles [st0 + c tpc, st0 + (c + 1) tpc) of the slice
                __syncthreads();
                stage(c);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
            const int kt0 = st0 + c * tpc;
            const int ks = Policy::CUTS_BELOW && kt_begin > kt0 ? kt_begin : kt0;
            const int ke = !active ? ks : (kt_end < kt0 + tpc ? kt_end : kt0 + tpc);
            const int cb = kt0 << 6;                         // LDS row of key `key` is key - cb (cb is a multiple of 64)
            for (int kt = ks; kt < ke; ++kt) {
                f32x4 sc[4];
                attn_score_tile<RB, NKK, SWZ>(sK, kt, cb, l15, g, qf, sc);
                pol.mask(sc, kt, nkt, g, q, qb0, len);
                attn_softmax_step<NDT>(sc, m_run, l_run, o, scale_log2e);
                attn_pv_tile<RB, NDT, SWZ>(sV, kt, cb, vkey, vcol, vhalf, sc, o);
            }
        }  // pieces
        if (!active) continue;
        const float inv = attn_inv_denominator(l_run);
        if (q < len) attn_store_bf16<NDT>(out + (int64_t)(row0 + q) * ldo + h * HD + 4 * g, o, inv);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------
// The launch of one of these kernels: its dynamic LDS (kpad keys of K + V) with the opt-in latched per KERN (`most`: the most bytes it ever asks for), the
// profiler scope, the launch, the launch check.  The kernels take (qkv, out, cu, fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e, own...).
template <auto KERN, int HD, int NW, class... Own>
static inline int attn_gqa_launch(const char* fn, size_t most, const void* d_qkv, void* d_out, const int32_t* d_cu, int64_t nseq, int fixed_len, int q_heads,
                                  int kv_heads, int nslices, int kpad, float scale_log2e, hipStream_t s, Own... own) {
    const size_t lds = (size_t)kpad * HD * 4;
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)KERN, lds, most, done, fn);
    if (rc != MQ_OK) return rc;
    MqProfScope prof(2, s);
    hipLaunchKernelGGL(KERN, dim3((unsigned)(nseq * kv_heads * nslices)), dim3(NW * 64), lds, s, (const bf16_t*)d_qkv, (bf16_t*)d_out, d_cu, fixed_len,
                       q_heads, kv_heads, nslices, kpad, scale_log2e, own...);
    MQ_CHECK_LAUNCH(fn);
    return MQ_OK;
}
