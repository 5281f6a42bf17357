// The tile core of the LDS-staged flash-style attention kernels (included by attention.hip, attention_alibi.hip, attention_disentangled.hip,
// attention_full.hip, attention_gqa256.hip, attention_relbias.hip and attention_window.hip; by attention_gqa.hip and attention_gqa256_causal.hip through
// attention_gqa_core.h, which holds the one work split those two share): what one
// wave does with one 64-key tile for its 16 queries, and the host arithmetic their entry points share.  The kernels differ in the work split — which keys
// a workgroup stages, which tiles a query block visits — and keep that, their register budgets and their measured choices in their own files.
//
// K [keys, HD] and V [keys, HD] of one (sequence, K/V head) lie row-major in LDS, written by LDS-DMA (global_load_lds: every 1-KiB piece is in flight at
// once, no register round trip), the 16-B chunks of a row XOR-swizzled: chunk c of key k lives in slot c ^ (k & SWZ).  A wave runs an online softmax over
// 64-key tiles with both GEMMs on v_mfma_f32_16x16x32_bf16, operands swapped:
//
//   S^T = K . Q^T    (so every lane's 16 scores belong to ONE query: the row max / row sum need only two xor-shuffles, no LDS round trip)
//   O^T = V^T . P^T  (the P^T fragment a lane needs as MFMA B-operand is exactly the set of probabilities it already holds; the k-slot <-> key
//                     permutation is applied identically to the V^T A-operand, which is legal because the contraction is permutation-invariant)
//
// Lane = (l15 = lane & 15, g = lane >> 4).  The lane's query is block * 16 + l15; its 16 scores of tile kt are the keys 64 kt + 16 t + 4 g + r
// (sc[t][r]); its 4 output values per 16-wide dim tile dt are dims 16 dt + 4 g .. + 3.  Template parameters: RB = bytes per LDS row, NC = 16-B chunk
// slots per row, SWZ = swizzle mask, NKK = 32-deep MFMA k-chunks of a Q.K dot product, NDT = 16-wide output-dim tiles, NW = wave64s per workgroup.
#pragma once
#include "common.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));

// ---- stage K and V rows [base_key, base_key + rows_here) into LDS rows 0 ..: 1024 / RB rows per LDS-DMA; lane -> (row = RPP piece + lane / NC, physical
// chunk = lane % NC) fetches the logical chunk that lives there.  base_key is a multiple of 64, so LDS row & SWZ == key & SWZ.  Rows past the sequence
// re-read its last row (finite values; their scores are masked and their probabilities are exactly 0).  NCS < NC: the head has only NCS chunks in global memory; the slots
// past them get any finite filler (they meet zero Q dims).  The caller waits (vmcnt(0)) and synchronises.
template <int RB, int NC, int SWZ, int NW, int NCS = NC>
__device__ __forceinline__ void attn_stage_piece(char* sK, char* sV, const bf16_t* kb, const bf16_t* vb, int ld, int base_key, int rows_here, int len,
                                                 int lane, int wave) {
    constexpr int RPP = 1024 / RB;
    const int np8 = rows_here / RPP;
    const int srow = lane / NC, pchunk = lane % NC;
    for (int p = wave; p < 2 * np8; p += NW) {
        const bool is_v = p >= np8;
        const int piece = is_v ? p - np8 : p;
        const int row = piece * RPP + srow;
        const int key = base_key + row < len ? base_key + row : len - 1;
        int lc = pchunk ^ (row & SWZ);
        if (NCS < NC) lc = lc < NCS ? lc : 0;
        const bf16_t* src = (is_v ? vb : kb) + (int64_t)key * ld + (lc << 3);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)((is_v ? sV : sK) + piece * 1024), 16, 0, 0);
    }
}

// ---- S^T tile: sc[t][r] = q . k over keys 64 kt + 16 t + 4 g + r.  qf[kk] holds dims 32 kk + 8 g .. + 7 of the lane's query; cb = the global key of LDS
// row 0 (a multiple of 64).  Two shapes of the same arithmetic, because the register allocation follows the shape: attn_score_keys (one 16-key row,
// RETURNS its accumulator) is what attention.hip calls per row — on attn_score_tile its bias forms spill and one 128-wide form loses a wave per SIMD;
// attn_score_tile (fills sc[] in one body) is what the other three call — built from attn_score_keys, attention_gqa_kernel<causal, 128> takes 122
// registers for 118 and measured 3 % slower.
template <int RB, int NKK, int SWZ>
__device__ __forceinline__ f32x4 attn_score_keys(const char* sK, int key, int cb, int g, const bf16x8 (&qf)[NKK]) {   // key = this lane's A-operand row
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
        const bf16x8 kf = *(const bf16x8*)(sK + (key - cb) * RB + (((g + 4 * kk) ^ (key & SWZ)) << 4));
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], acc, 0, 0, 0);
    }
    return acc;
}
template <int RB, int NKK, int SWZ>
__device__ __forceinline__ void attn_score_tile(const char* sK, int kt, int cb, int l15, int g, const bf16x8 (&qf)[NKK], f32x4 (&sc)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int key = kt * 64 + t * 16 + l15;  // A-operand row
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            const bf16x8 kf = *(const bf16x8*)(sK + (key - cb) * RB + (((g + 4 * kk) ^ (key & SWZ)) << 4));
            sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], sc[t], 0, 0, 0);
        }
    }
}

// ---- masks.  Each opens with a wave-uniform test, so tiles that need no mask skip the per-key compares / selects.  (The test stays in the same
// function body as the selects it guards: split off into a helper that returns a bool, the register allocation of the callers changes and the window
// kernel loses a wave per SIMD.)  qb0 = the first query of the lane's 16-query block.
// Causal / ragged tail: needed only on the ragged last tile and (causal) on tiles that reach past the block's first query
template <int MASK>
__device__ __forceinline__ void attn_mask_causal(f32x4 (&sc)[4], int kt, int nkt, int g, int q, int qb0, int len) {
    bool need_mask = (kt == nkt - 1) && (len & 63);
    if (MASK != MQ_MASK_NONE) need_mask = need_mask || (kt * 64 + 63 > qb0);
    if (need_mask) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * 64 + t * 16 + g * 4 + r;
                bool valid = key < len;
                if (MASK != MQ_MASK_NONE) valid = valid && (key <= q);
                // CoCa's class-token row (the sequence's LAST row) does not see its own key (open_clip build_cls_mask, see marqo_hip.h)
                if (MASK == MQ_MASK_CAUSAL_CLS) valid = valid && !(q == len - 1 && key == q && len > 1);
                sc[t][r] = valid ? sc[t][r] : -INFINITY;
            }
    }
}
// Band |q - key| <= hw: a tile wholly inside the band of all 16 queries of the block and inside the sequence is interior
__device__ __forceinline__ void attn_mask_band(f32x4 (&sc)[4], int kt, int g, int q, int qb0, int hw, int len) {
    const bool interior = kt * 64 >= qb0 + 15 - hw && kt * 64 + 63 <= qb0 + hw && kt * 64 + 63 < len;
    if (!interior) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * 64 + t * 16 + g * 4 + r;
                const bool valid = key < len && key >= q - hw && key <= q + hw;
                sc[t][r] = valid ? sc[t][r] : -INFINITY;
            }
    }
}

// Causal band q - window < key <= q (Mistral's sliding window): a tile at or behind the block's first query, inside the sequence, and at or past the
// lowest key the block's LAST query sees is interior.  With window >= len no key is cut below, and what is left is attn_mask_causal<MQ_MASK_CAUSAL>.
__device__ __forceinline__ void attn_mask_causal_window(f32x4 (&sc)[4], int kt, int nkt, int g, int q, int qb0, int window, int len) {
    const bool need_mask = ((kt == nkt - 1) && (len & 63)) || (kt * 64 + 63 > qb0) || (kt * 64 <= qb0 + 15 - window);
    if (need_mask) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * 64 + t * 16 + g * 4 + r;
                const bool valid = key < len && key <= q && key > q - window;
                sc[t][r] = valid ? sc[t][r] : -INFINITY;
            }
    }
}

// ---- online-softmax step: sc becomes the tile's probabilities relative to the new running max.  The max runs on the RAW scores (the softmax scale is
// positive); scale and shift fold into one FMA per element.  A query that sees no key of this tile keeps m_run (from -1e30): its probabilities here are
// exp2(-inf) = 0 and alpha = 1.  o and l_run are rescaled only when some query's running max moved (rare after the first tiles).
template <int NDT>
__device__ __forceinline__ void attn_softmax_step(f32x4 (&sc)[4], float& m_run, float& l_run, f32x4 (&o)[NDT], float scale_log2e) {
    float mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])), fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
    mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(sc[2][0], sc[2][1]), fmaxf(sc[2][2], sc[2][3])), fmaxf(fmaxf(sc[3][0], sc[3][1]), fmaxf(sc[3][2], sc[3][3]))));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float neg_mc = -m_new * scale_log2e;
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sc[t][r] = __builtin_amdgcn_exp2f(fmaf(sc[t][r], scale_log2e, neg_mc));
            psum += sc[t][r];
        }
    if (__any(m_new != m_run)) {
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2e);
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[dt] *= alpha;
    }
    l_run += psum;
    m_run = m_new;
}

// ---- O^T += V^T . P^T over the tile's two 32-key halves.  The V^T operand is produced by ds_read_b64_tr_b16 (the hardware 4x4 transpose read) straight
// from the row-major V — no transposed copy exists.  Lane (d = 16 dt + l15, g) needs V[keys 16 (2u) + 4g .. + 3][d] and V[keys 16 (2u + 1) + 4g .. + 3][d]:
// the read hands output lane 4r + c of a 16-lane block element c of the 8 bytes fetched by lanes r, r + 4, r + 8, r + 12 of that block, so source lane
// (g, l15) fetches V[key0 + 4g + l15 / 4][4 (l15 % 4) .. + 3].  Its per-lane constants: vkey = 4 g + (l15 >> 2), vcol = (l15 & 3) >> 1 (which 16-B chunk
// of the dim tile), vhalf = (l15 & 1) << 3 (which 8 bytes of the chunk).
template <int RB, int NDT, int SWZ>
__device__ __forceinline__ void attn_pv_tile(const char* sV, int kt, int cb, int vkey, int vcol, int vhalf, const f32x4 (&sc)[4], f32x4 (&o)[NDT]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        union { uint32_t w[4]; bf16x8 v; } pf;
        pf.w[0] = pack_bf16x2(sc[2 * u][0], sc[2 * u][1]);
        pf.w[1] = pack_bf16x2(sc[2 * u][2], sc[2 * u][3]);
        pf.w[2] = pack_bf16x2(sc[2 * u + 1][0], sc[2 * u + 1][1]);
        pf.w[3] = pack_bf16x2(sc[2 * u + 1][2], sc[2 * u + 1][3]);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            union { s16x4 t[2]; bf16x8 v; } vf;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const int key = kt * 64 + (2 * u + tt) * 16 + vkey;
                const char* vp = sV + (key - cb) * RB + ((((dt << 1) | vcol) ^ (key & SWZ)) << 4) + vhalf;
                vf.t[tt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)vp);
            }
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, pf.v, o[dt], 0, 0, 0);
        }
    }
}

// ---- epilogue: 1 / (the query's softmax denominator), summed over the 4 lanes that share the query (every lane of the wave calls it), and the lane's
// 4 values of one dim tile as bf16; orow = the query's output row + 4 g
__device__ __forceinline__ float attn_inv_denominator(float l_run) {
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    return 1.0f / l_tot;
}
template <int NDT>
__device__ __forceinline__ void attn_store_bf16(bf16_t* orow, const f32x4 (&o)[NDT], float inv) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
        uint2 p;
        p.x = pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv);
        p.y = pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv);
        *(uint2*)(orow + dt * 16) = p;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------
// Keys of K + V the LDS image holds: the longest sequence in whole 64-key tiles, at most `cap` (what fits the CU's 160 KiB at the kernel's row width);
// a sequence longer than that streams through the LDS in pieces of kpad keys
static inline int attn_kpad(int maxl, int cap) {
    const int need = ((maxl + 63) / 64) * 64;
    return need < cap ? need : cap;
}
// The same for a band kernel whose workgroup owns 64 queries: it can reach its own tile and ceil(hw / 64) on either side, never more than the sequence has
static inline int attn_band_kpad(int hw, int maxl, int cap) {
    const int reach = 1 + 2 * ((hw + 63) / 64), seq_tiles = (maxl + 63) / 64;
    const int need = (reach < seq_tiles ? reach : seq_tiles) * 64;
    return need < cap ? need : cap;
}

// Dynamic LDS above 64 KiB needs an opt-in.  `lds` varies from call to call and the opt-in is latched once per device (`done`: one per kernel
// instantiation): it is made for `most`, the most the kernel ever asks for, so a call with short sequences or a small band in front of one that needs more
// leaves the limit where the larger one needs it.  (attention.hip does not use this: it sets the attribute on every launch above 64 KiB to that call's
// own `lds`, so no call depends on an earlier one; it predates the latch and keeps what its callers have always run.)
static inline int attn_ensure_lds(const void* kern, size_t lds, size_t most, std::atomic<uint64_t>& done, const char* fn) {
    if (lds <= 64 * 1024) return MQ_OK;
    const hipError_t e = mq_ensure_dyn_lds(kern, (int)most, done);
    if (e == hipSuccess) return MQ_OK;
    mq_set_error("%s: hipFuncSetAttribute: %s", fn, hipGetErrorString(e));
    return MQ_ERR_HIP;
}

// The argument checks the entry points share word for word; `fn` (a string literal) is the entry point's name, which the message begins with.  They are
// separate so that each entry point keeps the order of its checks, its own among them.
#define ATTN_ARG_PTRS(fn, qkv, out) MQ_CHECK_ARG((qkv) && (out), fn ": null pointer")
#define ATTN_ARG_SEQS(fn, fixed_len, cu) MQ_CHECK_ARG((fixed_len) > 0 || (cu), fn ": need fixed_len or cu_seqlens")
#define ATTN_ARG_MAXL(fn, maxl) MQ_CHECK_ARG((maxl) >= 1 && (maxl) <= 8192, fn ": max sequence length %d unsupported (1..8192)", maxl)
#define ATTN_ARG_GRID(fn, blocks) MQ_CHECK_ARG((blocks) < (1LL << 31), fn ": grid too large")
#define ATTN_ARG_GROUPS(fn, q_heads, kv_heads)                                                              \
    MQ_CHECK_ARG((q_heads) >= 1 && (kv_heads) >= 1 && (q_heads) <= 1024 && (q_heads) % (kv_heads) == 0,     \
                 fn ": q_heads %d must be a multiple of kv_heads %d (1..1024 query heads)", q_heads, kv_heads)
