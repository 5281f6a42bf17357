// Bidirectional attention with a clamped relative-position bias, the attention of the T5 encoders (transformers T5EncoderModel: sentence-t5, gtr-t5,
// flan-t5 / T5 v1.1 encoder fine-tunes): bf16, 64- or 128-wide heads, packed or fixed-length sequences,
//
//   scores[q, k] = scale * (q . k) + bias[h][clamp(k - q, -D, D) + D]          out = softmax(scores) V
//
// T5's bucket function is constant for |k - q| >= relative_attention_max_distance, so a table of 2 D + 1 values per head with a clamped index is exact at
// any length; the table is used as it is (nothing is pre-divided by the scale) and `scale` is the caller's (T5: 1.0).
//
// The tile math is attention_core.h's (chunks swizzled by key & (NC - 1), bf16 P / fp32 normaliser); what is this file's own:
//
//   - Work split.  A sequence's queries are split into SLICES of 64 (four 16-query blocks, one per wave).  One workgroup of 4 wave64s per (sequence,
//     head, slice) stages the head's K and V — the whole sequence when it fits the LDS, else in pieces of kpad keys — and each wave runs its block over
//     every key tile.  A lone 512-token query on 12 heads is 96 workgroups, not 12.  Every slice stages the sequence's K / V again (from L2 after the
//     first): slice 64 x 4 waves against 128 x 8 is a choice nobody measured — throughput was not part of the work that added this kernel.
//   - The bias.  The head's 2 D + 1 values lie in LDS behind the K / V image (fp32, at most 8196 bytes at D = 1024), copied once per workgroup.  A tile
//     that lies D or more keys to one side of all 16 queries of the block takes ONE value (bias[0] or bias[2 D], kept in registers: a wave-uniform
//     test); the tiles around the diagonal gather 16 values per lane from LDS (consecutive lanes read consecutive or equal addresses: no bank conflict
//     beyond the broadcast).  No per-pair global read.
//   - The score is formed as fmaf(q . k, scale, bias) in fp32 and the softmax runs on it with scale 1 (log2(e) alone folds into the exponent).
//   - LDS: K + V at 2 HD bytes per key each, plus the bias: 576 keys at 64-wide heads (144 KiB + bias), 256 keys at 128-wide heads (128 KiB + bias) —
//     one 64-key tile less than the bias-free kernels hold, because the 160 KiB are shared with the table.  Longer sequences stream through in pieces.
//
// Compiler report (gfx950, -O3, resource remarks), 4 waves per workgroup, slice 64:
//   attention_relbias_kernel<64>:  94 VGPRs, 76 SGPRs, no VGPR / SGPR spill, no scratch, no static LDS, 4 waves / SIMD by registers
//   attention_relbias_kernel<128>: 130 VGPRs, 76 SGPRs, no VGPR / SGPR spill, no scratch, no static LDS, 3 waves / SIMD by registers
// Two registers over the 128 of a fourth wave at 128-wide heads: it matters only where the LDS image lets four workgroups share a CU (sequences of up to
// 64 keys); from 129 keys on the image (>= 96 KiB) leaves one workgroup per CU whatever the registers allow.  No occupancy request was tried or measured.
#include "attention_core.h"

namespace {

constexpr int RB_NW = 4;               // wave64s per workgroup = 16-query blocks per slice
constexpr int RB_SLICE = RB_NW * 16;   // queries per workgroup: one 64-key tile's worth
constexpr int RB_MAX_D = 1024;         // largest clamp distance: (2 * 1024 + 1) floats of LDS
constexpr size_t RB_LDS_MOST = 160 * 1024;

// keys of K + V the LDS holds next to the largest bias table, in whole 64-key tiles
constexpr int rb_lds_keys(int hd) { return (int)((RB_LDS_MOST - (2 * RB_MAX_D + 1) * 4) / ((size_t)hd * 4) / 64) * 64; }
static_assert(rb_lds_keys(64) == 576 && rb_lds_keys(128) == 256, "LDS budget of the K / V image next to the bias table");

template <int HD>
__global__ __launch_bounds__(RB_NW * 64) void attention_relbias_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                       int fixed_len, int heads, int nslices, int kpad, const float* __restrict__ rel_bias,
                                                                       int D, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = HD * 2;       // bytes per K / V row in LDS (128 or 256)
    constexpr int NC = HD / 8;       // 16-byte chunk slots per LDS row (8 or 16)
    constexpr int NKK = HD / 32;     // 32-deep MFMA k-chunks of a Q.K dot product
    constexpr int NDT = HD / 16;     // 16-wide output-dim tiles
    char* sK = smem;                                         // [kpad][RB], 16-B chunks XOR-swizzled by (key & (NC - 1))
    char* sV = smem + (size_t)kpad * RB;                     // [kpad][RB], same image
    float* sB = (float*)(smem + 2 * (size_t)kpad * RB);      // [2 D + 1]: the head's bias, entry d + D for key - query == d (clamped)

    const unsigned sh = blockIdx.x / (unsigned)nslices;
    const int slice = (int)(blockIdx.x - sh * (unsigned)nslices);
    const int seq = sh / heads, h = sh - seq * heads;
    int row0, len;
    if (fixed_len > 0) { row0 = seq * fixed_len; len = fixed_len; }
    else { row0 = cu[seq]; len = cu[seq + 1] - row0; }
    const int q0 = slice * RB_SLICE;
    if (len <= 0 || q0 >= len) return;     // (the whole workgroup: no barrier has been reached)
    const int inner = heads * HD, ld = 3 * inner;
    const bf16_t* qb = qkv + (int64_t)row0 * ld + h * HD;
    const bf16_t* kb = qb + inner;
    const bf16_t* vb = qb + 2 * inner;
    const int nkt = (len + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // the sequence's key tiles pass through the LDS in nchunks pieces of tpc tiles (one piece when they fit)
    const int tpc = kpad >> 6;
    const int nchunks = (nkt + tpc - 1) / tpc;
    auto stage = [&](int c) {
        const int tiles_here = nkt - c * tpc < tpc ? nkt - c * tpc : tpc;
        attn_stage_piece<RB, NC, NC - 1, RB_NW>(sK, sV, kb, vb, ld, (c * tpc) << 6, tiles_here << 6, len, lane, wave);
    };

    const int l15 = lane & 15, g = lane >> 4;
    const int qb0 = q0 + wave * 16;             // this wave's 16-query block
    const bool active = qb0 < len;              // wave-uniform; an idle wave still stages and keeps the barriers
    const int q = qb0 + l15;                    // this lane's query (B-operand column / output row)

    stage(0);
    for (int i = threadIdx.x; i < 2 * D + 1; i += RB_NW * 64) sB[i] = rel_bias[(int64_t)h * (2 * D + 1) + i];
    // Q fragments (dims 32 kk + 8 g .. + 7 of query row q, clamped to the sequence) are fetched while the K / V DMA is in flight
    bf16x8 qf[NKK];
    {
        const int qr = q < len ? q : len - 1;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) qf[kk] = *(const bf16x8*)(qb + (int64_t)qr * ld + 8 * g + 32 * kk);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const float b_lo = sB[0], b_hi = sB[2 * D];   // the bias of every key D or more behind / ahead of the query

    const int vkey = 4 * g + (l15 >> 2);    // per-lane constants of the V^T transpose reads
    const int vcol = (l15 & 3) >> 1, vhalf = (l15 & 1) << 3;

    float m_run = -1e30f, l_run = 0.f;
    f32x4 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < nchunks; ++c) {
        if (c > 0) {   // refill the LDS with the next piece of the sequence (the bias behind the image stays)
            __syncthreads();
            stage(c);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        const int kt0 = c * tpc;
        const int kt1 = !active ? kt0 : (nkt < kt0 + tpc ? nkt : kt0 + tpc);
        const int cb = kt0 << 6;                         // LDS row of global key `key` is key - cb
        for (int kt = kt0; kt < kt1; ++kt) {
            f32x4 sc[4];
            attn_score_tile<RB, NKK, NC - 1>(sK, kt, cb, l15, g, qf, sc);
            // score = scale * (q . k) + bias[clamp(key - q)]: key - q = d0 + 16 t + 4 g + r - l15 lies in [d0 - 15, d0 + 63] for the whole block
            const int d0 = kt * 64 - qb0;
            if (d0 - 15 >= D || d0 + 63 <= -D) {
                const float b = d0 > 0 ? b_hi : b_lo;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[t][r] = fmaf(sc[t][r], scale, b);
            } else {
                const int dl = d0 + 4 * g - l15 + D;     // the table index of (t, r) = (0, 0), in front of the clamp to [0, 2 D]
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        int idx = dl + 16 * t + r;
                        idx = idx < 0 ? 0 : (idx > 2 * D ? 2 * D : idx);
                        sc[t][r] = fmaf(sc[t][r], scale, sB[idx]);
                    }
            }
            attn_mask_causal<MQ_MASK_NONE>(sc, kt, nkt, g, q, qb0, len);     // (the ragged last tile: keys past the sequence)
            attn_softmax_step<NDT>(sc, m_run, l_run, o, 1.44269504088896340736f);
            attn_pv_tile<RB, NDT, NC - 1>(sV, kt, cb, vkey, vcol, vhalf, sc, o);
        }
    }
    if (!active) return;     // (after the last barrier)
    const float inv = attn_inv_denominator(l_run);
    if (q < len) attn_store_bf16<NDT>(out + (int64_t)(row0 + q) * inner + h * HD + 4 * g, o, inv);
}

template <int HD>
int launch_relbias(const void* d_qkv, void* d_out, const int32_t* d_cu, int64_t nseq, int fixed_len, int heads, int nslices, int kpad, const float* d_rel_bias,
                   int D, float scale, hipStream_t s) {
    const size_t lds = (size_t)kpad * HD * 4 + (size_t)(2 * D + 1) * 4;
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)attention_relbias_kernel<HD>, lds, RB_LDS_MOST, done, "mq_attention_relbias");
    if (rc != MQ_OK) return rc;
    hipLaunchKernelGGL((attention_relbias_kernel<HD>), dim3((unsigned)(nseq * heads * nslices)), dim3(RB_NW * 64), lds, s, (const bf16_t*)d_qkv, (bf16_t*)d_out,
                       d_cu, fixed_len, heads, nslices, kpad, d_rel_bias, D, scale);
    return MQ_OK;
}

}  // namespace

// d_qkv bf16 [rows, 3 inner] = (q | k | v), inner = heads head_dim, head h of each third at columns h head_dim ..; d_out bf16 [rows, inner]; d_rel_bias fp32
// [heads][2 max_distance + 1], entry (h, d + max_distance) = the bias of key - query == d, the two ends standing for everything beyond; sequences packed
// (d_cu_seqlens int32 [nseq + 1]; max_len = the longest) or fixed_len > 0 (d_cu_seqlens NULL ok).
extern "C" int mq_attention_relbias(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t heads,
                                    int32_t head_dim, const float* d_rel_bias, int32_t max_distance, float scale, void* stream) {
    ATTN_ARG_PTRS("mq_attention_relbias", d_qkv, d_out);
    MQ_CHECK_ARG(d_rel_bias, "mq_attention_relbias: null bias table");
    MQ_CHECK_ARG(head_dim == 64 || head_dim == 128, "mq_attention_relbias: head_dim %d unsupported (64 or 128)", head_dim);
    MQ_CHECK_ARG(heads >= 1 && heads <= 1024, "mq_attention_relbias: heads %d outside [1, 1024]", heads);
    MQ_CHECK_ARG(max_distance >= 1 && max_distance <= RB_MAX_D, "mq_attention_relbias: max_distance %d outside [1, %d]", max_distance, RB_MAX_D);
    MQ_CHECK_ARG(scale > 0.f && scale <= 1e6f, "mq_attention_relbias: scale %g must be positive and finite", (double)scale);
    ATTN_ARG_SEQS("mq_attention_relbias", fixed_len, d_cu_seqlens);
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    ATTN_ARG_MAXL("mq_attention_relbias", maxl);
    const int nslices = (maxl + RB_SLICE - 1) / RB_SLICE;
    ATTN_ARG_GRID("mq_attention_relbias", nseq * heads * nslices);
    const int kpad = attn_kpad(maxl, rb_lds_keys(head_dim));
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(2, s);
    const int rc = head_dim == 64 ? launch_relbias<64>(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, heads, nslices, kpad, d_rel_bias, max_distance, scale, s)
                                  : launch_relbias<128>(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, heads, nslices, kpad, d_rel_bias, max_distance, scale, s);
    if (rc != MQ_OK) return rc;
    MQ_CHECK_LAUNCH("mq_attention_relbias");
    return MQ_OK;
}
