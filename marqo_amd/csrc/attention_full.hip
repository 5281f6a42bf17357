// Plain bidirectional attention split over query slices, the attention of the NomicBERT encoders (nomic-embed-text-v1 / -v1.5 / -v1-unsupervised,
// snowflake-arctic-embed-m-long: up to 8192 tokens): bf16, 64-wide heads, packed or fixed-length sequences,
//
//   out = softmax(scale * (q . k)) V                                  every key of the sequence contributes; no bias, no band, no mask
//
// mq_attention (attention.hip) computes the same function with one workgroup per (sequence, head): built for T <= 512, it leaves a single long document
// on `heads` of the chip's 256 CUs and re-stages the K / V image once per round of query blocks.  Here the tile math is attention_core.h's (chunks
// swizzled by key & (NC - 1), bf16 P / fp32 normaliser) and the work split is attention_alibi.hip's: a sequence's queries are split into SLICES of 64
// (four 16-query blocks, one per wave), one workgroup of 4 wave64s per (sequence, head, slice) stages the head's K and V by LDS-DMA — the whole sequence
// when it fits the LDS, else in pieces of kpad keys — and each wave runs its block over every key tile.  Every slice stages the sequence's K / V again
// (from L2 after the first).  What differs from the ALiBi kernel:
//
//   - No slopes pointer, no distance, no per-score arithmetic between the score MFMAs and the softmax: the scores stay raw and the softmax scale folds
//     into the one FMA per element of attn_softmax_step (scale * log2(e), as mq_attention does).  The running max is taken on the raw scores, which is
//     the same query's max because scale > 0 (the entry point refuses anything else).
//   - LDS: K + V at 2 HD bytes per key each and nothing else: 160 KiB / 256 B = 640 keys at 64-wide heads.  Longer sequences stream through in pieces.
//
// Bounds (read before running): blockIdx.x < nseq * heads * nslices; a workgroup whose slice starts past its sequence returns before any barrier; staging
// clamps every source row to len - 1 and writes LDS rows [0, tiles_here * 64) with tiles_here <= kpad / 64; a wave visits only tiles kt < nkt of the
// piece that is resident, so LDS row key - cb lies in [0, kpad); Q rows are clamped to len - 1 and only q < len is stored.
//
// Compiler report (gfx950, -O3, resource remarks), 4 waves per workgroup, slice 64:
//   attention_full_kernel<64>:  72 VGPRs + 17 AGPRs, 76 SGPRs, no VGPR / SGPR spill, no scratch, no static LDS (dynamic: 256 B per key of the image, at
//                               most 160 KiB), 5 waves / SIMD by registers                (the ALiBi kernel: 92 + 20, 88, 4 waves)
// From 129 keys on the image (>= 96 KiB of the CU's 160 KiB) leaves one workgroup per CU whatever the registers allow; no occupancy request was tried.
#include "attention_core.h"

namespace {

constexpr int FA_NW = 4;               // wave64s per workgroup = 16-query blocks per slice
constexpr int FA_SLICE = FA_NW * 16;   // queries per workgroup: one 64-key tile's worth
constexpr size_t FA_LDS_MOST = 160 * 1024;

// keys of K + V the LDS holds, in whole 64-key tiles
constexpr int fa_lds_keys(int hd) { return (int)(FA_LDS_MOST / ((size_t)hd * 4) / 64) * 64; }
static_assert(fa_lds_keys(64) == 640, "LDS budget of the K / V image");

template <int HD>
__global__ __launch_bounds__(FA_NW * 64) void attention_full_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                    int fixed_len, int heads, int nslices, int kpad, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = HD * 2;       // bytes per K / V row in LDS
    constexpr int NC = HD / 8;       // 16-byte chunk slots per LDS row
    constexpr int NKK = HD / 32;     // 32-deep MFMA k-chunks of a Q.K dot product
    constexpr int NDT = HD / 16;     // 16-wide output-dim tiles
    char* sK = smem;                                         // [kpad][RB], 16-B chunks XOR-swizzled by (key & (NC - 1))
    char* sV = smem + (size_t)kpad * RB;                     // [kpad][RB], same image

    const unsigned sh = blockIdx.x / (unsigned)nslices;
    const int slice = (int)(blockIdx.x - sh * (unsigned)nslices);
    const int seq = sh / heads, h = sh - seq * heads;
    int row0, len;
    if (fixed_len > 0) { row0 = seq * fixed_len; len = fixed_len; }
    else { row0 = cu[seq]; len = cu[seq + 1] - row0; }
    const int q0 = slice * FA_SLICE;
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
        attn_stage_piece<RB, NC, NC - 1, FA_NW>(sK, sV, kb, vb, ld, (c * tpc) << 6, tiles_here << 6, len, lane, wave);
    };

    const int l15 = lane & 15, g = lane >> 4;
    const int qb0 = q0 + wave * 16;             // this wave's 16-query block
    const bool active = qb0 < len;              // wave-uniform; an idle wave still stages and keeps the barriers
    const int q = qb0 + l15;                    // this lane's query (B-operand column / output row)

    stage(0);
    // Q fragments (dims 32 kk + 8 g .. + 7 of query row q, clamped to the sequence) are fetched while the K / V DMA is in flight
    bf16x8 qf[NKK];
    {
        const int qr = q < len ? q : len - 1;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) qf[kk] = *(const bf16x8*)(qb + (int64_t)qr * ld + 8 * g + 32 * kk);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const int vkey = 4 * g + (l15 >> 2);    // per-lane constants of the V^T transpose reads
    const int vcol = (l15 & 3) >> 1, vhalf = (l15 & 1) << 3;

    float m_run = -1e30f, l_run = 0.f;
    f32x4 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < nchunks; ++c) {
        if (c > 0) {   // refill the LDS with the next piece of the sequence
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
            attn_mask_causal<MQ_MASK_NONE>(sc, kt, nkt, g, q, qb0, len);     // (the ragged last tile: keys past the sequence)
            attn_softmax_step<NDT>(sc, m_run, l_run, o, scale_log2e);        // (every query sees key 64 kt of every tile it visits: kt < nkt)
            attn_pv_tile<RB, NDT, NC - 1>(sV, kt, cb, vkey, vcol, vhalf, sc, o);
        }
    }
    if (!active) return;     // (after the last barrier)
    const float inv = attn_inv_denominator(l_run);
    if (q < len) attn_store_bf16<NDT>(out + (int64_t)(row0 + q) * inner + h * HD + 4 * g, o, inv);
}

template <int HD>
int launch_full(const void* d_qkv, void* d_out, const int32_t* d_cu, int64_t nseq, int fixed_len, int heads, int nslices, int kpad, float scale,
                hipStream_t s) {
    const size_t lds = (size_t)kpad * HD * 4;
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)attention_full_kernel<HD>, lds, FA_LDS_MOST, done, "mq_attention_full");
    if (rc != MQ_OK) return rc;
    hipLaunchKernelGGL((attention_full_kernel<HD>), dim3((unsigned)(nseq * heads * nslices)), dim3(FA_NW * 64), lds, s, (const bf16_t*)d_qkv, (bf16_t*)d_out,
                       d_cu, fixed_len, heads, nslices, kpad, 1.44269504088896340736f * scale);
    return MQ_OK;
}

}  // namespace

// d_qkv bf16 [rows, 3 inner] = (q | k | v), inner = heads head_dim, head h of each third at columns h head_dim ..; d_out bf16 [rows, inner]; sequences
// packed (d_cu_seqlens int32 [nseq + 1]; max_len = the longest) or fixed_len > 0 (d_cu_seqlens NULL ok).
extern "C" int mq_attention_full(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t heads,
                                 int32_t head_dim, float scale, void* stream) {
    ATTN_ARG_PTRS("mq_attention_full", d_qkv, d_out);
    MQ_CHECK_ARG(head_dim == 64, "mq_attention_full: head_dim %d unsupported (64: the head width of the NomicBERT checkpoints)", head_dim);
    MQ_CHECK_ARG(heads >= 1 && heads <= 1024, "mq_attention_full: heads %d outside [1, 1024]", heads);
    MQ_CHECK_ARG(scale > 0.f && scale <= 1e6f, "mq_attention_full: scale %g must be positive and finite", (double)scale);
    ATTN_ARG_SEQS("mq_attention_full", fixed_len, d_cu_seqlens);
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    ATTN_ARG_MAXL("mq_attention_full", maxl);
    const int nslices = (maxl + FA_SLICE - 1) / FA_SLICE;
    ATTN_ARG_GRID("mq_attention_full", nseq * heads * nslices);
    const int kpad = attn_kpad(maxl, fa_lds_keys(head_dim));
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(2, s);
    const int rc = launch_full<64>(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, heads, nslices, kpad, scale, s);
    if (rc != MQ_OK) return rc;
    MQ_CHECK_LAUNCH("mq_attention_full");
    return MQ_OK;
}
