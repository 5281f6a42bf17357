// Bidirectional attention with an ALiBi bias, the attention of the JinaBERT encoders (jina-embeddings-v2-small-en / -base-en and MosaicBERT-style ALiBi
// encoders with the same block): bf16, 64-wide heads, packed or fixed-length sequences,
//
//   scores[q, k] = fmaf(q . k, scale, -slopes[h] * |k - q|)          out = softmax(scores) V
//
// Unmasked: EVERY key of the sequence contributes, however steep the head (no tile is skipped because its probabilities would be negligible).  The
// slopes are the caller's (fp32 [heads]); how they are derived is not this file's business.
//
// The tile math is attention_core.h's (chunks swizzled by key & (NC - 1), bf16 P / fp32 normaliser); the work split is attention_relbias.hip's: a
// sequence's queries are split into SLICES of 64 (four 16-query blocks, one per wave), one workgroup of 4 wave64s per (sequence, head, slice) stages the
// head's K and V — the whole sequence when it fits the LDS, else in pieces of kpad keys — and each wave runs its block over every key tile.  Every slice
// stages the sequence's K / V again (from L2 after the first); throughput was not part of the work that added this kernel.  What is this file's own:
//
//   - The bias lives in registers: no table, no global or LDS read per pair.  The distance of element (t, r) of a 64-key tile from the lane's query is
//     d0 + 16 t + 4 g + r - l15 with d0 = 64 kt - qb0: an integer the lane already has.  The lane keeps dl = d0 + 4 g - l15 as a float (exact: below
//     2^24), adds the compile-time 16 t + r (exact), multiplies by the slope — ONE rounding, the product of the formula above — and the score is the FMA.
//   - A tile that lies wholly on one side of the wave's 16 queries (d0 - 15 >= 0 or d0 + 63 <= 0: a wave-uniform test) has a uniform sign: the sign rides
//     in the slope and nothing takes an absolute value.  Only the tiles that cut the diagonal — at most two per block — form |.|.  Both paths form the
//     same product, so a score's bits do not depend on the path.
//   - The slope is one float per workgroup, read through the kernel's const pointer (a scalar load).
//   - LDS: K + V at 2 HD bytes per key each and nothing else: 160 KiB / 256 B = 640 keys at 64-wide heads, the image of the bias-free kernels (the
//     relative-bias kernel gives one tile of it to its table).  Longer sequences stream through in pieces.
//
// Compiler report (gfx950, -O3, resource remarks), 4 waves per workgroup, slice 64:
//   attention_alibi_kernel<64>:  92 VGPRs + 20 AGPRs, 88 SGPRs, no VGPR / SGPR spill, no scratch, no static LDS, 4 waves / SIMD by registers
// The compiler forms the 16 biases of a tile with packed fp32 adds / multiplies / FMAs (8 of each); packed operands take no |.| modifier, so the
// diagonal path pays 16 more v_and_b32 per tile than the uniform one — that, not the branch, is what the split saves.  As at the relative-bias kernel,
// from 129 keys on the image (>= 96 KiB) leaves one workgroup per CU whatever the registers allow; no occupancy request was tried or measured.
#include "attention_core.h"

namespace {

constexpr int AL_NW = 4;               // wave64s per workgroup = 16-query blocks per slice
constexpr int AL_SLICE = AL_NW * 16;   // queries per workgroup: one 64-key tile's worth
constexpr size_t AL_LDS_MOST = 160 * 1024;

// keys of K + V the LDS holds, in whole 64-key tiles
constexpr int al_lds_keys(int hd) { return (int)(AL_LDS_MOST / ((size_t)hd * 4) / 64) * 64; }
static_assert(al_lds_keys(64) == 640, "LDS budget of the K / V image");

template <int HD>
__global__ __launch_bounds__(AL_NW * 64) void attention_alibi_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                     int fixed_len, int heads, int nslices, int kpad, const float* __restrict__ slopes,
                                                                     float scale) {
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
    const int q0 = slice * AL_SLICE;
    if (len <= 0 || q0 >= len) return;     // (the whole workgroup: no barrier has been reached)
    const int inner = heads * HD, ld = 3 * inner;
    const bf16_t* qb = qkv + (int64_t)row0 * ld + h * HD;
    const bf16_t* kb = qb + inner;
    const bf16_t* vb = qb + 2 * inner;
    const int nkt = (len + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float slope = slopes[h];         // (h is workgroup-uniform: a scalar load)

    // the sequence's key tiles pass through the LDS in nchunks pieces of tpc tiles (one piece when they fit)
    const int tpc = kpad >> 6;
    const int nchunks = (nkt + tpc - 1) / tpc;
    auto stage = [&](int c) {
        const int tiles_here = nkt - c * tpc < tpc ? nkt - c * tpc : tpc;
        attn_stage_piece<RB, NC, NC - 1, AL_NW>(sK, sV, kb, vb, ld, (c * tpc) << 6, tiles_here << 6, len, lane, wave);
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
            // score = scale * (q . k) - slope * |key - q|: key - q = d0 + 16 t + 4 g + r - l15 lies in [d0 - 15, d0 + 63] for the whole block
            const int d0 = kt * 64 - qb0;
            const float dl = (float)(d0 + 4 * g - l15);     // the distance of (t, r) = (0, 0), signed; |.| <= 8192 + 63: exact
            if (d0 - 15 >= 0 || d0 + 63 <= 0) {
                const float sl = d0 > 0 ? -slope : slope;   // the sign of the whole tile rides in the slope
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[t][r] = fmaf(sc[t][r], scale, sl * (dl + (float)(16 * t + r)));
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[t][r] = fmaf(sc[t][r], scale, -slope * fabsf(dl + (float)(16 * t + r)));
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
int launch_alibi(const void* d_qkv, void* d_out, const int32_t* d_cu, int64_t nseq, int fixed_len, int heads, int nslices, int kpad, const float* d_slopes,
                 float scale, hipStream_t s) {
    const size_t lds = (size_t)kpad * HD * 4;
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)attention_alibi_kernel<HD>, lds, AL_LDS_MOST, done, "mq_attention_alibi");
    if (rc != MQ_OK) return rc;
    hipLaunchKernelGGL((attention_alibi_kernel<HD>), dim3((unsigned)(nseq * heads * nslices)), dim3(AL_NW * 64), lds, s, (const bf16_t*)d_qkv, (bf16_t*)d_out,
                       d_cu, fixed_len, heads, nslices, kpad, d_slopes, scale);
    return MQ_OK;
}

}  // namespace

// d_qkv bf16 [rows, 3 inner] = (q | k | v), inner = heads head_dim, head h of each third at columns h head_dim ..; d_out bf16 [rows, inner]; d_slopes fp32
// [heads], head h's score bias is -d_slopes[h] * |key - query|; sequences packed (d_cu_seqlens int32 [nseq + 1]; max_len = the longest) or
// fixed_len > 0 (d_cu_seqlens NULL ok).
extern "C" int mq_attention_alibi(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t heads,
                                  int32_t head_dim, const float* d_slopes, float scale, void* stream) {
    ATTN_ARG_PTRS("mq_attention_alibi", d_qkv, d_out);
    MQ_CHECK_ARG(d_slopes, "mq_attention_alibi: null slopes");
    MQ_CHECK_ARG(head_dim == 64, "mq_attention_alibi: head_dim %d unsupported (64: the head width of the JinaBERT checkpoints)", head_dim);
    MQ_CHECK_ARG(heads >= 1 && heads <= 1024, "mq_attention_alibi: heads %d outside [1, 1024]", heads);
    MQ_CHECK_ARG(scale > 0.f && scale <= 1e6f, "mq_attention_alibi: scale %g must be positive and finite", (double)scale);
    ATTN_ARG_SEQS("mq_attention_alibi", fixed_len, d_cu_seqlens);
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    ATTN_ARG_MAXL("mq_attention_alibi", maxl);
    const int nslices = (maxl + AL_SLICE - 1) / AL_SLICE;
    ATTN_ARG_GRID("mq_attention_alibi", nseq * heads * nslices);
    const int kpad = attn_kpad(maxl, al_lds_keys(head_dim));
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(2, s);
    const int rc = launch_alibi<64>(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, heads, nslices, kpad, d_slopes, scale, s);
    if (rc != MQ_OK) return rc;
    MQ_CHECK_LAUNCH("mq_attention_alibi");
    return MQ_OK;
}
