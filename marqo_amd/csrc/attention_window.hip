// Sliding-window (band) attention of the ModernBERT local layers: query i attends the keys j of its own sequence with |i - j| <= half_window
// (inclusive on both sides, no causal mask, no bias; bf16, 64-wide heads; packed or fixed-length sequences).
//
// A band kernel, not a mask over full attention.  The tile math is attention_core.h's (128-byte LDS rows, chunks swizzled by key & 7); what is this
// file's own is WHICH keys a workgroup stages and which tiles a query block visits:
//
//   - A sequence's queries are split into SLICES of 64 (four 16-query blocks, one per wave).  One workgroup per (sequence, head, slice).
//   - The workgroup stages only the 64-key tiles its slice can reach: tiles floor((q0 - hw) / 64) .. floor((q_last + hw) / 64), clipped to the sequence
//     — the slice's own tile plus a halo of ceil(hw / 64) tiles on either side (hw = 64: 3 tiles = 48 KiB of LDS, three workgroups per CU).  A sliding
//     layer at T tokens therefore reads O(T * window) keys, not O(T^2).  A band wider than the LDS holds (more than 640 keys: hw > 256) goes through
//     it in pieces of 640 keys.
//   - A 16-query block visits only the tiles that intersect ITS band, floor((16 b - hw) / 64) .. floor((16 b + 15 + hw) / 64).
//   - A tile cut by the band's edge (or by the end of the sequence) masks per key; a tile inside the band of all 16 queries takes the unmasked path.
#include "attention_core.h"

namespace {

constexpr int WIN_NW = 4;             // wave64s per workgroup = 16-query blocks per slice
constexpr int WIN_SLICE = WIN_NW * 16;  // queries per workgroup: one 64-key tile's worth, so a slice starts on a tile boundary
constexpr int WIN_LDS_KEYS = 640;     // K + V rows of 128 B each: 640 keys = 160 KiB

__global__ __launch_bounds__(WIN_NW * 64) void attention_window_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                        int fixed_len, int W, int heads, int nslices, int kpad, int hw, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = 128;   // bytes per K / V row in LDS
    constexpr int NC = 8;     // 16-byte chunk slots per row
    constexpr int SWZ = 7;    // chunk c of key k lives in slot c ^ (k & 7)
    char* sK = smem;                      // [kpad][RB]
    char* sV = smem + (size_t)kpad * RB;  // [kpad][RB], same image

    const unsigned sh = blockIdx.x / (unsigned)nslices;
    const int slice = (int)(blockIdx.x - sh * (unsigned)nslices);
    const int seq = sh / heads, h = sh - seq * heads;
    int row0, len;
    if (fixed_len > 0) { row0 = seq * fixed_len; len = fixed_len; }
    else { row0 = cu[seq]; len = cu[seq + 1] - row0; }
    const int q0 = slice * WIN_SLICE;
    if (len <= 0 || q0 >= len) return;     // (the whole workgroup: no barrier has been reached)
    const int ld = 3 * W;
    const bf16_t* qb = qkv + (int64_t)row0 * ld + h * 64;
    const bf16_t* kb = qb + W;
    const bf16_t* vb = qb + 2 * W;
    const int nkt = (len + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // key tiles [kt_lo, kt_hi) the slice's band reaches; they pass through the LDS in nchunks pieces of tpc tiles (one piece when they fit)
    const int q_last = q0 + WIN_SLICE - 1 < len - 1 ? q0 + WIN_SLICE - 1 : len - 1;
    const int kt_lo = (q0 - hw > 0 ? q0 - hw : 0) >> 6;
    const int kt_hi = (((q_last + hw) >> 6) < nkt - 1 ? ((q_last + hw) >> 6) : nkt - 1) + 1;
    const int tpc = kpad >> 6;
    const int nchunks = (kt_hi - kt_lo + tpc - 1) / tpc;
    auto stage = [&](int c) {
        const int tiles_here = kt_hi - (kt_lo + c * tpc) < tpc ? kt_hi - (kt_lo + c * tpc) : tpc;
        attn_stage_piece<RB, NC, SWZ, WIN_NW>(sK, sV, kb, vb, ld, (kt_lo + c * tpc) << 6, tiles_here << 6, len, lane, wave);
    };

    const int l15 = lane & 15, g = lane >> 4;
    const int qblk = slice * WIN_NW + wave;     // this wave's 16-query block (index in the sequence)
    const int qb0 = qblk * 16;
    const bool active = qb0 < len;              // wave-uniform; an idle wave still stages and keeps the barriers
    const int q = qb0 + l15;                    // this lane's query (B-operand column / output row)
    // the block's own band, in tiles
    int bk_lo = 0, bk_hi = 0;
    if (active) {
        const int ql = qb0 + 15 < len - 1 ? qb0 + 15 : len - 1;
        bk_lo = (qb0 - hw > 0 ? qb0 - hw : 0) >> 6;
        bk_hi = (((ql + hw) >> 6) < nkt - 1 ? ((ql + hw) >> 6) : nkt - 1) + 1;
    }

    stage(0);
    // Q fragments (dims 32 kk + 8 g .. + 7 of query row q, clamped to the sequence) are fetched while the K / V DMA is in flight
    bf16x8 qf[2];
    {
        const int qr = q < len ? q : len - 1;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) qf[kk] = *(const bf16x8*)(qb + (int64_t)qr * ld + 8 * g + 32 * kk);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const int vkey = 4 * g + (l15 >> 2);    // per-lane constants of the V^T transpose reads
    const int vcol = (l15 & 3) >> 1, vhalf = (l15 & 1) << 3;

    float m_run = -1e30f, l_run = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < nchunks; ++c) {
        if (c > 0) {   // refill the LDS with the next piece of the band
            __syncthreads();
            stage(c);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        const int ct0 = kt_lo + c * tpc;
        const int ct1 = ct0 + tpc < kt_hi ? ct0 + tpc : kt_hi;
        const int t0 = bk_lo > ct0 ? bk_lo : ct0;
        const int t1 = bk_hi < ct1 ? bk_hi : ct1;
        const int cb = ct0 << 6;                         // LDS row of global key `key` is key - cb
        for (int kt = t0; kt < t1; ++kt) {
            f32x4 sc[4];
            attn_score_tile<RB, 2, SWZ>(sK, kt, cb, l15, g, qf, sc);
            attn_mask_band(sc, kt, g, q, qb0, hw, len);
            attn_softmax_step<4>(sc, m_run, l_run, o, scale_log2e);
            attn_pv_tile<RB, 4, SWZ>(sV, kt, cb, vkey, vcol, vhalf, sc, o);
        }
    }
    if (!active) return;     // (after the last barrier)
    const float inv = attn_inv_denominator(l_run);
    if (q < len) attn_store_bf16<4>(out + (int64_t)(row0 + q) * W + h * 64 + 4 * g, o, inv);
}

}  // namespace

// d_qkv bf16 [rows, 3W] (columns q | k | v, head h owns columns 64h .. 64h + 63 of each third), d_out bf16 [rows, W]; sequences packed (d_cu_seqlens int32
// [nseq + 1]; max_len = the longest) or fixed_len > 0 (d_cu_seqlens NULL ok).  half_window >= 0: query i sees keys i - half_window .. i + half_window of
// its sequence.  A window that covers every sequence whole (half_window >= max_len - 1) IS full attention and runs mq_attention's kernel.
extern "C" int mq_attention_window(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t W,
                                   int32_t heads, int32_t half_window, void* stream) {
    ATTN_ARG_PTRS("mq_attention_window", d_qkv, d_out);
    MQ_CHECK_ARG(heads >= 1 && W == heads * 64, "mq_attention_window: 64-wide heads only (W=%d heads=%d)", W, heads);
    ATTN_ARG_SEQS("mq_attention_window", fixed_len, d_cu_seqlens);
    MQ_CHECK_ARG(half_window >= 0, "mq_attention_window: half_window %d < 0", half_window);
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    ATTN_ARG_MAXL("mq_attention_window", maxl);
    if (half_window >= maxl - 1) return mq_attention(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, max_len, W, heads, MQ_MASK_NONE, stream);
    const int nslices = (maxl + WIN_SLICE - 1) / WIN_SLICE;
    ATTN_ARG_GRID("mq_attention_window", nseq * heads * nslices);
    const int kpad = attn_band_kpad(half_window, maxl, WIN_LDS_KEYS);
    const size_t lds = (size_t)kpad * 128 * 2;
    hipStream_t s = (hipStream_t)stream;
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)attention_window_kernel, lds, WIN_LDS_KEYS * 128 * 2, done, "mq_attention_window");
    if (rc != MQ_OK) return rc;
    MqProfScope prof(2, s);
    const float scale_log2e = 1.44269504088896340736f / 8.0f;   // 1 / sqrt(64) * log2(e)
    hipLaunchKernelGGL(attention_window_kernel, dim3((unsigned)(nseq * heads * nslices)), dim3(WIN_NW * 64), lds, s, (const bf16_t*)d_qkv, (bf16_t*)d_out,
                       d_cu_seqlens, (int)fixed_len, (int)W, (int)heads, nslices, kpad, (int)half_window, scale_log2e);
    MQ_CHECK_LAUNCH("mq_attention_window");
    return MQ_OK;
}
