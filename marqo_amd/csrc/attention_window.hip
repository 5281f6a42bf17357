// Sliding-window (band) attention of the ModernBERT local layers: query i attends the keys j of its own sequence with |i - j| <= half_window
// (inclusive on both sides, no causal mask, no bias; bf16, 64-wide heads; packed or fixed-length sequences).
//
// A band kernel, not a mask over full attention.  The pieces are those of attention.hip — K and V row-major in LDS by LDS-DMA with the 16-B chunks
// XOR-swizzled by (key & 7), S^T = K . Q^T and O^T = V^T . P^T on v_mfma_f32_16x16x32_bf16, V^T through ds_read_b64_tr_b16, the online softmax
// over 64-key tiles in the swapped-operand form — what differs is WHICH keys a workgroup stages and which tiles a query block visits:
//
//   - A sequence's queries are split into SLICES of 64 (four 16-query blocks, one per wave).  One workgroup per (sequence, head, slice).
//   - The workgroup stages only the 64-key tiles its slice can reach: tiles floor((q0 - hw) / 64) .. floor((q_last + hw) / 64), clipped to the sequence
//     — the slice's own tile plus a halo of ceil(hw / 64) tiles on either side (hw = 64: 3 tiles = 48 KiB of LDS, three workgroups per CU).  A sliding
//     layer at T tokens therefore reads O(T * window) keys, not O(T^2).  A band wider than the LDS holds (more than 640 keys: hw > 256) goes through
//     it in pieces of 640 keys.
//   - A 16-query block visits only the tiles that intersect ITS band, floor((16 b - hw) / 64) .. floor((16 b + 15 + hw) / 64).
//   - A tile cut by the band's edge (or by the end of the sequence) masks per key; a tile inside the band of all 16 queries takes the unmasked path.
#include "common.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int WIN_NW = 4;             // wave64s per workgroup = 16-query blocks per slice
constexpr int WIN_SLICE = WIN_NW * 16;  // queries per workgroup: one 64-key tile's worth, so a slice starts on a tile boundary
constexpr int WIN_LDS_KEYS = 640;     // K + V rows of 128 B each: 640 keys = 160 KiB

__global__ __launch_bounds__(WIN_NW * 64) void attention_window_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                        int fixed_len, int W, int heads, int nslices, int kpad, int hw, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = 128;   // bytes per K / V row in LDS
    constexpr int NC = 8;     // 16-byte chunk slots per row
    constexpr int RPP = 8;    // rows per 1-KiB LDS-DMA piece
    char* sK = smem;                      // [kpad][RB], 16-B chunks XOR-swizzled by (key & 7)
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

    // ---- stage K and V of piece c: 8 rows x 128 bytes per LDS-DMA; lane -> (row = 8 piece + lane / 8, physical chunk = lane % 8) fetches the logical
    // chunk that lives there.  Rows past the sequence re-read its last row (finite values; their scores are masked).
    auto stage = [&](int c) {
        const int base = (kt_lo + c * tpc) << 6;      // first key of the piece: a multiple of 64, so LDS row & 7 == key & 7
        const int tiles_here = kt_hi - (kt_lo + c * tpc) < tpc ? kt_hi - (kt_lo + c * tpc) : tpc;
        const int np8 = (tiles_here << 6) / RPP;
        const int srow = lane / NC, pchunk = lane % NC;
        for (int p = wave; p < 2 * np8; p += WIN_NW) {
            const bool is_v = p >= np8;
            const int piece = is_v ? p - np8 : p;
            const int row = piece * RPP + srow;
            const int key = base + row < len ? base + row : len - 1;
            const int lc = pchunk ^ (row & (NC - 1));
            const bf16_t* src = (is_v ? vb : kb) + (int64_t)key * ld + (lc << 3);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)((is_v ? sV : sK) + piece * 1024), 16, 0, 0);
        }
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

    // per-lane constants of the V^T transpose reads: source lane (g, l15) fetches 4 consecutive d of key 4g + l15/4
    const int vkey = 4 * g + (l15 >> 2);
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
            // ---- S^T tile: keys 64kt + 16t + 4g + r for this lane's query -----------------------
            f32x4 sc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                const int key = kt * 64 + t * 16 + l15;  // A-operand row
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const bf16x8 kf = *(const bf16x8*)(sK + (key - cb) * RB + (((g + 4 * kk) ^ (key & (NC - 1))) << 4));
                    sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], sc[t], 0, 0, 0);
                }
            }
            // a tile wholly inside the band of all 16 queries and inside the sequence skips the per-key compares (a wave-uniform test)
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
            // running max on the RAW scores (the softmax scale is positive); scale and shift fold into one FMA per element.  A query whose band misses
            // this tile keeps m_run (from -1e30): its probabilities here are exp2(-inf) = 0 and alpha = 1
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
                for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
            }
            l_run += psum;
            m_run = m_new;

            // ---- O^T += V^T . P^T over the tile's two 32-key halves (operand layout: attention.hip) --------------------------------
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                union { uint32_t w[4]; bf16x8 v; } pf;
                pf.w[0] = pack_bf16x2(sc[2 * u][0], sc[2 * u][1]);
                pf.w[1] = pack_bf16x2(sc[2 * u][2], sc[2 * u][3]);
                pf.w[2] = pack_bf16x2(sc[2 * u + 1][0], sc[2 * u + 1][1]);
                pf.w[3] = pack_bf16x2(sc[2 * u + 1][2], sc[2 * u + 1][3]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    union { s16x4 t[2]; bf16x8 v; } vf;
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) {
                        const int key = kt * 64 + (2 * u + tt) * 16 + vkey;
                        const char* vp = sV + (key - cb) * RB + ((((dt << 1) | vcol) ^ (key & (NC - 1))) << 4) + vhalf;
                        vf.t[tt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)vp);
                    }
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, pf.v, o[dt], 0, 0, 0);
                }
            }
        }
    }
    if (!active) return;     // (after the last barrier)
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    const float inv = 1.0f / l_tot;
    if (q < len) {
        bf16_t* orow = out + (int64_t)(row0 + q) * W + h * 64 + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            uint2 p;
            p.x = pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv);
            p.y = pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv);
            *(uint2*)(orow + dt * 16) = p;
        }
    }
}

}  // namespace

// d_qkv bf16 [rows, 3W] (columns q | k | v, head h owns columns 64h .. 64h + 63 of each third), d_out bf16 [rows, W]; sequences packed (d_cu_seqlens int32
// [nseq + 1]; max_len = the longest) or fixed_len > 0 (d_cu_seqlens NULL ok).  half_window >= 0: query i sees keys i - half_window .. i + half_window of
// its sequence.  A window that covers every sequence whole (half_window >= max_len - 1) IS full attention and runs mq_attention's kernel.
extern "C" int mq_attention_window(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t W,
                                   int32_t heads, int32_t half_window, void* stream) {
    MQ_CHECK_ARG(d_qkv && d_out, "mq_attention_window: null pointer");
    MQ_CHECK_ARG(heads >= 1 && W == heads * 64, "mq_attention_window: 64-wide heads only (W=%d heads=%d)", W, heads);
    MQ_CHECK_ARG(fixed_len > 0 || d_cu_seqlens, "mq_attention_window: need fixed_len or cu_seqlens");
    MQ_CHECK_ARG(half_window >= 0, "mq_attention_window: half_window %d < 0", half_window);
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    MQ_CHECK_ARG(maxl >= 1 && maxl <= 8192, "mq_attention_window: max sequence length %d unsupported (1..8192)", maxl);
    if (half_window >= maxl - 1) return mq_attention(d_qkv, d_out, d_cu_seqlens, nseq, fixed_len, max_len, W, heads, MQ_MASK_NONE, stream);
    const int nslices = (maxl + WIN_SLICE - 1) / WIN_SLICE;
    MQ_CHECK_ARG(nseq * heads * nslices < (1LL << 31), "mq_attention_window: grid too large");
    // tiles a slice can reach: its own and ceil(hw / 64) on either side, never more than the sequence has
    const int reach = 1 + 2 * ((half_window + 63) / 64), seq_tiles = (maxl + 63) / 64;
    const int need = (reach < seq_tiles ? reach : seq_tiles) * 64;
    const int kpad = need < WIN_LDS_KEYS ? need : WIN_LDS_KEYS;
    const size_t lds = (size_t)kpad * 128 * 2;
    hipStream_t s = (hipStream_t)stream;
    if (lds > 64 * 1024) {
        // `lds` varies from call to call and the opt-in is latched once per device: it is made for the most the kernel ever asks for (640 keys, 160 KiB),
        // so a call with a small band in front of one with a wide band leaves the limit where the wide one needs it
        static std::atomic<uint64_t> done{0};
        hipError_t e = mq_ensure_dyn_lds((const void*)attention_window_kernel, WIN_LDS_KEYS * 128 * 2, done);
        if (e != hipSuccess) { mq_set_error("mq_attention_window: hipFuncSetAttribute: %s", hipGetErrorString(e)); return MQ_ERR_HIP; }
    }
    MqProfScope prof(2, s);
    const float scale_log2e = 1.44269504088896340736f / 8.0f;   // 1 / sqrt(64) * log2(e)
    hipLaunchKernelGGL(attention_window_kernel, dim3((unsigned)(nseq * heads * nslices)), dim3(WIN_NW * 64), lds, s, (const bf16_t*)d_qkv, (bf16_t*)d_out,
                       d_cu_seqlens, (int)fixed_len, (int)W, (int)heads, nslices, kpad, (int)half_window, scale_log2e);
    MQ_CHECK_LAUNCH("mq_attention_window");
    return MQ_OK;
}
