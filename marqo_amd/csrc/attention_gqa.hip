// Grouped-query attention of the decoder-style embedders (Qwen3-Embedding, gte-Qwen2: transformers Qwen3Model / Qwen2Model): q_heads query heads read
// kv_heads K/V heads, query head h reads K/V head h / G with G = q_heads / kv_heads (transformers' repeat_kv: consecutive query heads share), causal or
// unmasked, bf16, 64- or 128-wide heads, packed or fixed-length sequences.
//
// The pieces are those of attention.hip — K and V row-major in LDS by LDS-DMA with the 16-B chunks XOR-swizzled by (key & (NC - 1)), S^T = K . Q^T and
// O^T = V^T . P^T on v_mfma_f32_16x16x32_bf16, V^T through ds_read_b64_tr_b16, the online softmax over 64-key tiles in the swapped-operand form — what
// differs is the work split:
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
#include "common.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));

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
    constexpr int RPP = 1024 / RB;   // rows per 1-KiB LDS-DMA piece (8 or 4)
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

    // ---- stage K and V of piece c: RPP rows x RB bytes per LDS-DMA; lane -> (row = RPP piece + lane / NC, physical chunk = lane % NC) fetches the
    // logical chunk that lives there.  Rows past the sequence re-read its last row (finite values; their scores are masked).
    auto stage = [&](int c) {
        const int base = (c * tpc) << 6;       // first key of the piece: a multiple of 64, so LDS row & (NC - 1) == key & (NC - 1)
        const int tiles_here = skt - c * tpc < tpc ? skt - c * tpc : tpc;
        const int np8 = (tiles_here << 6) / RPP;
        const int srow = lane / NC, pchunk = lane % NC;
        for (int p = wave; p < 2 * np8; p += GQA_NW) {
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
    if (nchunks == 1) {
        stage(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    const int l15 = lane & 15, g = lane >> 4;
    // per-lane constants of the V^T transpose reads: source lane (g, l15) fetches 4 consecutive d of key 4g + l15/4
    const int vkey = 4 * g + (l15 >> 2);
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
                // ---- S^T tile: keys 64kt + 16t + 4g + r for this lane's query -----------------------
                f32x4 sc[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const int key = kt * 64 + t * 16 + l15;  // A-operand row
#pragma unroll
                    for (int kk = 0; kk < NKK; ++kk) {
                        const bf16x8 kf = *(const bf16x8*)(sK + (key - cb) * RB + (((g + 4 * kk) ^ (key & (NC - 1))) << 4));
                        sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], sc[t], 0, 0, 0);
                    }
                }
                // masking is needed only on the ragged last tile and (causal) on tiles that reach past the block's first query: a wave-uniform test
                bool need_mask = (kt == nkt - 1) && (len & 63);
                if (MASK == MQ_MASK_CAUSAL) need_mask = need_mask || (kt * 64 + 63 > qb0);
                if (need_mask) {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int key = kt * 64 + t * 16 + g * 4 + r;
                            bool valid = key < len;
                            if (MASK == MQ_MASK_CAUSAL) valid = valid && (key <= q);
                            sc[t][r] = valid ? sc[t][r] : -INFINITY;
                        }
                }
                // running max on the RAW scores (the softmax scale is positive); scale and shift fold into one FMA per element
                float mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])), fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
                mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(sc[2][0], sc[2][1]), fmaxf(sc[2][2], sc[2][3])), fmaxf(fmaxf(sc[3][0], sc[3][1]), fmaxf(sc[3][2], sc[3][3]))));
                mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float m_new = fmaxf(m_run, mx);   // finite: every query sees at least key 0, in the first tile it visits
                const float neg_mc = -m_new * scale_log2e;
                float psum = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        sc[t][r] = __builtin_amdgcn_exp2f(fmaf(sc[t][r], scale_log2e, neg_mc));
                        psum += sc[t][r];
                    }
                if (__any(m_new != m_run)) {  // rescale only when some query's running max moved
                    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2e);
                    l_run *= alpha;
#pragma unroll
                    for (int dt = 0; dt < NDT; ++dt) o[dt] *= alpha;
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
                    for (int dt = 0; dt < NDT; ++dt) {
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
        }  // pieces
        if (!active) continue;
        float l_tot = l_run + __shfl_xor(l_run, 16, 64);
        l_tot += __shfl_xor(l_tot, 32, 64);
        const float inv = 1.0f / l_tot;
        if (q < len) {
            bf16_t* orow = out + (int64_t)(row0 + q) * ldo + h * HD + 4 * g;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                uint2 p;
                p.x = pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv);
                p.y = pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv);
                *(uint2*)(orow + dt * 16) = p;
            }
        }
    }
}

template <int MASK, int HD>
int launch_gqa(const void* d_qkv, void* d_out, const int32_t* d_cu, int64_t nseq, int fixed_len, int q_heads, int kv_heads, int nslices, int kpad,
               hipStream_t s) {
    const size_t lds = (size_t)kpad * HD * 4;
    if (lds > 64 * 1024) {
        // `lds` varies from call to call and the opt-in is latched once per device: it is made for the most the kernel ever asks for (160 KiB), so a
        // call with short sequences in front of one with long sequences leaves the limit where the long one needs it
        static std::atomic<uint64_t> done{0};
        hipError_t e = mq_ensure_dyn_lds((const void*)attention_gqa_kernel<MASK, HD>, 160 * 1024, done);
        if (e != hipSuccess) { mq_set_error("mq_attention_gqa: hipFuncSetAttribute: %s", hipGetErrorString(e)); return MQ_ERR_HIP; }
    }
    const float scale_log2e = 1.44269504088896340736f / sqrtf((float)HD);   // 1 / sqrt(head dim) * log2(e)
    hipLaunchKernelGGL((attention_gqa_kernel<MASK, HD>), dim3((unsigned)(nseq * kv_heads * nslices)), dim3(GQA_NW * 64), lds, s, (const bf16_t*)d_qkv,
                       (bf16_t*)d_out, d_cu, fixed_len, q_heads, kv_heads, nslices, kpad, scale_log2e);
    return MQ_OK;
}

}  // namespace

// d_qkv bf16 [rows, (q_heads + 2 kv_heads) head_dim] = (q | k | v), head h of each part at columns h head_dim ..; d_out bf16 [rows, q_heads head_dim];
// sequences packed (d_cu_seqlens int32 [nseq + 1]; max_len = the longest) or fixed_len > 0 (d_cu_seqlens NULL ok).
extern "C" int mq_attention_gqa(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len,
                                int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t mask, void* stream) {
    MQ_CHECK_ARG(d_qkv && d_out, "mq_attention_gqa: null pointer");
    MQ_CHECK_ARG(head_dim == 64 || head_dim == 128, "mq_attention_gqa: head_dim %d unsupported (64 or 128)", head_dim);
    MQ_CHECK_ARG(q_heads >= 1 && kv_heads >= 1 && q_heads <= 1024 && q_heads % kv_heads == 0,
                 "mq_attention_gqa: q_heads %d must be a multiple of kv_heads %d (1..1024 query heads)", q_heads, kv_heads);
    MQ_CHECK_ARG(mask == MQ_MASK_NONE || mask == MQ_MASK_CAUSAL, "mq_attention_gqa: mask %d unsupported (MQ_MASK_NONE or MQ_MASK_CAUSAL)", mask);
    MQ_CHECK_ARG(fixed_len > 0 || d_cu_seqlens, "mq_attention_gqa: need fixed_len or cu_seqlens");
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    MQ_CHECK_ARG(maxl >= 1 && maxl <= 8192, "mq_attention_gqa: max sequence length %d unsupported (1..8192)", maxl);
    const int nslices = (maxl + GQA_SLICE - 1) / GQA_SLICE;
    MQ_CHECK_ARG(nseq * kv_heads * nslices < (1LL << 31), "mq_attention_gqa: grid too large");
    // K + V rows of head_dim bf16 each live in the CU's 160 KiB of LDS: 640 keys (head_dim 64) / 320 keys (128); what a slice needs beyond that streams
    const int cap = head_dim == 64 ? 640 : 320;
    const int need = ((maxl + 63) / 64) * 64;
    const int kpad = need < cap ? need : cap;
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
