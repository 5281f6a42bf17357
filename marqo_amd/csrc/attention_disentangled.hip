// Bidirectional DISENTANGLED attention, the attention of the DeBERTa-v2 / -v3 encoders (transformers DebertaV2Model with relative_attention and
// pos_att_type c2p | p2c: the mxbai-rerank-*-v1 and cross-encoder/*-deberta-v3-* rerankers): bf16, 64-wide heads, packed or fixed-length sequences,
//
//   scores[q, k] = scale * ( Q_q . K_k  +  Q_q . Kr[h][idx(q - k)]  +  K_k . Qr[h][idx(q - k)] )          out = softmax(scores) V
//
// Kr / Qr (bf16 [heads][2 S][64]) are the projected position tables, idx(d) in [0, 2 S - 1] the bucket of the distance d = query - key.  The bucket
// function is NOT formed here: the caller hands over a table d_idx (int32 [2 reach + 1], entry d + reach = idx(d)) that it built on the host from the
// model's own formula — a ceil(log(.)) re-derived in device arithmetic would move a bucket with one ulp.  Both position terms read the same index; the
// p2c term belongs to the KEY row (K_k . Qr), not the query row.
//
// Two launches, no [T, T] tensor in global memory:
//
//   1. disentangled_strips_kernel (MFMA).  idx is non-decreasing in d, so a call whose longest sequence has maxl tokens reads only the buckets
//      [win_lo, win_hi] = [idx(-(maxl - 1)), idx(maxl - 1)] — the caller passes the two ends (it owns the table).  For every token row and head the
//      pass writes two fp32 STRIPS of winp = win rounded up to 16 values into the workspace:
//        C[row][h][j] = Q_row . Kr[h][win_lo + j]          P[row][h][j] = K_row . Qr[h][win_lo + j]
//      layout [row][head][C | P][winp].  One workgroup of 4 waves per (64 rows, head, C | P); a wave holds its 16 rows as the MFMA's B operand and walks
//      the window 16 table rows at a time (A operand, read from global memory: a head's table is at most 256 KiB and lives in L2), so a lane's 4
//      results are 4 CONSECUTIVE strip values of one row: one 16-byte store.  Position scores are accumulated and stored in fp32: rounded to bf16 they
//      would put an error of 2^-9 |c2p| into the exponent.
//   2. attention_disentangled_kernel.  The work split and tile math of attention_alibi.hip (one workgroup of 4 wave64s per (sequence, head, 64-query
//      slice), K / V through the LDS in pieces of kpad keys, attention_core.h's tile steps).  Behind the K / V image the LDS holds the slice's own part
//      of the index table as int16 strip offsets j = clamp(idx(d) - win_lo, 0, win - 1) for d in [q0 - (len - 1), min(q0 + 63, len - 1)] (at most
//      len + 63 entries, 16.2 KiB at 8192 tokens).  After attn_score_tile a lane reads, per pair, the offset from LDS and the two strip values
//      C[q][j] + P[key][j] from global memory (L2: the strips were just written), adds them to q . k and multiplies by `scale`; softmax and P V are the
//      shared steps.  The clamp of j keeps a table that breaks its contract (not monotone, ends outside the window) inside the strips: wrong scores,
//      no wild read.  Keys past the sequence in the ragged last tile read key len - 1's strip and are masked to -inf afterwards; an idle wave
//      (its 16 queries lie past the sequence) stages, keeps the barriers and visits no tile, as in the siblings.
//
// LDS: 512 keys of K + V (128 KiB) + the offsets (at most 16.2 KiB).  Longer sequences stream through in pieces of 512 keys.
// Workspace: rows * heads * 2 * winp * 4 bytes, winp <= 2 S.  The caller bounds it by calling per GROUP of sequences (csrc/deberta.hip: 256 MiB, a
// constant nobody measured).  Two global gathers per (query, key) pair make this kernel slower than its siblings; throughput was not part of the work
// that added it, and neither the strip pass nor the gather has been profiled.
//
// Compiler report (gfx950, -O3, resource remarks), 4 waves per workgroup:
//   disentangled_strips_kernel:         24 VGPRs + 4 AGPRs, 25 SGPRs, no VGPR / SGPR spill, no scratch, no LDS, 8 waves / SIMD by registers
//   attention_disentangled_kernel<64>:  90 VGPRs + 32 AGPRs, 81 SGPRs, no VGPR / SGPR spill, no scratch, no static LDS, 4 waves / SIMD by registers
// (the LDS image decides the residency of the second: from 129 keys on one workgroup per CU, as in the siblings)
#include "attention_core.h"

namespace {

constexpr int DA_NW = 4;               // wave64s per workgroup = 16-query blocks per slice
constexpr int DA_SLICE = DA_NW * 16;   // queries per workgroup: one 64-key tile's worth
constexpr int DA_MAX_SPAN = 1024;      // largest position_buckets: strips of at most 2048 values
constexpr int DA_LDS_KEYS = 512;       // keys of K + V the LDS holds (128 KiB) next to the slice's index offsets
constexpr size_t DA_LDS_MOST = (size_t)DA_LDS_KEYS * 64 * 4 + (size_t)(8192 + DA_SLICE) * 2;
static_assert(DA_LDS_MOST <= 160 * 1024 && DA_LDS_MOST % 16 == 0, "LDS budget of the K / V image next to the index offsets");

static inline int da_winp(int win) { return (win + 15) & ~15; }
static inline size_t da_strip_bytes(int64_t rows, int heads, int win) { return (size_t)rows * heads * 2 * da_winp(win) * 4; }

// ---- pass 1: the two strips of every (row, head).  grid (ceil(rows / 64), heads, 2); z = 0: C = Q . Kr^T, z = 1: P = K . Qr^T -----------------------------
// Reads: token rows base + [0, rows) of qkv (a row past the call's last is clamped to it and not stored), table rows clamped to [0, 2 span - 1].
// Writes: strips [rows][heads][2][winp], nothing else.
__global__ __launch_bounds__(DA_NW * 64) void disentangled_strips_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ cu, int64_t rows, int heads,
                                                                         const bf16_t* __restrict__ pos_key, const bf16_t* __restrict__ pos_query, int span,
                                                                         int lo, int winp, float* __restrict__ strips) {
    constexpr int HD = 64;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, which = blockIdx.z;
    const int64_t base = cu ? cu[0] : 0;
    const int64_t r0 = (int64_t)blockIdx.x * 64 + wave * 16;
    if (r0 >= rows) return;                                   // (wave-uniform; the kernel has no barrier)
    const int64_t tok = r0 + l15;
    const int64_t tokc = tok < rows ? tok : rows - 1;
    const int inner = heads * HD, ld = 3 * inner;
    const bf16_t* src = qkv + (base + tokc) * ld + which * inner + h * HD + 8 * g;
    const bf16x8 b0 = *(const bf16x8*)src, b1 = *(const bf16x8*)(src + 32);
    const bf16_t* table = (which ? pos_query : pos_key) + (int64_t)h * 2 * span * HD + 8 * g;
    float* dst = strips + ((tokc * heads + h) * 2 + which) * winp + 4 * g;
    for (int j0 = 0; j0 < winp; j0 += 16) {
        int tr = lo + j0 + l15;
        tr = tr > 2 * span - 1 ? 2 * span - 1 : tr;           // (the padding columns past the window: any table row, finite values nobody reads)
        const bf16_t* ta = table + (int64_t)tr * HD;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)ta, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(ta + 32), b1, acc, 0, 0, 0);
        if (tok < rows) *(f32x4*)(dst + j0) = acc;            // D[table row 4 g + r][token l15]: strip values j0 + 4 g .. + 3 of the lane's token
    }
}

// ---- pass 2 ---------------------------------------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(DA_NW * 64) void attention_disentangled_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                            int fixed_len, int heads, int nslices, int kpad, const float* __restrict__ strips,
                                                                            int winp, const int32_t* __restrict__ idx, int reach, int lo, int win, float scale,
                                                                            int rows, int maxl) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = HD * 2;       // bytes per K / V row in LDS
    constexpr int NC = HD / 8;       // 16-byte chunk slots per LDS row
    constexpr int NKK = HD / 32;     // 32-deep MFMA k-chunks of a Q.K dot product
    constexpr int NDT = HD / 16;     // 16-wide output-dim tiles
    char* sK = smem;                                         // [kpad][RB], 16-B chunks XOR-swizzled by (key & (NC - 1))
    char* sV = smem + (size_t)kpad * RB;                     // [kpad][RB], same image
    short* sJ = (short*)(smem + 2 * (size_t)kpad * RB);      // [nent]: the strip offset of distance dmin + e

    const unsigned sh = blockIdx.x / (unsigned)nslices;
    const int slice = (int)(blockIdx.x - sh * (unsigned)nslices);
    const int seq = sh / heads, h = sh - seq * heads;
    int row0, len, base;
    if (fixed_len > 0) { row0 = seq * fixed_len; len = fixed_len; base = 0; }
    else { row0 = cu[seq]; len = cu[seq + 1] - row0; base = cu[0]; }
    const int q0 = slice * DA_SLICE;
    if (len <= 0 || q0 >= len) return;     // (the whole workgroup: no barrier has been reached)
    // a sequence the call's own numbers do not cover (longer than max_len: the offsets and the index table are sized by it; rows outside the strips) is
    // left alone rather than read out of bounds
    if (len > maxl || row0 < base || row0 - base + len > rows) return;
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
        attn_stage_piece<RB, NC, NC - 1, DA_NW>(sK, sV, kb, vb, ld, (c * tpc) << 6, tiles_here << 6, len, lane, wave);
    };

    const int l15 = lane & 15, g = lane >> 4;
    const int qb0 = q0 + wave * 16;             // this wave's 16-query block
    const bool active = qb0 < len;              // wave-uniform; an idle wave still stages and keeps the barriers
    const int q = qb0 + l15;                    // this lane's query (B-operand column / output row)
    const int qr = q < len ? q : len - 1;

    stage(0);
    // the slice's distances: query - key over queries [q0, min(q0 + 63, len - 1)] and keys [0, len - 1]; |d| <= len - 1 <= reach (the entry point's check)
    const int dmin = q0 - (len - 1);
    const int dmax = q0 + DA_SLICE - 1 < len - 1 ? q0 + DA_SLICE - 1 : len - 1;
    const int nent = dmax - dmin + 1;
    for (int e = threadIdx.x; e < nent; e += DA_NW * 64) {
        int j = idx[reach + dmin + e] - lo;
        j = j < 0 ? 0 : (j > win - 1 ? win - 1 : j);
        sJ[e] = (short)j;
    }
    // Q fragments (dims 32 kk + 8 g .. + 7 of query row q, clamped to the sequence) are fetched while the K / V DMA is in flight
    bf16x8 qf[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) qf[kk] = *(const bf16x8*)(qb + (int64_t)qr * ld + 8 * g + 32 * kk);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const int vkey = 4 * g + (l15 >> 2);    // per-lane constants of the V^T transpose reads
    const int vcol = (l15 & 3) >> 1, vhalf = (l15 & 1) << 3;
    // the strips: C of the lane's query row, P of the sequence's key rows (kstr floats from one key to the next)
    const int64_t kstr = (int64_t)heads * 2 * winp;
    const float* cq = strips + ((int64_t)(row0 - base + qr) * heads + h) * 2 * winp;
    const float* pk = strips + ((int64_t)(row0 - base) * heads + h) * 2 * winp + winp;

    float m_run = -1e30f, l_run = 0.f;
    f32x4 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < nchunks; ++c) {
        if (c > 0) {   // refill the LDS with the next piece of the sequence (the offsets behind the image stay)
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
            // score = scale * (q . k + C[q][j] + P[key][j]), j = the offset of query - key; key of (t, r) = k00 + 16 t + r
            const int k00 = kt * 64 + 4 * g;
            const int e00 = qr - dmin - k00;             // the entry of (t, r) = (0, 0); a key past the sequence falls below 0 and is clamped
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int key = k00 + 16 * t + r;
                    key = key < len ? key : len - 1;
                    int e = e00 - 16 * t - r;
                    e = e < 0 ? 0 : e;
                    const int j = sJ[e];
                    sc[t][r] = (sc[t][r] + (cq[j] + pk[key * kstr + j])) * scale;
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

}  // namespace

// the strips of `rows` token rows on `heads` heads over the bucket window [win_lo, win_hi]
extern "C" size_t mq_attention_disentangled_workspace_bytes(int64_t rows, int32_t heads, int32_t win_lo, int32_t win_hi) {
    if (rows <= 0 || heads <= 0 || win_lo < 0 || win_hi < win_lo || win_hi - win_lo + 1 > 2 * DA_MAX_SPAN) return 0;
    return da_strip_bytes(rows, heads, win_hi - win_lo + 1);
}

// d_qkv bf16 [.., 3 inner] = (q | k | v), inner = heads head_dim, head h of each third at columns h head_dim ..; d_out bf16 [.., inner]; sequences packed
// (d_cu_seqlens int32 [nseq + 1], ABSOLUTE row offsets into d_qkv / d_out — d_cu_seqlens[0] need not be 0, so a caller can run a batch in groups by
// moving this pointer; max_len = the longest) or fixed_len > 0 (d_cu_seqlens NULL ok).  rows = the call's token rows (d_cu_seqlens[nseq] -
// d_cu_seqlens[0], or nseq * fixed_len): it sizes the strips; a row past it is neither read nor written.  d_pos_key / d_pos_query bf16 [heads][2 span][64];
// d_idx int32 [2 reach + 1], entry d + reach = the bucket of query - key == d; [win_lo, win_hi] = the buckets of d = -(max_len - 1) and max_len - 1.
extern "C" int mq_attention_disentangled(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int64_t rows, int32_t fixed_len,
                                         int32_t max_len, int32_t heads, int32_t head_dim, const void* d_pos_key, const void* d_pos_query,
                                         const int32_t* d_idx, int32_t reach, int32_t span, int32_t win_lo, int32_t win_hi, float scale, void* d_workspace,
                                         size_t workspace_bytes, void* stream) {
    ATTN_ARG_PTRS("mq_attention_disentangled", d_qkv, d_out);
    MQ_CHECK_ARG(d_pos_key && d_pos_query && d_idx, "mq_attention_disentangled: null position table (pos_key / pos_query / idx)");
    MQ_CHECK_ARG(head_dim == 64, "mq_attention_disentangled: head_dim %d unsupported (64: the head width of the DeBERTa checkpoints)", head_dim);
    MQ_CHECK_ARG(heads >= 1 && heads <= 1024, "mq_attention_disentangled: heads %d outside [1, 1024]", heads);
    MQ_CHECK_ARG(span >= 1 && span <= DA_MAX_SPAN, "mq_attention_disentangled: span %d outside [1, %d]", span, DA_MAX_SPAN);
    MQ_CHECK_ARG(reach >= 0 && reach <= 8191, "mq_attention_disentangled: reach %d outside [0, 8191]", reach);
    MQ_CHECK_ARG(win_lo >= 0 && win_lo <= win_hi && win_hi <= 2 * span - 1, "mq_attention_disentangled: bucket window [%d, %d] outside [0, %d]", win_lo, win_hi,
                 2 * span - 1);
    MQ_CHECK_ARG(scale > 0.f && scale <= 1e6f, "mq_attention_disentangled: scale %g must be positive and finite", (double)scale);
    ATTN_ARG_SEQS("mq_attention_disentangled", fixed_len, d_cu_seqlens);
    if (nseq <= 0) return MQ_OK;
    const int maxl = fixed_len > 0 ? fixed_len : max_len;
    ATTN_ARG_MAXL("mq_attention_disentangled", maxl);
    MQ_CHECK_ARG(maxl <= reach + 1, "mq_attention_disentangled: max sequence length %d is beyond the index table's reach + 1 = %d", maxl, reach + 1);
    MQ_CHECK_ARG(rows >= nseq && rows <= nseq * (int64_t)maxl && (fixed_len <= 0 || rows == nseq * (int64_t)fixed_len) && rows < (1LL << 31),
                 "mq_attention_disentangled: rows %lld does not fit %lld sequences of at most %d tokens", (long long)rows, (long long)nseq, maxl);
    const int nslices = (maxl + DA_SLICE - 1) / DA_SLICE;
    ATTN_ARG_GRID("mq_attention_disentangled", nseq * heads * nslices);
    MQ_CHECK_ARG((rows + 63) / 64 < (1LL << 31) && heads <= 65535, "mq_attention_disentangled: grid too large");
    const int win = win_hi - win_lo + 1, winp = da_winp(win);
    MQ_CHECK_ARG(d_workspace, "mq_attention_disentangled: null workspace");
    const size_t need = da_strip_bytes(rows, heads, win);
    if (workspace_bytes < need) {
        mq_set_error("mq_attention_disentangled: workspace %zu < required %zu", workspace_bytes, need);
        return MQ_ERR_WORKSPACE;
    }
    const int kpad = attn_kpad(maxl, DA_LDS_KEYS);
    const size_t lds = (size_t)kpad * 64 * 4 + (((size_t)(maxl + DA_SLICE) * 2 + 15) & ~(size_t)15);
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(2, s);
    static std::atomic<uint64_t> done{0};
    const int rc = attn_ensure_lds((const void*)attention_disentangled_kernel<64>, lds, DA_LDS_MOST, done, "mq_attention_disentangled");
    if (rc != MQ_OK) return rc;
    const int32_t* cu = fixed_len > 0 ? nullptr : d_cu_seqlens;
    hipLaunchKernelGGL(disentangled_strips_kernel, dim3((unsigned)((rows + 63) / 64), (unsigned)heads, 2), dim3(DA_NW * 64), 0, s, (const bf16_t*)d_qkv, cu, rows,
                       heads, (const bf16_t*)d_pos_key, (const bf16_t*)d_pos_query, span, win_lo, winp, (float*)d_workspace);
    hipLaunchKernelGGL((attention_disentangled_kernel<64>), dim3((unsigned)(nseq * heads * nslices)), dim3(DA_NW * 64), lds, s, (const bf16_t*)d_qkv,
                       (bf16_t*)d_out, d_cu_seqlens, fixed_len, heads, nslices, kpad, (const float*)d_workspace, winp, d_idx, reach, win_lo, win, scale, (int)rows, maxl);
    MQ_CHECK_LAUNCH("mq_attention_disentangled");
    return MQ_OK;
}
