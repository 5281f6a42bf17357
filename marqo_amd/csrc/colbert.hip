// Late-interaction (ColBERT) reranking on the BERT tower: score(q, d) = sum_i max_j q_i . d_j over unit token vectors.
//   * mq_maxsim: the score.  One workgroup (4 wave64s) per document.  The document's token vectors stream through LDS in 64-token tiles (LDS-DMA, two
//     buffers: tile t + 1 is in flight under tile t's MFMAs; the image is attention_core.h's: 16-B chunks XOR-swizzled by the row).  Q is the stationary
//     operand: every wave holds ALL of Q (<= 64 rows) as MFMA B fragments in registers, loaded once.  Inside a tile wave w owns token rows 16 w .. 16 w + 15
//     (one A fragment, read once, multiplied into the up to four 16-query blocks): S^T = D . Q^T on v_mfma_f32_16x16x32_bf16, so a lane's 4 values of a
//     block belong to ONE query and fold into that query's running maximum at once: no score leaves the registers.  Splitting the TOKENS of a tile over the
//     waves, not the tiles, keeps all four busy from 49 tokens on (a 30-token hit: two); one workgroup per document keeps a call of a few hundred hits on
//     as many CUs.  Tokens past the document's end (the next document's rows) and keep = 0 tokens are -inf by index.  The end: max over the 4 lanes of a
//     query (two xor shuffles), over the 4 waves (LDS, fixed order), then one xor-butterfly sum over the queries.  Every dot product is one MFMA chain
//     over k = 0, 32, ...: a document's bits depend on nothing but Q and its own rows.
//   * mq_colbert_project: fp32 rows -> bf16 unit rows [rows, D], one launch.  64 rows per workgroup; the Linear's weight [D, W] goes through LDS in
//     64-column steps (LDS-DMA, two buffers) shared by the 4 waves, the rows come straight from global memory (fp32 -> bf16 in registers, the next step's
//     loads behind this step's MFMAs).  Y^T = L . X^T, so a lane's D / 4 values belong to one row: its sum of squares needs two xor shuffles and the row
//     is normalised and rounded in the tile that produced it.
//   * mq_attention_keyprefix: sequences of <= 64 rows whose rows attend keys [0, n_keys) only (ColBERT's [MASK]-padded query: the padding rows are
//     queries, never keys).  One workgroup per (sequence, head), one 16-query block per wave, ONE key tile: attention_core.h's tile core with the mask
//     `key < n_keys`.
//   * mq_score_colbert: embedding + BERT blocks for the documents (mq_encoder_forward) and for the query (the post-LN block loop on the fp32 stream with
//     the key-prefix attention), the projection on both sides, the keep mask from a skip table, mq_maxsim.
#include "attention_core.h"
#include "packed_text.h"

int mq_cast_bf16(const float* d_x, void* d_out, int64_t n, hipStream_t s);   // rowops.hip

namespace {
// rows [first, first + nrows) of a row-major bf16 matrix (leading dimension ld) -> LDS rows 0 .. nrows - 1 of RB bytes, 1024 B per LDS-DMA, chunk c of
// LDS row r in slot c ^ (r & (NC - 1)).  Rows past `last` re-read row `last`; NCS < NC: the matrix has only NCS chunks per row, the other slots get chunk 0
// (never consumed).  nrows is a multiple of 1024 / RB.  The caller waits (vmcnt(0)) and synchronises.
template <int RB, int NC, int NCS, int NW>
__device__ __forceinline__ void stage_rows(char* dst, const bf16_t* src, int64_t ld, int first, int nrows, int last, int lane, int wave) {
    constexpr int RPP = 1024 / RB;
    const int srow = lane / NC, pchunk = lane % NC;
    for (int p = wave; p < nrows / RPP; p += NW) {
        const int row = p * RPP + srow;
        const int r = first + row < last ? first + row : last;
        int lc = pchunk ^ (row & (NC - 1));
        if (NCS < NC) lc = lc < NCS ? lc : 0;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (int64_t)r * ld + (lc << 3)),
                                         (__attribute__((address_space(3))) void*)(dst + p * 1024), 16, 0, 0);
    }
}

template <int RB, int NC>
__device__ __forceinline__ bf16x8 lds_fragment(const char* base, int row, int chunk) {
    return *(const bf16x8*)(base + row * RB + ((chunk ^ (row & (NC - 1))) << 4));
}

// ---- MaxSim ------------------------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void maxsim_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ docs, const int32_t* __restrict__ cu,
                                                     const uint8_t* __restrict__ keep, int Lq, int64_t rows, float* __restrict__ scores) {
    constexpr int RB = D == 64 ? 128 : 256, NC = RB / 16, NCS = D / 8, NKK = D / 32;
    static_assert(D == 64 || D == 96 || D == 128, "token vectors of 64, 96 or 128 dims");
    __shared__ __attribute__((aligned(16))) char sD[2][64 * RB];
    __shared__ float sM[4][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int64_t row0 = cu[blockIdx.x];
    int len = cu[blockIdx.x + 1] - (int)row0;
    if (row0 < 0 || row0 >= rows) len = 0;
    else if (len > rows - row0) len = (int)(rows - row0);
    if (len <= 0) {                              // (block-uniform) no token: the maximum over nothing
        if (threadIdx.x == 0) scores[blockIdx.x] = -INFINITY;
        return;
    }
    const bf16_t* db = docs + row0 * D;
    const uint8_t* kp = keep + row0;
    const int ntiles = (len + 63) >> 6;
    stage_rows<RB, NC, NCS, 4>(sD[0], db, D, 0, 64, len - 1, lane, wave);

    // Q as B fragments: block qb, k-chunk kk = dims 32 kk + 8 g .. + 7 of query 16 qb + l15 (rows past Lq repeat the last one and are dropped at the end)
    const int nqb = (Lq + 15) >> 4;
    bf16x8 qf[4][NKK];
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
        const int qr = qb * 16 + l15 < Lq ? qb * 16 + l15 : Lq - 1;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) qf[qb][kk] = *(const bf16x8*)(q + qr * D + 32 * kk + 8 * g);
    }
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};

    for (int t = 0; t < ntiles; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                         // tile t is in sD[t & 1]; every wave is done with tile t - 1, whose buffer the next DMA overwrites
        if (t + 1 < ntiles) stage_rows<RB, NC, NCS, 4>(sD[(t + 1) & 1], db, D, (t + 1) * 64, 64, len - 1, lane, wave);
        const int tok0 = t * 64 + wave * 16;
        if (tok0 >= len) continue;               // (wave-uniform)
        const char* base = sD[t & 1];
        bf16x8 df[NKK];
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) df[kk] = lds_fragment<RB, NC>(base, wave * 16 + l15, g + 4 * kk);
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tok = tok0 + 4 * g + r;
            ok[r] = tok < len && kp[tok < len ? tok : len - 1] != 0;
        }
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
            if (qb >= nqb) break;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[kk], qf[qb][kk], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) m[qb] = fmaxf(m[qb], ok[r] ? acc[r] : -INFINITY);
        }
    }
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
        m[qb] = fmaxf(m[qb], __shfl_xor(m[qb], 16, 64));
        m[qb] = fmaxf(m[qb], __shfl_xor(m[qb], 32, 64));
        if (g == 0) sM[wave][qb * 16 + l15] = m[qb];
    }
    __syncthreads();
    if (wave == 0) {
        float v = fmaxf(fmaxf(sM[0][lane], sM[1][lane]), fmaxf(sM[2][lane], sM[3][lane]));
        v = wave_sum(lane < Lq ? v : 0.f);
        if (lane == 0) scores[blockIdx.x] = v;
    }
}

// ---- projection + L2 normalisation --------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void colbert_project_kernel(const float* __restrict__ x, const bf16_t* __restrict__ lw, bf16_t* __restrict__ out,
                                                              int64_t rows, int W, float eps) {
    constexpr int NCT = D / 16;
    __shared__ __attribute__((aligned(16))) char sW[2][D * 128];     // [D rows][64 k] bf16 per buffer
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int64_t row = (int64_t)blockIdx.x * 64 + wave * 16 + l15;
    const float* xr = x + (row < rows ? row : rows - 1) * W + 8 * g;    // this lane's B-operand row: dims k0 + 32 kk + 8 g .. + 7
    const int nk = W >> 6;
    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 xn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xn[i] = *(const f32x4*)(xr + 32 * (i >> 1) + 4 * (i & 1));
    stage_rows<128, 8, 8, 4>(sW[0], lw, W, 0, D, D - 1, lane, wave);
    for (int ks = 0; ks < nk; ++ks) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        union { uint32_t w[4]; bf16x8 v; } xf[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            xf[kk].w[0] = pack_bf16x2(xn[2 * kk][0], xn[2 * kk][1]);
            xf[kk].w[1] = pack_bf16x2(xn[2 * kk][2], xn[2 * kk][3]);
            xf[kk].w[2] = pack_bf16x2(xn[2 * kk + 1][0], xn[2 * kk + 1][1]);
            xf[kk].w[3] = pack_bf16x2(xn[2 * kk + 1][2], xn[2 * kk + 1][3]);
        }
        if (ks + 1 < nk) {
            stage_rows<128, 8, 8, 4>(sW[(ks + 1) & 1], lw + (ks + 1) * 64, W, 0, D, D - 1, lane, wave);
#pragma unroll
            for (int i = 0; i < 4; ++i) xn[i] = *(const f32x4*)(xr + (ks + 1) * 64 + 32 * (i >> 1) + 4 * (i & 1));
        }
        const char* base = sW[ks & 1];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_fragment<128, 8>(base, ct * 16 + l15, g + 4 * kk), xf[kk].v, acc[ct], 0, 0, 0);
    }
    // acc[ct][r] = y[row][16 ct + 4 g + r]: the row's sum of squares over this lane, then over the 4 lanes that share the row
    float ss = 0.f;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) ss = fmaf(acc[ct][r], acc[ct][r], ss);
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    const float inv = 1.0f / fmaxf(sqrtf(ss), eps);
    if (row < rows) {
        bf16_t* orow = out + row * D + 4 * g;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            uint2 p;
            p.x = pack_bf16x2(acc[ct][0] * inv, acc[ct][1] * inv);
            p.y = pack_bf16x2(acc[ct][2] * inv, acc[ct][3] * inv);
            *(uint2*)(orow + ct * 16) = p;
        }
    }
}

// ---- key-prefix attention -----------------------------------------------------------------------------------------------------------------------------
// HD = LDS row width (64 | 128), HS = head stride in memory = dims computed (attention.hip's parameters)
template <int HD, int HS>
__global__ __launch_bounds__(256) void attention_keyprefix_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ cu,
                                                                  const int32_t* __restrict__ n_keys, int W, int heads, float scale_log2e) {
    constexpr int RB = HD * 2, NC = HD / 8, NCS = HS / 8, NKK = (HS + 31) / 32, NDT = HS / 16;
    __shared__ __attribute__((aligned(16))) char sK[64 * RB];
    __shared__ __attribute__((aligned(16))) char sV[64 * RB];
    const int seq = blockIdx.x / heads, h = blockIdx.x - seq * heads;
    const int row0 = cu[seq];
    int len = cu[seq + 1] - row0;
    len = len > 64 ? 64 : len;                   // (the entry point has refused longer sequences)
    if (len <= 0) return;
    int nk = n_keys[seq];
    nk = nk < 1 ? 1 : (nk > len ? len : nk);
    const int ld = 3 * W;
    const bf16_t* qb = qkv + (int64_t)row0 * ld + h * HS;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    attn_stage_piece<RB, NC, NC - 1, 4, NCS>(sK, sV, qb + W, qb + 2 * W, ld, 0, 64, len, lane, wave);
    const int q = wave * 16 + l15;
    bf16x8 qf[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
        const int col = 8 * g + 32 * kk;
        qf[kk] = (HS % 32 != 0 && col >= HS) ? bf16x8{0, 0, 0, 0, 0, 0, 0, 0} : *(const bf16x8*)(qb + (int64_t)(q < len ? q : len - 1) * ld + col);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave * 16 >= len) return;                // (wave-uniform, behind the only barrier)
    f32x4 sc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        sc[t] = attn_score_keys<RB, NKK, NC - 1>(sK, t * 16 + l15, 0, g, qf);
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[t][r] = t * 16 + 4 * g + r < nk ? sc[t][r] : -INFINITY;
    }
    float m_run = -1e30f, l_run = 0.f;
    f32x4 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    attn_softmax_step<NDT>(sc, m_run, l_run, o, scale_log2e);        // (key 0 is never masked: m_run is finite)
    attn_pv_tile<RB, NDT, NC - 1>(sV, 0, 0, 4 * g + (l15 >> 2), (l15 & 3) >> 1, (l15 & 1) << 3, sc, o);
    const float inv = attn_inv_denominator(l_run);
    if (q < len) attn_store_bf16<NDT>(out + (int64_t)(row0 + q) * W + h * HS + 4 * g, o, inv);
}

// keep[r] = 0 for the ids of the skip table (punctuation), 1 otherwise; {0, Lq} and n_keys of the query behind it
__global__ __launch_bounds__(256) void colbert_keep_kernel(const int32_t* __restrict__ ids, const uint8_t* __restrict__ skip, int vocab, int64_t rows,
                                                           uint8_t* __restrict__ keep, int32_t* __restrict__ meta, int Lq, int n_keys) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r == 0) { meta[0] = 0; meta[1] = Lq; meta[2] = n_keys; }
    if (r >= rows) return;
    int id = ids[r];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    keep[r] = skip ? (skip[id] ? 0 : 1) : 1;
}

bool colbert_dim_ok(int D) { return D == 64 || D == 96 || D == 128; }
int attn_width(const mq_encoder_cfg* c) { return c->attn_width ? c->attn_width : c->width; }

struct ColbertPlan { size_t off_xd, off_encd, encd_bytes, off_xq, off_qh, off_qa, off_qf, off_qe, off_de, off_keep, off_meta, total; };
ColbertPlan colbert_plan(const mq_bert_cfg* cfg, int D, int Lq, int64_t rows, int64_t nseq) {
    ColbertPlan p;
    Off ws;
    const mq_encoder_cfg* e = &cfg->enc;
    const int W = e->width, Wa = attn_width(e), F = e->mlp_dim;
    p.off_xd = ws.take((size_t)rows * W * 4);                         // the documents' fp32 stream
    p.encd_bytes = mq_encoder_workspace_bytes(e, rows, nseq);
    p.off_encd = ws.take(p.encd_bytes);
    p.off_xq = ws.take((size_t)Lq * W * 4);                           // the query's fp32 stream, its bf16 copy, attention output, qkv | fc1 output
    p.off_qh = ws.take((size_t)Lq * W * 2);
    p.off_qa = ws.take((size_t)Lq * Wa * 2);
    p.off_qf = ws.take((size_t)Lq * (3 * Wa > F ? 3 * Wa : F) * 2);
    p.off_qe = ws.take((size_t)Lq * D * 2);                           // unit rows of both sides
    p.off_de = ws.take((size_t)rows * D * 2);
    p.off_keep = ws.take((size_t)rows);
    p.off_meta = ws.take(16);
    p.total = ws.end();
    return p;
}
}  // namespace

extern "C" int mq_maxsim(const void* d_q, const void* d_docs, const int32_t* d_cu, const uint8_t* d_keep, int64_t n, int64_t rows, int32_t Lq, int32_t D,
                         float* d_scores, void* stream) {
    MQ_CHECK_ARG(Lq >= 1 && Lq <= 64, "mq_maxsim: Lq=%d must be in [1, 64]", Lq);
    MQ_CHECK_ARG(colbert_dim_ok(D), "mq_maxsim: D=%d must be 64, 96 or 128", D);
    MQ_CHECK_ARG(n < (1ll << 31) && rows >= 0 && rows < (1ll << 31), "mq_maxsim: n=%lld rows=%lld too large", (long long)n, (long long)rows);
    if (n <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_q && d_docs && d_cu && d_keep && d_scores, "mq_maxsim: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(4, s);
#define MQ_MAXSIM_LAUNCH(DD)                                                                                                              \
    hipLaunchKernelGGL(maxsim_kernel<DD>, dim3((unsigned)n), dim3(256), 0, s, (const bf16_t*)d_q, (const bf16_t*)d_docs, d_cu, d_keep, \
                       (int)Lq, rows, d_scores)
    if (D == 64) MQ_MAXSIM_LAUNCH(64);
    else if (D == 96) MQ_MAXSIM_LAUNCH(96);
    else MQ_MAXSIM_LAUNCH(128);
#undef MQ_MAXSIM_LAUNCH
    MQ_CHECK_LAUNCH("mq_maxsim");
    return MQ_OK;
}

extern "C" int mq_colbert_project(const float* d_x, const void* d_linear_w, void* d_out, int64_t rows, int32_t W, int32_t D, float eps, void* stream) {
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= 2048, "mq_colbert_project: W=%d must be a multiple of 64, at most 2048", W);
    MQ_CHECK_ARG(colbert_dim_ok(D), "mq_colbert_project: D=%d must be 64, 96 or 128", D);
    MQ_CHECK_ARG(eps > 0.f, "mq_colbert_project: eps=%g must be positive", (double)eps);
    MQ_CHECK_ARG(rows < (1ll << 31), "mq_colbert_project: rows=%lld too large", (long long)rows);
    if (rows <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_x && d_linear_w && d_out, "mq_colbert_project: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(0, s, 2.0 * (double)rows * W * D);
#define MQ_PROJECT_LAUNCH(DD)                                                                                                                   \
    hipLaunchKernelGGL(colbert_project_kernel<DD>, dim3((unsigned)cdiv64(rows, 64)), dim3(256), 0, s, d_x, (const bf16_t*)d_linear_w, \
                       (bf16_t*)d_out, rows, (int)W, eps)
    if (D == 64) MQ_PROJECT_LAUNCH(64);
    else if (D == 96) MQ_PROJECT_LAUNCH(96);
    else MQ_PROJECT_LAUNCH(128);
#undef MQ_PROJECT_LAUNCH
    MQ_CHECK_LAUNCH("mq_colbert_project");
    return MQ_OK;
}

extern "C" int mq_attention_keyprefix(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, const int32_t* d_n_keys,
                                      const int32_t* h_n_keys, int64_t nseq, int32_t W, int32_t heads, void* stream) {
    ATTN_ARG_PTRS("mq_attention_keyprefix", d_qkv, d_out);
    MQ_CHECK_ARG(heads >= 1 && W % heads == 0, "mq_attention_keyprefix: W=%d is not a multiple of heads=%d", W, heads);
    const int hs = W / heads;
    MQ_CHECK_ARG(hs == 64 || hs == 96 || hs == 112 || hs == 128, "mq_attention_keyprefix: head dim must be 64, 96, 112 or 128 (W=%d heads=%d)", W, heads);
    if (nseq <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_cu_seqlens && h_cu_seqlens && d_n_keys && h_n_keys, "mq_attention_keyprefix: null cu_seqlens / n_keys");
    for (int64_t i = 0; i < nseq; ++i) {
        const int len = h_cu_seqlens[i + 1] - h_cu_seqlens[i];
        MQ_CHECK_ARG(len >= 1 && len <= 64 && h_n_keys[i] >= 1 && h_n_keys[i] <= len,
                     "mq_attention_keyprefix: sequence %lld has n_rows=%d n_keys=%d (1 <= n_keys <= n_rows <= 64)", (long long)i, len, h_n_keys[i]);
    }
    ATTN_ARG_GRID("mq_attention_keyprefix", nseq * heads);
    hipStream_t s = (hipStream_t)stream;
    const float scale_log2e = 1.44269504088896340736f / sqrtf((float)hs);
    MqProfScope prof(2, s);
#define MQ_KEYPREFIX_LAUNCH(HD, HS)                                                                                                            \
    hipLaunchKernelGGL((attention_keyprefix_kernel<HD, HS>), dim3((unsigned)(nseq * heads)), dim3(256), 0, s, (const bf16_t*)d_qkv, (bf16_t*)d_out, \
                       d_cu_seqlens, d_n_keys, (int)W, (int)heads, scale_log2e)
    if (hs == 64) MQ_KEYPREFIX_LAUNCH(64, 64);
    else if (hs == 96) MQ_KEYPREFIX_LAUNCH(128, 96);
    else if (hs == 112) MQ_KEYPREFIX_LAUNCH(128, 112);
    else MQ_KEYPREFIX_LAUNCH(128, 128);
#undef MQ_KEYPREFIX_LAUNCH
    MQ_CHECK_LAUNCH("mq_attention_keyprefix");
    return MQ_OK;
}

extern "C" size_t mq_score_colbert_workspace_bytes(const mq_bert_cfg* cfg, int32_t D, int32_t Lq, int64_t rows, int64_t nseq) {
    if (!cfg || rows <= 0 || nseq <= 0 || Lq <= 0 || D <= 0 || cfg->enc.width <= 0) return 0;
    return colbert_plan(cfg, D, Lq, rows, nseq).total;
}

extern "C" int mq_score_colbert(const mq_bert_cfg* cfg, const mq_bert_weights* w, const void* d_linear_w, int32_t D, const uint8_t* d_skip,
                                const int32_t* d_query_ids, int32_t Lq, int32_t n_keys, const int32_t* d_doc_ids, const int32_t* d_cu_seqlens,
                                const int32_t* h_cu_seqlens, int64_t nseq, float* d_scores, void* d_query_emb, void* d_doc_emb, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
    const char* what = "mq_score_colbert";
    MQ_CHECK_ARG(cfg && w && d_linear_w && d_scores, "%s: null pointer", what);
    const mq_encoder_cfg* e = &cfg->enc;
    MQ_CHECK_ARG(e->precision == MQ_PREC_BF16, "%s: bf16 encoders only (precision %d)", what, e->precision);
    MQ_CHECK_ARG(e->post_ln == 1 && e->mask == MQ_MASK_NONE, "%s: BERT is post-LN with full attention", what);
    MQ_CHECK_ARG(!e->d_rope_inv_freq && !e->d_rope_table && !e->mlp_glu && !e->d_rel_bias, "%s: plain BERT encoders only", what);
    MQ_CHECK_ARG(e->act == MQ_ACT_GELU || e->act == MQ_ACT_QUICKGELU, "%s: act %d unsupported", what, e->act);
    MQ_CHECK_ARG(w->word_emb && w->pos_emb && w->emb_ln_g && w->emb_ln_b && (w->blocks || e->layers == 0), "%s: null weight pointer", what);
    const int W = e->width, F = e->mlp_dim, Wa = attn_width(e);
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= 2048 && F >= 64 && F % 64 == 0 && e->heads >= 1 && e->layers >= 0, "%s: W=%d mlp_dim=%d heads=%d", what, W, F,
                 e->heads);
    MQ_CHECK_ARG(colbert_dim_ok(D), "%s: D=%d must be 64, 96 or 128", what, D);
    MQ_CHECK_ARG(Lq >= 1 && Lq <= 64 && Lq <= cfg->max_pos && n_keys >= 1 && n_keys <= Lq, "%s: Lq=%d n_keys=%d (1 <= n_keys <= Lq <= min(64, max_pos))", what,
                 Lq, n_keys);
    MQ_CHECK_ARG(nseq < (1ll << 31), "%s: nseq=%lld too large", what, (long long)nseq);
    if (nseq <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_query_ids, "%s: null query ids", what);
    int maxl = 0;
    int64_t rows = 0;
    MQ_TRY(packed_begin(what, d_doc_ids, d_cu_seqlens, h_cu_seqlens, nseq, cfg->max_pos, d_workspace, &maxl, &rows));
    const ColbertPlan p = colbert_plan(cfg, D, Lq, rows, nseq);
    MQ_TRY(packed_workspace(what, workspace_bytes, p.total));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_workspace;
    float* xd = (float*)(base + p.off_xd);
    float* xq = (float*)(base + p.off_xq);
    void *qh = base + p.off_qh, *qa = base + p.off_qa, *qf = base + p.off_qf;
    void* qe = d_query_emb ? d_query_emb : (void*)(base + p.off_qe);
    void* de = d_doc_emb ? d_doc_emb : (void*)(base + p.off_de);
    uint8_t* keep = (uint8_t*)(base + p.off_keep);
    int32_t* meta = (int32_t*)(base + p.off_meta);      // {0, Lq}: the query's cu_seqlens; n_keys
    const int32_t h_qcu[2] = {0, Lq}, h_qnk[1] = {n_keys};
    const float eps = 1e-12f;                           // torch.nn.functional.normalize's

    hipLaunchKernelGGL(colbert_keep_kernel, dim3((unsigned)cdiv64(rows, 256)), dim3(256), 0, s, d_doc_ids, d_skip, (int)cfg->vocab, rows, keep, meta, (int)Lq,
                       (int)n_keys);
    MQ_CHECK_LAUNCH(what);
    // documents: ordinary packed sequences, as mq_encode_bert runs them
    MQ_TRY(mq_embed_tokens(d_doc_ids, d_cu_seqlens, nseq, w->word_emb, w->pos_emb, w->type_emb, w->emb_ln_g, w->emb_ln_b, xd, nullptr, W, cfg->vocab,
                           e->ln_eps, 0, s));
    MQ_TRY(mq_encoder_forward(e, w->blocks, xd, rows, d_cu_seqlens, nseq, 0, maxl, base + p.off_encd, p.encd_bytes, s));
    MQ_TRY(mq_colbert_project(xd, d_linear_w, de, rows, W, D, eps, s));
    // the query: x = ln1(x + out(attn(qkv(x)))) ; x = ln2(x + fc2(act(fc1(x)))) on the fp32 stream, rows [n_keys, Lq) never keys
    MQ_TRY(mq_embed_tokens(d_query_ids, meta, 1, w->word_emb, w->pos_emb, w->type_emb, w->emb_ln_g, w->emb_ln_b, xq, nullptr, W, cfg->vocab, e->ln_eps, 0, s));
    MQ_TRY(mq_cast_bf16(xq, qh, (int64_t)Lq * W, s));
    const int act_flag = e->act == MQ_ACT_QUICKGELU ? MQ_EPI_QUICKGELU : MQ_EPI_GELU;
    const int res_flags = MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32;
    for (int l = 0; l < e->layers; ++l) {
        const mq_block_weights& b = w->blocks[l];
        MQ_CHECK_ARG(b.qkv_w && b.out_w && b.fc1_w && b.fc2_w && b.ln1_g && b.ln2_g, "%s: layer %d has null weights", what, l);
        MQ_TRY(mq_gemm_bf16(qh, W, b.qkv_w, W, b.qkv_b, nullptr, qf, 3 * Wa, Lq, 3 * Wa, W, MQ_EPI_BIAS, s));
        MQ_TRY(mq_attention_keyprefix(qf, qa, meta, h_qcu, meta + 2, h_qnk, 1, Wa, e->heads, s));
        MQ_TRY(mq_gemm_bf16(qa, Wa, b.out_w, Wa, b.out_b, xq, xq, W, Lq, W, Wa, res_flags, s));
        MQ_TRY(mq_layernorm(xq, nullptr, b.ln1_g, b.ln1_b, qh, xq, Lq, W, e->ln_eps, s));
        MQ_TRY(mq_gemm_bf16(qh, W, b.fc1_w, W, b.fc1_b, nullptr, qf, F, Lq, F, W, MQ_EPI_BIAS | act_flag, s));
        MQ_TRY(mq_gemm_bf16(qf, F, b.fc2_w, F, b.fc2_b, xq, xq, W, Lq, W, F, res_flags, s));
        MQ_TRY(mq_layernorm(xq, nullptr, b.ln2_g, b.ln2_b, qh, xq, Lq, W, e->ln_eps, s));
    }
    MQ_TRY(mq_colbert_project(xq, d_linear_w, qe, Lq, W, D, eps, s));
    return mq_maxsim(qe, de, d_cu_seqlens, keep, nseq, rows, Lq, D, d_scores, s);
}
