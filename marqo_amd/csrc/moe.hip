// Routed mixture-of-experts MLP (nomic-embed-text-v2-moe: 2 of 8 experts per token): a router, a device-side plan and a GROUPED bf16 MFMA GEMM over
// segments whose sizes the host never learns — one stream, no sync, no allocation, no float atomics, no integer atomics either.
//
//   mq_moe_route       logits = x Wr^T from the FP32 stream x and an fp32 Wr (the choice of expert is the one place where a bf16 rounding changes the
//                      result discretely), fp32 softmax over E <= 16, top-k (k = 1, 2) on the logits with the LOWER index winning a tie; the weights
//                      are the softmax values, not renormalised.  One wave64 per row: the row sits in registers, a lane owns float4 chunks lane, lane + 64,
//                      ..., one butterfly sum per expert.
//   mq_moe_plan        a stable counting sort of the k rows flat entries i = row k + j by expert, ONE workgroup of 16 waves: wave w owns a contiguous
//                      range of entries and walks it 64 at a time (coalesced); a ballot per expert gives every entry its rank among the wave's earlier
//                      entries of the same expert, lane e keeps the wave's counter of expert e.  Pass 1 counts, an exclusive scan in (expert, wave)
//                      order turns the 16 x E counters into first slots, pass 2 repeats the walk and writes slot_row / slot_w / row_slot.  A slot's
//                      position is a function of the entries in front of it only: deterministic, ascending row inside an expert.  The same launch writes
//                      expert_off[E + 1] and the row-tile table of the grouped GEMM — (expert, first slot) per tile of `bm` slots, a tile never
//                      straddles two experts — and the tile count in front of it.
//   mq_moe_gemm        out[slot, :] = epi(A[src(slot), :] W[e(slot)]^T), W [E][N][K] bf16 K-contiguous.  Grid = (N / BN, tile bound): the host sizes it
//                      from  sum_e ceil(n_e / BM) <= floor(k rows / BM) + E ; a workgroup whose tile index is past the device-side count returns before
//                      its first barrier.  UP: A rows are GATHERED from h through slot_row — the LDS-DMA staging (gemm_loop.h: dma16) takes a per-lane
//                      source offset, so the gather is the address of the piece, not a pass of its own — the epilogue is the erf GELU of MQ_EPI_GELU and
//                      stores bf16 P[slot, F].  DOWN: A = P, contiguous per expert, the epilogue multiplies by the slot's routing weight and stores fp32
//                      Y[slot, W].  Rows of a ragged last tile of a segment are clamped on read (the segment's last slot) and not stored.
//   mq_moe_combine_ln  x = LN(((x + Y[row_slot[r, 0]]) + Y[row_slot[r, 1]]) + bias) in exactly that order -> fp32 x and bf16 h, one wave per row.
//
// The grouped GEMM's tile body.  Operands go global -> LDS by LDS-DMA in 8-row x 128-byte pieces (1 KiB per wave instruction) into a ring of NS stages
// of one 64-deep k-step; the tiles are [rows][128 B] with the 16-byte chunk index XOR-swizzled by (row & 7) on the lane's SOURCE address and again on
// the ds_read_b128 side (gemm_bf16.hip's layout).  Per k-step: vmcnt((NS - 2) pieces-per-stage) + one barrier (stage kt has landed for everybody, and
// everybody is done with the buffer of stage kt - 1), the DMA of stage kt + NS - 1 into that buffer, the fragment reads of stage kt (inline-asm reads
// with a hand-placed lgkmcnt(0): hipcc cannot tell them from the DMA writes in flight and would drain vmcnt in front of every read), then the MFMAs.
// Requests past the last k-step go out with a zero-sized descriptor (no traffic), which keeps the wait counts one straight-line body.  Operands are fed
// swapped (mfma(Wfrag, Afrag)) so a lane owns 4 consecutive n of one output row: 8 / 16-byte stores.
//
// Two regimes, two tile heights over the same body:
//   * an indexing batch (64 x 512 tokens, 8 k rows per expert): BM x BN = 128 x 128, 4 waves as 2 x 2, 64 x 64 per wave = 16 accumulators
//     v_mfma_f32_16x16x32_bf16, 32 MFMAs per 16 fragment reads and 8 DMA pieces; 2 stages = 64 KiB of LDS, two workgroups per CU.  blockIdx.x walks
//     the column tiles of one row tile: neighbours share the gathered A tile through L2, and with N / BN a multiple of 8 an XCD keeps meeting the same
//     three column tiles of the expert's matrix.
//   * a single query (one or two rows per expert): the launch is bound by reading E x 2 weight matrices once (75 MB at the checkpoint's shape), the MFMA
//     work is noise and a 128-row tile would be 126 rows of padding.  BM x BN = 32 x 64, 4 waves side by side along N (32 x 16 each), 4 stages of 12 KiB:
//     three k-steps of weight rows in flight per workgroup, N / 64 x (tiles) workgroups so that the whole chip streams the weights.
//   The host picks the height from k rows / E (mq_moe_tile_rows: above 64 slots per expert the tall tile); no device-side decision.
// EVERY tile of either height accumulates an output element in ONE accumulator over k = 0, 32, 64, ... in that order: no split-K, no in-kernel tail.  A
// token's bits therefore do not depend on the tile height, on its slot, or on what else is in the batch (the promise gemm_sched.h documents).
//
// Bounds (read before running).  route: row < rows, chunk c < W / 4, Wr row e < E.  plan: entries i < n = k rows; expert ids are clamped to [0, E);
// slots are < n by construction (a permutation); tiles are written at index < max_tiles.  gemm: tile rows are clamped to the segment's last slot
// (>= first slot: a tile exists only for a non-empty range), W rows to N - 1, k offsets to K - 64 by nk = K / 64; the gather offset row * lda * 2 is
// 32-bit (the host refuses rows * K * 2 >= 2^32); stores at row < the segment's end and n + 3 < N.  combine: slots are clamped to [0, nslots).
//
// Compiler report (gfx950, -O3, resource remarks; compiled without the packed fp32 VALU forms), 256 threads per workgroup unless noted:
//   moe_gemm_kernel<UP / DOWN, tall 128 x 128>:  90 VGPRs + 76 AGPRs, 36 / 40 SGPRs, 64 KiB LDS (dynamic): two workgroups per CU by LDS
//   moe_gemm_kernel<UP / DOWN, short 32 x 64>:   34 VGPRs + 12 AGPRs, 44 / 42 SGPRs, 48 KiB LDS (dynamic): three workgroups per CU by LDS
//   moe_route_kernel<CH = 1 / 2 / 3 / 4 / 6 / 8>:      28 / 32 / 36 / 42 / 52 / 62 VGPRs, 56 - 68 SGPRs, 8 waves per SIMD
//   moe_plan_kernel (1024 threads):                    22 VGPRs, 50 SGPRs, 1248 B LDS
//   moe_combine_ln_kernel<CH = 1 / 2 / 3 / 4 / 6 / 8>: 26 / 29 / 37 / 46 / 61 / 76 VGPRs, 27 - 50 SGPRs, 8 waves per SIMD (CH = 8: 6)
// No VGPR / SGPR spill and no scratch in any of them.  Measured on an MI355X: DESIGN.md, "Routed experts".
#include "common.h"
#include "gemm_loop.h"

namespace {

constexpr int MOE_MAX_E = 16;
constexpr int MOE_BM_TALL = 128, MOE_BM_SHORT = 32;
constexpr int MOE_TALL_FROM = 64;       // slots per expert (k rows / E) above which the tall tile runs
constexpr int PLAN_WAVES = 16;

// ---- router ------------------------------------------------------------------------------------------------------------------------------------------
template <int CH>
__global__ __launch_bounds__(256) void moe_route_kernel(const float* __restrict__ x, const float* __restrict__ Wr, int32_t* __restrict__ top_e,
                                                       float* __restrict__ top_w, int64_t rows, int W, int E, int k) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nch = W >> 2;
    f32x4 v[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        v[i] = c < nch ? *(const f32x4*)(x + row * W + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float logit[MOE_MAX_E];
#pragma unroll
    for (int e = 0; e < MOE_MAX_E; ++e) {
        logit[e] = -INFINITY;
        if (e < E) {        // (wave-uniform)
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int c = lane + i * 64;
                if (c < nch) {
                    const f32x4 w = *(const f32x4*)(Wr + (int64_t)e * W + c * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s = fmaf(v[i][j], w[j], s);
                }
            }
            logit[e] = wave_sum(s);
        }
    }
    // top-k on the logits (the softmax is monotone; its rounding could tie what the logits do not): strict >, ascending e -> the lower index wins a tie
    int e0 = 0, e1 = -1;
    float l0 = logit[0], l1 = -INFINITY;
#pragma unroll
    for (int e = 1; e < MOE_MAX_E; ++e)
        if (logit[e] > l0) { l0 = logit[e]; e0 = e; }
#pragma unroll
    for (int e = 0; e < MOE_MAX_E; ++e)
        if (e != e0 && e < E && (e1 < 0 || logit[e] > l1)) { l1 = logit[e]; e1 = e; }
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < MOE_MAX_E; ++e)
        if (e < E) sum += expf(logit[e] - l0);
    if (lane == 0) {
        top_e[row * k] = e0;
        top_w[row * k] = 1.0f / sum;        // expf(l0 - l0) = 1
        if (k == 2) {
            top_e[row * 2 + 1] = e1;
            top_w[row * 2 + 1] = expf(l1 - l0) / sum;
        }
    }
}

// ---- plan: stable counting sort + tile table ---------------------------------------------------------------------------------------------------------
// tiles: [0] = tile count, [1 + 2 t] = expert of tile t, [2 + 2 t] = its first slot
__global__ __launch_bounds__(PLAN_WAVES * 64) void moe_plan_kernel(const int32_t* __restrict__ top_e, const float* __restrict__ top_w, int n, int k, int E,
                                                                  int bm, int max_tiles, int32_t* __restrict__ expert_off, int32_t* __restrict__ slot_row,
                                                                  float* __restrict__ slot_w, int32_t* __restrict__ row_slot, int32_t* __restrict__ tiles) {
    __shared__ int cnt[PLAN_WAVES][MOE_MAX_E];      // per (wave, expert): entries, then the first slot's offset inside the expert's segment
    __shared__ int tot[MOE_MAX_E];
    __shared__ int off[MOE_MAX_E + 1], tbase[MOE_MAX_E + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (n + PLAN_WAVES * 64 - 1) / (PLAN_WAVES * 64) * 64;     // entries per wave, a multiple of 64
    const int i0 = min(wave * per, n), i1 = min(i0 + per, n);
    const uint64_t below = (1ull << lane) - 1ull;
    auto expert_of = [&](int i) {
        if (i >= i1) return -1;
        const int e = top_e[i];
        return e < 0 ? 0 : (e >= E ? E - 1 : e);
    };
    int c = 0;      // lane e: this wave's entries of expert e
    for (int b = i0; b < i1; b += 64) {
        const int e = expert_of(b + lane);
        for (int q = 0; q < E; ++q) {
            const uint64_t m = __ballot(e == q);
            if (lane == q) c += __popcll(m);
        }
    }
    if (lane < MOE_MAX_E) cnt[wave][lane] = lane < E ? c : 0;
    __syncthreads();
    if (tid < E) {
        int run = 0;
#pragma unroll
        for (int w = 0; w < PLAN_WAVES; ++w) { const int t = cnt[w][tid]; cnt[w][tid] = run; run += t; }
        tot[tid] = run;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0, tb = 0;
        for (int e = 0; e < E; ++e) { off[e] = o; tbase[e] = tb; o += tot[e]; tb += (tot[e] + bm - 1) / bm; }
        off[E] = o;
        tbase[E] = tb;
    }
    __syncthreads();
    if (tid <= E) expert_off[tid] = off[tid];
    if (tid == 0) tiles[0] = min(tbase[E], max_tiles);
    for (int e = 0; e < E; ++e) {
        const int nt = tbase[e + 1] - tbase[e];
        for (int t = tid; t < nt; t += PLAN_WAVES * 64) {
            const int idx = tbase[e] + t;
            if (idx < max_tiles) { tiles[1 + 2 * idx] = e; tiles[2 + 2 * idx] = off[e] + t * bm; }
        }
    }
    int pos = lane < E ? off[lane] + cnt[wave][lane] : 0;       // lane e: the next slot of expert e for this wave
    for (int b = i0; b < i1; b += 64) {
        const int i = b + lane, e = expert_of(i);
        int rank = 0, add = 0;
        for (int q = 0; q < E; ++q) {
            const uint64_t m = __ballot(e == q);
            if (e == q) rank = __popcll(m & below);
            if (lane == q) add = __popcll(m);
        }
        const int base = __shfl(pos, e < 0 ? 0 : e, 64);
        if (e >= 0) {
            const int slot = base + rank;
            slot_row[slot] = i / k;
            slot_w[slot] = top_w[i];
            row_slot[i] = slot;
        }
        pos += add;
    }
}

// ---- grouped GEMM --------------------------------------------------------------------------------------------------------------------------------------
constexpr int MOE_UP = 0, MOE_DOWN = 1;

template <int FORM, int WM, int WN, int MT, int NT, int NS>
__global__ __launch_bounds__(256) void moe_gemm_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Wt, const int32_t* __restrict__ tiles,
                                                      const int32_t* __restrict__ expert_off, const int32_t* __restrict__ slot_row,
                                                      const float* __restrict__ slot_w, void* __restrict__ out, int N, int K, unsigned a_bytes) {
    static_assert(WM * WN == 4, "four waves");
    constexpr int BM = WM * MT * 16, BN = WN * NT * 16;
    constexpr int NPA = BM / 32, NPW = BN / 32, NLD = NPA + NPW;      // LDS-DMA pieces (8 rows) per wave per stage
    constexpr int A_TILE = BM * 128, STAGE = (BM + BN) * 128;
    static_assert(BM % 32 == 0 && BN % 32 == 0 && NS >= 2 && (NS - 2) * NLD < 64, "piece split / vmcnt range");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int rt = blockIdx.y;
    if (rt >= tiles[0]) return;         // past the device-side tile count: before the first barrier
    const int e = tiles[1 + 2 * rt], s0 = tiles[2 + 2 * rt];
    const int mrows = min(BM, expert_off[e + 1] - s0);       // >= 1
    const int n0 = blockIdx.x * BN;
    const bf16_t* Wb = Wt + (int64_t)e * N * K;
    const bf16_t* Ab = FORM == MOE_UP ? A : A + (int64_t)s0 * K;
    const unsigned a_rec = FORM == MOE_UP ? a_bytes : (unsigned)mrows * (unsigned)K * 2u;
    const unsigned w_rec = (unsigned)N * (unsigned)K * 2u;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l15 = lane & 15, g = lane >> 4;

    // ---- staging: wave w owns A pieces [NPA w, NPA (w + 1)) and W pieces [NPW w, NPW (w + 1)); lane -> (row = 8 piece + lane / 8, physical chunk lane % 8)
    const int srow = lane >> 3;
    const unsigned chunk_off = (unsigned)(((lane & 7) ^ srow) * 16);
    unsigned a_vo[NPA], w_vo[NPW];
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
        int r = (wave * NPA + i) * 8 + srow;
        r = r < mrows ? r : mrows - 1;
        const unsigned src = FORM == MOE_UP ? (unsigned)slot_row[s0 + r] : (unsigned)r;
        a_vo[i] = src * (unsigned)K * 2u + chunk_off;
    }
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
        int gn = n0 + (wave * NPW + i) * 8 + srow;
        gn = gn < N ? gn : N - 1;
        w_vo[i] = (unsigned)gn * (unsigned)K * 2u + chunk_off;
    }
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned dma_a0 = lds0 + (unsigned)wave * (NPA * 1024), dma_w0 = lds0 + A_TILE + (unsigned)wave * (NPW * 1024);
    const int nk = K / BK;
    auto issue = [&](int kt) {      // stage kt -> buffer kt % NS; past the last k-step: zero-sized descriptors, no traffic
        const unsigned buf = (unsigned)(kt % NS) * STAGE, soff = (unsigned)kt * (BK * 2);
        const unsigned ar = kt < nk ? a_rec : 0u, wr = kt < nk ? w_rec : 0u;
#pragma unroll
        for (int i = 0; i < NPA; ++i)
            dma16(__builtin_amdgcn_make_buffer_rsrc((void*)Ab, 0, ar, 0x00020000), a_vo[i], kt < nk ? soff : 0u, dma_a0 + buf + (unsigned)i * 1024u);
#pragma unroll
        for (int i = 0; i < NPW; ++i)
            dma16(__builtin_amdgcn_make_buffer_rsrc((void*)Wb, 0, wr, 0x00020000), w_vo[i], kt < nk ? soff : 0u, dma_w0 + buf + (unsigned)i * 1024u);
    };

    // ---- fragment read addresses: logical chunk g + 4 kk of row l15 (+ 16 t), (row & 7) == (l15 & 7)
    const unsigned sw0 = (unsigned)((g ^ (l15 & 7)) << 4), sw1 = (unsigned)(((g + 4) ^ (l15 & 7)) << 4);
    const unsigned a_row = lds0 + (unsigned)((wm * (16 * MT) + l15) * 128);
    const unsigned w_row = lds0 + A_TILE + (unsigned)((wn * (16 * NT) + l15) * 128);

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s = 0; s < NS - 1; ++s) issue(s);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * NLD) : "memory");      // my pieces of stage kt landed (loads retire in issue order)
        __builtin_amdgcn_s_barrier();       // ... everybody's; and everybody is done reading the buffer of stage kt - 1
        asm volatile("" ::: "memory");
        issue(kt + NS - 1);
        const unsigned buf = (unsigned)(kt % NS) * STAGE;
        bf16x8 af0[MT], af1[MT], wf0[NT], wf1[NT];
        static_for<MT>([&](auto t_tag) {
            constexpr int t = decltype(t_tag)::value;
            af0[t] = lds_read16<t * 2048>(a_row + sw0 + buf);
            af1[t] = lds_read16<t * 2048>(a_row + sw1 + buf);
        });
        static_for<NT>([&](auto t_tag) {
            constexpr int t = decltype(t_tag)::value;
            wf0[t] = lds_read16<t * 2048>(w_row + sw0 + buf);
            wf1[t] = lds_read16<t * 2048>(w_row + sw1 + buf);
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int t = 0; t < MT; ++t) { landed(af0[t]); landed(af1[t]); }
#pragma unroll
        for (int t = 0; t < NT; ++t) { landed(wf0[t]); landed(wf1[t]); }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf0[j], af0[i], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1[j], af1[i], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the trailing zero-sized requests

    // ---- epilogue: a lane owns out[slot s0 + r][n .. n + 3], r = 16 (MT wm + i) + l15, n = n0 + 16 (NT wn + j) + 4 g
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int r = (wm * MT + i) * 16 + l15;
        if (r >= mrows) continue;
        const int64_t slot = s0 + r;
        const float rw = FORM == MOE_DOWN ? slot_w[slot] : 1.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n0 + (wn * NT + j) * 16 + 4 * g;
            if (n >= N) continue;
            if (FORM == MOE_UP) {
                const f32x4 v = gelu_erf4(acc[i][j]);
                uint2 pk;
                pk.x = pack_bf16x2(v[0], v[1]);
                pk.y = pack_bf16x2(v[2], v[3]);
                *(uint2*)((bf16_t*)out + slot * N + n) = pk;
            } else {
                *(f32x4*)((float*)out + slot * N + n) = acc[i][j] * rw;
            }
        }
    }
}

template <int FORM, int WM, int WN, int MT, int NT, int NS>
int launch_gemm(const void* A, const void* W, const int32_t* tiles, const int32_t* expert_off, const int32_t* slot_row, const float* slot_w, void* out,
                int max_tiles, int N, int K, unsigned a_bytes, hipStream_t s) {
    constexpr int BM = WM * MT * 16, BN = WN * NT * 16;
    constexpr size_t lds = (size_t)NS * (BM + BN) * 128;
    static_assert(lds <= 64 * 1024, "no dynamic-LDS attribute is set");
    hipLaunchKernelGGL((moe_gemm_kernel<FORM, WM, WN, MT, NT, NS>), dim3((unsigned)((N + BN - 1) / BN), (unsigned)max_tiles), dim3(256), lds, s,
                       (const bf16_t*)A, (const bf16_t*)W, tiles, expert_off, slot_row, slot_w, out, N, K, a_bytes);
    MQ_CHECK_LAUNCH("mq_moe_gemm");
    return MQ_OK;
}

// ---- combine + LayerNorm -------------------------------------------------------------------------------------------------------------------------------
template <int CH>
__global__ __launch_bounds__(256) void moe_combine_ln_kernel(float* x, const float* __restrict__ Y, const int32_t* __restrict__ row_slot,
                                                            const float* __restrict__ bias, const float* __restrict__ gam, const float* __restrict__ bet,
                                                            bf16_t* __restrict__ h, int64_t rows, int W, int k, int nslots, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nch = W >> 2;
    int sl[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int s = row_slot[row * k + (j < k ? j : 0)];
        sl[j] = s < 0 ? 0 : (s >= nslots ? nslots - 1 : s);
    }
    f32x4 v[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        if (c >= nch) { v[i] = f32x4{0.f, 0.f, 0.f, 0.f}; continue; }
        f32x4 t = *(const f32x4*)(x + row * W + c * 4) + *(const f32x4*)(Y + (int64_t)sl[0] * W + c * 4);
        if (k == 2) t = t + *(const f32x4*)(Y + (int64_t)sl[1] * W + c * 4);
        v[i] = t + *(const f32x4*)(bias + c * 4);
    }
    ln_normalize_row<CH>(v, lane, nch, W, eps);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        if (c >= nch) continue;
        const f32x4 gv = *(const f32x4*)(gam + c * 4), bv = *(const f32x4*)(bet + c * 4);
        f32x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = v[i][j] * gv[j] + bv[j];
        *(f32x4*)(x + row * W + c * 4) = y;
        uint2 pk;
        pk.x = pack_bf16x2(y[0], y[1]);
        pk.y = pack_bf16x2(y[2], y[3]);
        *(uint2*)(h + row * W + c * 4) = pk;
    }
}

int check_moe_shape(const char* what, int64_t rows, int32_t E, int32_t k) {
    MQ_CHECK_ARG(E >= 2 && E <= MOE_MAX_E, "%s: experts %d outside [2, 16]", what, E);
    MQ_CHECK_ARG((k == 1 || k == 2) && k <= E, "%s: top_k %d must be 1 or 2", what, k);
    MQ_CHECK_ARG(rows >= 0 && rows <= (int64_t)1 << 29, "%s: rows %lld outside [0, 2^29]", what, (long long)rows);
    return MQ_OK;
}
int check_bm(const char* what, int32_t bm) {
    MQ_CHECK_ARG(bm == MOE_BM_TALL || bm == MOE_BM_SHORT, "%s: tile height %d (128 or 32; mq_moe_tile_rows picks one)", what, bm);
    return MQ_OK;
}

}  // namespace

extern "C" int32_t mq_moe_tile_rows(int64_t rows, int32_t experts, int32_t top_k) {
    return experts > 0 && rows * top_k / experts > MOE_TALL_FROM ? MOE_BM_TALL : MOE_BM_SHORT;
}

extern "C" int64_t mq_moe_max_tiles(int64_t rows, int32_t experts, int32_t top_k, int32_t bm) {
    return bm > 0 ? rows * top_k / bm + experts : 0;
}

extern "C" int mq_moe_route(const float* d_x, const float* d_router_w, int32_t* d_top_e, float* d_top_w, int64_t rows, int32_t W, int32_t experts,
                            int32_t top_k, void* stream) {
    MQ_CHECK_ARG(d_x && d_router_w && d_top_e && d_top_w, "mq_moe_route: null pointer");
    MQ_TRY(check_moe_shape("mq_moe_route", rows, experts, top_k));
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= 2048, "mq_moe_route: width %d must be a multiple of 64, at most 2048", W);
    if (rows == 0) return MQ_OK;
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(3, s);
    MQ_DISPATCH_CH(W, hipLaunchKernelGGL((moe_route_kernel<CH>), dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, d_x, d_router_w, d_top_e, d_top_w, rows,
                                         W, experts, top_k));
    MQ_CHECK_LAUNCH("mq_moe_route");
    return MQ_OK;
}

extern "C" int mq_moe_plan(const int32_t* d_top_e, const float* d_top_w, int64_t rows, int32_t experts, int32_t top_k, int32_t bm, int32_t* d_expert_off,
                           int32_t* d_slot_row, float* d_slot_w, int32_t* d_row_slot, int32_t* d_tiles, void* stream) {
    MQ_CHECK_ARG(d_top_e && d_top_w && d_expert_off && d_slot_row && d_slot_w && d_row_slot && d_tiles, "mq_moe_plan: null pointer");
    MQ_TRY(check_moe_shape("mq_moe_plan", rows, experts, top_k));
    MQ_TRY(check_bm("mq_moe_plan", bm));
    if (rows == 0) return MQ_OK;
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(3, s);
    hipLaunchKernelGGL(moe_plan_kernel, dim3(1), dim3(PLAN_WAVES * 64), 0, s, d_top_e, d_top_w, (int)(rows * top_k), top_k, experts, bm,
                       (int)mq_moe_max_tiles(rows, experts, top_k, bm), d_expert_off, d_slot_row, d_slot_w, d_row_slot, d_tiles);
    MQ_CHECK_LAUNCH("mq_moe_plan");
    return MQ_OK;
}

extern "C" int mq_moe_gemm(int32_t form, const void* d_A, const void* d_W, const int32_t* d_tiles, const int32_t* d_expert_off, const int32_t* d_slot_row,
                           const float* d_slot_w, void* d_out, int64_t rows, int32_t experts, int32_t top_k, int32_t bm, int32_t N, int32_t K, void* stream) {
    MQ_CHECK_ARG(form == MQ_MOE_UP || form == MQ_MOE_DOWN, "mq_moe_gemm: form %d (MQ_MOE_UP or MQ_MOE_DOWN)", form);
    MQ_CHECK_ARG(d_A && d_W && d_tiles && d_expert_off && d_slot_row && d_slot_w && d_out, "mq_moe_gemm: null pointer");
    MQ_TRY(check_moe_shape("mq_moe_gemm", rows, experts, top_k));
    MQ_TRY(check_bm("mq_moe_gemm", bm));
    MQ_CHECK_ARG(N >= 64 && N % 64 == 0 && K >= 64 && K % 64 == 0, "mq_moe_gemm: N %d and K %d must be multiples of 64", N, K);
    MQ_CHECK_ARG((int64_t)N * K * 2 < (int64_t)1 << 32, "mq_moe_gemm: an expert matrix of N %d x K %d is past the 32-bit staging offsets", N, K);
    MQ_CHECK_ARG(rows * K * 2 < (int64_t)1 << 32, "mq_moe_gemm: rows %lld x K %d is past the 32-bit gather offsets", (long long)rows, K);
    if (rows == 0) return MQ_OK;
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(0, s, 2.0 * (double)rows * top_k * (double)N * (double)K);
    const int mt = (int)mq_moe_max_tiles(rows, experts, top_k, bm);
    MQ_CHECK_ARG(mt <= 65535, "mq_moe_gemm: %d row tiles of %d slots are past the grid's 65535", mt, bm);
    const unsigned a_bytes = (unsigned)(rows * K * 2);
#define MQ_MOE_GEMM(FORM)                                                                                                                                \
    (bm == MOE_BM_TALL ? launch_gemm<FORM, 2, 2, 4, 4, 2>(d_A, d_W, d_tiles, d_expert_off, d_slot_row, d_slot_w, d_out, mt, N, K, a_bytes, s)            \
                       : launch_gemm<FORM, 1, 4, 2, 1, 4>(d_A, d_W, d_tiles, d_expert_off, d_slot_row, d_slot_w, d_out, mt, N, K, a_bytes, s))
    return form == MQ_MOE_UP ? MQ_MOE_GEMM(MOE_UP) : MQ_MOE_GEMM(MOE_DOWN);
#undef MQ_MOE_GEMM
}

extern "C" int mq_moe_combine_ln(float* d_x, const float* d_Y, const int32_t* d_row_slot, const float* d_bias, const float* d_g, const float* d_b,
                                 void* d_h_bf16, int64_t rows, int32_t W, int32_t top_k, float eps, void* stream) {
    MQ_CHECK_ARG(d_x && d_Y && d_row_slot && d_bias && d_g && d_b && d_h_bf16, "mq_moe_combine_ln: null pointer");
    MQ_CHECK_ARG(top_k == 1 || top_k == 2, "mq_moe_combine_ln: top_k %d must be 1 or 2", top_k);
    MQ_CHECK_ARG(W >= 64 && W % 64 == 0 && W <= 2048, "mq_moe_combine_ln: width %d must be a multiple of 64, at most 2048", W);
    MQ_CHECK_ARG(rows >= 0 && rows <= (int64_t)1 << 29, "mq_moe_combine_ln: rows %lld outside [0, 2^29]", (long long)rows);
    if (rows == 0) return MQ_OK;
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(1, s);
    MQ_DISPATCH_CH(W, hipLaunchKernelGGL((moe_combine_ln_kernel<CH>), dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, d_x, d_Y, d_row_slot, d_bias, d_g,
                                         d_b, (bf16_t*)d_h_bf16, rows, W, top_k, (int)(rows * top_k), eps));
    MQ_CHECK_LAUNCH("mq_moe_combine_ln");
    return MQ_OK;
}
