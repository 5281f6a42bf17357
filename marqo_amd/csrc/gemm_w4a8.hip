// MXFP4 x MXFP8 (W4A8) TILED GEMM on the MX matrix instruction, and the activation quantiser in front of it (Mistral / Llama with weight_precision
// "mxfp4-a8": the calls of an MXFP4-only tower that are too tall for the skinny kernel).
//
//   out[M, N] = epi( dequant(A8[M, K]) @ dequant(W4[N, K])^T )
//
// W4: the e2m1 codes and e8m0 block scales EXACTLY as mq_quantize_weights_mxfp4 writes them (the top of gemm_small_w4.hip): the tower keeps one copy.
// A8: e4m3fn codes and one e8m0 scale per 32 consecutive k, written by mq_quantize_rows_mxfp8 below.  Both operands go to
// v_mfma_scale_f32_16x16x128_f8f6f4 as they are stored — no decode, one MFMA per 128 k and 16 x 16 outputs, the block scales applied by the instruction.
// Any M >= 1, N % 4 == 0, K % 64 == 0.
//
// The activation format.  scale = 2^ceil(log2(absmax_block / 448)) (1 for an all-zero block; the exponent is kept inside [-100, 100], so the byte
// 127 + exponent is never 0xff = NaN), code = RNE(a / scale) in e4m3fn: |a / scale| <= 448, nothing saturates (blocks above 448 x 2^100 aside, which
// are clamped).  A code times 2^k is exactly a bf16 value.
// Storage (private to this file: the quantiser writes it, the GEMM reads it).  One buffer of mq_a8_bytes(M, ld8, K) bytes:
//   * codes [M, ld8], ld8 >= ceil(K / 128) 128, ld8 % 16 == 0: a row is whole 128-byte chunks, a 32-block is 32 consecutive bytes.  The weight storage
//     fixes the order inside a block: the MFMA's fp4 operand is 4 registers, lane group g holding block g; it takes dword g of each of the chunk's
//     four 16-byte pieces, and byte i of the dword of piece q holds k = 8 q + i in its low nibble (fp4 position 8 q + 2 i) and k = 8 q + 4 + i in its
//     high nibble (position 8 q + 2 i + 1).  So inside a block byte 8 q + 2 i holds k = 8 q + i and byte 8 q + 2 i + 1 holds k = 8 q + 4 + i: each
//     8-group in the order [0, 4, 1, 5, 2, 6, 3, 7].  A block's dot product does not care, as long as both operands agree.
//     The MFMA's fp8 operand is 8 registers and is NOT 32 consecutive k per lane (measured with one-hot operands on an MI355X): registers 0 .. 3 of lane
//     group g are positions 16 g .. 16 g + 15 of the 128, registers 4 .. 7 positions 64 + 16 g .. + 15 — two 64-deep halves — while the scale of block b
//     comes from lane group b on both operands.  So lane group g reads the 16-byte pieces g and 4 + g of the row's chunk, and supplies block g's scale.
//   * scales behind the codes, at byte M ld8: 512 bytes per (128-row tile, chunk), tile-major; byte g 128 + l15 8 + mt of such a record is block g of
//     tile row 16 mt + l15.  That is the GEMM's register image: ONE 8-byte load gives lane (l15, g) its scale for each of the 8 row tiles, and the MFMA's
//     scale byte select (an immediate) picks mt & 3 of dword mt >> 2.  The records of rows past M in the last tile are never written and feed only sums
//     that are never stored.
//   * A half last chunk (K % 128 == 64) is padded with code 0 and scale byte 127 — on both operands (mq_quantize_weights_mxfp4 pads the same way) —
//     so lane groups 2 and 3 contribute exactly zero there, and no byte that the MFMA reads is a stray 0x7f / 0xff (an e4m3 NaN).
// The quantiser: a workgroup per row, a thread per 16 consecutive k (two 16-byte loads, one 16-byte store), two neighbouring lanes per block; one read pass.
//
// The GEMM: a 128 x 256 output tile per workgroup, 8 wave64s SIDE BY SIDE ALONG N, a k-step of one 128-deep chunk = ONE MX MFMA per 16 x 16 outputs
// (the tile, the tile walk and the epilogue are gemm_w4.hip's).  Per chunk and wave: 2 W fragments, 8 A fragments, 16 MFMAs.
//   * W never enters the LDS and is never decoded.  Per chunk and column tile a lane loads the 16 bytes gemm_w4.hip loads (dword j = its lane group's
//     eight codes of block j) and the dword of scales.  The MFMA wants the TRANSPOSE across the lane groups (lane group g: dword g of the four pieces):
//     two v_permlane32_swap and two v_permlane16_swap per column tile, and a shift brings scale byte g down.
//   * A8 through an LDS ring by LDS-DMA (dma16): a stage is 128 rows x 128 B = 16 KB, wave w stages rows [16 w, 16 w + 16) in 2 pieces of 8 rows.  The
//     eight 16-byte pieces of a row are XOR-swizzled on the SOURCE address with gemm_fp8.hip's function of the row, under which a ds_read_b128 of a
//     fragment (logical piece g, then 4 + g, of row 16 mt + l15) hits 16 distinct slots per 16 lanes.  The A scales go global -> VGPR beside the W loads.
//   * Everything is issued TWO chunks ahead, by one cursor: at chunk s the W codes and scales and the A scales of chunk s + 2 (into the register slot
//     chunk s has just emptied: the loop is unrolled by two, so a slot is a fixed set of registers and nothing pending is ever copied), then the two
//     LDS-DMA pieces of stage s + 2 into the ring buffer stage s - 1 left: 7 vector-memory operations per chunk and wave, retired in issue order.
//       top of chunk s : s_waitcnt vmcnt(7) — all but the newest 7 have landed: everything chunk s - 2 issued, stage s and the registers of chunk s
//                        among it; only what chunk s - 1 issued may still be in flight — then the barrier: every wave's pieces of stage s are there, and
//                        every wave has finished reading stage s - 1;
//       then           : the loads of chunk s + 2, the 16 ds_read_b128 of chunk s, and 8 x (wait for one fragment, 2 MFMAs).
//     Three stages (48 KB) are what this form can use: the wait that proves chunk s drains every older operation.  Past the workgroup's last tile the
//     A descriptor's size drops to 0 (no traffic) and the cursor stays on its last chunk: the count per chunk, what vmcnt(7) leans on, is the same
//     everywhere.  A tile's epilogue stores sit in the same counter behind the loads in flight: the next wait is then stricter than it needs to be, never looser.
//   * A half last chunk needs no special case: the pads above make it a chunk like any other, and no A byte past the row's chunks is read.
//   * Determinism: one accumulator per output, k in chunk order by one wave, no split-K; which rows share a tile changes nothing a row's sums see.
// Departures from the design the feature was specified with: (1) W by ONE 16-byte load and the permlane transpose, not four dword loads — a quarter of the
// W load instructions, and each dword load would touch the same 16 cache lines as the 16-byte one; the dword form was not built, so not measured;
// (2) the A scales in a tile-major record of their own, not 4 bytes per row: a per-row layout costs 8 scattered dword loads per chunk and lane, this
// one 8-byte load; (3) two chunks of issue-ahead on BOTH operands where gemm_w4.hip has one on W: a chunk here is 16 MFMAs, not 64, so one chunk hides
// half the latency.  Ring depths other than 3 were not run (see above: a deeper ring needs a deeper W slot ring with it).  DESIGN.md §3 / §6.
//
// Measured (profiles/w4a8_gemm.txt, 1x MI355X): quantiser + GEMM 0.54 - 0.65 x mq_gemm_w4's time at the four Mistral-7B GEMMs and 512 / 2048 / 8192 rows,
// 0.68 - 1.23 x mq_gemm_bf16's on the dequantised copy; the GEMM alone reaches 0.70 - 0.80 of the sustained bf16 MFMA rate at 8192 rows.  The
// instruction's 128-deep sum is not an fp32 sum: its error stays near 2^-13 of the sum of magnitudes (tests/test_gemm_w4a8_gpu.py).
//
// Compiler report (gfx950, this unit): the GEMM, 3 instantiations, one per epilogue: 204 VGPRs, no AGPRs, no scratch, no spill each -> 2 waves per
// SIMD = the one workgroup per CU the launch asks for (48 KB of LDS).  The quantiser: 42 VGPRs, no scratch -> 8 waves per SIMD.
#include "common.h"
#include "gemm_loop.h"
#include "gemm_sched.h"
#include "w4_decode.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int A8_BM = 128, A8_BN = 256, A8_NW = 8, A8_MT = A8_BM / 16, A8_NT = 2, A8_NS = 3;
constexpr int A8_STAGE = A8_BM * W4_BK;              // 16 KB of e4m3 codes
constexpr int A8_PIECES = A8_BM / 8 / A8_NW;         // LDS-DMA pieces (8 rows x 128 B = 1 KiB) per wave and stage
constexpr int A8_OPS = 2 * A8_NT + 1 + A8_PIECES;    // vector-memory operations per chunk and wave: W codes + W scales, the A scales, the pieces
constexpr int A8_SLOTS = 256;                        // one workgroup per CU
constexpr int A8_REC = A8_BM * 4;                    // bytes of A scales per (row tile, chunk)

// gemm_fp8.hip's piece swizzle: u = (row >> 1) & 7;  f = u for u in {0, 1, 6, 7}, u ^ 2 for u in {2, 3, 4, 5}
__device__ __forceinline__ int a8_swz(int row) {
    const int u = (row >> 1) & 7;
    return u ^ ((((u >> 1) ^ (u >> 2)) & 1) << 1);
}

// a 32-byte fragment = two ds_read_b128 as inline asm (the compiler cannot tell an LDS read from the LDS-DMA writes in flight: gemm_bf16.hip)
template <int OFF>
__device__ __forceinline__ i32x8 a8_read32(unsigned addr0, unsigned addr1) {
    i32x4 lo, hi;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(lo) : "v"(addr0), "n"(OFF));
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(hi) : "v"(addr1), "n"(OFF));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// the 4 x 4 dword transpose across the lane groups: in, register j of lane group g = codes of (block j, piece g); out, register q of lane group g =
// (block g, piece q) — the 32 codes of block g in the MFMA's fp4 order.  permlane32_swap exchanges lanes 32 .. 63 of its first operand with lanes
// 0 .. 31 of its second, permlane16_swap the odd 16-lane rows of the first with the even rows of the second.
__device__ __forceinline__ i32x8 a8_transpose(const u32x4& r) {
    const auto s02 = __builtin_amdgcn_permlane32_swap(r[0], r[2], false, false);
    const auto s13 = __builtin_amdgcn_permlane32_swap(r[1], r[3], false, false);
    const auto p01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
    const auto p23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
    return i32x8{(int)p01[0], (int)p01[1], (int)p23[0], (int)p23[1], 0, 0, 0, 0};   // (an fp4 operand is read from the first four registers)
}

template <int FLAGS>
__global__ __launch_bounds__(A8_NW * 64) void gemm_w4a8_kernel(const uint8_t* __restrict__ A8, int64_t ld8, const uint8_t* __restrict__ AS, const uint8_t* __restrict__ W4,
                                                               int64_t ld4, const uint8_t* __restrict__ S, int64_t lds, const float* __restrict__ bias, const void* residual,
                                                               void* out, int64_t ldc, int M, int N, int nk, int tiles_n, int num_tiles, int cgroup, int band_rows,
                                                               unsigned a_bytes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool F32_OUT = (FLAGS & MQ_EPI_OUT_F32) != 0;
    const GemmTileMap<A8_BM, A8_BN> tile_map(num_tiles, tiles_n, M, cgroup, band_rows);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;

    // ---- sources of the cursor's tile.  A staging: piece i of wave w is tile rows 16 w + 8 i .. + 7; lane -> (row + lane / 8, physical piece lane % 8),
    // which fetches the logical piece (lane % 8) ^ a8_swz(row).  W: lane (l15, g) of column tile t reads weight row n0 + 32 w + 16 t + l15 (a column past
    // N reads the last row: never stored).  A scales: the record of (row tile, chunk), bytes g 128 + l15 8 .. + 7.
    unsigned a_vo[A8_PIECES];
    const uint8_t* wrow[A8_NT];
    const uint32_t* srow[A8_NT];
    const uint8_t* asrc;
    auto set_sources = [&](int m0, int n0) {
#pragma unroll
        for (int i = 0; i < A8_PIECES; ++i) {
            const int row = wave * 16 + i * 8 + (lane >> 3);
            int gm = m0 + row; gm = gm < M ? gm : M - 1;
            a_vo[i] = (unsigned)gm * (unsigned)ld8 + (unsigned)(((lane & 7) ^ a8_swz(row)) * 16);
        }
#pragma unroll
        for (int t = 0; t < A8_NT; ++t) {
            int gn = n0 + wave * 32 + t * 16 + l15; gn = gn < N ? gn : N - 1;
            wrow[t] = W4 + (int64_t)gn * ld4 + g * 16;
            srow[t] = (const uint32_t*)(S + (int64_t)gn * lds);
        }
        asrc = AS + (int64_t)(m0 / A8_BM) * nk * A8_REC + g * 128 + l15 * 8;
    };
    int l_vbid = blockIdx.x, l_k = 0;   // the cursor: (tile, chunk) of the next loads, two chunks ahead of the MFMAs
    unsigned a_rec = a_bytes;
    {
        int m0, n0;
        tile_map.origin(blockIdx.x, m0, n0);
        set_sources(m0, n0);
    }
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned dma0 = lds0 + (unsigned)wave * (16 * W4_BK);
    u32x4 wq[2][A8_NT];     // the two register slots: chunk s is in slot s & 1
    uint32_t ws[2][A8_NT];
    uint2 as[2];
    auto issue = [&](auto slot_tag, int buf) {
        constexpr int P = decltype(slot_tag)::value;
#pragma unroll
        for (int t = 0; t < A8_NT; ++t) {
            wq[P][t] = *(const u32x4*)(wrow[t] + (int64_t)l_k * 64);
            ws[P][t] = srow[t][l_k];
        }
        as[P] = *(const uint2*)(asrc + (int64_t)l_k * A8_REC);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < A8_PIECES; ++i)
            dma16(__builtin_amdgcn_make_buffer_rsrc((void*)A8, 0, a_rec, 0x00020000), a_vo[i], (unsigned)l_k * W4_BK, dma0 + (unsigned)(buf * A8_STAGE + i * 1024));
        __builtin_amdgcn_sched_barrier(0);
        if (l_k + 1 < nk) ++l_k;
        else if (l_vbid + (int)gridDim.x < num_tiles) {
            l_k = 0;
            l_vbid += gridDim.x;
            int m0, n0;
            tile_map.origin(l_vbid, m0, n0);
            set_sources(m0, n0);
        } else a_rec = 0;   // past the last tile: the loads repeat its last chunk (never used), the pieces move nothing
    };

    // ---- prologue: chunks 0 and 1 of the workgroup's walk (the first vmcnt(7) leaves exactly chunk 1's operations in flight)
    issue(std::integral_constant<int, 0>{}, 0);
    issue(std::integral_constant<int, 1>{}, 1);

    // fragment reads: row 16 mt + l15 (a8_swz(row) = a8_swz(l15)), logical pieces g and 4 + g (the 8-register operand's two halves, see the top)
    const unsigned fr = (unsigned)a8_swz(l15);
    const unsigned rd0 = lds0 + (unsigned)(l15 * W4_BK) + (((unsigned)g ^ fr) << 4), rd1 = lds0 + (unsigned)(l15 * W4_BK) + (((4u + g) ^ fr) << 4);

    f32x4 acc[A8_MT][A8_NT];
    auto zero_acc = [&]() {
#pragma unroll
        for (int mt = 0; mt < A8_MT; ++mt)
#pragma unroll
            for (int t = 0; t < A8_NT; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    zero_acc();
    int c_vbid = blockIdx.x, kc = 0, cur = 0;   // the MFMAs' tile and chunk; the ring buffer chunk s reads
    int cm0, cn0;
    tile_map.origin(c_vbid, cm0, cn0);

    // one chunk out of register slot P; true when the workgroup's last tile is finished
    auto step = [&](auto slot_tag) -> bool {
        constexpr int P = decltype(slot_tag)::value;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A8_OPS) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        i32x8 wf[A8_NT];
        int wsc[A8_NT];
#pragma unroll
        for (int t = 0; t < A8_NT; ++t) {
            wf[t] = a8_transpose(wq[P][t]);
            wsc[t] = (int)(ws[P][t] >> (8 * g));   // (the MFMA reads byte 0)
        }
        const int asc[2] = {(int)as[P].x, (int)as[P].y};
        __builtin_amdgcn_sched_barrier(0);
        issue(slot_tag, cur == 0 ? A8_NS - 1 : cur - 1);
        const unsigned b0 = rd0 + (unsigned)(cur * A8_STAGE), b1 = rd1 + (unsigned)(cur * A8_STAGE);
        i32x8 af[A8_MT];   // the chunk's 16 reads go out together; the MFMAs of row tile mt wait for its two only (LDS reads return in order)
        static_for<A8_MT>([&](auto mt_tag) { constexpr int mt = decltype(mt_tag)::value; af[mt] = a8_read32<mt * 16 * W4_BK>(b0, b1); });
        static_for<A8_MT>([&](auto mt_tag) {
            constexpr int mt = decltype(mt_tag)::value;
            asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * (A8_MT - 1 - mt)) : "memory");
            landed(af[mt]);
#pragma unroll
            for (int t = 0; t < A8_NT; ++t)
                acc[mt][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[t], af[mt], acc[mt][t], /*fp4*/ 4, /*e4m3*/ 0, 0, wsc[t], mt & 3, asc[mt >> 2]);
            __builtin_amdgcn_sched_barrier(0);   // (else the scheduler gathers all 16 MFMAs behind the last wait)
        });
        // (nothing else keeps the chunk's MFMAs — pure, their results unused until the next chunk — in front of the next barrier: gemm_fp8.hip)
#pragma unroll
        for (int mt = 0; mt < A8_MT; ++mt)
#pragma unroll
            for (int t = 0; t < A8_NT; ++t) landed(acc[mt][t]);
        cur = cur + 1 == A8_NS ? 0 : cur + 1;
        if (++kc < nk) return false;
        // ---- epilogue: lane owns out[m][n .. n + 3], m = cm0 + 16 mt + l15, n = cn0 + 32 wave + 16 t + 4 g
#pragma unroll
        for (int t = 0; t < A8_NT; ++t) {
            const int n = cn0 + wave * 32 + t * 16 + g * 4;
            if (n >= N) continue;
            f32x4 bias_v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (FLAGS & MQ_EPI_BIAS) bias_v = *(const f32x4*)(bias + n);
#pragma unroll
            for (int mt = 0; mt < A8_MT; ++mt) {
                const int m = cm0 + mt * 16 + l15;
                if (m >= M) continue;
                f32x4 v = acc[mt][t];
                if (FLAGS & MQ_EPI_BIAS) v += bias_v;
                const int64_t o = (int64_t)m * ldc + n;
                if (FLAGS & MQ_EPI_RESIDUAL) v += *(const f32x4*)((const float*)residual + o);
                if (F32_OUT) {
                    *(f32x4*)((float*)out + o) = v;
                } else {
                    uint2 q;
                    q.x = pack_bf16x2(v[0], v[1]);
                    q.y = pack_bf16x2(v[2], v[3]);
                    *(uint2*)((bf16_t*)out + o) = q;
                }
            }
        }
        kc = 0;
        c_vbid += gridDim.x;
        if (c_vbid >= num_tiles) return true;
        tile_map.origin(c_vbid, cm0, cn0);
        zero_acc();
        return false;
    };
    for (;;) {
        if (step(std::integral_constant<int, 0>{})) break;
        if (step(std::integral_constant<int, 1>{})) break;
    }
    // the trailing (out-of-range) requests must have retired before the workgroup's LDS can be handed to another one
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- the activation quantiser: a workgroup per row, a thread per 16 consecutive k = 16 bytes of codes, two neighbouring lanes per 32-block ----
__global__ __launch_bounds__(256) void quantize_rows_mxfp8_kernel(const bf16_t* __restrict__ A, int64_t lda, uint8_t* __restrict__ A8, int64_t ld8,
                                                                  uint8_t* __restrict__ AS, int K, int nk) {
    const int64_t row = blockIdx.x;
    const bf16_t* a = A + row * lda;
    uint8_t* o = A8 + row * ld8;
    uint8_t* so = AS + (row >> 7) * nk * A8_REC + (row & 15) * 8 + ((row >> 4) & 7);   // + chunk 512 + block 128
    for (int k = threadIdx.x * 16; k < nk * W4_BK; k += 4096) {
        uint8_t* sb = so + (k >> 7) * A8_REC + ((k >> 5) & 3) * 128;
        if (k >= K) {   // the padding of a half last chunk (K % 32 == 0: the two lanes of a block leave together)
            *(u32x4*)(o + k) = u32x4{0u, 0u, 0u, 0u};
            if (!(k & 16)) *sb = 127;
            continue;
        }
        const u32x4 p[2] = {*(const u32x4*)(a + k), *(const u32x4*)(a + k + 8)};
        float x[16];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x[2 * e] = __uint_as_float(p[e >> 2][e & 3] << 16);
            x[2 * e + 1] = __uint_as_float(p[e >> 2][e & 3] & 0xffff0000u);
        }
        float mx = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, fabsf(x[e]));
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        // 2^ceil(log2(mx / 448)) without a logarithm: mx = f 2^e with f in [0.5, 1), 448 = 0.875 x 2^9, so the ceiling is e - 9 for f <= 0.875, e - 8 above
        int ex = 0;
        if (mx > 0.f) {
            int e;
            const float f = frexpf(mx, &e);
            ex = min(max(f <= 0.875f ? e - 9 : e - 8, -100), 100);
        }
        const float inv = ldexpf(1.f, -ex);
        if (!(k & 16)) *sb = (uint8_t)(127 + ex);
        auto code = [&](int e) { return __builtin_amdgcn_fmed3f(x[e] * inv, -448.f, 448.f); };   // (the product is exact; the clamp acts above 448 x 2^100 only)
        u32x4 c;
#pragma unroll
        for (int h = 0; h < 2; ++h) {   // an 8-group in the order [0, 4, 1, 5, 2, 6, 3, 7]
            int lo = __builtin_amdgcn_cvt_pk_fp8_f32(code(8 * h + 0), code(8 * h + 4), 0, false);
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(code(8 * h + 1), code(8 * h + 5), lo, true);
            int hi = __builtin_amdgcn_cvt_pk_fp8_f32(code(8 * h + 2), code(8 * h + 6), 0, false);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(code(8 * h + 3), code(8 * h + 7), hi, true);
            c[2 * h] = (uint32_t)lo;
            c[2 * h + 1] = (uint32_t)hi;
        }
        *(u32x4*)(o + k) = c;
    }
}

struct A8Args { const void* A8; int64_t ld8; const void* W4; int64_t ld4; const void* S; int64_t lds; const float* bias; const void* residual; void* out; int64_t ldc; int64_t M; int N, K; };

template <int FLAGS>
int launch_a8(const A8Args& a, hipStream_t s) {
    constexpr int LDS = A8_NS * A8_STAGE;
    static std::atomic<uint64_t> attr_done{0};
    auto kern = gemm_w4a8_kernel<FLAGS>;
    if (hipError_t e = mq_ensure_dyn_lds((const void*)kern, LDS, attr_done); e != hipSuccess) {
        mq_set_error("mq_gemm_w4a8: hipFuncSetAttribute: %s", hipGetErrorString(e));
        return MQ_ERR_HIP;
    }
    const int nk = (int)w4_chunks(a.K);
    const uint8_t* scales = (const uint8_t*)a.A8 + (size_t)a.M * (size_t)a.ld8;
    // the codes go through 32-bit buffer offsets, in rows of whole chunks: row chunks as the other tiled GEMMs (whole 128-row tiles: the scale records follow)
    return gemm_row_chunks("mq_gemm_w4a8", a.M, a.N, nk * W4_BK, a.ld8, 0, 1, A8_BM, A8_BN, A8_SLOTS, [&](int64_t r0, int m, const GemmGeom& g) {
        const GemmRows v = gemm_rows_from<FLAGS, 1>(r0, a.A8, a.ld8, (const float*)a.residual, a.out, a.ldc);
        hipLaunchKernelGGL(kern, dim3(g.grid), dim3(A8_NW * 64), LDS, s, (const uint8_t*)v.A, a.ld8, scales + (size_t)(r0 / A8_BM) * nk * A8_REC, (const uint8_t*)a.W4, a.ld4,
                           (const uint8_t*)a.S, a.lds, a.bias, (const void*)v.residual, v.out, a.ldc, m, a.N, nk, g.tiles_n, g.num_tiles, g.cgroup, g.band_rows, g.a_bytes);
        MQ_CHECK_LAUNCH("mq_gemm_w4a8");
        return MQ_OK;
    });
}

int check_a8(const char* who, int64_t ld8, int64_t M, int64_t K) {
    MQ_CHECK_ARG(K >= W4_KMULT && K % W4_KMULT == 0 && K < (1LL << 30), "%s: K=%ld must be a multiple of %d", who, (long)K, W4_KMULT);
    MQ_CHECK_ARG(M >= 1 && M < (1LL << 31), "%s: M=%ld unsupported", who, (long)M);
    MQ_CHECK_ARG(ld8 % 16 == 0 && ld8 >= w4_chunks(K) * W4_BK, "%s: ld8=%ld must be a multiple of 16 and at least %ld (128 code bytes per 128-deep chunk)", who, (long)ld8,
                 (long)(w4_chunks(K) * W4_BK));
    return MQ_OK;
}

}  // namespace

extern "C" size_t mq_a8_bytes(int64_t M, int64_t ld8, int64_t K) {
    if (M < 1 || ld8 < 1 || K < 1) return 0;
    return (size_t)M * (size_t)ld8 + (size_t)cdiv64(M, A8_BM) * (size_t)w4_chunks(K) * A8_REC;
}

extern "C" int mq_quantize_rows_mxfp8(const void* d_A, int64_t lda, void* d_A8, int64_t ld8, int64_t M, int64_t K, void* stream) {
    MQ_CHECK_ARG(d_A && d_A8, "mq_quantize_rows_mxfp8: null pointer");
    MQ_TRY(check_a8("mq_quantize_rows_mxfp8", ld8, M, K));
    MQ_CHECK_ARG(lda % 8 == 0 && lda >= K, "mq_quantize_rows_mxfp8: lda=%ld must keep 16-byte rows of K elements", (long)lda);
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(1, s);
    hipLaunchKernelGGL(quantize_rows_mxfp8_kernel, dim3((unsigned)M), dim3(256), 0, s, (const bf16_t*)d_A, lda, (uint8_t*)d_A8, ld8, (uint8_t*)d_A8 + (size_t)M * (size_t)ld8,
                       (int)K, (int)w4_chunks(K));
    MQ_CHECK_LAUNCH("mq_quantize_rows_mxfp8");
    return MQ_OK;
}

extern "C" int mq_gemm_w4a8(const void* d_A8, int64_t ld8, const void* d_W4, int64_t ld4, const void* d_scale, int64_t lds, const float* d_bias, const void* d_residual,
                            void* d_out, int64_t ldc, int64_t M, int64_t N, int64_t K, int flags, void* stream) {
    MQ_CHECK_ARG(d_A8 && d_W4 && d_scale && d_out, "mq_gemm_w4a8: null operand");
    MQ_TRY(check_a8("mq_gemm_w4a8", ld8, M, K));
    MQ_CHECK_ARG(N >= 4 && N % 4 == 0 && N < (1LL << 31) - A8_BN, "mq_gemm_w4a8: shape M=%ld N=%ld K=%ld unsupported (M >= 1, N a multiple of 4)", (long)M, (long)N, (long)K);
    MQ_CHECK_ARG(!(flags & MQ_EPI_BIAS) || d_bias, "mq_gemm_w4a8: MQ_EPI_BIAS without bias");
    MQ_CHECK_ARG(!(flags & MQ_EPI_RESIDUAL) || d_residual, "mq_gemm_w4a8: MQ_EPI_RESIDUAL without residual");
    MQ_CHECK_ARG(ldc % 4 == 0 && ldc >= N, "mq_gemm_w4a8: ldc=%ld must keep 16-byte rows of N elements", (long)ldc);
    MQ_CHECK_ARG(ld4 % 16 == 0 && ld4 >= w4_chunks(K) * 64, "mq_gemm_w4a8: ld4=%ld must be a multiple of 16 and at least %ld (64 bytes per 128-deep chunk)", (long)ld4,
                 (long)(w4_chunks(K) * 64));
    MQ_CHECK_ARG(lds % 4 == 0 && lds >= w4_chunks(K) * 4, "mq_gemm_w4a8: lds=%ld must be a multiple of 4 and at least %ld (4 scale bytes per 128-deep chunk)", (long)lds,
                 (long)(w4_chunks(K) * 4));
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(0, s, 2.0 * (double)M * (double)N * (double)K);
    const A8Args a{d_A8, ld8, d_W4, ld4, d_scale, lds, d_bias, d_residual, d_out, ldc, M, (int)N, (int)K};
    switch (flags) {
        case 0: return launch_a8<0>(a, s);
        case MQ_EPI_BIAS: return launch_a8<MQ_EPI_BIAS>(a, s);
        case MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32: return launch_a8<MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32>(a, s);   // fp32 residual, may alias out
        default:
            mq_set_error("mq_gemm_w4a8: unsupported epilogue flag combination 0x%x", flags);
            return MQ_ERR_INVALID;
    }
}
