// MXFP4 W4A16 TILED GEMM for the decoder towers' indexing batches (Mistral / Llama with weight_precision "mxfp4-only": no bf16 block matrix is resident,
// every call too tall for the skinny kernel of gemm_small_w4.hip runs here, from the same codes).
//
//   out[M, N] = epi( A[M, K] @ dequant(W4[N, K])^T ),   A bf16, W4 e2m1 codes + e8m0 block scales exactly as mq_quantize_weights_mxfp4 writes them
//
// (the format and its fragment-major storage: the top of gemm_small_w4.hip; the decode: w4_decode.h).  Any M >= 1, N % 4 == 0, K % 64 == 0.
//
// Design: a 128 x 256 output tile per workgroup, 8 wave64s SIDE BY SIDE ALONG N, a k-step of one 128-deep chunk (four 32-blocks = four MFMA k-steps).
//   * W never enters the LDS.  Wave w owns columns [32 w, 32 w + 32) of the tile — two 16-column tiles — for ALL 8 row tiles.  Per chunk and column
//     tile a lane loads 16 B of codes (the B fragments of four mfma_f32_16x16x32_bf16) and one dword of scales, global -> VGPR; it decodes each
//     fragment once (w4_table + w4_decode8, ~32 VALU) and feeds it to 8 MFMAs, one per row tile.  No two waves decode the same codes.  The codes and
//     scales of chunk s + 1 are issued at the top of chunk s, under its 64 MFMAs.
//   * A through an LDS ring by LDS-DMA (dma16, gemm_loop.h): a stage is the tile's 128 rows x 128 k = 32 KB, rows of 256 B whose sixteen 16-byte
//     pieces are XOR-swizzled with (row & 15) on the SOURCE address, so that the 16 rows of a fragment read hit 16 different bank groups.  All 8 waves
//     read the same A fragments (ds_read_b128, 8 per 32-block and wave); wave w stages rows [16 w, 16 w + 16) in 4 pieces of 4 rows.
//   * Ring discipline, THREE stages (96 KB, one workgroup per CU), one barrier per chunk.  Vector-memory operations retire in issue order, and a
//     chunk issues 4 W loads, then 4 LDS-DMA pieces:
//       top of chunk s : s_waitcnt vmcnt(4) — all but the newest 4 operations have landed: everything chunk s - 2 and earlier issued (stage s among
//                        it) and chunk s - 1's W loads (the codes of chunk s); only stage s + 1 may still be in flight — then the barrier: every
//                        wave's pieces of stage s are there, and every wave has finished reading stage s - 1;
//       then           : the W loads of chunk s + 1, the 4 pieces of stage s + 2 into the buffer stage s - 1 just left, and the 4 x (2 decodes,
//                        8 LDS reads, 16 MFMAs) of chunk s.
//     So an A stage has two chunks (128 MFMAs per wave) to land and the codes one.  The in-order counter is why a fourth stage buys nothing in this
//     form: the wait that proves the codes of chunk s also drains every older piece.  The walk runs on across the workgroup's tiles (the DMA cursor
//     two chunks ahead of the MFMAs, the W cursor one); past the last tile the A descriptor's size drops to 0 (no traffic, zeros) and the W cursor
//     stays on its last chunk, which keeps the count of operations per chunk — what vmcnt(4) leans on — the same everywhere.
//   * A row's last chunk may be half (K % 128 == 64): its upper two blocks are skipped (their codes are zero, but the A bytes past K are not ours).
//   * Tile walk: GemmTileMap (gemm_loop.h), persistent, 256 slots.  Determinism: one accumulator per output, k summed in chunk order by one wave, no
//     split-K; which rows share a tile changes nothing a row's sums see.
//   * Epilogue: a lane owns out[m][n .. n + 3] (operands are fed swapped, as everywhere here): bias, fp32 residual (may alias out: a lane reads the
//     element it then writes), 8- or 16-byte stores.
// Departures from the design the feature was specified with: none in form (8 waves x 32 columns against 128 rows, W global -> VGPR, A by LDS-DMA);
// the ring has 3 stages, not "the whole 160 KB", for the reason above.  NOT built: the fallback form (decode W to bf16 into the LDS, both operands from
// the LDS), a two-chunk-ahead W prefetch (it would free the ring's fourth stage), v_cvt_scalef32_pk_bf16_fp4 (not tried).  DESIGN.md §3 / §6.
//
// Measured: 1.35 - 2.03 x mq_gemm_bf16's time on the dequantised copy at the Mistral-7B GEMMs, 0.41 of the sustained MFMA rate.
//
// Compiler report (gfx950, this unit, 3 instantiations, one per epilogue): 134 VGPRs, no AGPRs, no scratch, no spill each -> 3 waves per SIMD by
// registers; the 96 KB of LDS make it one workgroup = 2 waves per SIMD.
#include "common.h"
#include "gemm_loop.h"
#include "gemm_sched.h"
#include "w4_decode.h"

namespace {

constexpr int T4_BM = 128, T4_BN = 256, T4_NW = 8, T4_MT = T4_BM / 16, T4_NT = 2, T4_NS = 3;
constexpr int T4_STAGE = T4_BM * W4_BK * 2;          // 32 KB
constexpr int T4_PIECES = T4_BM / 4 / T4_NW;         // LDS-DMA pieces (4 rows = 1 KiB each) per wave and stage
constexpr int T4_SLOTS = 256;                        // one workgroup per CU

template <int FLAGS>
__global__ __launch_bounds__(T4_NW * 64) void gemm_w4_kernel(const bf16_t* __restrict__ A, int64_t lda, const uint8_t* __restrict__ W4, int64_t ld4,
                                                             const uint8_t* __restrict__ S, int64_t lds, const float* __restrict__ bias, const void* residual,
                                                             void* out, int64_t ldc, int M, int N, int K, int tiles_n, int num_tiles, int cgroup, int band_rows,
                                                             unsigned a_bytes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool F32_OUT = (FLAGS & MQ_EPI_OUT_F32) != 0;
    const GemmTileMap<T4_BM, T4_BN> tile_map(num_tiles, tiles_n, M, cgroup, band_rows);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int nk = (K + W4_BK - 1) / W4_BK;

    // ---- A staging: piece i of wave w is tile rows 16 w + 4 i .. + 3; lane -> (row + lane / 16, physical 16-B piece lane % 16), which fetches the
    // logical piece (lane % 16) ^ (row & 15), row & 15 = 4 i + lane / 16
    unsigned a_vo[T4_PIECES];
    auto set_a_sources = [&](int m0) {
#pragma unroll
        for (int i = 0; i < T4_PIECES; ++i) {
            const int r15 = 4 * i + g;
            int gm = m0 + wave * 16 + r15; gm = gm < M ? gm : M - 1;
            a_vo[i] = (unsigned)gm * (unsigned)lda * 2u + (unsigned)((l15 ^ r15) * 16);
        }
    };
    // ---- W fragments: lane (l15, g) of column tile t reads weight row n0 + 32 w + 16 t + l15 (a column past N reads the last row: never stored)
    const uint8_t* wrow[T4_NT];
    const uint32_t* srow[T4_NT];
    auto set_w_sources = [&](int n0) {
#pragma unroll
        for (int t = 0; t < T4_NT; ++t) {
            int gn = n0 + wave * 32 + t * 16 + l15; gn = gn < N ? gn : N - 1;
            wrow[t] = W4 + (int64_t)gn * ld4 + g * 16;
            srow[t] = (const uint32_t*)(S + (int64_t)gn * lds);
        }
    };
    int d_vbid = blockIdx.x, d_k = 0;   // the DMA cursor (two chunks ahead of the MFMAs)
    int w_vbid = blockIdx.x, w_k = 0;   // the W cursor (one chunk ahead)
    unsigned a_rec = a_bytes;
    {
        int m0, n0;
        tile_map.origin(blockIdx.x, m0, n0);
        set_a_sources(m0);
        set_w_sources(n0);
    }
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned dma0 = lds0 + (unsigned)wave * (16 * 256);
    auto issue_a_stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < T4_PIECES; ++i)
            dma16(__builtin_amdgcn_make_buffer_rsrc((void*)A, 0, a_rec, 0x00020000), a_vo[i], (unsigned)d_k * (W4_BK * 2), dma0 + (unsigned)(buf * T4_STAGE + i * 1024));
        if (++d_k == nk) {
            d_k = 0;
            d_vbid += gridDim.x;
            if (d_vbid < num_tiles) {
                int m0, n0;
                tile_map.origin(d_vbid, m0, n0);
                set_a_sources(m0);
            } else a_rec = 0;
        }
    };
    u32x4 wq[T4_NT];
    uint32_t ws[T4_NT];
    auto load_w = [&](u32x4 (&q)[T4_NT], uint32_t (&sc)[T4_NT]) {
#pragma unroll
        for (int t = 0; t < T4_NT; ++t) {
            q[t] = *(const u32x4*)(wrow[t] + (int64_t)w_k * 64);
            sc[t] = srow[t][w_k];
        }
        if (w_k + 1 < nk) ++w_k;
        else if (w_vbid + (int)gridDim.x < num_tiles) {
            w_k = 0;
            w_vbid += gridDim.x;
            int m0, n0;
            tile_map.origin(w_vbid, m0, n0);
            set_w_sources(n0);
        }   // (else: stay on the last chunk — loaded again, never used)
    };

    // ---- prologue: stage 0, the codes of chunk 0, stage 1 (in this order: the first vmcnt(4) leaves exactly stage 1 in flight)
    issue_a_stage(0);
    __builtin_amdgcn_sched_barrier(0);
    load_w(wq, ws);
    __builtin_amdgcn_sched_barrier(0);
    issue_a_stage(1);
    __builtin_amdgcn_sched_barrier(0);

    // fragment reads: row mt 16 + l15 (row & 15 = l15), logical piece 4 j + g
    const char* a_row = smem + l15 * 256;
    int cur = 0;   // the ring buffer chunk s reads
    for (int c_vbid = blockIdx.x; c_vbid < num_tiles; c_vbid += gridDim.x) {
        int cm0, cn0;
        tile_map.origin(c_vbid, cm0, cn0);
        f32x4 acc[T4_MT][T4_NT];
#pragma unroll
        for (int mt = 0; mt < T4_MT; ++mt)
#pragma unroll
            for (int t = 0; t < T4_NT; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < nk; ++kc) {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(T4_PIECES) : "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            u32x4 wnext[T4_NT];
            uint32_t snext[T4_NT];
            load_w(wnext, snext);
            __builtin_amdgcn_sched_barrier(0);
            issue_a_stage(cur == 0 ? T4_NS - 1 : cur - 1);
            __builtin_amdgcn_sched_barrier(0);
            const char* st = a_row + cur * T4_STAGE;
            const int nb = min(4, (K - kc * W4_BK) / 32);   // 4, or 2 in a half last chunk
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nb) {
                    bf16x8 wf[T4_NT];
#pragma unroll
                    for (int t = 0; t < T4_NT; ++t) wf[t] = w4_decode8(wq[t][j], w4_table((ws[t] >> (8 * j)) & 0xffu));
                    const int po = ((4 * j + g) ^ l15) * 16;
                    bf16x8 af[T4_MT];   // the block's 8 fragment reads go out together, in front of its MFMAs
#pragma unroll
                    for (int mt = 0; mt < T4_MT; ++mt) af[mt] = *(const bf16x8*)(st + mt * (16 * 256) + po);
#pragma unroll
                    for (int mt = 0; mt < T4_MT; ++mt)
#pragma unroll
                        for (int t = 0; t < T4_NT; ++t) acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t], af[mt], acc[mt][t], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < T4_NT; ++t) {
                wq[t] = wnext[t];
                ws[t] = snext[t];
            }
            cur = cur + 1 == T4_NS ? 0 : cur + 1;
        }
        // ---- epilogue: lane owns out[m][n .. n + 3], m = cm0 + 16 mt + l15, n = cn0 + 32 wave + 16 t + 4 g
#pragma unroll
        for (int t = 0; t < T4_NT; ++t) {
            const int n = cn0 + wave * 32 + t * 16 + g * 4;
            if (n >= N) continue;
            f32x4 bias_v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (FLAGS & MQ_EPI_BIAS) bias_v = *(const f32x4*)(bias + n);
#pragma unroll
            for (int mt = 0; mt < T4_MT; ++mt) {
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
    }
    // the trailing (out-of-range) requests must have retired before the workgroup's LDS can be handed to another one
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

struct T4Args { const void* A; int64_t lda; const void* W4; int64_t ld4; const void* S; int64_t lds; const float* bias; const void* residual; void* out; int64_t ldc; int64_t M; int N, K; };

template <int FLAGS>
int launch_t4(const T4Args& a, hipStream_t s) {
    constexpr int LDS = T4_NS * T4_STAGE;
    static std::atomic<uint64_t> attr_done{0};
    auto kern = gemm_w4_kernel<FLAGS>;
    if (hipError_t e = mq_ensure_dyn_lds((const void*)kern, LDS, attr_done); e != hipSuccess) {
        mq_set_error("mq_gemm_w4: hipFuncSetAttribute: %s", hipGetErrorString(e));
        return MQ_ERR_HIP;
    }
    // A goes through 32-bit buffer offsets: row chunks as the other tiled GEMMs (the codes and scales are addressed by 64-bit pointers: ldw = 0 here)
    return gemm_row_chunks("mq_gemm_w4", a.M, a.N, a.K, a.lda, 0, 2, T4_BM, T4_BN, T4_SLOTS, [&](int64_t r0, int m, const GemmGeom& g) {
        const GemmRows v = gemm_rows_from<FLAGS, 2>(r0, a.A, a.lda, (const float*)a.residual, a.out, a.ldc);
        hipLaunchKernelGGL(kern, dim3(g.grid), dim3(T4_NW * 64), LDS, s, (const bf16_t*)v.A, a.lda, (const uint8_t*)a.W4, a.ld4, (const uint8_t*)a.S, a.lds, a.bias,
                           (const void*)v.residual, v.out, a.ldc, m, a.N, a.K, g.tiles_n, g.num_tiles, g.cgroup, g.band_rows, g.a_bytes);
        MQ_CHECK_LAUNCH("mq_gemm_w4");
        return MQ_OK;
    });
}

}  // namespace

extern "C" int mq_gemm_w4(const void* d_A, int64_t lda, const void* d_W4, int64_t ld4, const void* d_scale, int64_t lds, const float* d_bias, const void* d_residual,
                          void* d_out, int64_t ldc, int64_t M, int64_t N, int64_t K, int flags, void* stream) {
    MQ_CHECK_ARG(d_A && d_W4 && d_scale && d_out, "mq_gemm_w4: null operand");
    MQ_CHECK_ARG(K >= W4_KMULT && K % W4_KMULT == 0 && K < (1LL << 30), "mq_gemm_w4: K=%ld must be a multiple of %d", (long)K, W4_KMULT);
    MQ_CHECK_ARG(M >= 1 && N >= 4 && N % 4 == 0 && N < (1LL << 31) - T4_BN, "mq_gemm_w4: shape M=%ld N=%ld K=%ld unsupported (M >= 1, N a multiple of 4)", (long)M, (long)N,
                 (long)K);
    MQ_CHECK_ARG(!(flags & MQ_EPI_BIAS) || d_bias, "mq_gemm_w4: MQ_EPI_BIAS without bias");
    MQ_CHECK_ARG(!(flags & MQ_EPI_RESIDUAL) || d_residual, "mq_gemm_w4: MQ_EPI_RESIDUAL without residual");
    MQ_CHECK_ARG(lda % 8 == 0 && lda >= K && ldc % 4 == 0 && ldc >= N, "mq_gemm_w4: lda=%ld / ldc=%ld must keep 16-byte rows of K / N elements", (long)lda, (long)ldc);
    MQ_CHECK_ARG(ld4 % 16 == 0 && ld4 >= w4_chunks(K) * 64, "mq_gemm_w4: ld4=%ld must be a multiple of 16 and at least %ld (64 bytes per 128-deep chunk)", (long)ld4,
                 (long)(w4_chunks(K) * 64));
    MQ_CHECK_ARG(lds % 4 == 0 && lds >= w4_chunks(K) * 4, "mq_gemm_w4: lds=%ld must be a multiple of 4 and at least %ld (4 scale bytes per 128-deep chunk)", (long)lds,
                 (long)(w4_chunks(K) * 4));
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(0, s, 2.0 * (double)M * (double)N * (double)K);
    const T4Args a{d_A, lda, d_W4, ld4, d_scale, lds, d_bias, d_residual, d_out, ldc, M, (int)N, (int)K};
    switch (flags) {
        case 0: return launch_t4<0>(a, s);
        case MQ_EPI_BIAS: return launch_t4<MQ_EPI_BIAS>(a, s);
        case MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32: return launch_t4<MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32>(a, s);   // fp32 residual, may alias out
        default:
            mq_set_error("mq_gemm_w4: unsupported epilogue flag combination 0x%x", flags);
            return MQ_ERR_INVALID;
    }
}
