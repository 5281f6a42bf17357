// MXFP4 W4A16 skinny GEMM for the decoder towers' query path (Mistral / Llama: a single query is bound by weight bytes; 4.25 bits per weight).
//
//   out[M, N] = epi( A[M, K] @ dequant(W4[N, K])^T ),   A bf16, W4 e2m1 codes, one e8m0 power-of-two scale per block of 32 consecutive k
//
// The weight format (shared with mq_quantize_weights_mxfp4 below and tests/w4_ref.py), OCP MX FP4 with K % 64 == 0:
//   scale[n, b] = 2^ceil(log2(absmax_block / 6)) (1 for an all-zero block; the exponent is kept inside [-100, 100]), stored as the e8m0 byte 127 + exponent;
//   code = RNE(w / scale) onto {0, 0.5, 1, 1.5, 2, 3, 4, 6} with a sign bit: code = s.ee.m, magnitude index 0 .. 7 in grid order; a tie goes to the
//   neighbour whose mantissa bit m is 0 (the even index).  absmax <= 6 scale, so nothing saturates (blocks above 6 x 2^100 aside, which no weight holds).
// An e2m1 value times 2^k is exactly a bf16 value: the quantiser rewrites the bf16 weight with decode x scale, and the tiled bf16 kernels that run
// the calls too tall for this one compute with the same numbers.
//
// Storage (private to this file: the quantiser writes it, the kernel reads it, everything else sees values).  K is walked in chunks of 128 = four
// blocks; a row's last chunk is padded with zero codes when K % 128 == 64.  Codes [N, ld4] bytes, ld4 >= ceil(K / 128) 64: chunk c of row n is 64
// bytes, FRAGMENT-MAJOR: the 16 bytes at c 64 + g 16 belong to lane group g (0 .. 3) and hold one dword per block j (0 .. 3) of the chunk; dword j
// holds the eight codes of k = c 128 + j 32 + g 8 + e, e = 0 .. 7 — the 8 k of lane group g in the B fragment of one mfma_f32_16x16x32_bf16 —,
// byte i of the dword = code e = i in its LOW nibble and code e = 4 + i in its HIGH nibble.  Scales [N, lds] bytes, lds >= ceil(K / 128) 4: byte
// c 4 + j is block j of chunk c.  So one 16-byte load gives a lane its codes for four MFMAs, one 4-byte load the four scales, and dword j, scale
// byte j and MFMA j line up; the A fragment of MFMA j is the natural 16 B at k = c 128 + j 32 + g 8.
//
// Design:
//   * Block scale and MFMA step coincide: a 32-block is one mfma_f32_16x16x32_bf16 k-step, and the scale is folded into the decoded bf16 fragment
//     before the MFMA as an exponent: the fp32 accumulator never sees a scale.
//   * Decode by a table in registers: for a block's scale byte a lane builds the eight scaled magnitudes' bf16 LOW bytes and HIGH bytes as two
//     8-byte tables (four VGPRs, ~9 VALU); v_perm_b32 looks four codes up per instruction (selector = the 3 magnitude bits, one AND away from the
//     packed dword), the sign bit is OR'ed into the high bytes, two more v_perm_b32 interleave low and high bytes into bf16 pairs: 8 perms + 6
//     logic ops per 8 codes, no conversion instruction, no arithmetic on the values.  Zero (index 0 decodes to 0 at every scale) and the
//     one subnormal (index 1 = 0.5: exponent field of the scale's own, mantissa 0) are table entries like any other, and an exponent kept inside
//     [-100, 100] cannot underflow or overflow bf16 (0.5 x 2^-100 .. 6 x 2^100).  v_cvt_scalef32_pk_bf16_fp4 was not tried: DESIGN.md §3.
//   * Work split (gemm_small_w8.hip's): a workgroup owns 16 output columns for all rows of its row group (<= 80), its NW waves split K into
//     contiguous runs of chunks; partial sums meet in LDS and are added in wave order (deterministic), then bias / residual, 8- or 16-byte stores.
//   * Issue-ahead, retuned for half the bytes per k: a group is G chunks (G x 128 k: 16 G bytes of codes per lane); the codes and scales of group
//     i + 1 are issued behind group i's A loads and before its decode and MFMAs.  A chunk costs 16 MT VGPRs of A fragments; the measured plan is
//     G = 1 — one 128-deep chunk per group, the k depth of the W8 kernel's two —, deeper groups were slower (dispatch_w4_plan below).  G changes
//     no bit (a wave walks its chunks in k order whatever the grouping).
// A row's bits do not depend on the other rows of the call: NW is chosen from (N, K) alone, a wave's chunk run from (K, NW), and a padded block
// (both operands zero) adds +0 to a sum that is never -0.
//
// Compiler report (gfx950, this unit, 66 GEMM instantiations + the quantiser): no scratch, no spill anywhere, at most 203 VGPRs (depth 2, 4 row tiles).
// The committed plan (depth 1), VGPRs [+ AGPRs] -> waves per SIMD the registers allow, 1 .. 5 row tiles: 8 waves 60 -> 8, 75 -> 6, 96 -> 5, 118 -> 4,
// 140 -> 3; 4 waves 56 + 4 -> 8, 67 + 8 -> 6, 84 + 12 -> 5, 102 + 16 -> 4, 121 + 20 -> 3; the same for the three epilogues.  Quantiser: 41 -> 8.
#include "common.h"
#include "knobs.h"
#include "w4_decode.h"

bool mq_gemm_small_ok(int64_t M, int64_t N, int64_t K, bool ln);
bool mq_gemm_small_grouped_ok(int64_t M, int64_t N, int64_t K);

namespace {

constexpr int W4_BN = 16;       // output columns per workgroup
constexpr int W4_MAX_MT = 5;    // 16-row tiles per row group: 80 rows, as gemm_small.hip
// (W4_BK = 128, W4_KMULT = 64, W4Table / w4_table / w4_decode8, w4_chunks: w4_decode.h, shared with the tiled kernel)

template <int FLAGS, int MT, int NW, int G>
__global__ __launch_bounds__(NW * 64) void gemm_small_w4_kernel(const bf16_t* __restrict__ A, int64_t lda, const uint8_t* __restrict__ W4, int64_t ld4,
                                                                const uint8_t* __restrict__ S, int64_t lds, const float* __restrict__ bias, const void* residual,
                                                                void* out, int64_t ldc, int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool F32_OUT = (FLAGS & MQ_EPI_OUT_F32) != 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * W4_BN;
    if (gridDim.y > 1) {   // row groups: workgroup (x, y) owns slice x for rows [y 16 MT, (y + 1) 16 MT); the slice comes from HBM once, then from L2
        const int64_t r0 = (int64_t)blockIdx.y * (MT * 16);
        A += r0 * lda;
        if (FLAGS & MQ_EPI_RESIDUAL) residual = (const char*)residual + r0 * ldc * 4;
        out = (char*)out + r0 * ldc * (F32_OUT ? 4 : 2);
        M = min(M - (int)r0, MT * 16);
    }
    f32x4* part = (f32x4*)smem;   // [NW][MT][64 lanes]

    const int nchunks = (K + W4_BK - 1) / W4_BK;
    const int per = (nchunks + NW - 1) / NW;
    const int c0 = wave * per, c1 = min(c0 + per, nchunks);
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wn = n0 + l15 < N ? n0 + l15 : N - 1;   // (a column past N reads the last row: its sums are never stored)
    const uint8_t* wrow = W4 + (int64_t)wn * ld4 + g * 16;
    const uint32_t* srow = (const uint32_t*)(S + (int64_t)wn * lds);
    const bf16_t* arow[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) arow[t] = A + (int64_t)min(t * 16 + l15, M - 1) * lda + g * 8;

    u32x4 wq[G];
    uint32_t ws[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        wq[j] = c0 + j < c1 ? *(const u32x4*)(wrow + (int64_t)(c0 + j) * 64) : u32x4{0u, 0u, 0u, 0u};
        ws[j] = c0 + j < c1 ? srow[c0 + j] : 0x7f7f7f7fu;
    }
    for (int kc = c0; kc < c1; kc += G) {
        bf16x8 af[G][4][MT];
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int k0 = (kc + j) * W4_BK + b * 32;               // (K % 64 == 0: a block is inside K or past it as a whole)
                const bool in_k = kc + j < c1 && k0 < K;
                const int ka = in_k ? k0 : c0 * W4_BK;                  // (an address inside the row either way)
#pragma unroll
                for (int t = 0; t < MT; ++t) af[j][b][t] = in_k && t * 16 + l15 < M ? *(const bf16x8*)(arow[t] + ka) : bf16x8{};
            }
        u32x4 wnext[G];   // the HBM stream of the next group, in flight under this group's decode and MFMAs
        uint32_t snext[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            wnext[j] = kc + G + j < c1 ? *(const u32x4*)(wrow + (int64_t)(kc + G + j) * 64) : u32x4{0u, 0u, 0u, 0u};
            snext[j] = kc + G + j < c1 ? srow[kc + G + j] : 0x7f7f7f7fu;
        }
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const bf16x8 wf = w4_decode8(wq[j][b], w4_table((ws[j] >> (8 * b)) & 0xffu));
#pragma unroll
                for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[j][b][t], acc[t], 0, 0, 0);
            }
#pragma unroll
        for (int j = 0; j < G; ++j) {
            wq[j] = wnext[j];
            ws[j] = snext[j];
        }
    }
    // ---- cross-wave reduction in LDS, fixed order ----
#pragma unroll
    for (int t = 0; t < MT; ++t) part[(wave * MT + t) * 64 + lane] = acc[t];
    __syncthreads();
    // ---- epilogue: wave w finishes row tiles w, w + NW, ...; a lane owns out[m][n .. n + 3], m = t 16 + l15, n = n0 + 4 g ----
    const int n = n0 + g * 4;
    if (n >= N) return;
    f32x4 bias_v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (FLAGS & MQ_EPI_BIAS) bias_v = *(const f32x4*)(bias + n);
    for (int t = wave; t < MT; t += NW) {
        const int m = t * 16 + l15;
        if (m >= M) continue;
        f32x4 v = part[(0 * MT + t) * 64 + lane];
#pragma unroll
        for (int w = 1; w < NW; ++w) v += part[(w * MT + t) * 64 + lane];
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

struct W4Args { const void* A; int64_t lda; const void* W4; int64_t ld4; const void* S; int64_t lds; const float* bias; const void* residual; void* out; int64_t ldc; int M, N, K; };

template <int FLAGS, int MT, int NW, int G>
int launch_w4(const W4Args& a, hipStream_t s) {
    const size_t lds = (size_t)NW * MT * 64 * 16;   // <= 40 KB
    const unsigned groups = (unsigned)((a.M + MT * 16 - 1) / (MT * 16));
    hipLaunchKernelGGL((gemm_small_w4_kernel<FLAGS, MT, NW, G>), dim3((unsigned)((a.N + W4_BN - 1) / W4_BN), groups), dim3(NW * 64), lds, s, (const bf16_t*)a.A,
                       a.lda, (const uint8_t*)a.W4, a.ld4, (const uint8_t*)a.S, a.lds, a.bias, a.residual, a.out, a.ldc, a.M, a.N, a.K);
    MQ_CHECK_LAUNCH("mq_gemm_small_w4");
    return MQ_OK;
}

// Waves per workgroup and chunks per group, from the sweep over the four Mistral-7B GEMMs at 8 / 32 / 80 rows.  Waves from N alone, so
// that a row's sums do not depend on the row count: up to 256 column slices (N <= 4096: one workgroup per CU at most) run 8 waves — N = 4096,
// K = 14336, 8 rows: 17.6 us against 24.1 —, wider weights 4 (N = 28672, 80 rows: 144 us against 151).  One chunk per group (128 k: what two of the
// W8 kernel's chunks hold) was the fastest depth or within about 2 % of it at every point; 4 chunks cost up to 35 % (N = 28672, 8 rows, 8 waves).  "w4_waves" / "w4_depth" (mq_tune) force a variant where it is instantiated (depth 4 up to 2 row tiles, 2 up to 4:
// 16 MT G VGPRs of A fragments): how the sweep was run.
template <int FLAGS, int MT>
int dispatch_w4_plan(const W4Args& a, hipStream_t s) {
    const bool w8 = mq_w4_waves == 4 || mq_w4_waves == 8 ? mq_w4_waves == 8 : a.N <= 4096;
    constexpr int GMAX = MT <= 2 ? 4 : MT <= 4 ? 2 : 1;
    const int want = mq_w4_depth == 2 || mq_w4_depth == 4 ? (int)mq_w4_depth : 1;
    const int depth = want < GMAX ? want : GMAX;
    if constexpr (GMAX >= 4)
        if (depth == 4) return w8 ? launch_w4<FLAGS, MT, 8, 4>(a, s) : launch_w4<FLAGS, MT, 4, 4>(a, s);
    if constexpr (GMAX >= 2)
        if (depth == 2) return w8 ? launch_w4<FLAGS, MT, 8, 2>(a, s) : launch_w4<FLAGS, MT, 4, 2>(a, s);
    return w8 ? launch_w4<FLAGS, MT, 8, 1>(a, s) : launch_w4<FLAGS, MT, 4, 1>(a, s);
}

template <int FLAGS>
int dispatch_w4_mt(const W4Args& a, hipStream_t s) {
    // more than 80 rows: the fewest row groups of at most 5 row tiles, then the smallest height that covers them (as gemm_small.hip)
    const int mt_all = (a.M + 15) / 16, groups = (mt_all + W4_MAX_MT - 1) / W4_MAX_MT;
    const int mt = (mt_all + groups - 1) / groups;
    if (mt <= 1) return dispatch_w4_plan<FLAGS, 1>(a, s);
    if (mt <= 2) return dispatch_w4_plan<FLAGS, 2>(a, s);
    if (mt <= 3) return dispatch_w4_plan<FLAGS, 3>(a, s);
    if (mt <= 4) return dispatch_w4_plan<FLAGS, 4>(a, s);
    return dispatch_w4_plan<FLAGS, 5>(a, s);
}

// ---- the quantiser: one workgroup per weight row, a thread per 8 consecutive k = one dword of codes, four neighbouring lanes per 32-block:
//      block absmax -> exponent -> codes -> the bf16 row rewritten with decode(code) * scale; the padding of a last half chunk gets zero codes ----
__global__ __launch_bounds__(256) void quantize_mxfp4_kernel(bf16_t* __restrict__ W, int64_t ldw, uint8_t* __restrict__ W4, int64_t ld4, uint8_t* __restrict__ S,
                                                             int64_t lds, int K) {
    bf16_t* w = W + (int64_t)blockIdx.x * ldw;
    uint8_t* o = W4 + (int64_t)blockIdx.x * ld4;
    uint8_t* so = S + (int64_t)blockIdx.x * lds;
    const int kpad = (K + W4_BK - 1) / W4_BK * W4_BK;
    for (int k = threadIdx.x * 8; k < kpad; k += 2048) {
        const int c = k >> 7, j = (k >> 5) & 3, g = (k >> 3) & 3;
        uint32_t* dst = (uint32_t*)(o + c * 64 + g * 16 + j * 4);
        if (k >= K) {   // (K % 32 == 0: the four lanes of a block leave together)
            *dst = 0u;
            if (g == 0) so[c * 4 + j] = 127;
            continue;
        }
        const u32x4 p = *(const u32x4*)(w + k);
        float x[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x[2 * e] = __uint_as_float(p[e] << 16);
            x[2 * e + 1] = __uint_as_float(p[e] & 0xffff0000u);
        }
        float mx = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf(x[e]));
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        // 2^ceil(log2(mx / 6)) without a logarithm: mx = f 2^e with f in [0.5, 1), 6 = 0.75 x 2^3, so mx / 6 = (f / 0.75) 2^(e - 3) and the ceiling is
        // e - 3 for f <= 0.75, e - 2 above; kept inside [-100, 100] (0.5 x 2^-100 .. 6 x 2^100 are bf16 normals with room to spare)
        int ex = 0;
        if (mx > 0.f) {
            int e;
            const float f = frexpf(mx, &e);
            ex = min(max(f <= 0.75f ? e - 3 : e - 2, -100), 100);
        }
        const float sc = ldexpf(1.f, ex), inv = ldexpf(1.f, -ex);
        if (g == 0) so[c * 4 + j] = (uint8_t)(127 + ex);
        uint32_t code = 0u, back[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            // RNE onto the grid: steps of 0.5 below 2 (index = 2 a), 1 below 4 (a + 2), 2 up to 6 (a / 2 + 4); rintf's ties go to the even integer,
            // which is the even index = mantissa bit 0 in each of the three ranges (and the ranges meet on grid points)
            const float a = fabsf(x[e]) * inv;
            const int mi = a < 2.f ? (int)rintf(a * 2.f) : a < 4.f ? (int)rintf(a) + 2 : min((int)rintf(a * 0.5f) + 4, 7);
            const uint32_t sign = __float_as_uint(x[e]) >> 31;
            code |= (sign << 3 | (uint32_t)mi) << (e < 4 ? 8 * e : 8 * (e - 4) + 4);
            const float v = mi < 2 ? 0.5f * (float)mi : ldexpf(1.f + 0.5f * (float)(mi & 1), (mi >> 1) - 1);
            back[e] = (__float_as_uint(v * sc) | sign << 31) >> 16;       // exact: nothing below bit 16
        }
        *dst = code;
        u32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = back[2 * e] | back[2 * e + 1] << 16;
        *(u32x4*)(w + k) = r;
    }
}

}  // namespace

// exactly the calls gemm_small.hip takes (<= 80 rows in one group, up to small_m_grouped in row groups) whose K is a whole number of 64-deep half chunks
extern "C" int mq_gemm_small_w4_ok(int64_t M, int64_t N, int64_t K) {
    return (mq_gemm_small_ok(M, N, K, false) || mq_gemm_small_grouped_ok(M, N, K)) && K % W4_KMULT == 0;
}

extern "C" int mq_gemm_small_w4(const void* d_A, int64_t lda, const void* d_W4, int64_t ld4, const void* d_scale, int64_t lds, const float* d_bias,
                                const void* d_residual, void* d_out, int64_t ldc, int64_t M, int64_t N, int64_t K, int flags, void* stream) {
    MQ_CHECK_ARG(d_A && d_W4 && d_scale && d_out, "mq_gemm_small_w4: null operand");
    MQ_CHECK_ARG(K >= W4_KMULT && K % W4_KMULT == 0, "mq_gemm_small_w4: K=%ld must be a multiple of %d", (long)K, W4_KMULT);
    MQ_CHECK_ARG(mq_gemm_small_w4_ok(M, N, K), "mq_gemm_small_w4: shape M=%ld N=%ld K=%ld unsupported", (long)M, (long)N, (long)K);
    MQ_CHECK_ARG(!(flags & MQ_EPI_BIAS) || d_bias, "mq_gemm_small_w4: MQ_EPI_BIAS without bias");
    MQ_CHECK_ARG(!(flags & MQ_EPI_RESIDUAL) || d_residual, "mq_gemm_small_w4: MQ_EPI_RESIDUAL without residual");
    MQ_CHECK_ARG(lda % 8 == 0 && lda >= K && ldc % 4 == 0 && ldc >= N, "mq_gemm_small_w4: lda=%ld / ldc=%ld must keep 16-byte rows of K / N elements", (long)lda, (long)ldc);
    MQ_CHECK_ARG(ld4 % 16 == 0 && ld4 >= w4_chunks(K) * 64, "mq_gemm_small_w4: ld4=%ld must be a multiple of 16 and at least %ld (64 bytes per 128-deep chunk)",
                 (long)ld4, (long)(w4_chunks(K) * 64));
    MQ_CHECK_ARG(lds % 4 == 0 && lds >= w4_chunks(K) * 4, "mq_gemm_small_w4: lds=%ld must be a multiple of 4 and at least %ld (4 scale bytes per 128-deep chunk)",
                 (long)lds, (long)(w4_chunks(K) * 4));
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(0, s, 2.0 * (double)M * (double)N * (double)K);
    const W4Args a{d_A, lda, d_W4, ld4, d_scale, lds, d_bias, d_residual, d_out, ldc, (int)M, (int)N, (int)K};
    switch (flags) {
        case 0: return dispatch_w4_mt<0>(a, s);
        case MQ_EPI_BIAS: return dispatch_w4_mt<MQ_EPI_BIAS>(a, s);
        case MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32: return dispatch_w4_mt<MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32>(a, s);   // fp32 residual, may alias out
        default:
            mq_set_error("mq_gemm_small_w4: unsupported epilogue flag combination 0x%x", flags);
            return MQ_ERR_INVALID;
    }
}

extern "C" int mq_quantize_weights_mxfp4(void* d_W_bf16, int64_t ldw, void* d_W4, int64_t ld4, void* d_scale, int64_t lds, int64_t N, int64_t K, void* stream) {
    MQ_CHECK_ARG(d_W_bf16 && d_W4 && d_scale, "mq_quantize_weights_mxfp4: null pointer");
    MQ_CHECK_ARG(N >= 1 && N < (1LL << 31) && K >= W4_KMULT && K % W4_KMULT == 0 && K < (1LL << 30), "mq_quantize_weights_mxfp4: bad shape N=%ld K=%ld (K a multiple of %d)",
                 (long)N, (long)K, W4_KMULT);
    MQ_CHECK_ARG(ldw % 8 == 0 && ldw >= K, "mq_quantize_weights_mxfp4: ldw=%ld must keep 16-byte rows of K elements", (long)ldw);
    MQ_CHECK_ARG(ld4 % 16 == 0 && ld4 >= w4_chunks(K) * 64, "mq_quantize_weights_mxfp4: ld4=%ld must be a multiple of 16 and at least %ld (64 bytes per 128-deep chunk)",
                 (long)ld4, (long)(w4_chunks(K) * 64));
    MQ_CHECK_ARG(lds % 4 == 0 && lds >= w4_chunks(K) * 4, "mq_quantize_weights_mxfp4: lds=%ld must be a multiple of 4 and at least %ld (4 scale bytes per 128-deep chunk)",
                 (long)lds, (long)(w4_chunks(K) * 4));
    hipLaunchKernelGGL(quantize_mxfp4_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (bf16_t*)d_W_bf16, ldw, (uint8_t*)d_W4, ld4, (uint8_t*)d_scale, lds,
                       (int)K);
    MQ_CHECK_LAUNCH("mq_quantize_weights_mxfp4");
    return MQ_OK;
}
