// W8A16 skinny GEMM for the decoder towers' query path (Mistral / Llama: a single query is bound by weight bytes, and e4m3 weights halve them).
//
//   out[M, N] = epi( (A[M, K] @ decode(W8[N, K])^T) * scale[n] ),   A bf16, W8 e4m3fn codes, scale fp32 [N] = a power of two per output row
//
// The weight format (shared with mq_quantize_weights_pow2 below and tests/w8_ref.py): scale[n] = 2^ceil(log2(absmax_n / 448)) (1 for an all-zero row),
// codes = RNE(w / scale[n]): nothing saturates, no NaN code is emitted.  An e4m3 value has 3 mantissa bits, so decode(code) and decode(code) * 2^k
// are exactly bf16 values: the kernel multiplies bf16 activations with the EXACT bf16 image of the codes on the bf16 MFMA and applies 2^k once, in
// fp32, to the finished sum (exact as well).  The quantiser rewrites the bf16 weight with decode * scale, so the tiled bf16 kernels that run the
// calls too tall for this one compute with the same numbers.
//
// Work split (gemm_small.hip's, cut for a 1-byte stream):
//   * a workgroup owns 16 output columns for all rows of its row group (<= 80), its NW waves split K into contiguous runs of 64-deep chunks: the
//     weight matrix is streamed once, by the whole chip;
//   * lane (column l15, k-group g) loads 16 B = 16 consecutive codes of weight row n0 + l15 at k = c 64 + g 16: global -> VGPR, no LDS (a weight byte
//     is used by this wave only).  A chunk is two mfma_f32_16x16x32_bf16: MFMA 0 takes codes 0..7 against A at k = c 64 + g 16 + 0..7, MFMA 1 codes
//     8..15 against ... + 8..15 — the k-permutation inside a chunk is free as long as both operands use it, and A stays 16 B per lane and MFMA
//     (from L2: M x K bf16 is at most 2.3 MB);
//   * e4m3 -> bf16 in registers: v_cvt_pk_f32_fp8 gives two fp32 whose low 16 bits are zero (3 mantissa bits), one v_perm_b32 packs their high
//     halves: exact for all 254 finite codes, subnormals included (DESIGN.md §3 says why this form and not the scaled packed convert);
//   * the weight loads of group i + 1 (G chunks) are issued BEFORE the MFMAs of group i and behind group i's A loads: the HBM stream stays in
//     flight under the conversion and the matrix work, and waiting for A does not wait for it (loads return in order);
//   * partial sums meet in LDS and are added in wave order 0 .. NW - 1 (deterministic), times scale[n], then bias / residual, 8- or 16-byte stores.
// A row's bits do not depend on the other rows of the call: NW is chosen from (N, K) alone, a wave's chunk run from (K, NW), and a padded chunk
// (both operands zero) adds +0 to a sum that is never -0.
#include "common.h"
#include "knobs.h"

bool mq_gemm_small_ok(int64_t M, int64_t N, int64_t K, bool ln);
bool mq_gemm_small_grouped_ok(int64_t M, int64_t N, int64_t K);

namespace {

constexpr int W8_BN = 16;       // output columns per workgroup
constexpr int W8_MAX_MT = 5;    // 16-row tiles per row group: 80 rows, as gemm_small.hip
constexpr int W8_BK = 64;       // codes per lane-row and chunk: 4 k-groups x 16 B

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// four e4m3fn codes (one dword) -> four bf16 (two dwords), exact
__device__ __forceinline__ void e4m3x4_to_bf16x4(uint32_t q, uint32_t& lo, uint32_t& hi) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)q, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)q, true);
    lo = __builtin_amdgcn_perm(__float_as_uint(a[1]), __float_as_uint(a[0]), 0x07060302u);
    hi = __builtin_amdgcn_perm(__float_as_uint(b[1]), __float_as_uint(b[0]), 0x07060302u);
}

template <int FLAGS, int MT, int NW, int G>
__global__ __launch_bounds__(NW * 64) void gemm_small_w8_kernel(const bf16_t* __restrict__ A, int64_t lda, const uint8_t* __restrict__ W8, int64_t ldw,
                                                                const float* __restrict__ scale, const float* __restrict__ bias, const void* residual,
                                                                void* out, int64_t ldc, int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool F32_OUT = (FLAGS & MQ_EPI_OUT_F32) != 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * W8_BN;
    if (gridDim.y > 1) {   // row groups: workgroup (x, y) owns slice x for rows [y 16 MT, (y + 1) 16 MT); the slice comes from HBM once, then from L2
        const int64_t r0 = (int64_t)blockIdx.y * (MT * 16);
        A += r0 * lda;
        if (FLAGS & MQ_EPI_RESIDUAL) residual = (const char*)residual + r0 * ldc * 4;
        out = (char*)out + r0 * ldc * (F32_OUT ? 4 : 2);
        M = min(M - (int)r0, MT * 16);
    }
    f32x4* part = (f32x4*)smem;   // [NW][MT][64 lanes]

    const int nchunks = K / W8_BK;
    const int per = (nchunks + NW - 1) / NW;
    const int c0 = wave * per, c1 = min(c0 + per, nchunks);
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wn = n0 + l15;
    const uint8_t* wrow = W8 + (int64_t)(wn < N ? wn : N - 1) * ldw + g * 16;   // (a column past N reads the last row: its sums are never stored)
    const bf16_t* arow[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) arow[t] = A + (int64_t)min(t * 16 + l15, M - 1) * lda + g * 16;

    u32x4 wq[G];
#pragma unroll
    for (int j = 0; j < G; ++j) wq[j] = c0 + j < c1 ? *(const u32x4*)(wrow + (int64_t)(c0 + j) * W8_BK) : u32x4{0u, 0u, 0u, 0u};
    for (int kc = c0; kc < c1; kc += G) {
        bf16x8 af[G][2][MT];
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const bool in = kc + j < c1 && t * 16 + l15 < M;
                const bf16_t* p = arow[t] + (int64_t)(kc + j < c1 ? kc + j : c0) * W8_BK;
                af[j][0][t] = in ? *(const bf16x8*)p : bf16x8{};
                af[j][1][t] = in ? *(const bf16x8*)(p + 8) : bf16x8{};
            }
        u32x4 wnext[G];   // the HBM stream of the next group, in flight under this group's conversion and MFMAs
#pragma unroll
        for (int j = 0; j < G; ++j) wnext[j] = kc + G + j < c1 ? *(const u32x4*)(wrow + (int64_t)(kc + G + j) * W8_BK) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < G; ++j) {
            u32x4 b0, b1;
            uint32_t lo, hi;
            e4m3x4_to_bf16x4(wq[j][0], lo, hi); b0[0] = lo; b0[1] = hi;
            e4m3x4_to_bf16x4(wq[j][1], lo, hi); b0[2] = lo; b0[3] = hi;
            e4m3x4_to_bf16x4(wq[j][2], lo, hi); b1[0] = lo; b1[1] = hi;
            e4m3x4_to_bf16x4(wq[j][3], lo, hi); b1[2] = lo; b1[3] = hi;
            const bf16x8 w0 = __builtin_bit_cast(bf16x8, b0), w1 = __builtin_bit_cast(bf16x8, b1);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, af[j][0][t], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, af[j][1][t], acc[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < G; ++j) wq[j] = wnext[j];
    }
    // ---- cross-wave reduction in LDS, fixed order ----
#pragma unroll
    for (int t = 0; t < MT; ++t) part[(wave * MT + t) * 64 + lane] = acc[t];
    __syncthreads();
    // ---- epilogue: wave w finishes row tiles w, w + NW, ...; a lane owns out[m][n .. n + 3], m = t 16 + l15, n = n0 + 4 g ----
    const int n = n0 + g * 4;
    if (n >= N) return;
    const f32x4 sc = *(const f32x4*)(scale + n);
    f32x4 bias_v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (FLAGS & MQ_EPI_BIAS) bias_v = *(const f32x4*)(bias + n);
    for (int t = wave; t < MT; t += NW) {
        const int m = t * 16 + l15;
        if (m >= M) continue;
        f32x4 v = part[(0 * MT + t) * 64 + lane];
#pragma unroll
        for (int w = 1; w < NW; ++w) v += part[(w * MT + t) * 64 + lane];
        v *= sc;   // a power of two: exact
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

struct W8Args { const void* A; int64_t lda; const void* W8; int64_t ldw; const float* scale; const float* bias; const void* residual; void* out; int64_t ldc; int M, N, K; };

template <int FLAGS, int MT, int NW, int G>
int launch_w8(const W8Args& a, hipStream_t s) {
    const size_t lds = (size_t)NW * MT * 64 * 16;   // <= 40 KB
    const unsigned groups = (unsigned)((a.M + MT * 16 - 1) / (MT * 16));
    hipLaunchKernelGGL((gemm_small_w8_kernel<FLAGS, MT, NW, G>), dim3((unsigned)((a.N + W8_BN - 1) / W8_BN), groups), dim3(NW * 64), lds, s, (const bf16_t*)a.A,
                       a.lda, (const uint8_t*)a.W8, a.ldw, a.scale, a.bias, a.residual, a.out, a.ldc, a.M, a.N, a.K);
    MQ_CHECK_LAUNCH("mq_gemm_small_w8");
    return MQ_OK;
}

// Waves per workgroup and group depth, from the sweep over the four Mistral-7B GEMMs at 8 / 32 / 80 rows: up to 256 column slices
// (N <= 4096: one workgroup per CU at most) run 8 waves — at N = 4096, 8 rows: 7.3 us against 9.2 us (K = 4096), 17.2 against 25.5 (K = 14336) —
// wider weights 4 (N = 6144 and 28672, 80 rows: 41.9 against 44.2 us, 139 against 151); a depth of 2 chunks was the fastest or within 2 % of it at
// every point (4 costs VGPRs for the A fragments, G x 2 x MT x 4, and buys nothing behind the prefetch).  The wave count follows N alone, so a
// row's sums do not depend on the row count.  "w8_waves" / "w8_depth" (mq_tune) force a variant: how the sweep was run.
template <int FLAGS, int MT>
int dispatch_w8_plan(const W8Args& a, hipStream_t s) {
    const int nw = mq_w8_waves == 4 || mq_w8_waves == 8 ? (int)mq_w8_waves : (a.N <= 4096 ? 8 : 4);
    const int depth = mq_w8_depth == 4 ? 4 : 2;
    if (nw == 8) return depth == 4 ? launch_w8<FLAGS, MT, 8, 4>(a, s) : launch_w8<FLAGS, MT, 8, 2>(a, s);
    return depth == 4 ? launch_w8<FLAGS, MT, 4, 4>(a, s) : launch_w8<FLAGS, MT, 4, 2>(a, s);
}

template <int FLAGS>
int dispatch_w8_mt(const W8Args& a, hipStream_t s) {
    // more than 80 rows: the fewest row groups of at most 5 row tiles, then the smallest height that covers them (as gemm_small.hip)
    const int mt_all = (a.M + 15) / 16, groups = (mt_all + W8_MAX_MT - 1) / W8_MAX_MT;
    const int mt = (mt_all + groups - 1) / groups;
    if (mt <= 1) return dispatch_w8_plan<FLAGS, 1>(a, s);
    if (mt <= 2) return dispatch_w8_plan<FLAGS, 2>(a, s);
    if (mt <= 3) return dispatch_w8_plan<FLAGS, 3>(a, s);
    if (mt <= 4) return dispatch_w8_plan<FLAGS, 4>(a, s);
    return dispatch_w8_plan<FLAGS, 5>(a, s);
}

// ---- the quantiser: one workgroup per weight row; absmax -> exponent -> codes -> the bf16 row rewritten with decode(code) * scale ----
__global__ __launch_bounds__(256) void quantize_pow2_kernel(bf16_t* __restrict__ W, int64_t ldw, uint8_t* __restrict__ W8, int64_t ld8, float* __restrict__ scale,
                                                            int K) {
    __shared__ float red[4];
    bf16_t* w = W + (int64_t)blockIdx.x * ldw;
    uint8_t* o = W8 + (int64_t)blockIdx.x * ld8;
    float mx = 0.f;
    for (int k = threadIdx.x * 8; k < K; k += 2048) {
        const u32x4 p = *(const u32x4*)(w + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) mx = fmaxf(mx, fmaxf(fabsf(__uint_as_float(p[e] << 16)), fabsf(__uint_as_float(p[e] & 0xffff0000u))));
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    // 2^ceil(log2(mx / 448)) without a logarithm: mx = f 2^e with f in [0.5, 1), 448 = 0.875 x 2^9, so mx / 448 = (f / 0.875) 2^(e - 9) and the
    // ceiling is e - 9 for f <= 0.875, e - 8 above.  The exponent is kept >= -100 (rows smaller than 448 x 2^-100: their products with 2^-9, the
    // smallest e4m3 step, would leave the bf16 range), which no saturation rule needs: a larger scale only uses smaller codes.
    int ex = 0;
    if (mx > 0.f) {
        int e;
        const float f = frexpf(mx, &e);
        ex = max(f <= 0.875f ? e - 9 : e - 8, -100);
    }
    const float sc = ldexpf(1.f, ex), inv = ldexpf(1.f, -ex);
    if (threadIdx.x == 0) scale[blockIdx.x] = sc;
    for (int k = threadIdx.x * 8; k < K; k += 2048) {
        const u32x4 p = *(const u32x4*)(w + k);
        uint2 code;
        u32x4 back;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int wd = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(p[2 * h] << 16) * inv, __uint_as_float(p[2 * h] & 0xffff0000u) * inv, 0, false);
            wd = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(p[2 * h + 1] << 16) * inv, __uint_as_float(p[2 * h + 1] & 0xffff0000u) * inv, wd, true);
            (h ? code.y : code.x) = (uint32_t)wd;
            const auto a = __builtin_amdgcn_cvt_pk_f32_fp8(wd, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(wd, true);
            back[2 * h] = (__float_as_uint(a[0] * sc) >> 16) | (__float_as_uint(a[1] * sc) & 0xffff0000u);       // exact: nothing below bit 16
            back[2 * h + 1] = (__float_as_uint(b[0] * sc) >> 16) | (__float_as_uint(b[1] * sc) & 0xffff0000u);
        }
        *(uint2*)(o + k) = code;
        *(u32x4*)(w + k) = back;
    }
}

}  // namespace

// exactly the calls gemm_small.hip takes (<= 80 rows in one group, up to small_m_grouped in row groups) whose K is a whole number of 64-deep chunks
extern "C" int mq_gemm_small_w8_ok(int64_t M, int64_t N, int64_t K) {
    return (mq_gemm_small_ok(M, N, K, false) || mq_gemm_small_grouped_ok(M, N, K)) && K % W8_BK == 0;
}

extern "C" int mq_gemm_small_w8(const void* d_A, int64_t lda, const void* d_W8, int64_t ldw, const float* d_scale, const float* d_bias, const void* d_residual,
                                void* d_out, int64_t ldc, int64_t M, int64_t N, int64_t K, int flags, void* stream) {
    MQ_CHECK_ARG(d_A && d_W8 && d_scale && d_out, "mq_gemm_small_w8: null operand");
    MQ_CHECK_ARG(K >= W8_BK && K % W8_BK == 0, "mq_gemm_small_w8: K=%ld must be a multiple of %d", (long)K, W8_BK);
    MQ_CHECK_ARG(mq_gemm_small_w8_ok(M, N, K), "mq_gemm_small_w8: shape M=%ld N=%ld K=%ld unsupported", (long)M, (long)N, (long)K);
    MQ_CHECK_ARG(!(flags & MQ_EPI_BIAS) || d_bias, "mq_gemm_small_w8: MQ_EPI_BIAS without bias");
    MQ_CHECK_ARG(!(flags & MQ_EPI_RESIDUAL) || d_residual, "mq_gemm_small_w8: MQ_EPI_RESIDUAL without residual");
    MQ_CHECK_ARG(lda % 8 == 0 && ldw % 16 == 0 && ldc % 4 == 0, "mq_gemm_small_w8: leading dims must keep 16-byte rows");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(0, s, 2.0 * (double)M * (double)N * (double)K);
    const W8Args a{d_A, lda, d_W8, ldw, d_scale, d_bias, d_residual, d_out, ldc, (int)M, (int)N, (int)K};
    switch (flags) {
        case 0: return dispatch_w8_mt<0>(a, s);
        case MQ_EPI_BIAS: return dispatch_w8_mt<MQ_EPI_BIAS>(a, s);
        case MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32: return dispatch_w8_mt<MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32>(a, s);   // fp32 residual, may alias out
        default:
            mq_set_error("mq_gemm_small_w8: unsupported epilogue flag combination 0x%x", flags);
            return MQ_ERR_INVALID;
    }
}

extern "C" int mq_quantize_weights_pow2(void* d_W_bf16, int64_t ldw, void* d_W8, int64_t ld8, float* d_scale, int64_t N, int64_t K, void* stream) {
    MQ_CHECK_ARG(d_W_bf16 && d_W8 && d_scale, "mq_quantize_weights_pow2: null pointer");
    MQ_CHECK_ARG(N >= 1 && N < (1LL << 31) && K >= W8_BK && K % W8_BK == 0 && K < (1LL << 30), "mq_quantize_weights_pow2: bad shape N=%ld K=%ld (K a multiple of %d)",
                 (long)N, (long)K, W8_BK);
    MQ_CHECK_ARG(ldw % 8 == 0 && ld8 % 16 == 0 && ldw >= K && ld8 >= K, "mq_quantize_weights_pow2: leading dims must keep 16-byte rows");
    hipLaunchKernelGGL(quantize_pow2_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (bf16_t*)d_W_bf16, ldw, (uint8_t*)d_W8, ld8, d_scale, (int)K);
    MQ_CHECK_LAUNCH("mq_quantize_weights_pow2");
    return MQ_OK;
}
