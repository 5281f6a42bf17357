// ResNet CLIP image towers (OpenAI CLIP / open_clip ModifiedResNet: RN50, RN101, RN50x4, RN50x16, RN50x64).
// Activations stay NHWC as [pixels, C] bf16 rows, as in convnext.hip: every 1x1 convolution is a tiled GEMM (gemm_bf16.hip, MQ_EPI_RELU), BatchNorm is
// folded into the convolutions at load.  The kernels here are what has no GEMM form:
//   * conv3x3: the dense 3x3 convolution (stride 1, pad 1) as an implicit GEMM on the MFMA path — K ordered (ky, kx, c), the A tile gathered straight
//     from the activation while it is staged (LDS-DMA with a per-lane 64-bit source address), no im2col buffer;
//   * stem gather: the stride-2 3x3 stem convolution's 27 taps of the normalised pixels, zero-padded to 64 columns, for a GEMM;
//   * avgpool2: the 2x2 average pool of the blocks' main branch and of the downsample;
//   * attention pool: the mean token + positions, then single-query multi-head attention with one query per image (q, k, v and c_proj are GEMMs).
#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_loop.h"
#include "gemm_sched.h"

static_assert(sizeof(mq_resnet_cfg) == 56, "mq_resnet_cfg layout");
static_assert(sizeof(mq_resnet_block_weights) == 8 * 8 && sizeof(mq_resnet_weights) == 14 * 8, "mq_resnet weight layouts");

int mq_device_ok();   // runtime.hip

// 16 zero bytes: the source of every out-of-image (or out-of-K) tap of the implicit GEMM's A tile
__device__ uint4 mq_resnet_zero_line[1];

namespace {

// ---- implicit-GEMM 3x3 convolution ------------------------------------------------------------------------------------------------------------
//   y[p, n] = act( sum_{ky, kx, c} x[p + (ky - 1) W + (kx - 1), c] * Wt[n, (ky * 3 + kx) Cin + c] + bias[n] )     (taps outside p's own image: 0)
// The tile is gemm_nt_kernel's (32*MT) x 128 x 64 with 4 waves as 2 x 2 and the same swizzled [rows][128 B] LDS image and fragment reads, so that
// gemm_epilogue finishes it; the loop is the plain two-stage one (one barrier per k-step, the next stage's LDS-DMA in flight under the MFMAs).
// A (the activation): a lane stages 16 B = 8 consecutive k of one row.  Cin % 8 == 0, so the 8 k lie in ONE tap: (tap, c) advance by 64 per k-step
// and the source is x + (p + off(tap)) Cin + c — or the zero line when the tap falls outside the row's image (a per-row 9-bit mask, so a tile that
// spans several images never reads a neighbour's pixels), when tap >= 9 (K padding) or when the row is past M.  Addresses are 64-bit per lane
// (global_load_lds): no 32-bit offset limit on the activation.  W: [Cout, Kp] bf16 through a buffer descriptor as in gemm_nt_kernel.
template <int FLAGS, int MT>
__global__ __launch_bounds__(256, 2) void conv3x3_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ Wt, int64_t ldw,
                                                         const float* __restrict__ bias, bf16_t* __restrict__ out, int64_t ldc, int M, int N, int Cin,
                                                         int H, int W, int Kp, int tiles_n, int num_tiles, int cgroup, int band_rows, unsigned w_bytes,
                                                         int wide) {
    constexpr int BM = 32 * MT, BN = 128;
    constexpr int A_TILE_BYTES = BM * BK * 2, STAGE_BYTES = A_TILE_BYTES + BN * BK * 2;
    constexpr int NPW = 4;   // W pieces (8 rows) per wave and stage
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GemmTileMap<BM, BN> tile_map(num_tiles, tiles_n, M, cgroup, band_rows);
    int m0, n0;
    tile_map.origin(blockIdx.x, m0, n0);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l15 = lane & 15, g = lane >> 4;
    const int srow = lane >> 3;
    const int lchunk = (lane & 7) ^ (srow & 7);                 // the logical 16-B chunk this lane stages (swizzle on the source, as gemm_nt_kernel)
    const unsigned chunk_off = (unsigned)(lchunk * 16);

    // A rows of this lane: piece i = row m0 + wave * 8 MT + 8 i + srow; its byte offset in x and the taps that stay inside its image
    const int HW = H * W;
    int64_t a_base[MT];
    unsigned a_mask[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int r = m0 + wave * (8 * MT) + i * 8 + srow;
        a_base[i] = (int64_t)r * Cin * 2;
        unsigned mask = 0;
        if (r < M) {
            const int rem = r % HW, yy = rem / W, xx = rem - yy * W;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = yy + t / 3 - 1, ix = xx + t % 3 - 1;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) mask |= 1u << t;
            }
        }
        a_mask[i] = mask;
    }
    unsigned w_vo[NPW];
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
        int gn = n0 + wave * (8 * NPW) + i * 8 + srow; gn = gn < N ? gn : N - 1;
        w_vo[i] = (unsigned)gn * (unsigned)ldw * 2u + chunk_off;
    }
    const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)Wt, 0, w_bytes, 0x00020000);
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned dma_a0 = lds0 + (unsigned)wave * (8 * MT * 128), dma_w0 = lds0 + A_TILE_BYTES + (unsigned)wave * (8 * NPW * 128);
    const char* xb = (const char*)x;
    const char* zero = (const char*)mq_resnet_zero_line;

    // the (tap, channel) of this lane's chunk at the k-step being staged
    int tap = (lchunk * 8) / Cin, cc = (lchunk * 8) - tap * Cin;
    auto issue_stage = [&](int ks, unsigned bufoff) {
        const bool in_k = tap < 9;
        const int t = in_k ? tap : 0;
        const int64_t toff = ((int64_t)((t / 3 - 1) * W + (t % 3 - 1)) * Cin + cc) * 2;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const bool ok = in_k && ((a_mask[i] >> t) & 1u);
            const char* src = ok ? xb + a_base[i] + toff : zero;
            __builtin_amdgcn_global_load_lds((const void*)src, (lds_void_t*)(uintptr_t)(dma_a0 + bufoff + (unsigned)i * 1024u), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NPW; ++i) dma16(w_rs, w_vo[i], (unsigned)ks * (BK * 2), dma_w0 + bufoff + (unsigned)i * 1024u);
        cc += BK;
        while (cc >= Cin) { cc -= Cin; ++tap; }
    };

    const unsigned sw0 = (unsigned)((g ^ (l15 & 7)) << 4), sw1 = (unsigned)(((g + 4) ^ (l15 & 7)) << 4);
    const unsigned a_row = lds0 + (unsigned)((wm * (16 * MT) + l15) * 128);
    const unsigned w_row = lds0 + A_TILE_BYTES + (unsigned)((wn * 64 + l15) * 128);

    f32x4 acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = Kp / BK;
    unsigned bufoff = 0;
    issue_stage(0, 0);
    for (int ks = 0; ks < nk; ++ks) {
        // this stage has landed (every wave's pieces), and every wave is done reading the other buffer: it may be refilled
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (ks + 1 < nk) issue_stage(ks + 1, bufoff ^ (unsigned)STAGE_BYTES);
        bf16x8 wf[2][4], af[2][MT];
        static_for<4>([&](auto t_tag) {
            constexpr int t = decltype(t_tag)::value;
            wf[0][t] = lds_read16<t * 2048>(w_row + sw0 + bufoff);
            wf[1][t] = lds_read16<t * 2048>(w_row + sw1 + bufoff);
        });
        static_for<MT>([&](auto t_tag) {
            constexpr int t = decltype(t_tag)::value;
            af[0][t] = lds_read16<t * 2048>(a_row + sw0 + bufoff);
            af[1][t] = lds_read16<t * 2048>(a_row + sw1 + bufoff);
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int t = 0; t < 4; ++t) landed(wf[h][t]);
#pragma unroll
            for (int t = 0; t < MT; ++t) landed(af[h][t]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[h][nt], af[h][mt], acc[mt][nt], 0, 0, 0);
        bufoff ^= (unsigned)STAGE_BYTES;
    }
    gemm_epilogue<FLAGS, MT, MT, true>(acc, bias, nullptr, out, ldc, M, N, m0 + wm * (16 * MT), n0 + wn * 64, l15, g, wide != 0, nullptr, nullptr);
}

// ---- stem gather ------------------------------------------------------------------------------------------------------------------------------
// out[(img, oy, ox), (ky * 3 + kx) * 3 + c] = norm(pixel (2 oy + ky - 1, 2 ox + kx - 1), channel c), 0 outside the image and in columns 27..63.
// u8: [n, S, S, 3] HWC, normalised as (b / 255 - mean) / std; f32: [n, 3, S, S] already normalised.  One thread = one output row (8 x 16 B).
template <bool U8>
__global__ __launch_bounds__(256) void stem_gather_kernel(const void* __restrict__ in, bf16_t* __restrict__ out, int64_t rows, int S, float m0, float m1,
                                                          float m2, float s0, float s1, float s2) {
    const int G = S / 2;
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
        const int64_t img = r / ((int64_t)G * G);
        const int rem = (int)(r - img * G * G), oy = rem / G, ox = rem - oy * G;
        float v[32];
#pragma unroll
        for (int j = 0; j < 27; ++j) {
            const int t = j / 3, c = j % 3;
            const int iy = 2 * oy + t / 3 - 1, ix = 2 * ox + t % 3 - 1;
            float val = 0.f;
            if (iy >= 0 && iy < S && ix >= 0 && ix < S) {
                if (U8) val = ((float)((const uint8_t*)in)[((img * S + iy) * S + ix) * 3 + c] / 255.0f - mean[c]) / sd[c];
                else val = ((const float*)in)[((img * 3 + c) * S + iy) * (int64_t)S + ix];
            }
            v[j] = val;
        }
#pragma unroll
        for (int j = 27; j < 32; ++j) v[j] = 0.f;
        uint4* o = (uint4*)(out + r * 64);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = make_uint4(pack_bf16x2(v[8 * q], v[8 * q + 1]), pack_bf16x2(v[8 * q + 2], v[8 * q + 3]), pack_bf16x2(v[8 * q + 4], v[8 * q + 5]),
                              pack_bf16x2(v[8 * q + 6], v[8 * q + 7]));
#pragma unroll
        for (int q = 4; q < 8; ++q) o[q] = make_uint4(0u, 0u, 0u, 0u);
    }
}

__device__ __forceinline__ f32x2_t bf16x2_to_f32x2(uint32_t u) { return f32x2_t{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)}; }

// ---- 2x2 average pool: out[(img, oy, ox), c] = mean of the 4 pixels (2 oy + dy, 2 ox + dx); one thread = 8 channels ----------------------------
__global__ __launch_bounds__(256) void avgpool2_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, int64_t total, int H, int W, int C) {
    const int cv = C >> 3, Ho = H >> 1, Wo = W >> 1;
    for (int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x; gi < total; gi += (int64_t)gridDim.x * 256) {
        const int v = (int)(gi % cv);
        const int64_t orow = gi / cv;
        const int64_t img = orow / (Ho * Wo);
        const int rem = (int)(orow - img * Ho * Wo), oy = rem / Wo, ox = rem - oy * Wo;
        const int64_t i0 = (img * H + 2 * oy) * W + 2 * ox;
        const uint4 a = *(const uint4*)(x + i0 * C + v * 8), b = *(const uint4*)(x + (i0 + 1) * C + v * 8);
        const uint4 c = *(const uint4*)(x + (i0 + W) * C + v * 8), d = *(const uint4*)(x + (i0 + W + 1) * C + v * 8);
        const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w}, wc[4] = {c.x, c.y, c.z, c.w}, wd[4] = {d.x, d.y, d.z, d.w};
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x2_t s = ((bf16x2_to_f32x2(wa[k]) + bf16x2_to_f32x2(wb[k])) + (bf16x2_to_f32x2(wc[k]) + bf16x2_to_f32x2(wd[k]))) * 0.25f;
            o[k] = pack_bf16x2(s[0], s[1]);
        }
        *(uint4*)(out + orow * C + v * 8) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// ---- attention pool: tokens ---------------------------------------------------------------------------------------------------------------------
// tok[img, 0, c] = mean_p x[img, p, c] + pos[0, c];  tok[img, 1 + p, c] = x[img, p, c] + pos[1 + p, c]     (bf16 out; one workgroup per image)
__global__ __launch_bounds__(256) void ap_tokens_kernel(const bf16_t* __restrict__ x, const float* __restrict__ pos, bf16_t* __restrict__ tok, int HW,
                                                        int C) {
    const int64_t img = blockIdx.x;
    const bf16_t* xi = x + img * HW * (int64_t)C;
    bf16_t* ti = tok + img * (HW + 1) * (int64_t)C;
    const float inv = 1.0f / (float)HW;
    for (int v = threadIdx.x; v < (C >> 3); v += 256) {
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < HW; ++p) {
            const uint4 u = *(const uint4*)(xi + (int64_t)p * C + v * 8);
            const float4 q0 = *(const float4*)(pos + (int64_t)(p + 1) * C + v * 8), q1 = *(const float4*)(pos + (int64_t)(p + 1) * C + v * 8 + 4);
            const f32x2_t a0 = bf16x2_to_f32x2(u.x), a1 = bf16x2_to_f32x2(u.y), a2 = bf16x2_to_f32x2(u.z), a3 = bf16x2_to_f32x2(u.w);
            s[0] += a0[0]; s[1] += a0[1]; s[2] += a1[0]; s[3] += a1[1]; s[4] += a2[0]; s[5] += a2[1]; s[6] += a3[0]; s[7] += a3[1];
            *(uint4*)(ti + (int64_t)(p + 1) * C + v * 8) = make_uint4(pack_bf16x2(a0[0] + q0.x, a0[1] + q0.y), pack_bf16x2(a1[0] + q0.z, a1[1] + q0.w),
                                                                     pack_bf16x2(a2[0] + q1.x, a2[1] + q1.y), pack_bf16x2(a3[0] + q1.z, a3[1] + q1.w));
        }
        const float4 q0 = *(const float4*)(pos + v * 8), q1 = *(const float4*)(pos + v * 8 + 4);
        *(uint4*)(ti + v * 8) = make_uint4(pack_bf16x2(s[0] * inv + q0.x, s[1] * inv + q0.y), pack_bf16x2(s[2] * inv + q0.z, s[3] * inv + q0.w),
                                           pack_bf16x2(s[4] * inv + q1.x, s[5] * inv + q1.y), pack_bf16x2(s[6] * inv + q1.z, s[7] * inv + q1.w));
    }
}

// ---- attention pool: single-query attention, one query per image ----------------------------------------------------------------------------------
// out[img, h 64 + d] = sum_t softmax_t(q[img, h] . k[img, t, h]) v[img, t, h 64 + d]; q already carries the 1/8 scale (folded into q_proj at load).
// kv: [img, t] rows of 2 C (k | v).  One wave per (image, head): lane = token for the scores, lane = d for the weighted sum.
constexpr int AP_MAX_T = 256;
__global__ __launch_bounds__(64) void ap_attend_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv, bf16_t* __restrict__ out, int T,
                                                       int C) {
    __shared__ float qs[64];
    __shared__ float p[AP_MAX_T];
    const int64_t img = blockIdx.x;
    const int h = blockIdx.y, lane = threadIdx.x;
    qs[lane] = bf16_to_f32(q[img * C + h * 64 + lane]);
    __syncthreads();
    const bf16_t* kvi = kv + img * T * (int64_t)(2 * C);
    float mx = -INFINITY;
    for (int t = lane; t < T; t += 64) {
        const uint4* kr = (const uint4*)(kvi + (int64_t)t * (2 * C) + h * 64);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint4 u = kr[j];
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x2_t kk = bf16x2_to_f32x2(w[e]);
                s = fmaf(qs[8 * j + 2 * e], kk[0], s);
                s = fmaf(qs[8 * j + 2 * e + 1], kk[1], s);
            }
        }
        p[t] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int t = lane; t < T; t += 64) {
        const float e = __expf(p[t] - mx);
        p[t] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    __syncthreads();
    float o = 0.f;
    const bf16_t* vcol = kvi + C + h * 64 + lane;
    for (int t = 0; t < T; ++t) o = fmaf(p[t], bf16_to_f32(vcol[(int64_t)t * (2 * C)]), o);
    out[img * C + h * 64 + lane] = f32_to_bf16(o / sum);
}

}  // namespace

// ---- building blocks (C ABI) ------------------------------------------------------------------------------------------------------------------
namespace {

template <int FLAGS, int MT>
int launch_conv3x3(const void* x, const void* w, const float* b, void* y, int64_t ldc, int M, int N, int Cin, int H, int W, int Kp, hipStream_t s) {
    constexpr int BM = 32 * MT, BN = 128, LDS = 2 * (BM + BN) * BK * 2;
    static std::atomic<uint64_t> attr_done{0};
    auto kern = conv3x3_kernel<FLAGS, MT>;
    if (hipError_t e = mq_ensure_dyn_lds((const void*)kern, LDS, attr_done); e != hipSuccess) {
        mq_set_error("mq_resnet_conv3x3: hipFuncSetAttribute: %s", hipGetErrorString(e));
        return MQ_ERR_HIP;
    }
    GemmGeom g;
    g.tiles_n = (N + BN - 1) / BN;
    g.set_tiles_m((M + BM - 1) / BM, RESIDENT_SLOTS);
    const int wide = (ldc % 8 == 0 && ((uintptr_t)y & 15) == 0) ? 1 : 0;
    const unsigned w_bytes = (unsigned)((uint64_t)N * (uint64_t)Kp * 2);
    hipLaunchKernelGGL(kern, dim3((unsigned)g.num_tiles), dim3(256), LDS, s, (const bf16_t*)x, (const bf16_t*)w, (int64_t)Kp, b, (bf16_t*)y, ldc, M, N, Cin,
                       H, W, Kp, g.tiles_n, g.num_tiles, g.cgroup, g.band_rows, w_bytes, wide);
    MQ_CHECK_LAUNCH("mq_resnet_conv3x3");
    return MQ_OK;
}

}  // namespace

extern "C" int mq_resnet_conv3x3(const void* d_x, const void* d_w, const float* d_b, void* d_y, int64_t ldy, int64_t n, int32_t H, int32_t W, int32_t Cin,
                                 int32_t Cout, int32_t relu, void* stream) {
    MQ_CHECK_ARG(d_x && d_w && d_b && d_y, "mq_resnet_conv3x3: null operand");
    MQ_CHECK_ARG(Cin >= 8 && Cin % 8 == 0 && Cin <= 4096, "mq_resnet_conv3x3: Cin=%d must be a multiple of 8 (<= 4096)", Cin);
    MQ_CHECK_ARG(Cout >= 4 && Cout % 4 == 0 && Cout <= 4096, "mq_resnet_conv3x3: Cout=%d must be a multiple of 4 (<= 4096)", Cout);
    MQ_CHECK_ARG(ldy >= Cout && ldy % 4 == 0, "mq_resnet_conv3x3: ldy=%ld must be >= Cout and a multiple of 4", (long)ldy);
    MQ_CHECK_ARG(H >= 1 && W >= 1 && H <= 4096 && W <= 4096 && n >= 0, "mq_resnet_conv3x3: bad shape n=%ld H=%d W=%d", (long)n, H, W);
    MQ_CHECK_ARG((int64_t)n * H * W < (1 << 30), "mq_resnet_conv3x3: n*H*W=%ld rows exceed 2^30", (long)(n * H * W));
    MQ_CHECK_ARG(d_x != d_y, "mq_resnet_conv3x3: the output must not alias the input");
    MQ_CHECK_ARG(relu == 0 || relu == 1, "mq_resnet_conv3x3: relu=%d must be 0 or 1", relu);
    if (n == 0) return MQ_OK;
    MQ_TRY(mq_device_ok());
    const int Kp = (9 * Cin + BK - 1) / BK * BK;
    const int M = (int)(n * H * W);
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(0, s, 2.0 * (double)M * (double)Cout * 9.0 * (double)Cin);
    const int mt = g_tune.mt == 2 || g_tune.mt == 4 ? (int)g_tune.mt : (choose_mt(M, Cout) <= 2 ? 2 : 4);
    if (relu) {
        if (mt == 2) return launch_conv3x3<MQ_EPI_BIAS | MQ_EPI_RELU, 2>(d_x, d_w, d_b, d_y, ldy, M, Cout, Cin, H, W, Kp, s);
        return launch_conv3x3<MQ_EPI_BIAS | MQ_EPI_RELU, 4>(d_x, d_w, d_b, d_y, ldy, M, Cout, Cin, H, W, Kp, s);
    }
    if (mt == 2) return launch_conv3x3<MQ_EPI_BIAS, 2>(d_x, d_w, d_b, d_y, ldy, M, Cout, Cin, H, W, Kp, s);
    return launch_conv3x3<MQ_EPI_BIAS, 4>(d_x, d_w, d_b, d_y, ldy, M, Cout, Cin, H, W, Kp, s);
}

extern "C" int mq_resnet_stem_gather(const void* d_pixels, int32_t is_u8, void* d_out, int64_t n, int32_t S, const float* mean, const float* std,
                                     void* stream) {
    MQ_CHECK_ARG(d_pixels && d_out, "mq_resnet_stem_gather: null operand");
    MQ_CHECK_ARG(S >= 2 && S % 2 == 0 && S <= 4096 && n >= 0, "mq_resnet_stem_gather: bad shape n=%ld S=%d (S even)", (long)n, S);
    MQ_CHECK_ARG(!is_u8 || (mean && std), "mq_resnet_stem_gather: the u8 entry needs mean and std");
    if (n == 0) return MQ_OK;
    const int64_t rows = n * (S / 2) * (S / 2);
    const unsigned grid = (unsigned)(cdiv64(rows, 256) < 16384 ? cdiv64(rows, 256) : 16384);
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(5, s);
    if (is_u8)
        hipLaunchKernelGGL(stem_gather_kernel<true>, dim3(grid), dim3(256), 0, s, d_pixels, (bf16_t*)d_out, rows, (int)S, mean[0], mean[1], mean[2], std[0],
                           std[1], std[2]);
    else
        hipLaunchKernelGGL(stem_gather_kernel<false>, dim3(grid), dim3(256), 0, s, d_pixels, (bf16_t*)d_out, rows, (int)S, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
    MQ_CHECK_LAUNCH("mq_resnet_stem_gather");
    return MQ_OK;
}

extern "C" int mq_resnet_avgpool2(const void* d_x, void* d_out, int64_t n, int32_t H, int32_t W, int32_t C, void* stream) {
    MQ_CHECK_ARG(d_x && d_out, "mq_resnet_avgpool2: null operand");
    MQ_CHECK_ARG(C >= 8 && C % 8 == 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && n >= 0, "mq_resnet_avgpool2: bad shape H=%d W=%d C=%d", H, W, C);
    MQ_CHECK_ARG(d_x != d_out, "mq_resnet_avgpool2: the output must not alias the input");
    if (n == 0) return MQ_OK;
    const int64_t total = n * (H / 2) * (W / 2) * (C / 8);
    const unsigned grid = (unsigned)(cdiv64(total, 256) < 16384 ? cdiv64(total, 256) : 16384);
    MqProfScope prof(1, (hipStream_t)stream);
    hipLaunchKernelGGL(avgpool2_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)d_x, (bf16_t*)d_out, total, (int)H, (int)W, (int)C);
    MQ_CHECK_LAUNCH("mq_resnet_avgpool2");
    return MQ_OK;
}

extern "C" int mq_resnet_attnpool_tokens(const void* d_x, const float* d_pos, void* d_tokens, int64_t n, int32_t HW, int32_t C, void* stream) {
    MQ_CHECK_ARG(d_x && d_pos && d_tokens, "mq_resnet_attnpool_tokens: null operand");
    MQ_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= 8192 && HW >= 1 && HW + 1 <= AP_MAX_T && n >= 0 && n <= 65535,
                 "mq_resnet_attnpool_tokens: bad shape n=%ld HW=%d C=%d (C multiple of 8, HW + 1 <= %d)", (long)n, HW, C, AP_MAX_T);
    if (n == 0) return MQ_OK;
    MqProfScope prof(3, (hipStream_t)stream);
    hipLaunchKernelGGL(ap_tokens_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)d_x, d_pos, (bf16_t*)d_tokens, (int)HW, (int)C);
    MQ_CHECK_LAUNCH("mq_resnet_attnpool_tokens");
    return MQ_OK;
}

extern "C" int mq_resnet_attnpool_attend(const void* d_q, const void* d_kv, void* d_out, int64_t n, int32_t T, int32_t C, void* stream) {
    MQ_CHECK_ARG(d_q && d_kv && d_out, "mq_resnet_attnpool_attend: null operand");
    MQ_CHECK_ARG(C >= 64 && C % 64 == 0 && C <= 8192 && T >= 1 && T <= AP_MAX_T && n >= 0 && n <= 65535,
                 "mq_resnet_attnpool_attend: bad shape n=%ld T=%d C=%d (heads of 64, T <= %d)", (long)n, T, C, AP_MAX_T);
    if (n == 0) return MQ_OK;
    MqProfScope prof(2, (hipStream_t)stream);
    hipLaunchKernelGGL(ap_attend_kernel, dim3((unsigned)n, (unsigned)(C / 64)), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)d_q, (const bf16_t*)d_kv,
                       (bf16_t*)d_out, (int)T, (int)C);
    MQ_CHECK_LAUNCH("mq_resnet_attnpool_attend");
    return MQ_OK;
}

// ---- the tower -------------------------------------------------------------------------------------------------------------------------------
namespace {

int pad64(int c) { return (c + 63) / 64 * 64; }

struct RnPlan {
    size_t buf_bytes;   // each of the five activation buffers
    size_t off[5], total;
};

bool rn_cfg_ok(const mq_resnet_cfg* c) {
    // width % 16: the stem's inner width w / 2 must be a multiple of 8 (conv3x3) and every stage output 4 (w << i) a multiple of 64 (the GEMMs' K)
    if (!c || c->image_size < 64 || c->image_size % 32 != 0 || c->width < 16 || c->width % 16 != 0 || c->width > 256) return false;
    if (c->out_dim < 4 || c->out_dim % 4 != 0 || c->heads < 1 || c->heads * 64 != 32 * c->width) return false;
    const int g = c->image_size / 32;
    if (g * g + 1 > AP_MAX_T) return false;
    for (int i = 0; i < 4; ++i)
        if (c->layers[i] < 1 || c->layers[i] > 64) return false;
    return true;
}

// every activation the forward leaves fits one buffer: the largest [rows, channels] of the walk below
RnPlan rn_plan(const mq_resnet_cfg* c, int64_t n) {
    const int64_t S = c->image_size, w = c->width;
    int64_t best = 0;
    auto see = [&](int64_t rows, int64_t ch) { best = rows * ch > best ? rows * ch : best; };
    int64_t r = n * (S / 2) * (S / 2);
    see(r, 64);
    see(r, w / 2);
    see(r, pad64((int)w));
    r /= 4;
    int64_t inplanes = pad64((int)w);
    for (int st = 0; st < 4; ++st) {
        const int64_t P = pad64((int)(w << st)), out = 4 * (w << st);
        see(r, P);
        see(r, inplanes);
        if (st > 0) r /= 4;
        see(r, out);
        inplanes = out;
    }
    const int64_t T = (S / 32) * (S / 32) + 1, C = 32 * w;
    see(n * T, 2 * C);
    RnPlan p{};
    p.buf_bytes = align_up((size_t)best * 2, 256);
    size_t o = 0;
    for (int i = 0; i < 5; ++i) { p.off[i] = o; o += p.buf_bytes; }
    p.total = o;
    return p;
}

int rn_forward(const mq_resnet_cfg* c, const mq_resnet_weights* w, const void* d_pixels, bool is_u8, int64_t n, float* d_out, int normalize, void* d_ws,
               size_t ws_bytes, hipStream_t s) {
    MQ_CHECK_ARG(c && w && d_pixels && d_out && w->blocks, "mq_encode_resnet: null argument");
    MQ_CHECK_ARG(rn_cfg_ok(c), "mq_encode_resnet: unsupported cfg (image_size multiple of 32, width multiple of 16 <= 256, heads = width / 2, "
                               "(image_size / 32)^2 + 1 <= %d tokens)", AP_MAX_T);
    MQ_CHECK_ARG(n >= 1 && n <= 65535, "mq_encode_resnet: n=%ld out of range", (long)n);
    for (int i = 0; i < 3; ++i) MQ_CHECK_ARG(w->stem_w[i] && w->stem_b[i], "mq_encode_resnet: missing stem conv %d", i + 1);
    MQ_CHECK_ARG(w->pos && w->q_w && w->q_b && w->kv_w && w->kv_b && w->c_w && w->c_b, "mq_encode_resnet: missing attention-pool weights");
    const RnPlan p = rn_plan(c, n);
    MQ_CHECK_ARG(d_ws && ws_bytes >= p.total, "mq_encode_resnet: workspace %zu < %zu bytes", ws_bytes, p.total);
    char* ws = (char*)d_ws;
    void* X = ws + p.off[0];
    void* D = ws + p.off[1];
    void* A = ws + p.off[2];
    void* B = ws + p.off[3];
    void* Cb = ws + p.off[4];
    const int S = c->image_size, wd = c->width, c1 = wd / 2, wp = pad64(wd);
    constexpr int BR = MQ_EPI_BIAS | MQ_EPI_RELU;

    // stem: conv1 3x3 / 2 (gathered 27 taps -> GEMM), conv2, conv3 3x3 (BN folded, ReLU), avgpool 2
    int H = S / 2;
    int64_t rows = n * H * H;
    MQ_TRY(mq_resnet_stem_gather(d_pixels, is_u8 ? 1 : 0, A, n, S, c->mean, c->std, s));
    MQ_TRY(mq_gemm_bf16(A, 64, w->stem_w[0], 64, w->stem_b[0], nullptr, B, c1, rows, c1, 64, BR, s));
    MQ_TRY(mq_resnet_conv3x3(B, w->stem_w[1], w->stem_b[1], A, c1, n, H, H, c1, c1, 1, s));
    MQ_TRY(mq_resnet_conv3x3(A, w->stem_w[2], w->stem_b[2], B, wp, n, H, H, c1, wp, 1, s));
    MQ_TRY(mq_resnet_avgpool2(B, X, n, H, H, wp, s));
    H /= 2;
    rows = n * H * H;

    int inp = wp;
    const mq_resnet_block_weights* blk = w->blocks;
    for (int st = 0; st < 4; ++st) {
        const int P = pad64(wd << st), out = 4 * (wd << st);
        for (int j = 0; j < c->layers[st]; ++j, ++blk) {
            const bool down = st > 0 && j == 0;
            // the first block of every stage has the downsample branch (stage 1: the module's inplanes w != 4 w).  `inp` is the PADDED width here:
            // at w = 16 pad64(w) == 4 w, so comparing it with `out` would take layer1.0 for an identity block
            const bool has_ds = j == 0;
            MQ_CHECK_ARG(blk->conv1_w && blk->conv1_b && blk->conv2_w && blk->conv2_b && blk->conv3_w && blk->conv3_b && (!has_ds || (blk->ds_w && blk->ds_b)),
                         "mq_encode_resnet: missing weights of stage %d block %d", st + 1, j);
            MQ_TRY(mq_gemm_bf16(X, inp, blk->conv1_w, inp, blk->conv1_b, nullptr, A, P, rows, P, inp, BR, s));
            MQ_TRY(mq_resnet_conv3x3(A, blk->conv2_w, blk->conv2_b, B, P, n, H, H, P, P, 1, s));
            const void* main = B;
            const void* xin = X;
            int64_t rows_o = rows;
            if (down) {
                MQ_TRY(mq_resnet_avgpool2(B, A, n, H, H, P, s));
                MQ_TRY(mq_resnet_avgpool2(X, Cb, n, H, H, inp, s));
                main = A;
                xin = Cb;
                H /= 2;
                rows_o = n * H * H;
            }
            if (has_ds) {
                // identity = BN(conv1x1(avgpool(x))); conv3 + BN + identity + ReLU written over it, then it is the stream
                MQ_TRY(mq_gemm_bf16(xin, inp, blk->ds_w, inp, blk->ds_b, nullptr, D, out, rows_o, out, inp, MQ_EPI_BIAS, s));
                MQ_TRY(mq_gemm_bf16(main, P, blk->conv3_w, P, blk->conv3_b, (const float*)D, D, out, rows_o, out, P, BR | MQ_EPI_RESIDUAL, s));
                void* t = X; X = D; D = t;
            } else {
                MQ_TRY(mq_gemm_bf16(main, P, blk->conv3_w, P, blk->conv3_b, (const float*)X, X, out, rows_o, out, P, BR | MQ_EPI_RESIDUAL, s));
            }
            rows = rows_o;
            inp = out;
        }
    }
    // attention pool: tokens (mean + pixels, + positions) -> k | v of every token, q of token 0 -> one query per image and head -> c_proj
    const int C = 32 * wd, HW = H * H, T = HW + 1, E = c->out_dim;
    MQ_TRY(mq_resnet_attnpool_tokens(X, w->pos, A, n, HW, C, s));
    MQ_TRY(mq_gemm_bf16(A, C, w->kv_w, C, w->kv_b, nullptr, B, 2 * C, n * T, 2 * C, C, MQ_EPI_BIAS, s));
    MQ_TRY(mq_gemm_bf16(A, (int64_t)T * C, w->q_w, C, w->q_b, nullptr, Cb, C, n, C, C, MQ_EPI_BIAS, s));
    MQ_TRY(mq_resnet_attnpool_attend(Cb, B, D, n, T, C, s));
    MQ_TRY(mq_gemm_bf16(D, C, w->c_w, C, w->c_b, nullptr, d_out, E, n, E, C, MQ_EPI_BIAS | MQ_EPI_OUT_F32, s));
    if (normalize) MQ_TRY(mq_l2_normalize(d_out, d_out, n, E, s));
    return MQ_OK;
}

}  // namespace

extern "C" size_t mq_resnet_workspace_bytes(const mq_resnet_cfg* cfg, int64_t n_images) {
    if (!rn_cfg_ok(cfg) || n_images < 1) return 0;
    return rn_plan(cfg, n_images).total;
}

extern "C" int mq_encode_resnet_u8(const mq_resnet_cfg* cfg, const mq_resnet_weights* w, const uint8_t* d_pixels, int64_t n, float* d_out, int normalize,
                                   void* d_workspace, size_t workspace_bytes, void* stream) {
    return rn_forward(cfg, w, d_pixels, true, n, d_out, normalize, d_workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int mq_encode_resnet_f32(const mq_resnet_cfg* cfg, const mq_resnet_weights* w, const float* d_pixels, int64_t n, float* d_out, int normalize,
                                    void* d_workspace, size_t workspace_bytes, void* stream) {
    return rn_forward(cfg, w, d_pixels, false, n, d_out, normalize, d_workspace, workspace_bytes, (hipStream_t)stream);
}
