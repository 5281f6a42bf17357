// ConvNeXt image trunks (timm ConvNeXt behind open_clip's TimmModel, timm_pool "": the open_clip convnext_* CLIP towers).
// Activations stay NHWC as [pixels, C] bf16 rows, so every 1x1 convolution is a tiled GEMM (gemm_bf16.hip); the kernels here are what has no GEMM form:
//   * dwconv7: the block's depthwise 7x7 convolution + bias, which also leaves the (sum, sum of squares) of the bf16 values it stored per row and
//     64-channel slot (the slot-major partials of mq_gemm_bf16_rs) — the block's LayerNorm is then a finalise over them plus the fold into fc1;
//   * downsample gather: LayerNorm of every input pixel, 2x2 pixels gathered into one [4 C] row for the stride-2 GEMM ((ky, kx, c) order);
//   * pooled head: mean over the pixels of an image, then LayerNorm over C (timm's head.norm), one workgroup per image, any C <= 3072.
#include "common.h"

static_assert(sizeof(mq_convnext_cfg) == 72, "mq_convnext_cfg layout");
static_assert(sizeof(mq_convnext_block_weights) == 7 * 8 && sizeof(mq_convnext_weights) == 27 * 8, "mq_convnext weight layouts");

namespace {

// ---- depthwise 7x7 ----------------------------------------------------------------------------------------------------------------------
// One workgroup = one image, one 8 x 16 tile of output pixels, one 64-channel slot.  The tile plus its 3-pixel halo (14 x 22 pixels x 64 channels,
// bf16) is staged in LDS with 16-byte loads — every input is fetched from global memory once per slot — and the slot's 49 x 64 fp32 taps beside it.
// A thread owns 4 consecutive output pixels of one row x 8 channels: per kernel row it reads 10 input vectors once and reuses them for all 7 taps
// (28 packed FMAs per vector read), accumulating in fp32 pairs (v_pk_fma_f32).  The 8 lanes that share a pixel reduce its slot sums with shuffles.
constexpr int DW_TY = 8, DW_TX = 16, DW_HY = DW_TY + 6, DW_HX = DW_TX + 6;

__device__ __forceinline__ f32x2_t bf16x2_to_f32x2(uint32_t u) { return f32x2_t{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)}; }

__global__ __launch_bounds__(256) void dwconv7_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      bf16_t* __restrict__ y, float2* __restrict__ partials, int H, int W, int C, int tiles_x,
                                                      int64_t rows) {
    __shared__ uint4 tile[DW_HY * DW_HX * 8];   // [halo pixel][8 vectors of 8 channels]  39 424 B
    __shared__ float4 taps[49 * 16];            // [tap][64 channels]                       12 544 B
    const int slot = blockIdx.y, c0 = slot * 64;
    const int64_t img = blockIdx.z;
    const int ty0 = (int)(blockIdx.x / tiles_x) * DW_TY, tx0 = (int)(blockIdx.x % tiles_x) * DW_TX;
    const bf16_t* xi = x + img * H * W * C + c0;
    for (int i = threadIdx.x; i < DW_HY * DW_HX * 8; i += 256) {
        const int p = i >> 3, v = i & 7;
        const int iy = ty0 - 3 + p / DW_HX, ix = tx0 - 3 + p % DW_HX;
        uint4 val = make_uint4(0u, 0u, 0u, 0u);   // zero padding outside the image
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) val = *(const uint4*)(xi + ((int64_t)iy * W + ix) * C + v * 8);
        tile[i] = val;
    }
    for (int i = threadIdx.x; i < 49 * 16; i += 256) taps[i] = *(const float4*)(w + (int64_t)(i >> 4) * C + c0 + (i & 15) * 4);
    __syncthreads();

    const int cg = threadIdx.x & 7, r = threadIdx.x >> 3;
    const int oy = r >> 2, ox0 = (r & 3) * 4;
    f32x2_t acc[4][4];
    {
        const float4 b0 = *(const float4*)(bias + c0 + cg * 8), b1 = *(const float4*)(bias + c0 + cg * 8 + 4);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            acc[p][0] = f32x2_t{b0.x, b0.y}; acc[p][1] = f32x2_t{b0.z, b0.w};
            acc[p][2] = f32x2_t{b1.x, b1.y}; acc[p][3] = f32x2_t{b1.z, b1.w};
        }
    }
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {   // (not unrolled: the compiler would hoist all 70 vector reads and spill)
        f32x2_t in[10][4];
        const uint4* row = tile + ((oy + ky) * DW_HX + ox0) * 8 + cg;
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const uint4 u = row[j * 8];
            in[j][0] = bf16x2_to_f32x2(u.x); in[j][1] = bf16x2_to_f32x2(u.y);
            in[j][2] = bf16x2_to_f32x2(u.z); in[j][3] = bf16x2_to_f32x2(u.w);
        }
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const float4 wa = taps[(ky * 7 + kx) * 16 + cg * 2], wb = taps[(ky * 7 + kx) * 16 + cg * 2 + 1];
            const f32x2_t w2[4] = {f32x2_t{wa.x, wa.y}, f32x2_t{wa.z, wa.w}, f32x2_t{wb.x, wb.y}, f32x2_t{wb.z, wb.w}};
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = __builtin_elementwise_fma(in[p + kx][q], w2[q], acc[p][q]);
        }
    }
    const int gy = ty0 + oy;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int gx = tx0 + ox0 + p;
        uint4 o;
        o.x = pack_bf16x2(acc[p][0][0], acc[p][0][1]); o.y = pack_bf16x2(acc[p][1][0], acc[p][1][1]);
        o.z = pack_bf16x2(acc[p][2][0], acc[p][2][1]); o.w = pack_bf16x2(acc[p][3][0], acc[p][3][1]);
        // statistics of the values as STORED (the rows the fc1 GEMM reads)
        float s1 = 0.f, s2 = 0.f;
        const uint32_t words[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x2_t v = bf16x2_to_f32x2(words[k]);
            s1 += v[0] + v[1];
            s2 = fmaf(v[0], v[0], fmaf(v[1], v[1], s2));
        }
#pragma unroll
        for (int o8 = 1; o8 < 8; o8 <<= 1) { s1 += __shfl_xor(s1, o8, 64); s2 += __shfl_xor(s2, o8, 64); }
        if (gy < H && gx < W) {
            const int64_t prow = (img * H + gy) * W + gx;
            *(uint4*)(y + prow * C + c0 + cg * 8) = o;
            if (cg == 0) partials[(int64_t)slot * rows + prow] = make_float2(s1, s2);
        }
    }
}

// ---- downsample gather --------------------------------------------------------------------------------------------------------------------
// out[(img, oy, ox), (ky * 2 + kx) * C + c] = LN(x[(img, 2 oy + ky, 2 ox + kx), :])[c] with (mean, rstd) from mq_row_stats; one thread = 8 channels
__global__ __launch_bounds__(256) void ds_gather_kernel(const bf16_t* __restrict__ x, const float2* __restrict__ stats, const float* __restrict__ g,
                                                        const float* __restrict__ b, bf16_t* __restrict__ out, int64_t total, int H, int W, int C) {
    const int cv = C >> 3, Ho = H >> 1, Wo = W >> 1;
    for (int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x; gi < total; gi += (int64_t)gridDim.x * 256) {
        const int v = (int)(gi % cv);
        const int64_t t = gi / cv;
        const int q = (int)(t & 3);
        const int64_t orow = t >> 2;
        const int64_t img = orow / (Ho * Wo);
        const int rem = (int)(orow - img * Ho * Wo);
        const int oy = rem / Wo, ox = rem - oy * Wo;
        const int64_t irow = (img * H + 2 * oy + (q >> 1)) * W + 2 * ox + (q & 1);
        const uint4 u = *(const uint4*)(x + irow * C + v * 8);
        const float2 st = stats[irow];
        const float4 g0 = *(const float4*)(g + v * 8), g1 = *(const float4*)(g + v * 8 + 4);
        const float4 b0 = *(const float4*)(b + v * 8), b1 = *(const float4*)(b + v * 8 + 4);
        const f32x2_t x0 = bf16x2_to_f32x2(u.x), x1 = bf16x2_to_f32x2(u.y), x2 = bf16x2_to_f32x2(u.z), x3 = bf16x2_to_f32x2(u.w);
        uint4 o;
        o.x = pack_bf16x2((x0[0] - st.x) * st.y * g0.x + b0.x, (x0[1] - st.x) * st.y * g0.y + b0.y);
        o.y = pack_bf16x2((x1[0] - st.x) * st.y * g0.z + b0.z, (x1[1] - st.x) * st.y * g0.w + b0.w);
        o.z = pack_bf16x2((x2[0] - st.x) * st.y * g1.x + b1.x, (x2[1] - st.x) * st.y * g1.y + b1.y);
        o.w = pack_bf16x2((x3[0] - st.x) * st.y * g1.z + b1.z, (x3[1] - st.x) * st.y * g1.w + b1.w);
        *(uint4*)(out + orow * (4 * (int64_t)C) + q * C + v * 8) = o;
    }
}

// ---- pooled head ----------------------------------------------------------------------------------------------------------------------------
constexpr int POOL_MAX_C = 3072;

__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();   // (red is reused by consecutive calls)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void pool_ln_kernel(const bf16_t* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                      bf16_t* __restrict__ out_bf16, float* __restrict__ out_f32, int HW, int C, float eps) {
    __shared__ float m[POOL_MAX_C];
    __shared__ float red[4];
    const int64_t img = blockIdx.x;
    const bf16_t* xi = x + img * HW * C;
    const float inv_hw = 1.0f / (float)HW;
    for (int v = threadIdx.x; v < (C >> 3); v += 256) {
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < HW; ++p) {
            const uint4 u = *(const uint4*)(xi + (int64_t)p * C + v * 8);
            const uint32_t words[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) { const f32x2_t t = bf16x2_to_f32x2(words[k]); s[2 * k] += t[0]; s[2 * k + 1] += t[1]; }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) m[v * 8 + e] = s[e] * inv_hw;
    }
    __syncthreads();
    float s1 = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) s1 += m[c];
    const float mean = block_sum256(s1, red) / (float)C;
    float s2 = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) { const float d = m[c] - mean; s2 += d * d; }
    const float rstd = rsqrtf(block_sum256(s2, red) / (float)C + eps);
    for (int c = threadIdx.x; c < C; c += 256) {
        const float v = (m[c] - mean) * rstd * g[c] + b[c];
        if (out_bf16) out_bf16[img * C + c] = f32_to_bf16(v);
        if (out_f32) out_f32[img * C + c] = v;
    }
}

}  // namespace

// ---- building blocks (C ABI) ------------------------------------------------------------------------------------------------------------------
extern "C" int mq_convnext_dwconv(const void* d_x, const float* d_w, const float* d_b, void* d_y, float* d_partials, int64_t n, int32_t H, int32_t W,
                                  int32_t C, void* stream) {
    MQ_CHECK_ARG(d_x && d_w && d_b && d_y && d_partials, "mq_convnext_dwconv: null operand");
    MQ_CHECK_ARG(C >= 64 && C % 64 == 0 && C <= 4096, "mq_convnext_dwconv: C=%d must be a multiple of 64 (<= 4096)", C);
    MQ_CHECK_ARG(H >= 1 && W >= 1 && H <= 4096 && W <= 4096 && n <= 65535, "mq_convnext_dwconv: bad shape n=%ld H=%d W=%d", (long)n, H, W);
    MQ_CHECK_ARG(d_x != d_y, "mq_convnext_dwconv: the output must not alias the input");
    if (n <= 0) return MQ_OK;
    const int tiles_x = (W + DW_TX - 1) / DW_TX, tiles_y = (H + DW_TY - 1) / DW_TY;
    hipLaunchKernelGGL(dwconv7_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)(C / 64), (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)d_x, d_w, d_b, (bf16_t*)d_y, (float2*)d_partials, (int)H, (int)W, (int)C, tiles_x, n * H * W);
    MQ_CHECK_LAUNCH("mq_convnext_dwconv");
    return MQ_OK;
}

extern "C" int mq_convnext_downsample(const void* d_x, const float* d_stats, const float* d_g, const float* d_b, void* d_out, int64_t n, int32_t H,
                                      int32_t W, int32_t C, void* stream) {
    MQ_CHECK_ARG(d_x && d_stats && d_g && d_b && d_out, "mq_convnext_downsample: null operand");
    MQ_CHECK_ARG(C >= 8 && C % 8 == 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "mq_convnext_downsample: bad shape H=%d W=%d C=%d", H, W, C);
    if (n <= 0) return MQ_OK;
    const int64_t total = n * (H / 2) * (W / 2) * 4 * (C / 8);
    const unsigned grid = (unsigned)(cdiv64(total, 256) < 16384 ? cdiv64(total, 256) : 16384);
    MqProfScope prof(1, (hipStream_t)stream);
    hipLaunchKernelGGL(ds_gather_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)d_x, (const float2*)d_stats, d_g, d_b,
                       (bf16_t*)d_out, total, (int)H, (int)W, (int)C);
    MQ_CHECK_LAUNCH("mq_convnext_downsample");
    return MQ_OK;
}

extern "C" int mq_convnext_pool_ln(const void* d_x, const float* d_g, const float* d_b, void* d_out_bf16, float* d_out_f32, int64_t n, int32_t HW,
                                   int32_t C, float eps, void* stream) {
    MQ_CHECK_ARG(d_x && d_g && d_b && (d_out_bf16 || d_out_f32), "mq_convnext_pool_ln: null operand");
    MQ_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= POOL_MAX_C && HW >= 1, "mq_convnext_pool_ln: bad shape HW=%d C=%d (C multiple of 8, <= %d)", HW, C,
                 POOL_MAX_C);
    if (n <= 0) return MQ_OK;
    MqProfScope prof(4, (hipStream_t)stream);
    hipLaunchKernelGGL(pool_ln_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)d_x, d_g, d_b, (bf16_t*)d_out_bf16, d_out_f32,
                       (int)HW, (int)C, eps);
    MQ_CHECK_LAUNCH("mq_convnext_pool_ln");
    return MQ_OK;
}

// ---- the tower -------------------------------------------------------------------------------------------------------------------------------
namespace {

struct CnxPlan {
    int64_t rows0;        // n * (S / 4)^2
    size_t x_off, y_off, h_off, part_off, stats_off, pool_off, hid_off, total;
};

bool cnx_cfg_ok(const mq_convnext_cfg* c) {
    if (!c || c->image_size < 32 || c->image_size % 32 != 0 || c->out_dim < 4 || c->out_dim % 4 != 0) return false;
    if (c->head != MQ_CONVNEXT_HEAD_LINEAR && c->head != MQ_CONVNEXT_HEAD_MLP) return false;
    for (int i = 0; i < 4; ++i)
        if (c->depths[i] < 1 || c->dims[i] < 64 || c->dims[i] % 64 != 0 || c->dims[i] > POOL_MAX_C) return false;
    for (int i = 1; i < 4; ++i)
        if (c->dims[i - 1] > 2048) return false;   // the downsample LayerNorm's statistics (mq_row_stats)
    return c->dims[0] <= 2048;                     // the stem LayerNorm
}

CnxPlan cnx_plan(const mq_convnext_cfg* c, int64_t n) {
    CnxPlan p{};
    const int64_t G = c->image_size / 4;
    p.rows0 = n * G * G;
    // every stage halves the stream (a quarter of the pixels, twice the channels): stage 0 sizes every buffer
    const size_t stream = (size_t)p.rows0 * c->dims[0] * 2;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
    p.x_off = take(stream);
    p.y_off = take(stream);
    p.h_off = take(4 * stream > (size_t)p.rows0 * 64 * 2 ? 4 * stream : (size_t)p.rows0 * 64 * 2);   // fc1 hidden rows; the stem's patch matrix
    p.part_off = take((size_t)(c->dims[0] / 64) * p.rows0 * 8);
    p.stats_off = take((size_t)p.rows0 * 8);
    p.pool_off = take((size_t)n * c->dims[3] * 2);
    p.hid_off = take((size_t)n * 2 * c->out_dim * 2);
    p.total = off;
    return p;
}

int cnx_forward(const mq_convnext_cfg* c, const mq_convnext_weights* w, const void* d_pixels, bool is_u8, int64_t n, float* d_out, int normalize,
                void* d_ws, size_t ws_bytes, hipStream_t s) {
    MQ_CHECK_ARG(c && w && d_pixels && d_out && w->blocks, "mq_encode_convnext: null argument");
    MQ_CHECK_ARG(cnx_cfg_ok(c), "mq_encode_convnext: unsupported cfg (image_size multiple of 32; dims multiples of 64, <= 3072, stages 0-2 <= 2048)");
    MQ_CHECK_ARG(n >= 1 && n <= 65535, "mq_encode_convnext: n=%ld out of range", (long)n);
    MQ_CHECK_ARG(w->stem_w && w->stem_b && w->stem_ln_g && w->stem_ln_b && w->head_ln_g && w->head_ln_b && w->proj_w,
                 "mq_encode_convnext: missing stem / head weights");
    MQ_CHECK_ARG(c->head != MQ_CONVNEXT_HEAD_MLP || (w->proj_b && w->proj2_w), "mq_encode_convnext: the mlp head needs proj_b and proj2_w");
    const CnxPlan p = cnx_plan(c, n);
    MQ_CHECK_ARG(d_ws && ws_bytes >= p.total, "mq_encode_convnext: workspace %zu < %zu bytes", ws_bytes, p.total);
    char* ws = (char*)d_ws;
    void* x = ws + p.x_off;
    void* y = ws + p.y_off;
    void* h = ws + p.h_off;
    float* part = (float*)(ws + p.part_off);
    float* stats = (float*)(ws + p.stats_off);
    void* pooled = ws + p.pool_off;
    void* hid = ws + p.hid_off;
    const float eps = c->ln_eps;

    // stem: 4x4 stride-4 patches (K = 48, zero-padded to 64) -> GEMM + bias -> per-pixel LayerNorm into the stream
    int H = c->image_size / 4;
    int64_t rows = p.rows0;
    int C = c->dims[0];
    MQ_TRY(mq_patchify(d_pixels, is_u8, h, n, c->image_size, 4, 64, c->mean, c->std, s));
    MQ_TRY(mq_gemm_bf16(h, 64, w->stem_w, 64, w->stem_b, nullptr, y, C, rows, C, 64, MQ_EPI_BIAS, s));
    MQ_TRY(mq_layernorm_ex(y, 1, nullptr, w->stem_ln_g, w->stem_ln_b, x, nullptr, rows, C, eps, s));

    const mq_convnext_block_weights* blk = w->blocks;
    for (int st = 0; st < 4; ++st) {
        if (st > 0) {
            const int Cp = C;
            C = c->dims[st];
            MQ_CHECK_ARG(w->ds_ln_g[st] && w->ds_ln_b[st] && w->ds_w[st] && w->ds_b[st], "mq_encode_convnext: missing downsample weights of stage %d", st);
            MQ_TRY(mq_row_stats(x, stats, rows, Cp, eps, s));
            MQ_TRY(mq_convnext_downsample(x, stats, w->ds_ln_g[st], w->ds_ln_b[st], y, n, H, H, Cp, s));
            H /= 2;
            rows = n * H * H;
            MQ_TRY(mq_gemm_bf16(y, 4 * Cp, w->ds_w[st], 4 * Cp, w->ds_b[st], nullptr, x, C, rows, C, 4 * Cp, MQ_EPI_BIAS, s));
        }
        for (int j = 0; j < c->depths[st]; ++j, ++blk) {
            // x = x + gamma * fc2(GELU(fc1(LN(dwconv(x)))))   (gamma folded into fc2, the LayerNorm into fc1)
            MQ_TRY(mq_convnext_dwconv(x, blk->dw_w, blk->dw_b, y, part, n, H, H, C, s));
            MQ_TRY(mq_row_stats_finalize(part, C / 64, stats, rows, C, eps, s));
            MQ_TRY(mq_gemm_bf16_ln(y, C, blk->fc1_w, C, blk->fc1_b, blk->fc1_s, stats, h, 4 * C, rows, 4 * C, C, MQ_EPI_BIAS | MQ_EPI_GELU, s));
            // (bf16 residual read-modify-write in place: MQ_EPI_RESIDUAL without MQ_EPI_OUT_F32 takes d_residual as bf16 rows)
            MQ_TRY(mq_gemm_bf16(h, 4 * C, blk->fc2_w, 4 * C, blk->fc2_b, (const float*)x, x, C, rows, C, 4 * C, MQ_EPI_BIAS | MQ_EPI_RESIDUAL, s));
        }
    }
    // timm head (global average pool -> head.norm), then open_clip's projection head
    MQ_TRY(mq_convnext_pool_ln(x, w->head_ln_g, w->head_ln_b, pooled, nullptr, n, H * H, C, eps, s));
    const int E = c->out_dim;
    if (c->head == MQ_CONVNEXT_HEAD_LINEAR) {
        MQ_TRY(mq_gemm_bf16(pooled, C, w->proj_w, C, nullptr, nullptr, d_out, E, n, E, C, MQ_EPI_OUT_F32, s));
    } else {
        MQ_TRY(mq_gemm_bf16(pooled, C, w->proj_w, C, w->proj_b, nullptr, hid, 2 * E, n, 2 * E, C, MQ_EPI_BIAS | MQ_EPI_GELU, s));
        MQ_TRY(mq_gemm_bf16(hid, 2 * E, w->proj2_w, 2 * E, w->proj2_b, nullptr, d_out, E, n, E, 2 * E,
                            w->proj2_b ? (MQ_EPI_BIAS | MQ_EPI_OUT_F32) : MQ_EPI_OUT_F32, s));
    }
    if (normalize) MQ_TRY(mq_l2_normalize(d_out, d_out, n, E, s));
    return MQ_OK;
}

}  // namespace

extern "C" size_t mq_convnext_workspace_bytes(const mq_convnext_cfg* cfg, int64_t n_images) {
    if (!cnx_cfg_ok(cfg) || n_images < 1) return 0;
    return cnx_plan(cfg, n_images).total;
}

extern "C" int mq_encode_convnext_u8(const mq_convnext_cfg* cfg, const mq_convnext_weights* w, const uint8_t* d_pixels, int64_t n, float* d_out,
                                     int normalize, void* d_workspace, size_t workspace_bytes, void* stream) {
    return cnx_forward(cfg, w, d_pixels, true, n, d_out, normalize, d_workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int mq_encode_convnext_f32(const mq_convnext_cfg* cfg, const mq_convnext_weights* w, const float* d_pixels, int64_t n, float* d_out,
                                      int normalize, void* d_workspace, size_t workspace_bytes, void* stream) {
    return cnx_forward(cfg, w, d_pixels, false, n, d_out, normalize, d_workspace, workspace_bytes, (hipStream_t)stream);
}
