// LanguageBind video tower: what its temporal sub-block needs beyond the CLIP ViT kernels (reference: s2_inference/languagebind/video/
// modeling_video.py:209-231 — temporal embedding into the residual stream, temporal LayerNorm, attention ACROSS the T frames at each spatial token,
// residual add).  The activation stays in the frame-major order of the spatial blocks, row r = (b T + t) N + n, from the first layer to the last:
//   * temporal_embed_ln:  x[r] += temb[t] in place (fp32 stream; skipped at T == 1 as the reference skips it), then the temporal LayerNorm of the
//                         updated row as bf16 — the A operand of the temporal QKV GEMM.  One pass over the row, one wave64 per row.
//   * temporal_attention: softmax(q k^T / 8) v over the T rows {(b T + t) N + n} of every (b, n, head), read at their stride of N rows: the
//                         `(b t) n d <-> (b n) t d` transposes of the reference are never materialised.  64-wide heads, T <= 16.
//   * patchify_clip:      the bf16 im2col rows of mq_patchify for the B T frames in (b t) order, read straight from the `b c t h w` clip.
// The QKV / out-projection GEMMs around the attention are mq_gemm_bf16 calls of the engine (engine/languagebind.py).
#include "common.h"

namespace {
constexpr int TA_MAX_T = 16;       // frames a lane quad-row layout of one wave holds: 16 slots of 4 lanes
constexpr int TA_HD = 64;          // head width

template <int CH>
__global__ __launch_bounds__(256) void temporal_embed_ln_kernel(float* __restrict__ x, const float* __restrict__ temb, const float* __restrict__ g,
                                                                const float* __restrict__ b, bf16_t* __restrict__ out, int64_t rows, int T, int N,
                                                                int W, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int nch = W >> 2;
    const int t = (int)((r / N) % T);
    float* xr = x + r * W;
    f32x4 v[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        if (c < nch) {
            v[i] = *(const f32x4*)(xr + c * 4);
            if (temb) {
                v[i] += *(const f32x4*)(temb + (int64_t)t * W + c * 4);     // (one fp32 add per element: the stream carries x + temb[t] from here on)
                *(f32x4*)(xr + c * 4) = v[i];
            }
        } else {
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    ln_normalize_row<CH>(v, lane, nch, W, eps);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        if (c < nch) {
            const f32x4 gg = *(const f32x4*)(g + c * 4), bb = *(const f32x4*)(b + c * 4);
            uint2 p;
            p.x = pack_bf16x2(fmaf(v[i][0], gg[0], bb[0]), fmaf(v[i][1], gg[1], bb[1]));
            p.y = pack_bf16x2(fmaf(v[i][2], gg[2], bb[2]), fmaf(v[i][3], gg[3], bb[3]));
            *(uint2*)(out + r * W + c * 4) = p;
        }
    }
}

__device__ __forceinline__ void unpack8(const uint4 u, float (&f)[8]) {
    f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
    f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
    f[4] = __uint_as_float(u.z << 16); f[5] = __uint_as_float(u.z & 0xffff0000u);
    f[6] = __uint_as_float(u.w << 16); f[7] = __uint_as_float(u.w & 0xffff0000u);
}

// One work item = one (b, n, head): T rows of q | k | v, 128 bytes each.  A wave holds 16 / TP items (TP = T rounded up to a power of two): slot
// sl = lane / 4 = (item in the wave) TP + frame, and the 4 lanes of a slot hold 16 of the head's 64 columns each (two 16-byte chunks, chunk part
// and chunk part + 4, so that every load instruction reads 64 contiguous bytes per row).  Every q / k / v element is read from memory once; K and
// V go through LDS (17 x 16 bytes per slot: the pad keeps the slots of different items off each other's banks), Q stays in registers.  Scores,
// softmax and P V are fp32; the probabilities are never rounded.
template <int TP>
__global__ __launch_bounds__(256) void temporal_attention_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int64_t items, int T, int N,
                                                                 int W, int heads) {
    __shared__ uint4 kv[4][16][17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sl = lane >> 2, part = lane & 3;
    constexpr int IPW = 16 / TP;
    const int iw = sl / TP, t = sl - iw * TP;
    const int64_t item = ((int64_t)blockIdx.x * 4 + wave) * IPW + iw;
    const bool live = item < items && t < T;
    int64_t row = 0;
    int h = 0;
    if (live) {
        const int64_t bn = item / heads;
        h = (int)(item - bn * heads);
        const int64_t bb = bn / N;
        row = (bb * T + t) * N + (bn - bb * N);
    }
    const bf16_t* src = qkv + row * 3 * (int64_t)W + h * TA_HD + part * 8;
    uint4 q0 = {0, 0, 0, 0}, q1 = q0, k0 = q0, k1 = q0, v0 = q0, v1 = q0;
    if (live) {
        q0 = *(const uint4*)(src);          q1 = *(const uint4*)(src + 32);
        k0 = *(const uint4*)(src + W);      k1 = *(const uint4*)(src + W + 32);
        v0 = *(const uint4*)(src + 2 * W);  v1 = *(const uint4*)(src + 2 * W + 32);
    }
    kv[wave][sl][part] = k0;
    kv[wave][sl][part + 4] = k1;
    kv[wave][sl][8 + part] = v0;
    kv[wave][sl][12 + part] = v1;
    __syncthreads();       // (every thread of the block arrives: dead lanes carry zeros and store nothing)
    float q[16];
    {
        float a[8], c[8];
        unpack8(q0, a);
        unpack8(q1, c);
#pragma unroll
        for (int e = 0; e < 8; ++e) { q[e] = a[e]; q[8 + e] = c[e]; }
    }
    float s[TP];
    float m = -3.0e38f;
#pragma unroll
    for (int j = 0; j < TP; ++j) {
        float ka[8], kc[8];
        unpack8(kv[wave][iw * TP + j][part], ka);
        unpack8(kv[wave][iw * TP + j][part + 4], kc);
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(q[e], ka[e], d);
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(q[8 + e], kc[e], d);
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);          // the four lanes of a slot now hold the same sum (xor butterfly: identical order in each)
        s[j] = d;
        if (j < T) m = fmaxf(m, d);
    }
    const float c2 = 1.44269504088896340736f * 0.125f;      // log2(e) / sqrt(64)
    float l = 0.f;
    float o[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
#pragma unroll
    for (int j = 0; j < TP; ++j) {
        if (j < T) {
            const float p = exp2f((s[j] - m) * c2);
            l += p;
            float va[8], vc[8];
            unpack8(kv[wave][iw * TP + j][8 + part], va);
            unpack8(kv[wave][iw * TP + j][12 + part], vc);
#pragma unroll
            for (int e = 0; e < 8; ++e) { o[e] = fmaf(p, va[e], o[e]); o[8 + e] = fmaf(p, vc[e], o[8 + e]); }
        }
    }
    if (live) {
        const float inv = 1.0f / l;
        bf16_t* dst = out + row * (int64_t)W + h * TA_HD + part * 8;
        uint4 w0, w1;
        w0.x = pack_bf16x2(o[0] * inv, o[1] * inv);   w0.y = pack_bf16x2(o[2] * inv, o[3] * inv);
        w0.z = pack_bf16x2(o[4] * inv, o[5] * inv);   w0.w = pack_bf16x2(o[6] * inv, o[7] * inv);
        w1.x = pack_bf16x2(o[8] * inv, o[9] * inv);   w1.y = pack_bf16x2(o[10] * inv, o[11] * inv);
        w1.z = pack_bf16x2(o[12] * inv, o[13] * inv); w1.w = pack_bf16x2(o[14] * inv, o[15] * inv);
        *(uint4*)(dst) = w0;
        *(uint4*)(dst + 32) = w1;
    }
}

// mq_patchify's fp32 kernel with the frame's pixels found in the clip layout: frame f = b T + t, pixel (c, y, x) at ((b 3 + c) T + t) S S + y S + x.
// One thread produces 8 consecutive output columns (one 16-byte store).
__global__ __launch_bounds__(256) void patchify_clip_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t total_groups, int T, int S,
                                                            int P, int G, int Kp) {
    const int groups_per_row = Kp >> 3;
    const int PP = P * P;
    for (int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x; gi < total_groups; gi += (int64_t)gridDim.x * 256) {
        const int64_t prow = gi / groups_per_row;
        const int col0 = (int)(gi - prow * groups_per_row) * 8;
        const int64_t f = prow / (G * G);
        const int pidx = (int)(prow - f * (G * G));
        const int py = pidx / G, px = pidx - py * G;
        const int64_t bb = f / T;
        const int t = (int)(f - bb * T);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = col0 + e;
            float val = 0.f;
            if (col < 3 * PP) {
                const int c = col / PP;
                const int rem = col - c * PP;
                const int ky = rem / P, kx = rem - ky * P;
                val = in[(((bb * 3 + c) * T + t) * S + (py * P + ky)) * (int64_t)S + (px * P + kx)];
            }
            v[e] = val;
        }
        uint4 p;
        p.x = pack_bf16x2(v[0], v[1]);
        p.y = pack_bf16x2(v[2], v[3]);
        p.z = pack_bf16x2(v[4], v[5]);
        p.w = pack_bf16x2(v[6], v[7]);
        *(uint4*)(out + prow * Kp + col0) = p;
    }
}

template <int TP>
void launch_temporal_attention(const void* d_qkv, void* d_out, int64_t items, int T, int N, int W, int heads, hipStream_t s) {
    const int64_t per_block = 4 * (16 / TP);
    hipLaunchKernelGGL((temporal_attention_kernel<TP>), dim3((unsigned)cdiv64(items, per_block)), dim3(256), 0, s, (const bf16_t*)d_qkv, (bf16_t*)d_out,
                       items, T, N, W, heads);
}
}  // namespace

// ---- host entry points (C ABI, include/marqo_hip.h) -----------------------------------------------------------
extern "C" int mq_temporal_embed_ln(float* d_x, const float* d_temb, const float* d_g, const float* d_b, void* d_out_bf16, int64_t B, int32_t T,
                                    int32_t N, int32_t W, float eps, void* stream) {
    MQ_CHECK_ARG(W >= 4 && W % 4 == 0 && W <= 2048, "mq_temporal_embed_ln: W=%d must be a multiple of 4, at most 2048", W);
    MQ_CHECK_ARG(T >= 1 && N >= 1, "mq_temporal_embed_ln: T=%d and N=%d must be at least 1", T, N);
    MQ_CHECK_ARG(B >= 0 && B * (int64_t)T * N < (1ll << 31) * 4, "mq_temporal_embed_ln: B=%lld too large", (long long)B);
    if (B == 0) return MQ_OK;
    MQ_CHECK_ARG(d_x && d_temb && d_g && d_b && d_out_bf16, "mq_temporal_embed_ln: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(1, s);
    const int64_t rows = B * T * N;
    const float* temb = T == 1 ? nullptr : d_temb;     // modeling_video.py:214: no temporal embedding for a single frame
    MQ_DISPATCH_CH(W, hipLaunchKernelGGL((temporal_embed_ln_kernel<CH>), dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, d_x, temb, d_g, d_b,
                                         (bf16_t*)d_out_bf16, rows, T, N, W, eps));
    MQ_CHECK_LAUNCH("mq_temporal_embed_ln");
    return MQ_OK;
}

extern "C" int mq_temporal_attention(const void* d_qkv, void* d_out, int64_t B, int32_t T, int32_t N, int32_t W, int32_t heads, void* stream) {
    MQ_CHECK_ARG(heads >= 1 && W == heads * TA_HD, "mq_temporal_attention: 64-wide heads only (W=%d, heads=%d)", W, heads);
    MQ_CHECK_ARG(T >= 1 && T <= TA_MAX_T, "mq_temporal_attention: T=%d must be in [1, %d]", T, TA_MAX_T);
    MQ_CHECK_ARG(N >= 1, "mq_temporal_attention: N=%d must be at least 1", N);
    MQ_CHECK_ARG(B >= 0 && B * (int64_t)N * heads < (1ll << 31) && B * (int64_t)T * N < (1ll << 31), "mq_temporal_attention: B=%lld too large",
                 (long long)B);
    if (B == 0) return MQ_OK;
    MQ_CHECK_ARG(d_qkv && d_out, "mq_temporal_attention: null pointer");
    MQ_CHECK_ARG(((uintptr_t)d_qkv & 15) == 0 && ((uintptr_t)d_out & 15) == 0, "mq_temporal_attention: pointers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(2, s);
    const int64_t items = B * N * heads;
    if (T == 1) launch_temporal_attention<1>(d_qkv, d_out, items, T, N, W, heads, s);
    else if (T == 2) launch_temporal_attention<2>(d_qkv, d_out, items, T, N, W, heads, s);
    else if (T <= 4) launch_temporal_attention<4>(d_qkv, d_out, items, T, N, W, heads, s);
    else if (T <= 8) launch_temporal_attention<8>(d_qkv, d_out, items, T, N, W, heads, s);
    else launch_temporal_attention<16>(d_qkv, d_out, items, T, N, W, heads, s);
    MQ_CHECK_LAUNCH("mq_temporal_attention");
    return MQ_OK;
}

extern "C" int mq_patchify_clip(const float* d_in, void* d_out, int64_t B, int32_t T, int32_t S, int32_t P, int32_t Kp, void* stream) {
    MQ_CHECK_ARG(T >= 1 && P >= 1 && S >= P, "mq_patchify_clip: bad shape T=%d S=%d P=%d", T, S, P);
    MQ_CHECK_ARG(Kp % 8 == 0 && Kp >= 3 * P * P, "mq_patchify_clip: Kp=%d must be a multiple of 8 and at least 3 P^2 = %d", Kp, 3 * P * P);
    const hipStream_t s = (hipStream_t)stream;
    const int G = S / P;
    const int64_t total = B * T * G * G * (Kp >> 3);
    if (total <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_in && d_out, "mq_patchify_clip: null pointer");
    MqProfScope prof(5, s);
    const unsigned grid = (unsigned)(cdiv64(total, 256) < 16384 ? cdiv64(total, 256) : 16384);
    hipLaunchKernelGGL(patchify_clip_kernel, dim3(grid), dim3(256), 0, s, d_in, (bf16_t*)d_out, total, T, S, P, G, Kp);
    MQ_CHECK_LAUNCH("mq_patchify_clip");
    return MQ_OK;
}
