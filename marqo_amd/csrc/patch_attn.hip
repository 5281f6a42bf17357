// Attention-based image patching (the reference's 'dino-v1' / 'dino-v2' patch methods, s2_inference/processing/image.py + DINO_utils.py):
// what the class token of a DINO ViT looks at in the last block, and the boxes around the bright regions of those maps.
//
//   mq_attention_cls_probs  softmax of query row 0 of every (sequence, head) over all T keys — K is read once, V never
//   mq_attn_boxes           per (image, map) on the G x G patch grid, in LDS: rescale to uint8, Otsu threshold, 8-connected foreground
//                           components, the 4-connected background that reaches the frame, boxes of the components that touch it
//
// The reference works on the maps upsampled x patch by nearest neighbour; that changes neither the histogram's proportions nor the topology,
// so everything here runs on the grid and the caller multiplies the boxes by the patch size.
#include "common.h"

#include <float.h>

namespace {

// ---- class-token attention row ---------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per (sequence, head).  A key row of one head is 64 bf16 = 8 chunks of 16 bytes: 8 neighbouring lanes load one
// chunk each (a wave reads 8 whole key rows = 8 x 128 contiguous bytes per step), multiply it with their 8 query values (registers) and the
// partial sums meet through three xor-shuffles.  Raw scores wait in LDS; maximum and sum are wave reductions joined through LDS.
// All arithmetic is fp32 on exact bf16 x bf16 products (tests/dino_ref.py, cls_probs_budget, bounds the result from this order).
constexpr int CLS_THREADS = 256;
constexpr int CLS_MAX_T = 8192;     // fp32 scores in dynamic LDS: 32 KB at the most

__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
    v = is_max ? wave_max(v) : wave_sum(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                   // (red may still be read from the previous reduction)
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < CLS_THREADS / 64; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

__global__ __launch_bounds__(CLS_THREADS) void attention_cls_probs_kernel(const bf16_t* __restrict__ qkv, float* __restrict__ probs, int T, int W,
                                                                           int heads) {
    extern __shared__ float scores[];                  // [T]
    __shared__ float red[CLS_THREADS / 64];
    const int64_t seq = blockIdx.x / heads;
    const int head = blockIdx.x % heads;
    const int chunk = threadIdx.x & 7, sub = threadIdx.x >> 3;        // 32 keys per step of the workgroup
    const int64_t ld = 3 * (int64_t)W;
    const bf16_t* base = qkv + seq * T * ld + head * 64 + chunk * 8;
    float q[8];
    {
        const uint4 v = *(const uint4*)base;                          // query row 0, this lane's 8 columns
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            q[2 * i] = __uint_as_float(w[i] << 16);
            q[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
    for (int j0 = 0; j0 < T; j0 += CLS_THREADS / 8) {
        const int j = j0 + sub;
        float acc = 0.f;
        if (j < T) {
            const uint4 v = *(const uint4*)(base + (int64_t)j * ld + W);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc = fmaf(q[2 * i], __uint_as_float(w[i] << 16), acc);
                acc = fmaf(q[2 * i + 1], __uint_as_float(w[i] & 0xffff0000u), acc);
            }
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 4, 64);
        if (j < T && chunk == 0) scores[j] = acc;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = threadIdx.x; j < T; j += CLS_THREADS) m = fmaxf(m, scores[j]);
    m = block_reduce(m, true, red);
    float l = 0.f;
    for (int j = threadIdx.x; j < T; j += CLS_THREADS) {
        const float e = expf((scores[j] - m) * 0.125f);              // 1 / sqrt(64): exact
        scores[j] = e;                                                // (each thread rereads only what it wrote)
        l += e;
    }
    l = block_reduce(l, false, red);
    float* out = probs + (seq * heads + head) * (int64_t)(T - 1);
    for (int j = threadIdx.x + 1; j < T; j += CLS_THREADS) out[j - 1] = scores[j] / l;   // the class key stays in l and is not written
}

// ---- maps -> boxes ------------------------------------------------------------------------------------------------------------------
constexpr int BOX_THREADS = 256;
constexpr int BOX_MAX_G = 32;
constexpr int BOX_CELLS = BOX_MAX_G * BOX_MAX_G;

// OpenCV's getThreshVal_Otsu for 8-bit images, restated: double precision, classes lighter than FLT_EPSILON skipped, the first strict maximum wins.
// `hist` holds counts on the grid; the upsampled image has patch^2 times each count and patch^2 times the total, and for a power-of-two patch that
// scaling is exact in double — the threshold is the one of the upsampled image.  No fused multiply-adds: the host code this restates has none.
__device__ int otsu_threshold(const int* hist, int cells) {
#pragma clang fp contract(off)
    const double scale = 1.0 / (double)cells;
    double mu = 0.0;
    for (int i = 0; i < 256; ++i) mu += (double)i * (double)hist[i];
    mu *= scale;
    double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
    int max_val = 0;
    for (int i = 0; i < 256; ++i) {
        const double p_i = (double)hist[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1.0 - q1;
        if (fmin(q1, q2) < (double)FLT_EPSILON || fmax(q1, q2) > 1.0 - (double)FLT_EPSILON) continue;
        mu1 = (mu1 + (double)i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double d = mu1 - mu2;
        const double sigma = q1 * q2 * d * d;
        if (sigma > max_sigma) { max_sigma = sigma; max_val = i; }
    }
    return max_val;
}

// One workgroup per (image, map).  mode 0: one map per image, the mean over the heads of |p| (summed head by head in fp32, then divided: the order
// of NumPy's mean over the leading axis); mode 1: one map per head, negatives zeroed.  A map with maximum 0 (all zero; mode 1: nothing positive) divides
// 0 by 0: the NaN goes to level 0 in every cell, Otsu then returns 0, nothing is foreground and the count is 0 (the reference's cast of NaN to uint8
// is undefined, so there is nothing to match; tests/test_patch_attn_gpu.py, test_attn_boxes_map_without_a_positive_cell).
__global__ __launch_bounds__(BOX_THREADS) void attn_boxes_kernel(const float* __restrict__ probs, int heads, int G, int mode, int32_t* __restrict__ boxes,
                                                                 int32_t* __restrict__ counts, int max_boxes) {
    __shared__ float val[BOX_CELLS];
    __shared__ int label[BOX_CELLS];          // foreground: smallest raster index of the component so far; background: -1
    __shared__ int outer[BOX_CELLS];          // background cell joined to the frame through 4-neighbours
    __shared__ int x0[BOX_CELLS], y0[BOX_CELLS], x1[BOX_CELLS], y1[BOX_CELLS], ext[BOX_CELLS];   // per component, at its first cell
    __shared__ int hist[256];
    __shared__ float red[BOX_THREADS / 64];
    __shared__ int thresh;
    const int cells = G * G, tid = threadIdx.x;
    const int maps = mode == 0 ? 1 : heads;
    const int64_t img = blockIdx.x / maps;
    const int map = blockIdx.x % maps;
    const float* src = probs + (img * heads + (mode == 0 ? 0 : map)) * (int64_t)cells;

    float mx = 0.f;
    for (int c = tid; c < cells; c += BOX_THREADS) {
        float v;
        if (mode == 0) {
            v = fabsf(src[c]);
            for (int h = 1; h < heads; ++h) v += fabsf(src[(int64_t)h * cells + c]);
            v = v / (float)heads;
        } else {
            v = src[c];
            v = v < 0.f ? 0.f : v;
        }
        val[c] = v;
        mx = fmaxf(mx, v);
    }
    for (int i = tid; i < 256; i += BOX_THREADS) hist[i] = 0;
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    for (int c = tid; c < cells; c += BOX_THREADS) {
        float r = val[c] / mx;               // float32 division, multiplication, truncation: three roundings, as the host code does them
        r = r * 255.0f;
        const int u = r >= 0.f ? (r > 255.f ? 255 : (int)r) : 0;      // (0 / 0 -> 0)
        label[c] = u;
        atomicAdd(&hist[u], 1);
    }
    __syncthreads();
    if (tid == 0) thresh = otsu_threshold(hist, cells);
    __syncthreads();
    const int t = thresh;
    for (int c = tid; c < cells; c += BOX_THREADS) {
        const bool fg = label[c] > t;
        const int y = c / G, x = c - y * G;
        label[c] = fg ? c : -1;
        outer[c] = (!fg && (x == 0 || y == 0 || x == G - 1 || y == G - 1)) ? 1 : 0;
        x0[c] = G; y0[c] = G; x1[c] = -1; y1[c] = -1; ext[c] = 0;
    }
    __syncthreads();
    // both propagations to their fixed point (labels only fall, `outer` only rises: reading a neighbour mid-update is harmless)
    for (;;) {
        int changed = 0;
        for (int c = tid; c < cells; c += BOX_THREADS) {
            const int y = c / G, x = c - y * G;
            const int l = label[c];
            if (l >= 0) {
                int best = l;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int yy = y + dy, xx = x + dx;
                        if (yy < 0 || xx < 0 || yy >= G || xx >= G) continue;
                        const int n = label[yy * G + xx];
                        if (n >= 0 && n < best) best = n;
                    }
                if (best < l) { label[c] = best; changed = 1; }
            } else if (!outer[c]) {
                if ((x > 0 && outer[c - 1]) || (x < G - 1 && outer[c + 1]) || (y > 0 && outer[c - G]) || (y < G - 1 && outer[c + G])) {
                    outer[c] = 1;
                    changed = 1;
                }
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    // RETR_EXTERNAL: a component is reported when one of its cells lies on the frame or beside outer background
    for (int c = tid; c < cells; c += BOX_THREADS) {
        const int l = label[c];
        if (l < 0) continue;
        const int y = c / G, x = c - y * G;
        atomicMin(&x0[l], x); atomicMin(&y0[l], y); atomicMax(&x1[l], x); atomicMax(&y1[l], y);
        if (x == 0 || y == 0 || x == G - 1 || y == G - 1 || outer[c - 1] || outer[c + 1] || outer[c - G] || outer[c + G]) atomicOr(&ext[l], 1);
    }
    __syncthreads();
    if (tid == 0) {     // components in the raster order of their first cells (a few hundred cells: not worth a scan)
        int32_t* dst = boxes + (int64_t)blockIdx.x * max_boxes * 4;
        int n = 0;
        for (int c = 0; c < cells; ++c) {
            if (label[c] != c || !ext[c]) continue;
            if (n < max_boxes) {
                dst[n * 4 + 0] = x0[c]; dst[n * 4 + 1] = y0[c]; dst[n * 4 + 2] = x1[c] + 1; dst[n * 4 + 3] = y1[c] + 1;
            }
            ++n;
        }
        counts[blockIdx.x] = n;
    }
}

}  // namespace

extern "C" int mq_attention_cls_probs(const void* d_qkv, float* d_probs, int64_t nseq, int32_t T, int32_t W, int32_t heads, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    MQ_CHECK_ARG(d_qkv && d_probs, "attention_cls_probs: null pointer");
    MQ_CHECK_ARG(T >= 2 && T <= CLS_MAX_T, "attention_cls_probs: T=%d unsupported (2 .. %d: the class token and at least one key)", T, CLS_MAX_T);
    MQ_CHECK_ARG(heads >= 1 && W == heads * 64, "attention_cls_probs: W=%d must be heads=%d * 64", W, heads);
    MQ_CHECK_ARG(nseq >= 0 && nseq * heads < (int64_t)1 << 31, "attention_cls_probs: nseq=%lld out of range", (long long)nseq);
    if (nseq == 0) return MQ_OK;
    MqProfScope prof(2, s);
    hipLaunchKernelGGL(attention_cls_probs_kernel, dim3((unsigned)(nseq * heads)), dim3(CLS_THREADS), (size_t)T * sizeof(float), s,
                       (const bf16_t*)d_qkv, d_probs, T, W, heads);
    MQ_CHECK_LAUNCH("attention_cls_probs");
    return MQ_OK;
}

extern "C" int mq_attn_boxes(const float* d_probs, int64_t n, int32_t heads, int32_t G, int32_t mode, int32_t* d_boxes, int32_t* d_counts,
                             int32_t max_boxes, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    MQ_CHECK_ARG(d_probs && d_boxes && d_counts, "attn_boxes: null pointer");
    MQ_CHECK_ARG(G >= 1 && G <= BOX_MAX_G, "attn_boxes: G=%d unsupported (1 .. %d)", G, BOX_MAX_G);
    MQ_CHECK_ARG(heads >= 1 && (mode == 0 || mode == 1), "attn_boxes: heads=%d mode=%d (0: mean over heads, 1: per head)", heads, mode);
    MQ_CHECK_ARG(max_boxes >= 1, "attn_boxes: max_boxes=%d must be at least 1", max_boxes);
    MQ_CHECK_ARG(n >= 0 && n * heads < (int64_t)1 << 31, "attn_boxes: n=%lld out of range", (long long)n);
    if (n == 0) return MQ_OK;
    MqProfScope prof(4, s);
    hipLaunchKernelGGL(attn_boxes_kernel, dim3((unsigned)(n * (mode == 0 ? 1 : heads))), dim3(BOX_THREADS), 0, s, d_probs, heads, G, mode,
                       d_boxes, d_counts, max_boxes);
    MQ_CHECK_LAUNCH("attn_boxes");
    return MQ_OK;
}
