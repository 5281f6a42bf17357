// OWL-ViT image reranking: everything behind the image encoder (transformers' modeling_owlvit.py: image_text_embedder, OwlViTClassPredictionHead,
// OwlViTBoxPredictionHead, box_predictor) and the per-image top-k that keeps the detections on the device.
//   * owl_merge_ln:    post_layernorm of the class row and of every patch row, patch * class, layer_norm -> feats (bf16 for the GEMMs, fp32 for the row
//                      dot products).  One pass over the rows.
//   * owl_class_head:  on dense0's output e: e / (|e| + 1e-6) . t / (|t| + 1e-6) for up to 8 queries, the learned shift and ELU scale from feats,
//                      the query mask, the maximum over the queries and its sigmoid.
//   * owl_box_head:    dense2 (W -> 4) + bias + grid bias, sigmoid, centre -> corner format, times the target size.
//   * owl_topk:        per image the k best scores by rank counting (ties to the lower patch), their boxes and patch numbers.
// The W x W linears in between are mq_gemm_bf16 calls of the engine.  One wave64 per row, coalesced, bounds-guarded, untuned: all of it is bandwidth-
// trivial next to the encoder.
#include "common.h"
#include <float.h>

namespace {
constexpr int MAXC = 8;            // W <= 2048
constexpr int OWL_MAX_Q = 8;       // queries per image
constexpr int OWL_MAX_P = 8191;    // patches per image (mq_attention's 8192 tokens less the class token)

template <int CH>
__device__ __forceinline__ void load_row(const float* __restrict__ p, f32x4 (&v)[CH], int lane, int nch) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        v[i] = c < nch ? *(const f32x4*)(p + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int CH>
__device__ __forceinline__ void affine_row(f32x4 (&v)[CH], const float* __restrict__ g, const float* __restrict__ b, int lane, int nch) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + i * 64;
        if (c < nch) {
            const f32x4 gg = *(const f32x4*)(g + c * 4), bb = *(const f32x4*)(b + c * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] = fmaf(v[i][e], gg[e], bb[e]);
        } else {
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};       // (the lanes past the row must stay out of the next row's statistics)
        }
    }
}

// grid = ceil(n P / 4) blocks of 4 waves; wave -> patch row r = img P + p, which reads rows img T (class) and img T + 1 + p of x
template <int CH>
__global__ __launch_bounds__(256) void owl_merge_ln_kernel(const float* __restrict__ x, const float* __restrict__ pg, const float* __restrict__ pb,
                                                           const float* __restrict__ lg, const float* __restrict__ lb, bf16_t* __restrict__ fb,
                                                           float* __restrict__ ff, int64_t rows, int P, int W, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int64_t img = r / P;
    const int nch = W >> 2;
    const float* xc = x + img * (int64_t)(P + 1) * W;
    const float* xp = x + (img * (int64_t)(P + 1) + 1 + (r - img * P)) * W;
    f32x4 c[CH], v[CH];
    load_row<CH>(xc, c, lane, nch);
    ln_normalize_row<CH>(c, lane, nch, W, eps);
    affine_row<CH>(c, pg, pb, lane, nch);
    load_row<CH>(xp, v, lane, nch);
    ln_normalize_row<CH>(v, lane, nch, W, eps);
    affine_row<CH>(v, pg, pb, lane, nch);
#pragma unroll
    for (int i = 0; i < CH; ++i) v[i] *= c[i];
    ln_normalize_row<CH>(v, lane, nch, W, eps);
    affine_row<CH>(v, lg, lb, lane, nch);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int k = lane + i * 64;
        if (k < nch) {
            if (ff) *(f32x4*)(ff + r * W + k * 4) = v[i];
            if (fb) {
                uint2 p;
                p.x = pack_bf16x2(v[i][0], v[i][1]);
                p.y = pack_bf16x2(v[i][2], v[i][3]);
                *(uint2*)(fb + r * W + k * 4) = p;
            }
        }
    }
}

// one wave per patch row: e [rows, Dq] = dense0's output, f [rows, W] = feats, t [(n |) Q, Dq] = the model's query_embeds
__global__ __launch_bounds__(256) void owl_class_head_kernel(const float* __restrict__ e, const float* __restrict__ f, const float* __restrict__ t,
                                                             const int32_t* __restrict__ qmask, int64_t q_stride, const float* __restrict__ shift_w,
                                                             float shift_b, const float* __restrict__ scale_w, float scale_b, float* __restrict__ score,
                                                             float* __restrict__ logit, int32_t* __restrict__ label, int64_t rows, int P, int W, int Dq,
                                                             int Q) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int64_t img = r / P;
    const float* er = e + r * Dq;
    const float* tq = t + img * q_stride * Dq;
    const int32_t* mq = qmask ? qmask + img * q_stride : nullptr;
    float ee = 0.f, dot[OWL_MAX_Q], tt[OWL_MAX_Q];
#pragma unroll
    for (int q = 0; q < OWL_MAX_Q; ++q) dot[q] = tt[q] = 0.f;
    for (int j = lane; j < Dq; j += 64) {
        const float ev = er[j];
        ee = fmaf(ev, ev, ee);
#pragma unroll
        for (int q = 0; q < OWL_MAX_Q; ++q)
            if (q < Q) {
                const float tv = tq[(int64_t)q * Dq + j];
                dot[q] = fmaf(ev, tv, dot[q]);
                tt[q] = fmaf(tv, tv, tt[q]);
            }
    }
    const float* fr = f + r * W;
    float sh = 0.f, sc = 0.f;
    for (int j = lane; j < W; j += 64) {
        const float fv = fr[j];
        sh = fmaf(fv, shift_w[j], sh);
        sc = fmaf(fv, scale_w[j], sc);
    }
    ee = wave_sum(ee);
    sh = wave_sum(sh) + shift_b;
    sc = wave_sum(sc) + scale_b;
    const float scale = (sc > 0.f ? sc : expm1f(sc)) + 1.0f;      // ELU(.) + 1
    const float inv_e = 1.0f / (sqrtf(ee) + 1e-6f);
    float best = -FLT_MAX;       // torch.finfo(float32).min: what a masked query's logit becomes
    int arg = 0;
#pragma unroll
    for (int q = 0; q < OWL_MAX_Q; ++q)
        if (q < Q) {
            const float d = wave_sum(dot[q]), tn = wave_sum(tt[q]);
            float z = (d * inv_e / (sqrtf(tn) + 1e-6f) + sh) * scale;
            if (mq && mq[q] == 0) z = -FLT_MAX;
            if (z > best) { best = z; arg = q; }
        }
    if (lane == 0) {
        logit[r] = best;
        score[r] = 1.0f / (1.0f + expf(-best));
        label[r] = arg;
    }
}

// one wave per patch row: h bf16 [rows, W] = gelu(dense1(gelu(dense0(feats)))) as the GEMM's GELU epilogue leaves it, w2 [4, W]
__global__ __launch_bounds__(256) void owl_box_head_kernel(const bf16_t* __restrict__ h, const float* __restrict__ w2, const float* __restrict__ b2,
                                                           const float* __restrict__ box_bias, float* __restrict__ boxes, int64_t rows, int P, int W,
                                                           float tw, float th) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const bf16_t* hr = h + r * W;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = lane; j < W; j += 64) {
        const float hv = bf16_to_f32(hr[j]);
#pragma unroll
        for (int o = 0; o < 4; ++o) a[o] = fmaf(hv, w2[(int64_t)o * W + j], a[o]);
    }
    const int p = (int)(r % P);
    float s[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const float z = (wave_sum(a[o]) + b2[o]) + box_bias[p * 4 + o];
        s[o] = 1.0f / (1.0f + expf(-z));
    }
    if (lane == 0) {
        f32x4 out;
        out[0] = (s[0] - 0.5f * s[2]) * tw;
        out[1] = (s[1] - 0.5f * s[3]) * th;
        out[2] = (s[0] + 0.5f * s[2]) * tw;
        out[3] = (s[1] + 0.5f * s[3]) * th;
        *(f32x4*)(boxes + r * 4) = out;
    }
}

// one workgroup per image.  rank(i) = #{j : s_j > s_i or (s_j == s_i and j < i)} is a permutation of 0 .. P - 1, so the writes of the ranks
// below k land on distinct slots of [0, k).  NaN scores sort last.
__global__ __launch_bounds__(256) void owl_topk_kernel(const float* __restrict__ score, const float* __restrict__ boxes, int P, int k,
                                                       float* __restrict__ out_score, float* __restrict__ out_boxes, int32_t* __restrict__ out_patch) {
    __shared__ float key[OWL_MAX_P + 1];
    const int64_t img = blockIdx.x;
    const float* s = score + img * P;
    for (int i = threadIdx.x; i < P; i += 256) {
        const float v = s[i];
        key[i] = v != v ? -INFINITY : v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += 256) {
        const float v = key[i];
        int rank = 0;
        for (int j = 0; j < P; ++j) {
            const float u = key[j];
            rank += (u > v || (u == v && j < i)) ? 1 : 0;
        }
        if (rank < k) {
            const int64_t o = img * k + rank;
            out_score[o] = s[i];
            out_patch[o] = i;
            *(f32x4*)(out_boxes + o * 4) = *(const f32x4*)(boxes + (img * P + i) * 4);
        }
    }
}
}  // namespace

extern "C" int mq_owl_merge_ln(const float* d_x, const float* d_post_g, const float* d_post_b, const float* d_ln_g, const float* d_ln_b,
                               void* d_feats_bf16, float* d_feats_f32, int64_t n, int32_t T, int32_t W, float eps, void* stream) {
    MQ_CHECK_ARG(W >= 4 && W % 4 == 0 && W <= 64 * 4 * MAXC, "mq_owl_merge_ln: W=%d unsupported (a multiple of 4, at most %d)", W, 64 * 4 * MAXC);
    MQ_CHECK_ARG(T >= 2 && T - 1 <= OWL_MAX_P, "mq_owl_merge_ln: T=%d must be in [2, %d]", T, OWL_MAX_P + 1);
    MQ_CHECK_ARG(n >= 0 && n * (int64_t)(T - 1) < (1ll << 31) * 4, "mq_owl_merge_ln: n=%lld too large", (long long)n);
    if (n == 0) return MQ_OK;
    MQ_CHECK_ARG(d_x && d_post_g && d_post_b && d_ln_g && d_ln_b && (d_feats_bf16 || d_feats_f32), "mq_owl_merge_ln: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(1, s);
    const int64_t rows = n * (T - 1);
    MQ_DISPATCH_CH(W, hipLaunchKernelGGL((owl_merge_ln_kernel<CH>), dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, d_x, d_post_g, d_post_b, d_ln_g,
                                         d_ln_b, (bf16_t*)d_feats_bf16, d_feats_f32, rows, T - 1, W, eps));
    MQ_CHECK_LAUNCH("mq_owl_merge_ln");
    return MQ_OK;
}

extern "C" int mq_owl_class_head(const float* d_embeds, const float* d_feats, const float* d_queries, const int32_t* d_query_mask, int32_t per_image,
                                 const float* d_shift_w, float shift_b, const float* d_scale_w, float scale_b, float* d_scores, float* d_logits,
                                 int32_t* d_labels, int64_t n, int32_t P, int32_t W, int32_t Dq, int32_t Q, void* stream) {
    MQ_CHECK_ARG(W >= 1 && Dq >= 1 && P >= 1 && P <= OWL_MAX_P, "mq_owl_class_head: bad shape P=%d W=%d Dq=%d", P, W, Dq);
    MQ_CHECK_ARG(Q >= 1 && Q <= OWL_MAX_Q, "mq_owl_class_head: Q=%d must be in [1, %d]", Q, OWL_MAX_Q);
    MQ_CHECK_ARG(n >= 0 && n * (int64_t)P < (1ll << 31) * 4, "mq_owl_class_head: n=%lld too large", (long long)n);
    if (n == 0) return MQ_OK;
    MQ_CHECK_ARG(d_embeds && d_feats && d_queries && d_shift_w && d_scale_w && d_scores && d_logits && d_labels, "mq_owl_class_head: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(4, s);
    const int64_t rows = n * P;
    hipLaunchKernelGGL(owl_class_head_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, d_embeds, d_feats, d_queries, d_query_mask,
                       (int64_t)(per_image ? Q : 0), d_shift_w, shift_b, d_scale_w, scale_b, d_scores, d_logits, d_labels, rows, P, W, Dq, Q);
    MQ_CHECK_LAUNCH("mq_owl_class_head");
    return MQ_OK;
}

extern "C" int mq_owl_box_head(const void* d_hidden, const float* d_w2, const float* d_b2, const float* d_box_bias, float* d_boxes, int64_t n,
                               int32_t P, int32_t W, float target_w, float target_h, void* stream) {
    MQ_CHECK_ARG(W >= 1 && P >= 1 && P <= OWL_MAX_P, "mq_owl_box_head: bad shape P=%d W=%d", P, W);
    MQ_CHECK_ARG(n >= 0 && n * (int64_t)P < (1ll << 31) * 4, "mq_owl_box_head: n=%lld too large", (long long)n);
    if (n == 0) return MQ_OK;
    MQ_CHECK_ARG(d_hidden && d_w2 && d_b2 && d_box_bias && d_boxes, "mq_owl_box_head: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(4, s);
    const int64_t rows = n * P;
    hipLaunchKernelGGL(owl_box_head_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, (const bf16_t*)d_hidden, d_w2, d_b2, d_box_bias, d_boxes, rows, P,
                       W, target_w, target_h);
    MQ_CHECK_LAUNCH("mq_owl_box_head");
    return MQ_OK;
}

extern "C" int mq_owl_topk(const float* d_scores, const float* d_boxes, int64_t n, int32_t P, int32_t k, float* d_top_scores, float* d_top_boxes,
                           int32_t* d_top_patch, void* stream) {
    MQ_CHECK_ARG(P >= 1 && P <= OWL_MAX_P, "mq_owl_topk: P=%d must be in [1, %d]", P, OWL_MAX_P);
    MQ_CHECK_ARG(k >= 1 && k <= P, "mq_owl_topk: k=%d must be in [1, P=%d] (the caller clamps)", k, P);
    MQ_CHECK_ARG(n >= 0 && n < (1ll << 31), "mq_owl_topk: n=%lld too large", (long long)n);
    if (n == 0) return MQ_OK;
    MQ_CHECK_ARG(d_scores && d_boxes && d_top_scores && d_top_boxes && d_top_patch, "mq_owl_topk: null pointer");
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(4, s);
    hipLaunchKernelGGL(owl_topk_kernel, dim3((unsigned)n), dim3(256), 0, s, d_scores, d_boxes, P, k, d_top_scores, d_top_boxes, d_top_patch);
    MQ_CHECK_LAUNCH("mq_owl_topk");
    return MQ_OK;
}
