// LanguageBind video part: the front end in front of its tower (reference: s2_inference/languagebind/video/processing_video.py:20-93 — the frame
// pick, x / 255, NormalizeVideo, pytorchvideo's ShortSideScale, torchvision's CenterCropVideo, the horizontal flip) as ONE pass over the output:
//   * video_preprocess: decoded frames uint8 [T_in, H, W, 3] -> fp32 [3, T, S, S], one clip of the `b c t h w` tensor mq_patchify_clip reads.  One
//                       thread per output pixel (t, y, x) and all three channels: the four taps of
//                       torch.nn.functional.interpolate(mode="bilinear", align_corners=False) at the scaled frame's pixel (top + y, left + x'),
//                       x' = S - 1 - x under the flip, each tap normalised first ((u8 / 255 - mean) / std, both divisions IEEE: the reference
//                       normalises, then scales), blended rows first, then columns.  The scaled new_h x new_w frame is never stored.  The integers
//                       (which frames, new_h, new_w, top, left) are the host's (engine/video.py).  ARITHMETIC: the source coordinate and its
//                       fraction are fp64 (one per thread and axis), the taps and the blend fp32; with new == in the fractions are exactly 0 and the
//                       output IS the normalised input.
#include "common.h"

namespace {
constexpr int VP_MAX_SIDE = 16384;     // H, W, new_h, new_w: 3 H W and every product of two of them stay far below 2^31
constexpr int VP_MAX_S = 4096;
constexpr int VP_MAX_T = 4096;

struct VpNorm {
    float mean[3], std[3];
};

// PyTorch's area_pixel_compute_source_index (align_corners = False): the source coordinate, clamped at 0, its floor and the upper neighbour clamped
// at in - 1
__device__ __forceinline__ void vp_taps(int dst, double scale, int in, int& i0, int& i1, float& w1) {
    double src = ((double)dst + 0.5) * scale - 0.5;
    src = src < 0.0 ? 0.0 : src;
    int lo = (int)src;
    lo = lo < in - 1 ? lo : in - 1;
    i0 = lo;
    i1 = lo < in - 1 ? lo + 1 : lo;
    w1 = (float)(src - (double)lo);
}

__global__ __launch_bounds__(256) void video_preprocess_kernel(const uint8_t* __restrict__ frames, int64_t T_in, int H, int W, const int32_t* __restrict__ pick,
                                                               int T, int S, int new_h, int new_w, int top, int left, VpNorm nm, int flip,
                                                               float* __restrict__ out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int t = blockIdx.z;
    if (x >= S || y >= S) return;
    int64_t fi = pick[t];
    fi = fi < 0 ? 0 : (fi >= T_in ? T_in - 1 : fi);        // (a pick outside the clip is the caller's error: no read leaves the buffer)
    int y0, y1, x0, x1;
    float wy1, wx1;
    vp_taps(top + y, (double)H / (double)new_h, H, y0, y1, wy1);
    vp_taps(left + (flip ? S - 1 - x : x), (double)W / (double)new_w, W, x0, x1, wx1);
    const float wy0 = 1.0f - wy1, wx0 = 1.0f - wx1;
    const uint8_t* f = frames + fi * ((int64_t)H * W * 3);
    const uint8_t* p00 = f + ((int64_t)y0 * W + x0) * 3;
    const uint8_t* p01 = f + ((int64_t)y0 * W + x1) * 3;
    const uint8_t* p10 = f + ((int64_t)y1 * W + x0) * 3;
    const uint8_t* p11 = f + ((int64_t)y1 * W + x1) * 3;
    const int64_t plane = (int64_t)T * S * S;
    float* o = out + ((int64_t)t * S + y) * S + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float m = nm.mean[c], s = nm.std[c];
        const float v00 = ((float)p00[c] / 255.0f - m) / s, v01 = ((float)p01[c] / 255.0f - m) / s;
        const float v10 = ((float)p10[c] / 255.0f - m) / s, v11 = ((float)p11[c] / 255.0f - m) / s;
        o[c * plane] = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11);
    }
}
}  // namespace

// ---- host entry point (C ABI, include/marqo_hip.h) ------------------------------------------------------------
extern "C" int mq_video_preprocess(const uint8_t* d_frames, int64_t T_in, int32_t H, int32_t W, const int32_t* d_pick, int32_t T, int32_t S,
                                   int32_t new_h, int32_t new_w, int32_t top, int32_t left, const float* h_mean, const float* h_std, int32_t flip,
                                   float* d_out, void* stream) {
    MQ_CHECK_ARG(H >= 1 && W >= 1 && H <= VP_MAX_SIDE && W <= VP_MAX_SIDE, "mq_video_preprocess: frames of H=%d x W=%d: both sides must be in [1, %d]", H, W,
                 VP_MAX_SIDE);
    MQ_CHECK_ARG(T_in >= 1 && T_in < (1ll << 31), "mq_video_preprocess: T_in=%lld frames must be in [1, 2^31)", (long long)T_in);
    MQ_CHECK_ARG(T >= 1 && T <= VP_MAX_T, "mq_video_preprocess: T=%d picked frames must be in [1, %d]", T, VP_MAX_T);
    MQ_CHECK_ARG(S >= 1 && S <= VP_MAX_S, "mq_video_preprocess: S=%d must be in [1, %d]", S, VP_MAX_S);
    MQ_CHECK_ARG(new_h >= S && new_w >= S && new_h <= VP_MAX_SIDE && new_w <= VP_MAX_SIDE,
                 "mq_video_preprocess: the scaled frame new_h=%d x new_w=%d must hold the S=%d window and stay within %d a side", new_h, new_w, S, VP_MAX_SIDE);
    MQ_CHECK_ARG(top >= 0 && top <= new_h - S && left >= 0 && left <= new_w - S,
                 "mq_video_preprocess: the window at top=%d, left=%d leaves the %d x %d scaled frame (S=%d)", top, left, new_h, new_w, S);
    MQ_CHECK_ARG(flip == 0 || flip == 1, "mq_video_preprocess: flip=%d must be 0 or 1", flip);
    MQ_CHECK_ARG(d_frames && d_pick && d_out && h_mean && h_std, "mq_video_preprocess: null pointer");
    VpNorm nm;
    for (int c = 0; c < 3; ++c) {
        MQ_CHECK_ARG(h_std[c] > 0.f && h_std[c] == h_std[c] && h_mean[c] == h_mean[c], "mq_video_preprocess: mean[%d]=%g, std[%d]=%g: std must be positive", c,
                     (double)h_mean[c], c, (double)h_std[c]);
        nm.mean[c] = h_mean[c];
        nm.std[c] = h_std[c];
    }
    MQ_CHECK_ARG(((uintptr_t)d_pick & 3) == 0 && ((uintptr_t)d_out & 3) == 0, "mq_video_preprocess: d_pick and d_out must be 4-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(5, s);
    hipLaunchKernelGGL(video_preprocess_kernel, dim3((unsigned)cdiv64(S, 64), (unsigned)cdiv64(S, 4), (unsigned)T), dim3(256), 0, s, d_frames, T_in, H, W,
                       d_pick, T, S, new_h, new_w, top, left, nm, flip, d_out);
    MQ_CHECK_LAUNCH("mq_video_preprocess");
    return MQ_OK;
}
