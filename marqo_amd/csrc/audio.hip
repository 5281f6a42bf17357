// LanguageBind audio part: the front end in front of its CLIP ViT (reference: s2_inference/languagebind/audio/processing_audio.py — Kaldi fbank
// through torchaudio.compliance.kaldi.fbank, the three-crop "fusion", the (x - mean) / (2 std) normalisation) and the im2col rows of a
// NON-SQUARE picture (modeling_audio.py:767-811: image_size = [num_mel_bins, target_length]).
//   * fbank:         16 kHz waveform -> log-mel rows [m, bins]: 400-sample frames every 160, frame mean removed, pre-emphasis 0.97, symmetric Hann
//                    window, 512-point FFT, power spectrum of bins 0..255, triangular filters linear in mel(f) = 1127 ln(1 + f / 700) between 20 Hz
//                    and 8 kHz, log(max(e, FLT_EPSILON)).  One 256-thread workgroup per frame; the FFT is radix 2 in LDS, one butterfly per thread
//                    and stage.  A spectral bin feeds at most two filters (the falling side of one, the rising side of the next): the filterbank is
//                    a sparse accumulation.  ARITHMETIC: fp32 in, fp32 out, fp64 in between (window, twiddles, filter weights, the FFT, the sums).
//                    A narrow low filter of a 112-bin bank can hold a tiny share of the frame's energy, and an fp32 FFT's rounding is relative to
//                    the whole frame: it is the largest term of an fp32 evaluation's error on the log (tests/test_audio_gpu.py prints it).  512
//                    points per frame are microseconds in either precision, so the kernel does not carry that term: what is left is the rounding
//                    of the stored value.
//                    The mean of the whole waveform tensor (`audio_data -= audio_data.mean()`) is the first phase: per-block fp64 partial sums into
//                    the caller's workspace, summed in a fixed order by every frame's workgroup.
//   * mel_fusion:    the [3, bins, L] picture from the rows: row (start[c] + t) mod m, transposed through an LDS tile, normalised.
//   * patchify_rect: mq_patchify's fp32 kernel over an H x Wd picture.
//   * resample:      torchaudio.functional.resample at its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) as a polyphase
//                    filter: with o = orig / gcd and n = new / gcd, output f n + p is the dot product of row p of the host's tap table
//                    [n, K = 2 width + o] with the K samples of the zero-padded waveform from f o on.  A block stages the window of RS_OUT_PER_BLOCK
//                    or so outputs (whole output frames of n phases) in LDS; a thread then owns one phase of one frame.  ARITHMETIC as the fbank:
//                    fp32 in and out, the taps and the sum fp64 (the table is the host's fp64 one, never rounded): what is left is the rounding
//                    of the stored value.
#include "common.h"
#include <float.h>

namespace {
constexpr int FB_FRAME = 400;      // 25 ms at 16 kHz
constexpr int FB_SHIFT = 160;      // 10 ms
constexpr int FB_FFT = 512;        // round_to_power_of_two
constexpr int FB_MAX_BINS = 128;
constexpr int FB_MAX_PARTS = MQ_FBANK_WS_BYTES / 8;     // fp64 partial sums of the waveform in the workspace
constexpr int RS_OUT_PER_BLOCK = 512;                  // outputs a block aims at (whole frames of n phases)
constexpr int RS_MAX_WINDOW = 12288;                    // floats of LDS a block's window may take (48 KB)
constexpr int64_t RS_MAX_TAPS = MQ_RESAMPLE_MAX_TAPS;   // entries of the tap table
constexpr float FB_LOG_EPS = -15.9423847f;              // log(FLT_EPSILON) = -23 ln 2, rounded to nearest

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the 256 threads of a block, the same value in every thread (fixed order: butterfly per wave, then the four waves in order)
__device__ __forceinline__ double block_sum_f64(double v, double* sh4) {
    v = wave_sum_f64(v);
    __syncthreads();        // (sh4 may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

__global__ __launch_bounds__(256) void wave_partial_sums_kernel(const float* __restrict__ wave, int64_t n, double* __restrict__ parts) {
    __shared__ double sh4[4];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc += (double)wave[i];
    acc = block_sum_f64(acc, sh4);
    if (threadIdx.x == 0) parts[blockIdx.x] = acc;
}

// x_pad[j] = x[j - width], zero outside [0, len): block b owns output frames [b fpb, (b + 1) fpb), their window is x_pad[b fpb o, ... + (fpb - 1) o + K)
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ wave, int64_t len, const double* __restrict__ taps, int o, int n, int width,
                                                       int K, int fpb, int64_t out_len, float* __restrict__ out) {
    extern __shared__ float rs_win[];
    const float* x = wave + (int64_t)blockIdx.y * len;
    float* y = out + (int64_t)blockIdx.y * out_len;
    const int64_t f0 = (int64_t)blockIdx.x * fpb;
    const int64_t first = f0 * o - width;              // the waveform index of window slot 0
    const int span = (fpb - 1) * o + K;
    for (int i = threadIdx.x; i < span; i += 256) {
        const int64_t j = first + i;
        rs_win[i] = j >= 0 && j < len ? x[j] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < fpb * n; i += 256) {
        const int fl = i / n, p = i - fl * n;
        const int64_t oi = (f0 + fl) * n + p;
        if (oi >= out_len) continue;
        const double* tp = taps + (int64_t)p * K;
        const float* w = rs_win + fl * o;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc = fma(tp[k], (double)w[k], acc);
        y[oi] = (float)acc;
    }
}

__global__ __launch_bounds__(256) void fbank_kernel(const float* __restrict__ wave, const double* __restrict__ parts, int nparts, int64_t n_mean,
                                                    float* __restrict__ mel, int bins) {
    __shared__ double sh4[4];
    __shared__ double xs[FB_FRAME];          // the frame, mean removed
    __shared__ double2 d[FB_FFT];            // the FFT, in place
    __shared__ double2 tw[FB_FFT / 2];       // exp(-2 pi i k / 512)
    __shared__ double pw[FB_FFT / 2], wup[FB_FFT / 2], wdn[FB_FFT / 2];
    __shared__ int fj[FB_FFT / 2];
    const int t = threadIdx.x;
    const int64_t f = blockIdx.x;

    // ---- constants of this thread's spectral bin ----
    {
        double sn, cs;
        sincospi((double)t / 256.0, &sn, &cs);
        tw[t] = make_double2(cs, -sn);
        // filter b rises from mel_low + b delta to mel_low + (b + 1) delta and falls to mel_low + (b + 2) delta: a bin at position p = j + frac
        // (in units of delta above mel_low) gives frac to filter j and 1 - frac to filter j - 1
        const double mel_low = 1127.0 * log(1.0 + 20.0 / 700.0), mel_high = 1127.0 * log(1.0 + 8000.0 / 700.0);
        const double p = (1127.0 * log(1.0 + (double)t * (16000.0 / FB_FFT) / 700.0) - mel_low) * (double)(bins + 1) / (mel_high - mel_low);
        const double j = floor(p);
        fj[t] = (int)j;
        wup[t] = p - j;
        wdn[t] = 1.0 - (p - j);
    }
    // ---- the mean of the whole waveform tensor ----
    const double gmean = block_sum_f64(t < nparts ? parts[t] : 0.0, sh4) / (double)n_mean;

    // ---- the frame: whole-tensor mean, frame mean, pre-emphasis, window ----
    const float* src = wave + f * FB_SHIFT;
    const int i1 = t + 256;
    const double x0 = (double)src[t] - gmean;
    const double x1 = i1 < FB_FRAME ? (double)src[i1] - gmean : 0.0;
    const double fmean = block_sum_f64(x0 + x1, sh4) / (double)FB_FRAME;
    xs[t] = x0 - fmean;
    if (i1 < FB_FRAME) xs[i1] = x1 - fmean;
    d[t] = make_double2(0.0, 0.0);
    d[i1] = make_double2(0.0, 0.0);
    __syncthreads();
    d[__brev((unsigned)t) >> 23].x = (xs[t] - 0.97 * xs[t > 0 ? t - 1 : 0]) * (0.5 - 0.5 * cospi(2.0 * (double)t / (double)(FB_FRAME - 1)));
    if (i1 < FB_FRAME) d[__brev((unsigned)i1) >> 23].x = (xs[i1] - 0.97 * xs[i1 - 1]) * (0.5 - 0.5 * cospi(2.0 * (double)i1 / (double)(FB_FRAME - 1)));
    __syncthreads();
    // ---- 512-point FFT, radix 2, decimation in time: thread t owns butterfly t of every stage ----
#pragma unroll
    for (int s = 0; s < 9; ++s) {
        const int half = 1 << s;
        const int pos = t & (half - 1);
        const int a = ((t >> s) << (s + 1)) + pos, b = a + half;
        const double2 w = tw[pos << (8 - s)];
        const double2 u = d[a], v = d[b];
        const double2 vw = make_double2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
        d[a] = make_double2(u.x + vw.x, u.y + vw.y);
        d[b] = make_double2(u.x - vw.x, u.y - vw.y);
        __syncthreads();
    }
    pw[t] = d[t].x * d[t].x + d[t].y * d[t].y;
    __syncthreads();
    // ---- the filterbank: thread b sums its filter's bins in ascending order ----
    if (t < bins) {
        double e = 0.0;
        for (int k = 0; k < FB_FFT / 2; ++k) {
            const int j = fj[k];
            if (j == t) e = fma(wup[k], pw[k], e);
            else if (j == t + 1) e = fma(wdn[k], pw[k], e);
        }
        mel[f * bins + t] = e <= (double)FLT_EPSILON ? FB_LOG_EPS : (float)log(e);     // (a NaN goes through log)
    }
}

// 32 frames x 32 filters per block through an LDS tile: reads run along the filters of a mel row, writes along the frames of a picture row
__global__ __launch_bounds__(256) void mel_fusion_kernel(const float* __restrict__ mel, int64_t m, int bins, int64_t s0, int64_t s1, int64_t s2, float mean,
                                                         float two_std, float* __restrict__ px, int L) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = blockIdx.z;
    const int64_t start = c == 0 ? s0 : c == 1 ? s1 : s2;
    const int t0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tt = t0 + ty + 8 * j, ff = f0 + tx;
        if (tt < L && ff < bins) tile[ty + 8 * j][tx] = mel[((start + tt) % m) * bins + ff];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ff = f0 + ty + 8 * j, tt = t0 + tx;
        if (tt < L && ff < bins) px[((int64_t)c * bins + ff) * L + tt] = (tile[tx][ty + 8 * j] - mean) / two_std;
    }
}

// mq_patchify's fp32 kernel over an H x Wd picture: Gw patches per patch row, pixel (c, y, x) of picture i at ((i 3 + c) H + y) Wd + x.
// One thread produces 8 consecutive output columns (one 16-byte store).
__global__ __launch_bounds__(256) void patchify_rect_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t total_groups, int H, int Wd,
                                                            int P, int Gh, int Gw, int Kp) {
    const int groups_per_row = Kp >> 3;
    const int PP = P * P;
    for (int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x; gi < total_groups; gi += (int64_t)gridDim.x * 256) {
        const int64_t prow = gi / groups_per_row;
        const int col0 = (int)(gi - prow * groups_per_row) * 8;
        const int64_t img = prow / (Gh * Gw);
        const int pidx = (int)(prow - img * (Gh * Gw));
        const int py = pidx / Gw, px = pidx - py * Gw;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = col0 + e;
            float val = 0.f;
            if (col < 3 * PP) {
                const int c = col / PP;
                const int rem = col - c * PP;
                const int ky = rem / P, kx = rem - ky * P;
                val = in[((img * 3 + c) * H + (py * P + ky)) * (int64_t)Wd + (px * P + kx)];
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
}  // namespace

// ---- host entry points (C ABI, include/marqo_hip.h) -----------------------------------------------------------
extern "C" int mq_fbank(const float* d_wave, int64_t n, int64_t n_mean, int32_t sample_rate, int32_t bins, float* d_mel, void* d_ws, void* stream) {
    MQ_CHECK_ARG(sample_rate == 16000, "mq_fbank: sample_rate=%d is not served (16000 only: 400-sample frames every 160, 512-point FFT)", sample_rate);
    MQ_CHECK_ARG(bins >= 1 && bins <= FB_MAX_BINS, "mq_fbank: bins=%d must be in [1, %d]", bins, FB_MAX_BINS);
    MQ_CHECK_ARG(n >= FB_FRAME, "mq_fbank: n=%lld samples give no frame (at least %d)", (long long)n, FB_FRAME);
    MQ_CHECK_ARG(n < (1ll << 36) && n_mean >= n && n_mean < (1ll << 40), "mq_fbank: n=%lld, n_mean=%lld: n_mean must be at least n, and both below 2^36 / 2^40",
                 (long long)n, (long long)n_mean);
    MQ_CHECK_ARG(d_wave && d_mel && d_ws, "mq_fbank: null pointer");
    MQ_CHECK_ARG(((uintptr_t)d_ws & 7) == 0, "mq_fbank: the workspace must be 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(5, s);
    const int64_t m = 1 + (n - FB_FRAME) / FB_SHIFT;
    const int64_t want = cdiv64(n_mean, 256 * 16);
    const int nparts = (int)(want < FB_MAX_PARTS ? want : FB_MAX_PARTS);
    hipLaunchKernelGGL(wave_partial_sums_kernel, dim3(nparts), dim3(256), 0, s, d_wave, n_mean, (double*)d_ws);
    hipLaunchKernelGGL(fbank_kernel, dim3((unsigned)m), dim3(256), 0, s, d_wave, (const double*)d_ws, nparts, n_mean, d_mel, bins);
    MQ_CHECK_LAUNCH("mq_fbank");
    return MQ_OK;
}

extern "C" int mq_mel_fusion(const float* d_mel, int64_t m, int32_t bins, int64_t start0, int64_t start1, int64_t start2, float mean, float std,
                             float* d_px, int32_t L, void* stream) {
    MQ_CHECK_ARG(bins >= 1 && bins <= FB_MAX_BINS, "mq_mel_fusion: bins=%d must be in [1, %d]", bins, FB_MAX_BINS);
    MQ_CHECK_ARG(m >= 1 && m < (1ll << 31), "mq_mel_fusion: m=%lld rows must be in [1, 2^31)", (long long)m);
    MQ_CHECK_ARG(L >= 1 && L <= (1 << 20), "mq_mel_fusion: L=%d must be in [1, 2^20]", L);
    MQ_CHECK_ARG(std > 0.f && std == std && mean == mean, "mq_mel_fusion: mean=%g, std=%g: std must be positive", (double)mean, (double)std);
    const int64_t starts[3] = {start0, start1, start2};
    for (int c = 0; c < 3; ++c)
        MQ_CHECK_ARG(starts[c] >= 0 && starts[c] < m, "mq_mel_fusion: start[%d]=%lld must be in [0, m=%lld)", c, (long long)starts[c], (long long)m);
    MQ_CHECK_ARG(d_mel && d_px, "mq_mel_fusion: null pointer");
    const hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(5, s);
    hipLaunchKernelGGL(mel_fusion_kernel, dim3((unsigned)cdiv64(L, 32), (unsigned)cdiv64(bins, 32), 3), dim3(256), 0, s, d_mel, m, bins, starts[0],
                       starts[1], starts[2], mean, std * 2.0f, d_px, L);
    MQ_CHECK_LAUNCH("mq_mel_fusion");
    return MQ_OK;
}

extern "C" int mq_patchify_rect(const float* d_in, void* d_out, int64_t n, int32_t H, int32_t Wd, int32_t P, int32_t Kp, void* stream) {
    MQ_CHECK_ARG(P >= 1 && P <= 256 && H >= P && Wd >= P && H <= (1 << 16) && Wd <= (1 << 16), "mq_patchify_rect: bad shape H=%d Wd=%d P=%d", H, Wd, P);
    MQ_CHECK_ARG(H % P == 0 && Wd % P == 0, "mq_patchify_rect: H=%d and Wd=%d must be multiples of P=%d", H, Wd, P);
    MQ_CHECK_ARG(Kp % 8 == 0 && Kp >= 3 * P * P, "mq_patchify_rect: Kp=%d must be a multiple of 8 and at least 3 P^2 = %d", Kp, 3 * P * P);
    MQ_CHECK_ARG(n >= 0 && n < (1ll << 31) / ((int64_t)(H / P) * (Wd / P)), "mq_patchify_rect: n=%lld too large", (long long)n);
    const hipStream_t s = (hipStream_t)stream;
    const int Gh = H / P, Gw = Wd / P;
    const int64_t total = n * Gh * Gw * (Kp >> 3);
    if (total <= 0) return MQ_OK;
    MQ_CHECK_ARG(d_in && d_out, "mq_patchify_rect: null pointer");
    MQ_CHECK_ARG(((uintptr_t)d_out & 15) == 0, "mq_patchify_rect: the output must be 16-byte aligned");
    MqProfScope prof(5, s);
    const unsigned grid = (unsigned)(cdiv64(total, 256) < 16384 ? cdiv64(total, 256) : 16384);
    hipLaunchKernelGGL(patchify_rect_kernel, dim3(grid), dim3(256), 0, s, d_in, (bf16_t*)d_out, total, H, Wd, P, Gh, Gw, Kp);
    MQ_CHECK_LAUNCH("mq_patchify_rect");
    return MQ_OK;
}

static int64_t rs_gcd(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

extern "C" int mq_resample(const float* d_wave, int64_t channels, int64_t len, const double* d_taps, int32_t o, int32_t n, int32_t width, float* d_out,
                           void* stream) {
    MQ_CHECK_ARG(o >= 1 && n >= 1 && width >= 1 && rs_gcd(o, n) == 1, "mq_resample: o=%d, n=%d, width=%d: the reduced rate pair (coprime, positive) and a positive width",
                 o, n, width);
    MQ_CHECK_ARG(o != n, "mq_resample: o == n == %d: nothing to resample", o);
    const int64_t K = 2ll * width + o;
    MQ_CHECK_ARG(K <= RS_MAX_WINDOW && (int64_t)n * K <= RS_MAX_TAPS,
                 "mq_resample: o=%d, n=%d, width=%d: a table of n (2 width + o) = %lld taps (at most %lld) with rows of %lld (at most %d) is not served: "
                 "the two rates share too small a divisor", o, n, width, (long long)((int64_t)n * K), (long long)RS_MAX_TAPS, (long long)K, RS_MAX_WINDOW);
    MQ_CHECK_ARG(channels >= 1 && channels <= 65535 && len >= 1 && len < (1ll << 36), "mq_resample: channels=%lld, len=%lld: 1 to 65535 channels of 1 to 2^36 - 1 samples",
                 (long long)channels, (long long)len);
    MQ_CHECK_ARG(d_wave && d_taps && d_out, "mq_resample: null pointer");
    MQ_CHECK_ARG(((uintptr_t)d_taps & 7) == 0, "mq_resample: the tap table must be 8-byte aligned");
    const int64_t out_len = ((int64_t)n * len + o - 1) / o;
    const int64_t frames = cdiv64(out_len, n);
    int64_t fpb = cdiv64(RS_OUT_PER_BLOCK, n);
    const int64_t fit = (RS_MAX_WINDOW - K) / o + 1;           // frames whose window fits the LDS budget
    fpb = fpb < fit ? fpb : fit;
    fpb = fpb < frames ? fpb : frames;
    const int64_t blocks = cdiv64(frames, fpb);
    MQ_CHECK_ARG(blocks < (1ll << 31), "mq_resample: len=%lld gives %lld blocks (below 2^31)", (long long)len, (long long)blocks);
    const hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(5, s);
    const size_t lds = (size_t)((fpb - 1) * o + K) * sizeof(float);
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks, (unsigned)channels), dim3(256), lds, s, d_wave, len, d_taps, o, n, width, (int)K, (int)fpb,
                       out_len, d_out);
    MQ_CHECK_LAUNCH("mq_resample");
    return MQ_OK;
}
