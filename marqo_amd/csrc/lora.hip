// Per-sequence low-rank (LoRA) corrections of a Linear, the task adapters of jina-embeddings-v3: a row of sequence s with task t = task[s] gets
//
//   y += scale_t (x A_t^T) B_t^T                      A_t [R, K], B_t [N, r], r <= 16, R = r (one Linear) or 3 r (q | k | v stacked on one input)
//
// on top of the base GEMM, which runs once for all rows whatever their tasks.  task[s] < 0: no adapter — such a row's delta is not computed at all (its
// bits in an accumulate / in-place target stay what they were), it is not merely small.  One batch may mix tasks: the task is looked up PER ROW (a binary
// search of the row in cu_seqlens, or row / fixed_len), never per workgroup.
//
//   mq_lora_down    T[m, :] = scale_t (x[m, :] A_t^T), fp32 [rows, R], one read pass over x.  One wave64 per 32 rows (two 16-row MFMA tiles, four waves
//                   = 128 rows per workgroup), v_mfma_f32_16x16x32_bf16 with the operands swapped (adapter rows as A-operand, x rows as B-operand) so that a
//                   lane's four results belong to ONE x row (lane & 15): the per-row task is a per-lane value and a tile whose rows have different tasks
//                   runs the k-loop once per task PRESENT in the wave's rows (a wave-uniform vote) and every lane keeps the product of its own row's
//                   task.  x and A fragments come straight from global memory (16 B per lane; A_t is at most 128 KiB and stays in L2); no LDS.  Rows
//                   with no adapter get T = 0.
//   mq_lora_up      delta[m, n] = sum_j T[m, off(n) + j] B_t[n, j], off(n) = (n / (N / nblocks)) r: column block b of a stacked q | k | v reads its own r
//                   columns of T.  fp32 FMAs in the order j = 0 .. r - 1, a thread owns 4 consecutive columns of one row, a wave walks a row.  Modes:
//                   MQ_LORA_ACCUM out_f32 += delta ; MQ_LORA_WRITE out_f32 = delta (0 for rows without adapter) ; MQ_LORA_INPLACE out_bf16 = act(out_bf16 +
//                   delta), act none or the erf GELU of MQ_EPI_GELU (gelu_erf4) — rows without adapter: untouched (act none) or act(out) (GELU).
//   mq_lora_gather  T[m, :] = scale_t A_emb_t[id[m], :]: the down half of an embedding adapter (the table is stored transposed, [vocab, r] per task); its
//                   up half is mq_lora_up in MQ_LORA_ACCUM on the un-normalised embedding rows.
//
// Bounds (read before running).  down: a wave whose first row is past `rows` returns (no barrier in the kernel); x rows are clamped to rows - 1 and read
// columns 8 g + k .. + 7 < K <= lda; adapter rows past R are clamped to row 0 (their results are never stored); tasks read from memory are used only when
// 0 <= t < tasks; T is written at m < rows, n + 4 <= R (R % 4 == 0).  up: m < rows, n = 4 q + 3 < N (N % 4 == 0), T read at off + j + 3 < nblocks r = R,
// B at (n + e) r + j + 3 < N r.  gather: id clamped to [0, vocab).  The sequence index of a row is clamped to [0, nseq).
//
// Compiler report (gfx950, -O3, resource remarks), 256 threads per workgroup:
//   lora_down_kernel<1> / <2> / <3> / <4> (16-wide tiles of R):  44 + 8 / 58 + 16 / 84 + 24 / 94 + 32 VGPRs + AGPRs, 44 - 48 SGPRs, 8 / 6 / 4 / 4 waves
//                                                                per SIMD by registers
//   lora_up_kernel<mode, act> (accumulate, write, in place, in place + GELU):  68 / 68 / 68 / 70 VGPRs, 56 - 68 SGPRs, 7 waves per SIMD
//   lora_gather_kernel:                                          15 VGPRs, 36 SGPRs
// No VGPR / SGPR spill, no scratch and no LDS in any of them.  Not measured: throughput (the kernels were written for the memory-bound regime rows >> R; no timing was taken).
#include "common.h"

namespace {

constexpr int LD_NW = 4;                        // wave64s per workgroup
constexpr int LD_MT = 2;                        // 16-row tiles per wave
constexpr int LD_ROWS = LD_NW * LD_MT * 16;     // rows per workgroup of the down kernel
constexpr int UP_ROWS = 8;                      // rows per workgroup of the up kernel (a wave walks rows wave, wave + 4)

// task of packed row `row`: -1 for rows past the batch, sequences without adapter and ids outside [0, tasks)
__device__ __forceinline__ int lora_task_of(const int32_t* __restrict__ cu, const int32_t* __restrict__ seq_task, int nseq, int fixed_len, int tasks,
                                            int64_t row, int64_t rows) {
    if (row >= rows) return -1;
    int s;
    if (fixed_len > 0) {
        s = (int)(row / fixed_len);
        s = s < nseq ? s : nseq - 1;
    } else {
        int lo = 0, hi = nseq - 1;      // the last s with cu[s] <= row (empty sequences in front of it are skipped); cu[0] == 0 <= row
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((int64_t)cu[mid] <= row) lo = mid;
            else hi = mid - 1;
        }
        s = lo;
    }
    const int t = seq_task[s];
    return (t >= 0 && t < tasks) ? t : -1;
}

template <int NT>
__global__ __launch_bounds__(LD_NW * 64) void lora_down_kernel(const bf16_t* __restrict__ x, int64_t lda, const bf16_t* __restrict__ A,
                                                              const float* __restrict__ scale, const int32_t* __restrict__ seq_task,
                                                              const int32_t* __restrict__ cu, int nseq, int fixed_len, int tasks, int R, int K,
                                                              float* __restrict__ T, int64_t rows) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int64_t m0 = ((int64_t)blockIdx.x * LD_NW + wave) * (LD_MT * 16);
    if (m0 >= rows) return;
    int task[LD_MT];
    const bf16_t* xr[LD_MT];
    f32x4 out[LD_MT][NT];
#pragma unroll
    for (int mt = 0; mt < LD_MT; ++mt) {
        const int64_t m = m0 + mt * 16 + l15;       // this lane's x row of tile mt (B-operand column / output row)
        task[mt] = lora_task_of(cu, seq_task, nseq, fixed_len, tasks, m, rows);
        xr[mt] = x + (m < rows ? m : rows - 1) * lda + 8 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) out[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int t = 0; t < tasks; ++t) {
        bool mine = false;
#pragma unroll
        for (int mt = 0; mt < LD_MT; ++mt) mine |= task[mt] == t;
        if (!__any(mine)) continue;     // (wave-uniform: no row of this wave runs task t)
        const bf16_t* ar[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int r = nt * 16 + l15;            // this lane's adapter row (A-operand row); past R: row 0, never stored
            ar[nt] = A + ((int64_t)t * R + (r < R ? r : 0)) * K + 8 * g;
        }
        f32x4 acc[LD_MT][NT];
#pragma unroll
        for (int mt = 0; mt < LD_MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < K; k += 32) {
            bf16x8 xf[LD_MT];
#pragma unroll
            for (int mt = 0; mt < LD_MT; ++mt) xf[mt] = *(const bf16x8*)(xr[mt] + k);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const bf16x8 af = *(const bf16x8*)(ar[nt] + k);
#pragma unroll
                for (int mt = 0; mt < LD_MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf[mt], acc[mt][nt], 0, 0, 0);
            }
        }
        const float sc = scale[t];
#pragma unroll
        for (int mt = 0; mt < LD_MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                if (task[mt] == t) out[mt][nt] = acc[mt][nt] * sc;
    }
#pragma unroll
    for (int mt = 0; mt < LD_MT; ++mt) {
        const int64_t m = m0 + mt * 16 + l15;
        if (m >= rows) continue;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = nt * 16 + 4 * g;          // the lane's four adapter rows n .. n + 3 of row m
            if (n < R) *(f32x4*)(T + m * R + n) = out[mt][nt];
        }
    }
}

template <int MODE, int ACT>
__global__ __launch_bounds__(256) void lora_up_kernel(const float* __restrict__ T, int R, const bf16_t* __restrict__ B, int r, int block_cols,
                                                     const int32_t* __restrict__ seq_task, const int32_t* __restrict__ cu, int nseq, int fixed_len,
                                                     int tasks, void* out, int64_t ldc, int64_t rows, int N) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nq = N >> 2;
    const int64_t mb = (int64_t)blockIdx.x * UP_ROWS;
    for (int64_t m = mb + wave; m < mb + UP_ROWS && m < rows; m += 4) {
        const int t = lora_task_of(cu, seq_task, nseq, fixed_len, tasks, m, rows);      // (wave-uniform)
        if (t < 0 && (MODE == MQ_LORA_ACCUM || (MODE == MQ_LORA_INPLACE && ACT == 0))) continue;
        const float* Tr = T + m * R;
        const bf16_t* Bt = B + (int64_t)(t < 0 ? 0 : t) * N * r;
        for (int q = lane; q < nq; q += 64) {
            const int n = q << 2;
            f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
            if (t >= 0) {
                const float* Tb = Tr + (n / block_cols) * r;
                for (int j = 0; j < r; j += 4) {
                    const f32x4 tv = *(const f32x4*)(Tb + j);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint2 w = *(const uint2*)(Bt + (int64_t)(n + e) * r + j);
                        d[e] = fmaf(tv[0], __uint_as_float(w.x << 16), d[e]);
                        d[e] = fmaf(tv[1], __uint_as_float(w.x & 0xffff0000u), d[e]);
                        d[e] = fmaf(tv[2], __uint_as_float(w.y << 16), d[e]);
                        d[e] = fmaf(tv[3], __uint_as_float(w.y & 0xffff0000u), d[e]);
                    }
                }
            }
            if (MODE == MQ_LORA_ACCUM) {
                float* o = (float*)out + m * ldc + n;
                *(f32x4*)o = *(const f32x4*)o + d;
            } else if (MODE == MQ_LORA_WRITE) {
                *(f32x4*)((float*)out + m * ldc + n) = d;
            } else {
                bf16_t* o = (bf16_t*)out + m * ldc + n;
                const uint2 p = *(const uint2*)o;
                f32x4 v = f32x4{__uint_as_float(p.x << 16), __uint_as_float(p.x & 0xffff0000u), __uint_as_float(p.y << 16),
                                __uint_as_float(p.y & 0xffff0000u)};
                if (t >= 0) v += d;
                if (ACT) v = gelu_erf4(v);
                uint2 pk;
                pk.x = pack_bf16x2(v[0], v[1]);
                pk.y = pack_bf16x2(v[2], v[3]);
                *(uint2*)o = pk;
            }
        }
    }
}

__global__ __launch_bounds__(256) void lora_gather_kernel(const int32_t* __restrict__ ids, const float* __restrict__ A, const float* __restrict__ scale,
                                                         const int32_t* __restrict__ seq_task, const int32_t* __restrict__ cu, int nseq, int fixed_len,
                                                         int tasks, int r, int vocab, float* __restrict__ T, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one thread per (row, j)
    const int64_t m = i / r;
    if (m >= rows) return;
    const int j = (int)(i - m * r);
    const int t = lora_task_of(cu, seq_task, nseq, fixed_len, tasks, m, rows);
    float v = 0.f;
    if (t >= 0) {
        int id = ids[m];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        v = scale[t] * A[((int64_t)t * vocab + id) * r + j];
    }
    T[i] = v;
}

// what the three entry points check of their sequence arguments; *any = some sequence has an adapter
int lora_check_seqs(const char* what, const int32_t* d_seq_task, const int32_t* h_seq_task, const int32_t* d_cu, int64_t nseq, int32_t fixed_len,
                    int64_t rows, int32_t tasks, bool* any) {
    MQ_CHECK_ARG(d_seq_task && h_seq_task, "%s: null task list (device and host copies of int32 [nseq])", what);
    MQ_CHECK_ARG(tasks >= 1 && tasks <= 1024, "%s: tasks %d outside [1, 1024]", what, tasks);
    MQ_CHECK_ARG(nseq >= 0 && nseq <= (int64_t)1 << 30, "%s: nseq %lld outside [0, 2^30]", what, (long long)nseq);
    MQ_CHECK_ARG(rows >= 0 && rows <= (int64_t)1 << 30, "%s: rows %lld outside [0, 2^30]", what, (long long)rows);
    MQ_CHECK_ARG(fixed_len >= 0, "%s: fixed_len %d is negative", what, fixed_len);
    if (fixed_len > 0) MQ_CHECK_ARG(rows == nseq * fixed_len, "%s: rows %lld is not nseq %lld x fixed_len %d", what, (long long)rows, (long long)nseq, fixed_len);
    else MQ_CHECK_ARG(d_cu || nseq == 0, "%s: packed sequences need d_cu_seqlens", what);
    MQ_CHECK_ARG(nseq > 0 || rows == 0, "%s: rows %lld without a sequence", what, (long long)rows);
    *any = false;
    for (int64_t s = 0; s < nseq; ++s) {
        MQ_CHECK_ARG(h_seq_task[s] < tasks, "%s: task id %d of sequence %lld is not below tasks %d", what, h_seq_task[s], (long long)s, tasks);
        if (h_seq_task[s] >= 0) *any = true;
    }
    return MQ_OK;
}

template <int MODE, int ACT>
void launch_up(const float* T, int R, const void* B, int r, int block_cols, const int32_t* seq_task, const int32_t* cu, int64_t nseq, int fixed_len,
               int tasks, void* out, int64_t ldc, int64_t rows, int N, hipStream_t s) {
    hipLaunchKernelGGL((lora_up_kernel<MODE, ACT>), dim3((unsigned)cdiv64(rows, UP_ROWS)), dim3(256), 0, s, T, R, (const bf16_t*)B, r, block_cols, seq_task,
                       cu, (int)nseq, fixed_len, tasks, out, ldc, rows, N);
}

}  // namespace

extern "C" int mq_lora_down(const void* d_x, int64_t lda, const void* d_A, const float* d_scale, const int32_t* d_seq_task, const int32_t* h_seq_task,
                            const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int64_t rows, int32_t tasks, int32_t R, int32_t K, float* d_T,
                            void* stream) {
    MQ_CHECK_ARG(d_x && d_A && d_scale && d_T, "mq_lora_down: null pointer");
    MQ_CHECK_ARG(R >= 4 && R <= 64 && R % 4 == 0, "mq_lora_down: R %d must be a multiple of 4 in [4, 64]", R);
    MQ_CHECK_ARG(K >= 64 && K % 64 == 0 && K <= 1 << 20, "mq_lora_down: K %d must be a multiple of 64", K);
    MQ_CHECK_ARG(lda >= K && lda % 8 == 0, "mq_lora_down: lda %lld must be a multiple of 8, at least K %d", (long long)lda, K);
    bool any = false;
    MQ_TRY(lora_check_seqs("mq_lora_down", d_seq_task, h_seq_task, d_cu_seqlens, nseq, fixed_len, rows, tasks, &any));
    if (rows <= 0 || !any) return MQ_OK;      // (no sequence has an adapter: T is not written, and mq_lora_up reads none of it)
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(0, s);
    const dim3 grid((unsigned)cdiv64(rows, LD_ROWS)), block(LD_NW * 64);
#define MQ_LORA_DOWN(NT)                                                                                                                            \
    hipLaunchKernelGGL((lora_down_kernel<NT>), grid, block, 0, s, (const bf16_t*)d_x, lda, (const bf16_t*)d_A, d_scale, d_seq_task, d_cu_seqlens, \
                       (int)nseq, fixed_len, tasks, R, K, d_T, rows)
    switch ((R + 15) / 16) {
        case 1: MQ_LORA_DOWN(1); break;
        case 2: MQ_LORA_DOWN(2); break;
        case 3: MQ_LORA_DOWN(3); break;
        default: MQ_LORA_DOWN(4); break;
    }
#undef MQ_LORA_DOWN
    MQ_CHECK_LAUNCH("mq_lora_down");
    return MQ_OK;
}

extern "C" int mq_lora_up(const float* d_T, int32_t R, const void* d_B, int32_t r, int32_t nblocks, const int32_t* d_seq_task, const int32_t* h_seq_task,
                          const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int64_t rows, int32_t tasks, void* d_out, int64_t ldc, int32_t N,
                          int32_t mode, int32_t act, void* stream) {
    MQ_CHECK_ARG(d_T && d_B && d_out, "mq_lora_up: null pointer");
    MQ_CHECK_ARG(r >= 4 && r <= 16 && r % 4 == 0, "mq_lora_up: rank %d must be 4, 8, 12 or 16", r);
    MQ_CHECK_ARG(nblocks >= 1 && nblocks <= 16 && R == nblocks * r && R <= 64, "mq_lora_up: R %d is not nblocks %d x rank %d, at most 64", R, nblocks, r);
    MQ_CHECK_ARG(N >= 4 && N % 4 == 0 && N % nblocks == 0 && (N / nblocks) % 4 == 0 && N <= 1 << 24,
                 "mq_lora_up: N %d must be a multiple of 4 and of nblocks %d, each column block a multiple of 4", N, nblocks);
    MQ_CHECK_ARG(ldc >= N && ldc % 4 == 0, "mq_lora_up: ldc %lld must be a multiple of 4, at least N %d", (long long)ldc, N);
    MQ_CHECK_ARG(mode == MQ_LORA_ACCUM || mode == MQ_LORA_WRITE || mode == MQ_LORA_INPLACE, "mq_lora_up: bad mode %d", mode);
    MQ_CHECK_ARG(act == 0 || (act == MQ_ACT_GELU && mode == MQ_LORA_INPLACE), "mq_lora_up: act %d (0, or MQ_ACT_GELU with MQ_LORA_INPLACE)", act);
    bool any = false;
    MQ_TRY(lora_check_seqs("mq_lora_up", d_seq_task, h_seq_task, d_cu_seqlens, nseq, fixed_len, rows, tasks, &any));
    if (rows <= 0) return MQ_OK;
    if (!any && (mode == MQ_LORA_ACCUM || (mode == MQ_LORA_INPLACE && act == 0))) return MQ_OK;     // nothing to add anywhere
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(0, s);
    const int bc = N / nblocks;
    if (mode == MQ_LORA_ACCUM) launch_up<MQ_LORA_ACCUM, 0>(d_T, R, d_B, r, bc, d_seq_task, d_cu_seqlens, nseq, fixed_len, tasks, d_out, ldc, rows, N, s);
    else if (mode == MQ_LORA_WRITE) launch_up<MQ_LORA_WRITE, 0>(d_T, R, d_B, r, bc, d_seq_task, d_cu_seqlens, nseq, fixed_len, tasks, d_out, ldc, rows, N, s);
    else if (act == 0) launch_up<MQ_LORA_INPLACE, 0>(d_T, R, d_B, r, bc, d_seq_task, d_cu_seqlens, nseq, fixed_len, tasks, d_out, ldc, rows, N, s);
    else launch_up<MQ_LORA_INPLACE, 1>(d_T, R, d_B, r, bc, d_seq_task, d_cu_seqlens, nseq, fixed_len, tasks, d_out, ldc, rows, N, s);
    MQ_CHECK_LAUNCH("mq_lora_up");
    return MQ_OK;
}

extern "C" int mq_lora_gather(const int32_t* d_ids, const float* d_A_emb, const float* d_scale, const int32_t* d_seq_task, const int32_t* h_seq_task,
                              const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int64_t rows, int32_t tasks, int32_t r, int32_t vocab,
                              float* d_T, void* stream) {
    MQ_CHECK_ARG(d_ids && d_A_emb && d_scale && d_T, "mq_lora_gather: null pointer");
    MQ_CHECK_ARG(r >= 4 && r <= 16 && r % 4 == 0, "mq_lora_gather: rank %d must be 4, 8, 12 or 16", r);
    MQ_CHECK_ARG(vocab >= 1, "mq_lora_gather: vocab %d", vocab);
    bool any = false;
    MQ_TRY(lora_check_seqs("mq_lora_gather", d_seq_task, h_seq_task, d_cu_seqlens, nseq, fixed_len, rows, tasks, &any));
    if (rows <= 0 || !any) return MQ_OK;
    hipStream_t s = (hipStream_t)stream;
    MqProfScope prof(3, s);
    hipLaunchKernelGGL(lora_gather_kernel, dim3((unsigned)cdiv64(rows * r, 256)), dim3(256), 0, s, d_ids, d_A_emb, d_scale, d_seq_task, d_cu_seqlens, (int)nseq,
                       fixed_len, tasks, r, vocab, d_T, rows);
    MQ_CHECK_LAUNCH("mq_lora_gather");
    return MQ_OK;
}
