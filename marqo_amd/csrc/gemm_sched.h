// Host-side schedule of the persistent tiled GEMMs (gemm_bf16.hip, gemm_fp8.hip; gemm_wd.hip launches on the geometry gemm_bf16.hip makes): the tuning
// knobs, the resident slots, the tile-height cost model, the row chunks under the kernels' 32-bit buffer offsets and each launch's tile grid.
#pragma once
#include "common.h"
#include "knobs.h"

// tuning knobs: g_tune and mq_gemm_addr_limit (knobs.h; keys, environment names, defaults and values in knobs.hip's table).
// g_tune.tail: the big tile's in-kernel tail (GemmSk).  OFF by default: its rows carry a differently associated k-sum, so an embedding's bits would
// depend on whether its tokens sit in the last partial row tile of a batch — the towers promise the same bits wherever an item stands
// (tests/test_towers_gpu.py permutation equivariance; the coalescer and the ingest merging lean on it) — for +1.6 % / +3.9 % on the ViT-L/14 rows
// (profiles/r05p).  mq_tune("gemm_tail", 1) / MQ_GEMM_TAIL=1 turns it on; without it a ragged last row tile is a tile like any other.

// One launch's tile grid (the kernels' scheduling arguments)
struct GemmGeom {
    int tiles_n, tiles_m, num_tiles, cgroup, band_rows, grid;
    unsigned a_bytes, w_bytes;   // the operands' buffer-descriptor sizes
    // the grid of tiles_m row tiles on `slots` resident workgroups; L2 blocking only when there is something to block: more column tiles than one
    // group and at least two row panels per XCD
    void set_tiles_m(int tm, int slots) {
        tiles_m = tm;
        num_tiles = tiles_m * tiles_n;
        const int knob_cgroup = g_tune.cgroup;
        cgroup = (knob_cgroup > 0 && tiles_n > knob_cgroup && tiles_m >= 16) ? knob_cgroup : 0;
        band_rows = (tiles_m + 7) / 8;
        grid = num_tiles > slots ? slots : num_tiles;
    }
};

namespace {

constexpr int RESIDENT_SLOTS = 512;       // 256 CUs x 2 workgroups (the (32*MT) x 128 tiles)
constexpr int RESIDENT_SLOTS_WIDE = 256;  // 256 CUs x 1 workgroup (the big tiles)

// pick the tile height: minimise rounds x (MT + fixed per-tile overhead in 16-row units).  The tile HEIGHT is a free parameter because rows
// are guarded anyway; this removes most of the tile-quantisation loss at the towers' shapes (M = 12 800, N = 768: 600 128-row tiles = 2
// rounds on 512 slots, 480 160-row tiles = 1 round).
int choose_mt(int M, int N) {
    constexpr int BN = 128;
    const int tiles_n = (N + BN - 1) / BN;
    const int cands[4] = {2, 4, 5, 6};
    int best = 4;
    double best_cost = 1e30;
    for (int c = 0; c < 4; ++c) {
        const int mt = cands[c];
        const int bm = 32 * mt;
        const int64_t tiles = (int64_t)((M + bm - 1) / bm) * tiles_n;
        const int64_t rounds = (tiles + RESIDENT_SLOTS - 1) / RESIDENT_SLOTS;
        const double cost = (double)rounds * (mt + 1.25);
        if (cost < best_cost - 1e-9) { best_cost = cost; best = mt; }
    }
    return best;
}

// The kernels address both operands through 32-bit buffer offsets: the weight must fit one launch, a taller A goes in row chunks (rows are independent;
// whole BM-row tiles per chunk).  Calls f(r0, m, geom) for the chunk of m rows from row r0 on and returns the first error; `who` names the entry point.
template <class F>
int gemm_row_chunks(const char* who, int64_t M, int N, int K, int64_t lda, int64_t ldw, int elem_bytes, int BM, int BN, int slots, F&& f) {
    const uint64_t lim = mq_gemm_addr_limit, elem = (uint64_t)elem_bytes;
    const uint64_t w_bytes = ((uint64_t)(N - 1) * (uint64_t)ldw + (uint64_t)K) * elem;
    if (w_bytes > lim) {
        mq_set_error("%s: weight matrix of %llu bytes exceeds the %llu bytes a launch can address", who, (unsigned long long)w_bytes, (unsigned long long)lim);
        return MQ_ERR_INVALID;
    }
    int64_t max_rows = (uint64_t)K * elem > lim ? 0 : (int64_t)((lim - (uint64_t)K * elem) / ((uint64_t)lda * elem)) + 1;
    max_rows = max_rows / BM * BM;
    if (max_rows < BM) {
        mq_set_error("%s: lda=%ld too large", who, (long)lda);
        return MQ_ERR_INVALID;
    }
    for (int64_t r0 = 0; r0 < M; r0 += max_rows) {
        const int m = (int)((M - r0) < max_rows ? (M - r0) : max_rows);
        GemmGeom g;
        g.tiles_n = (N + BN - 1) / BN;
        g.set_tiles_m((m + BM - 1) / BM, slots);
        g.a_bytes = (unsigned)(((uint64_t)(m - 1) * (uint64_t)lda + (uint64_t)K) * elem);
        g.w_bytes = (unsigned)w_bytes;
        MQ_TRY(f(r0, m, g));
    }
    return MQ_OK;
}

// The row-indexed operands of a GEMM from row r on: A (ELEM bytes per element), the residual and the output, whose row strides follow the epilogue
// flags — out fp32 4 B, e4m3 1 B, else bf16 2 B; the residual is bf16 next to a bf16 out, else fp32.
struct GemmRows { const void* A; const float* residual; void* out; };
template <int FLAGS, int ELEM>
GemmRows gemm_rows_from(int64_t r, const void* A, int64_t lda, const float* residual, void* out, int64_t ldc) {
    const size_t out_row = (size_t)ldc * ((FLAGS & MQ_EPI_OUT_F32) ? 4 : (FLAGS & MQ_EPI_OUT_FP8) ? 1 : 2);
    const size_t res_row = (size_t)ldc * (((FLAGS & MQ_EPI_RESIDUAL) && !(FLAGS & MQ_EPI_OUT_F32)) ? 2 : 4);
    return {(const char*)A + (size_t)r * (size_t)lda * ELEM, residual ? (const float*)((const char*)residual + (size_t)r * res_row) : nullptr,
            (char*)out + (size_t)r * out_row};
}

}  // namespace
