// Building blocks shared by the tiled GEMM main loops (gemm_bf16.hip: both operands through the LDS ring; gemm_wd.hip: the W operand global -> VGPR;
// gemm_fp8.hip: the e4m3 loop, with a k-step of its own).
#pragma once
#include <type_traits>
#include <utility>
#include "common.h"

namespace {

constexpr int BK = 64;   // the bf16 k-step (elements)

// The persistent tiled GEMMs' (virtual) block -> tile map, XCD-aware and bijective: XCD k takes the k-th contiguous share of the tiles
// (as xcd_banded_block), walked row-major — or, with cgroup > 0, L2-blocked: bands of band_rows tile rows, each walked cgroup tile columns at a time (the last
// group narrower), so that an XCD's A panels and W column tiles fit its L2.  ONE map for gemm_nt_kernel, gemm_wd_kernel and gemm_fp8_kernel; built once at
// the top of a kernel (the per-launch terms are then computed once, not at every tile).
template <int BM, int BN>
struct GemmTileMap {
    int q, r, tiles_n, tiles_m, cgroup, band_rows;
    __device__ __forceinline__ GemmTileMap(int num_tiles, int tiles_n_, int M, int cgroup_, int band_rows_)
        : q(num_tiles >> 3), r(num_tiles & 7), tiles_n(tiles_n_), tiles_m((M + BM - 1) / BM), cgroup(cgroup_), band_rows(band_rows_) {}
    __device__ __forceinline__ void origin(int vbid, int& m0, int& n0) const {
        const int xcd = vbid & 7, idx = vbid >> 3;
        const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        int tm, tn;
        if (cgroup > 0) {
            const int band_tiles = band_rows * tiles_n;
            const int band = tile / band_tiles, rb = tile - band * band_tiles;
            const int rows_here = min(band_rows, tiles_m - band * band_rows);
            const int full = rows_here * cgroup, ncg_full = tiles_n / cgroup;
            int cg = rb / full, r2 = rb - cg * full, cw = cgroup;
            if (cg >= ncg_full) { cg = ncg_full; r2 = rb - ncg_full * full; cw = tiles_n - ncg_full * cgroup; }
            const int rr = r2 / cw;
            tm = band * band_rows + rr;
            tn = cg * cgroup + (r2 - rr * cw);
        } else {
            tm = tile / tiles_n;
            tn = tile - tm * tiles_n;
        }
        m0 = tm * BM;
        n0 = tn * BN;
    }
};

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, unsigned lds_wave_base) {
    // 16 B per lane; LDS destination = wave-uniform base (M0) + lane * 16; source = descriptor base + voff (per lane) + soff (scalar)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(uintptr_t)lds_wave_base, 16, voff, soff, 0, 0);
}
template <int OFF>
__device__ __forceinline__ bf16x8 lds_read16(unsigned addr) {
    i32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return __builtin_bit_cast(bf16x8, v);
}

// The compiler takes an inline asm's outputs as valid the moment the statement has executed, and a register-only consumer (an MFMA, a v_dot2c)
// has no ordering against the hand-placed `s_waitcnt lgkmcnt(0)` asm: the optimiser may sink it to right behind the ds_read that defines its operand —
// it did exactly that with the LN_APPLY statistics (40 v_dot2c moved into the loop latch, in front of the wait; tests/test_gemm_isa.py caught it).
// Passing the registers through an EMPTY asm behind the wait ties their consumers to it by data flow (volatile asms keep their order); no instruction.
template <class T>
__device__ __forceinline__ void landed(T& v) { asm volatile("" : "+v"(v)); }

template <int... Is, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, Is...>, F&& f) { (f(std::integral_constant<int, Is>{}), ...); }
// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>): every index is a compile-time constant inside f (register arrays stay
// registers; a run-time counter that the unroller has to fold first sent the fragment arrays to scratch)
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }

}  // namespace
