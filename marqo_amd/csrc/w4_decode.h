// The MXFP4 register decode shared by the W4A16 GEMMs (gemm_small_w4.hip: skinny; gemm_w4.hip: tiled): a block's scaled decode table and the
// eight-codes-per-dword lookup.  The storage format it reads is stated at the top of gemm_small_w4.hip.
#pragma once
#include "common.h"

namespace {

constexpr int W4_BK = 128;      // k per chunk: four 32-blocks, 16 B of codes per lane
constexpr int W4_KMULT = 64;    // K % 64 == 0 (a row's last chunk may be half)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the scaled decode table of one block: bf16(magnitude[i] x 2^(sb - 127)), i = 0 .. 7, low bytes in {tl1, tl0}, high bytes in {th1, th0} (byte i).
// Index 1 (0.5) has the exponent field e0 = sb - 1 and mantissa 0; index i >= 2 has e0 + (i >> 1) and mantissa bit 6 = i & 1; index 0 is 0.
struct W4Table { uint32_t tl0, tl1, th0, th1; };

__device__ __forceinline__ W4Table w4_table(uint32_t sb) {
    const uint32_t e0 = sb - 1, h = e0 >> 1, par = e0 & 1;
    W4Table t;
    t.tl0 = 0xC0800000u ^ (par * 0x80808000u);               // bit 7 = the exponent field's bit 0, bit 6 = the mantissa bit
    t.tl1 = 0xC0804000u ^ (par * 0x80808080u);
    t.th0 = h * 0x01010100u + par * 0x01010000u;             // (e0 + (i >> 1)) >> 1; sb <= 227 keeps every byte below 0x80: the sign bit stays free
    t.th1 = (h + 1) * 0x01010101u + par * 0x01010000u;
    return t;
}

// eight codes (one dword of the storage) -> eight bf16 at k offsets 0 .. 7, scale included
__device__ __forceinline__ bf16x8 w4_decode8(uint32_t q, const W4Table& t) {
    const uint32_t ev = q & 0x07070707u, od = (q >> 4) & 0x07070707u;     // magnitude indices of k offsets 0 .. 3 and 4 .. 7, one per byte
    const uint32_t le = __builtin_amdgcn_perm(t.tl1, t.tl0, ev), he = __builtin_amdgcn_perm(t.th1, t.th0, ev) | ((q & 0x08080808u) << 4);
    const uint32_t lo = __builtin_amdgcn_perm(t.tl1, t.tl0, od), ho = __builtin_amdgcn_perm(t.th1, t.th0, od) | (q & 0x80808080u);
    u32x4 d;
    d[0] = __builtin_amdgcn_perm(he, le, 0x05010400u);
    d[1] = __builtin_amdgcn_perm(he, le, 0x07030602u);
    d[2] = __builtin_amdgcn_perm(ho, lo, 0x05010400u);
    d[3] = __builtin_amdgcn_perm(ho, lo, 0x07030602u);
    return __builtin_bit_cast(bf16x8, d);
}

int64_t w4_chunks(int64_t K) { return (K + W4_BK - 1) / W4_BK; }

}  // namespace
