// Block-id equality masks of a column and the workgroup scan, shared by the two quad meshers (mmgen_quads.hip: the chunk-wide greedy stream,
// mmgen_section_quads.hip: the section-bucketed one).  Moved verbatim out of mmgen_quads.hip; that mesher's record-exact tests pin it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mm_math.cuh"

namespace mm {

// bit i = (byte i of a == byte i of b): exact zero-byte detect of a ^ b, then the eight 0x80 flags gathered by one multiply (no carries:
// the 64 partial products fall on 64 different bit positions)
MM_DEV uint32_t eq_bytes(uint64_t a, uint64_t b)
{
    const uint64_t x = a ^ b, k = 0x7f7f7f7f7f7f7f7full;
    const uint64_t zero = ~(((x & k) + k) | x | k);
    return (uint32_t)(((zero >> 7) * 0x0102040810204080ull) >> 56);
}

MM_DEV uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

// The per-column masks are 6 x u64 in registers, built by ROLLED loops over the six words (unrolled, the compiler hoists all of a column's loads
// and runs out of registers): the new word enters at the top and the others move down, so that after six pushes word w sits in a[w] and no
// register array is ever indexed by a variable.
MM_DEV void push_word(uint64_t a[6], uint64_t v) { a[0] = a[1]; a[1] = a[2]; a[2] = a[3]; a[3] = a[4]; a[4] = a[5]; a[5] = v; }

// bit y of eq[]: block y of column `me` == block y of column `other` (whole 8-byte words: xor, zero-byte detect, gather); all zero without a column
MM_DEV void column_equal(const uint4* __restrict__ me, const uint4* __restrict__ other, bool has, uint64_t eq[6])
{
#pragma unroll 1
    for (int w = 0; w < 6; ++w) {
        uint64_t e = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 a = me[4 * w + k], b = other[4 * w + k];
            e |= (uint64_t)(eq_bytes(u64_of(a.x, a.y), u64_of(b.x, b.y)) | (eq_bytes(u64_of(a.z, a.w), u64_of(b.z, b.w)) << 8)) << (16 * k);
        }
        push_word(eq, has ? e : 0ull);
    }
}

// bit y of eq[]: block y == block y - 1 of the same column (the column against itself shifted by one byte, carried from word to word)
MM_DEV void column_equal_below(const uint4* __restrict__ me, uint64_t eq[6])
{
    uint64_t below = 0;
#pragma unroll 1
    for (int w = 0; w < 6; ++w) {
        uint64_t e = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 a = me[4 * w + k];
            const uint64_t lo = u64_of(a.x, a.y), hi = u64_of(a.z, a.w);
            e |= (uint64_t)(eq_bytes(lo, (lo << 8) | (below >> 56)) | (eq_bytes(hi, (hi << 8) | (lo >> 56)) << 8)) << (16 * k);
            below = hi;
        }
        push_word(eq, e);
    }
    eq[0] &= ~1ull;                                        // nothing below y = 0
}

// ---- additions for the lit section mesher (mmgen_lit_section_quads.hip): the same byte equality over 16 LIGHT bytes under a mask.  m8 is the
// mask byte repeated eight times; masked bytes are compared, so with m8 == 0 every bit is set.
MM_DEV uint64_t mask_bytes8(uint32_t m) { return (uint64_t)(m & 0xffu) * 0x0101010101010101ull; }

// bit i = byte i of a == byte i of b under the mask, i = 0..15
MM_DEV uint32_t eq_bytes16_masked(const uint4& a, const uint4& b, uint64_t m8)
{
    return eq_bytes(u64_of(a.x, a.y) & m8, u64_of(b.x, b.y) & m8) | (eq_bytes(u64_of(a.z, a.w) & m8, u64_of(b.z, b.w) & m8) << 8);
}

// bit i = byte i of a == byte i - 1 of a under the mask; byte 0 is compared with `below`
MM_DEV uint32_t eq_bytes16_below_masked(const uint4& a, uint32_t below, uint64_t m8)
{
    const uint64_t lo = u64_of(a.x, a.y) & m8, hi = u64_of(a.z, a.w) & m8;
    return eq_bytes(lo, (lo << 8) | ((uint64_t)below & m8 & 0xffull)) | (eq_bytes(hi, (hi << 8) | (lo >> 56)) << 8);
}

MM_DEV uint32_t wave_incl_scan(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(v, d); if (lane >= d) v += u; }
    return v;
}

// inclusive scan of one value per lane over the workgroup's 256 lanes; total in *total.  Two barriers; s_wsum is free again on return.
MM_DEV uint32_t block_incl_scan(uint32_t v, int t, uint32_t* s_wsum, uint32_t* total)
{
    const int lane = t & 63, wave = t >> 6;
    const uint32_t incl = wave_incl_scan(v, lane);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    const uint32_t w0 = s_wsum[0], w1 = s_wsum[1], w2 = s_wsum[2], w3 = s_wsum[3];
    __syncthreads();
    *total = w0 + w1 + w2 + w3;
    return incl + (wave > 0 ? w0 : 0u) + (wave > 1 ? w1 : 0u) + (wave > 2 ? w2 : 0u);
}

}  // namespace mm
