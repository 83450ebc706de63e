// mmgen level-of-detail chunks for gfx950: s x s device-resident source chunks (s = 2, 4, 8) become one chunk-shaped volume of s^3-block
// cells in the standard slot layout, so that every consumer of "a pool of chunk slots" (rays, light, visibility, the meshers) takes the
// far field unchanged (contract: include/mmgen.h "level-of-detail chunks", design: DESIGN.md section 6.12).
//
//   k_lod_reduce<S>   one workgroup of 256 lanes per (LOD chunk, source chunk) pair.  A source chunk owns (16 / S)^2 whole coarse columns
//                     of the destination slot and writes all 384 bytes of each (result + the AIR above) with 16-byte stores: no memset,
//                     no second pass, no workgroup touches another one's bytes.  The column is walked in six passes of four 16-voxel
//                     words (64 / S slabs); the words of the next pass are in flight while this one is reduced.
//     A  lane = source column.  16-bit content mask per word; a slab never straddles a word, so N is a popcount of a masked field, y1 a
//        clz of it, and the look-ahead a run of ones in a 32-bit window of two adjacent masks (zero beyond y = 383).  The sample id is one
//        byte picked out of the registers already loaded.  Samples go to LDS as bytes [slab][z][x], 0 = the column has none.
//     B  lane = source column.  It reads its cell's S rows of S bytes back and counts the samples equal to its own with a SWAR zero-byte
//        test: votes << 8 | (255 - id) is one key for "most samples, ties to the lowest id".  Key (max) and N (sum) meet across the S lanes of
//        the cell's x run over DPP (quad_perm, row_half_mirror); the run's first lane publishes them in LDS.
//     C  lane = cell.  Max / sum over the S rows of the cell, the id or AIR into the output tile in LDS.
//   Two barriers per pass.  No atomics, no scratch, no floating point; 37 248 bytes of LDS at S = 2, 10 048 at S = 4, 3 552 at S = 8.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mm_math.cuh"
#include "mm_blockdata.cuh"
#include "mm_meshclass.cuh"
#include "../../include/mmgen.h"
#include "mmgen_prof.h"

namespace mm {

// 16 voxels of a column -> 16 bits "is content"
MM_DEV uint32_t lod_word_mask(const uint4& v, const uint8_t* s_cont)
{
    // terrain is long vertical runs: most words hold one block id 16 times - one lookup instead of 16
    if (v.x == v.y && v.x == v.z && v.x == v.w && v.x == ((v.x << 8) | (v.x >> 24))) return s_cont[v.x & 255u] ? 0xffffu : 0u;
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) m |= (uint32_t)s_cont[(q[k] >> (8 * j)) & 255u] << (4 * k + j);
    return m;
}

// byte y (0..23) of the six dwords d0..d5: a chain of selects over values, never an indexed array (by reference, the compiler turns the
// selects of loads into one load at a selected address: scratch)
MM_DEV uint32_t lod_pick(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t d4, uint32_t d5, uint32_t y)
{
    const uint32_t d = y >> 2;
    uint32_t w = d0;
    w = d == 1u ? d1 : w; w = d == 2u ? d2 : w; w = d == 3u ? d3 : w; w = d == 4u ? d4 : w; w = d == 5u ? d5 : w;
    return (w >> (8u * (y & 3u))) & 255u;
}

// how many of the four bytes of x are not zero
MM_DEV uint32_t lod_nonzero_bytes(uint32_t x) { return (uint32_t)__popc((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u); }

template <int CTRL>
MM_DEV uint32_t lod_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true); }

// max of key and sum of n over the S lanes of an aligned x run (all lanes of the wave active); every lane of the run gets both
template <int S>
MM_DEV void lod_run_reduce(uint32_t& key, uint32_t& n)
{
    key = max(key, lod_dpp<0xB1 /*quad_perm:[1,0,3,2]*/>(key)); n += lod_dpp<0xB1>(n);
    if (S >= 4) { key = max(key, lod_dpp<0x4E /*quad_perm:[2,3,0,1]*/>(key)); n += lod_dpp<0x4E>(n); }
    if (S == 8) { key = max(key, lod_dpp<0x141 /*row_half_mirror*/>(key)); n += lod_dpp<0x141>(n); }      // the quads are uniform by now
}

// A for one word of the lane's column (a, mask ma) under the word above it (b, mb): the sample of each of its 16 / S slabs into
// smp[256 slab], returns their N, 4 bits each.  The words are named registers and b is a literal after unrolling: nothing is indexed.
template <int S>
MM_DEV uint32_t lod_word_samples(uint4 a, uint4 b, uint32_t ma, uint32_t mb, uint8_t* smp)
{
    const uint32_t win = ma | (mb << 16);
    uint32_t npk = 0;
#pragma unroll
    for (int j = 0; j < 16 / S; ++j) {
        const int lo = j * S;
        const uint32_t field = (win >> lo) & ((1u << S) - 1u);
        uint32_t id = 0;
        if (field) {
            const uint32_t y1 = (uint32_t)(lo + 31 - __clz((int)field));                 // its highest content voxel inside the slab
            const uint32_t len = (uint32_t)__ffs((int)~(win >> y1)) - 1u;                 // the run of content from y1 up (bit 31 - y1 is 0)
            id = lod_pick(a.x, a.y, a.z, a.w, b.x, b.y, min(y1 + len - 1u, (uint32_t)(lo + 2 * S - 1)));
        }
        smp[256 * j] = (uint8_t)id;
        npk |= (uint32_t)__popc(field) << (4 * j);
    }
    return npk;
}

// B for the 16 / S slabs of one word: smp = the lane's own sample of the first, cell = the first column of its cell there, row = where the
// x run's first lane publishes.  Every lane of the wave runs this.
template <int S>
MM_DEV void lod_word_votes(uint32_t npk, const uint8_t* smp, const uint8_t* cell, uint32_t* row, int rowStride, bool first)
{
#pragma unroll
    for (int j = 0; j < 16 / S; ++j) {
        const uint32_t own = smp[256 * j];
        const uint8_t* c = cell + 256 * j;
        const uint32_t rep = own * 0x01010101u;
        uint32_t differ = 0;                               // bytes of the cell that are not `own`
        if (S == 2) differ = lod_nonzero_bytes(((uint32_t)*(const uint16_t*)c | ((uint32_t)*(const uint16_t*)(c + 16) << 16)) ^ rep);
        if (S == 4) {
#pragma unroll
            for (int r = 0; r < 4; ++r) differ += lod_nonzero_bytes(*(const uint32_t*)(c + 16 * r) ^ rep);
        }
        if (S == 8) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const uint2 w = *(const uint2*)(c + 16 * r);
                differ += lod_nonzero_bytes(w.x ^ rep) + lod_nonzero_bytes(w.y ^ rep);
            }
        }
        uint32_t key = own ? ((((uint32_t)(S * S) - differ) << 8) | (255u - own)) : 0u;
        uint32_t n = (npk >> (4 * j)) & 15u;
        lod_run_reduce<S>(key, n);
        if (first) row[rowStride * j] = key | (n << 16);
    }
}

template <int S>
__global__ void __launch_bounds__(256)
k_lod_reduce(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ srcIdx, uint8_t* __restrict__ lod, const int32_t* __restrict__ dstIdx)
{
    constexpr int G = 16 / S;                              // coarse columns of a source chunk along x and along z = slabs per word
    constexpr int P = 4 * G;                               // slabs per pass of four words
    constexpr int HY = MMGEN_CHUNK_HEIGHT / S;             // coarse voxels per column: a multiple of 16
    constexpr int RS = 16 * G + 1;                         // u32 per slab of s_row; odd, so that the lanes of C (slab fastest) spread over the banks
    __shared__ uint8_t s_cont[256];
    __shared__ __attribute__((aligned(16))) uint8_t s_smp[P][256];      // [slab][z][x]: the column's sample id, 0 = none
    __shared__ uint32_t s_row[P * RS];                     // [slab][z][x run]: key | N << 16 of the S columns of the run
    __shared__ __attribute__((aligned(16))) uint8_t s_out[G * G][HY];
    const int t = threadIdx.x, x = t & 15, z = t >> 4;
    const int i = blockIdx.x, q = blockIdx.y;              // q = qx + S qz
    const int src = srcIdx[(size_t)i * (S * S) + q];
    const int dst = dstIdx ? dstIdx[i] : i;
    // coarse column (X, Z) of this source chunk is column (qx G + X) + 16 (qz G + Z) of the slot, 24 16-byte words each
    uint4* out = (uint4*)(lod + (size_t)MMGEN_BLOCKS_PER_CHUNK * dst) + 24 * ((q % S) * G + 16 * (q / S) * G);
    if (src < 0) {                                         // (workgroup-uniform) absent: AIR
        for (int e = t; e < G * G * 24; e += 256) out[24 * ((e / 24) % G + 16 * ((e / 24) / G)) + e % 24] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    {
        const int tr = t < MMB_NUM_BLOCKS ? (int)MESH_TRANS(kBlockData[t]) : T_OPAQUE;      // ids beyond the enum are OPAQUE, as in the mesher
        s_cont[t] = (t != MMB_AIR && tr != T_XSHAPED) ? 1 : 0;
    }
    __syncthreads();
    const uint4* col = (const uint4*)(blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * src + 384 * t);
    uint4 v0 = col[0], v1 = col[1], v2 = col[2], v3 = col[3], v4 = col[4];      // the pass's four words and the one above them, for the look-ahead
    uint32_t m0 = lod_word_mask(v0, s_cont);
    const uint8_t* cell = &s_smp[0][16 * (z & ~(S - 1)) + (x & ~(S - 1))];       // the first column of the lane's cell
    uint32_t* row = &s_row[z * G + x / S];
    const bool first = (x & (S - 1)) == 0;

#pragma unroll 1
    for (int p = 0; p < 6; ++p) {
        // the next pass's new words 4 p + 5 .. 4 p + 8: in flight until the end of this pass; word 24 and beyond is AIR
        const int w = 4 * p + 5;
        uint4 n0 = col[min(w, 23)], n1 = col[min(w + 1, 23)], n2 = col[min(w + 2, 23)], n3 = col[min(w + 3, 23)];
        if (w + 3 > 23) n3 = make_uint4(0u, 0u, 0u, 0u);   // (the pass after the last one reads nothing of them)
        const uint32_t m1 = lod_word_mask(v1, s_cont), m2 = lod_word_mask(v2, s_cont), m3 = lod_word_mask(v3, s_cont), m4 = lod_word_mask(v4, s_cont);

        // ---- A: per slab of this column N and the sample
        const uint32_t a0 = lod_word_samples<S>(v0, v1, m0, m1, &s_smp[0][t]);
        const uint32_t a1 = lod_word_samples<S>(v1, v2, m1, m2, &s_smp[G][t]);
        const uint32_t a2 = lod_word_samples<S>(v2, v3, m2, m3, &s_smp[2 * G][t]);
        const uint32_t a3 = lod_word_samples<S>(v3, v4, m3, m4, &s_smp[3 * G][t]);
        __syncthreads();                                   // the samples of the pass are in LDS; C of the last pass has read s_row

        // ---- B: votes for the lane's own sample among the S x S of its cell; key and N over the x run
        lod_word_votes<S>(a0, &s_smp[0][t], cell, row, RS, first);
        lod_word_votes<S>(a1, &s_smp[G][t], cell + 256 * G, row + RS * G, RS, first);
        lod_word_votes<S>(a2, &s_smp[2 * G][t], cell + 512 * G, row + 2 * RS * G, RS, first);
        lod_word_votes<S>(a3, &s_smp[3 * G][t], cell + 768 * G, row + 3 * RS * G, RS, first);
        __syncthreads();                                   // the runs are in LDS; every read of s_smp is done

        // ---- C: lane = cell, slab fastest
        for (int c = t; c < P * G * G; c += 256) {
            const int j = c % P, cc = c / P, X = cc % G, Z = cc / G;
            uint32_t key = 0, n = 0;
#pragma unroll
            for (int r = 0; r < S; ++r) {
                const uint32_t e = s_row[j * RS + (Z * S + r) * G + X];
                key = max(key, e & 0xffffu); n += e >> 16;
            }
            s_out[cc][p * P + j] = (uint8_t)(2 * n >= (uint32_t)(S * S * S) ? 255u - (key & 255u) : (uint32_t)MMB_AIR);
        }
        v0 = v4; m0 = m4; v1 = n0; v2 = n1; v3 = n2; v4 = n3;
    }
    __syncthreads();
    for (int e = t; e < G * G * 24; e += 256) {
        const int cc = e / 24, w = e % 24;
        uint4 val = make_uint4(0u, 0u, 0u, 0u);            // the AIR above the content
        if (16 * w < HY) val = *(const uint4*)&s_out[cc][16 * w];
        out[24 * (cc % G + 16 * (cc / G)) + w] = val;
    }
}

}  // namespace mm

extern "C" {

int mmgen_lod_reduce(const uint8_t* d_blocks, const int32_t* d_src_idx, int n, int level, uint8_t* d_lod_blocks, const int32_t* d_dst_idx, void* stream)
{
    if (n < 0 || level < 1 || level > 3 || !d_blocks || !d_src_idx || !d_lod_blocks) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const dim3 grid(n, 1 << (2 * level));                  // (LOD chunk, source chunk of its footprint)
    if (level == 1) MMK_LAUNCH_NORET(mmk::KID_LOD_REDUCE, mm::k_lod_reduce<2>, grid, dim3(256), (hipStream_t)stream, d_blocks, d_src_idx, d_lod_blocks, d_dst_idx);
    else if (level == 2) MMK_LAUNCH_NORET(mmk::KID_LOD_REDUCE, mm::k_lod_reduce<4>, grid, dim3(256), (hipStream_t)stream, d_blocks, d_src_idx, d_lod_blocks, d_dst_idx);
    else MMK_LAUNCH_NORET(mmk::KID_LOD_REDUCE, mm::k_lod_reduce<8>, grid, dim3(256), (hipStream_t)stream, d_blocks, d_src_idx, d_lod_blocks, d_dst_idx);
    return (int)hipGetLastError();
}

}  // extern "C"
