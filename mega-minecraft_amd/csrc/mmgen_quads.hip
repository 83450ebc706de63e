// mmgen greedy quad mesher for gfx950: a chunk's visible faces merged into rectangles, one 64-bit record per quad (contract: include/mmgen.h
// "greedy-merged compact quad mesh", record layout: include/mmgen_types.h).  The reference has no such path; the face set is the display rule
// of Chunk::createVBOs (mm_meshclass.cuh), the merge rule and the order are this library's own and are stated in the header.
//
// One workgroup (4 waves) per chunk, one lane per column for everything that is per column, one lane per PLANE for the greedy:
//   1  classify the columns into class bit planes (LDS, mm_meshclass.cuh) and take each column's six face masks and its X mask out of them
//      as 6 x u64 per direction, IN REGISTERS: the planes' 46 KB are dead after that and the LDS work area is reused three times;
//   2  the X-shaped blocks: per-column popcounts, scanned over the workgroup (their masks then leave the registers);
//   3  phase C: F(+y), F(-y), then eqX, eqZ are TRANSPOSED by wave64 ballots (lane = column: one ballot of bit y over a wave's 64 columns is four
//               16-bit rows of the y plane); 768 planes of 16 x 16 bits, three per lane, wave v takes the planes with y % 4 == v so that the
//               few y levels that carry the terrain's surface spread over all four SIMDs;
//      phase A: the columns store F(+z), F(-z), eqY, eqX; 32 lanes (8 per wave) each walk one plane z = p of 16 rows x 384 bits;
//      phase B: F(+x), F(-x), eqY, eqZ; 32 lanes each walk one plane x = p;
//      the equality masks are 6 x u64 per column in registers, from whole 8-byte words of block ids (xor, zero-byte detect, multiply-gather):
//      bit y of eqY / eqX / eqZ says block(x, y, z) == block at y-1 / x-1 / z-1;
//      a run is ctz of the inverted, shifted mask F & eqQ (carried across the 64-bit words of a 384-bit row), it extends to the next row iff
//      that row's F & eqR contains the run's mask, and "covered" is the bit cleared from F in LDS (every plane is owned by one lane).
// k_quads<false> (count) stores the 833 group counts, k_quads<true> (fill) scans them in LDS and writes each group's records at its scanned
// offset in emission order: no atomics on global memory, no sorting.  Both are ONE traversal template, so they agree by construction; the fill
// additionally never writes beyond a group's counted records.  No matrix instructions: there is no contraction here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mm_math.cuh"
#include "mm_blockdata.cuh"
#include "mm_meshclass.cuh"
#include "mm_quadbits.cuh"
#include "../../include/mmgen.h"
#include "mmgen_prof.h"

namespace mm {

struct SideBuf { uint64_t fa[256][6], fb[256][6], eqq[256][6], eqr[256][6]; };      // per column: two face masks, equality along y and along the rows
struct TopBuf { uint64_t rows[384][4][4]; };                                         // [y][F(+y), F(-y), eqX, eqZ][wave]: 16 rows (z) of 16 bits (x)
struct ClassBuf { Planes P; uint8_t cls[256]; };
union QuadWork { ClassBuf c; SideBuf s; TopBuf y; };                                 // 49 152 bytes, used one after the other

MM_DEV uint64_t quad_word(int x, int y, int z, int kind, int dx, int dy, int dz, int b)
{
    return (uint64_t)(uint32_t)(x | (y << 4) | (z << 13) | (kind << 17) | (dx << 20)) | ((uint64_t)dy << 24) | ((uint64_t)dz << 33) | ((uint64_t)b << 37);
}

// bits [y0, y0 + len) of a 384-bit row, as they fall into 64-bit word w (w within the span)
MM_DEV uint64_t span_mask(int y0, int len, int w)
{
    const int lo = max(y0 - 64 * w, 0), hi = min(y0 + len - 64 * w, 64), n = hi - lo;
    return (n >= 64 ? ~0ull : ((1ull << n) - 1ull)) << lo;
}

// One side plane (direction d, p = z for +-z, p = x for +-x) per lane, 8 lanes per wave: rows r (16) x 384 bits.  colP / colR: column index
// step per plane / per row.  F is this direction's face masks in LDS and is consumed (a covered cell is a cleared bit).
template <bool FILL>
MM_DEV void side_planes(SideBuf& S, int t, int da, int db, int colP, int colR, uint32_t* s_grp, uint64_t* __restrict__ out, const uint8_t* __restrict__ chunk)
{
    const int lane = t & 63;
    if (lane >= 8) return;
    const int i = (t >> 6) * 8 + lane, p = i & 15, d = (i >> 4) ? db : da;
    uint64_t (*F)[6] = (i >> 4) ? S.fb : S.fa;
    const int g = 16 * d + p;
    const uint32_t off = FILL ? s_grp[g] : 0u, room = FILL ? s_grp[g + 1] - off : 0u;
    uint32_t n = 0;
#pragma unroll 1
    for (int r = 0; r < 16; ++r) {
        const int cr = p * colP + r * colR;
#pragma unroll 1
        for (int w = 0; w < 6; ++w) {
            uint64_t m;
            while ((m = F[cr][w]) != 0) {
                const int q0 = __builtin_ctzll(m), y0 = 64 * w + q0;
                // the run along y: cells that are faces, uncovered and equal to the cell below, word after word
                int len = 1;
                for (int ww = w, bit = q0 + 1;;) {
                    if (bit == 64) { bit = 0; if (++ww == 6) break; }
                    const uint64_t cont = (F[cr][ww] & S.eqq[cr][ww]) >> bit;      // zeros shifted in on top: at most 64 - bit ones
                    const int k = ~cont ? __builtin_ctzll(~cont) : 64;
                    len += k; bit += k;
                    if (bit < 64) break;
                }
                const int wl = w, wh = (y0 + len - 1) >> 6;
                // rows that continue the whole run with the same block
                int rows = 1;
                for (; r + rows < 16; ++rows) {
                    const int cn = cr + rows * colR;
                    bool whole = true;
                    for (int ww = wl; ww <= wh && whole; ++ww) {
                        const uint64_t mk = span_mask(y0, len, ww);
                        whole = ((F[cn][ww] & S.eqr[cn][ww]) & mk) == mk;
                    }
                    if (!whole) break;
                }
                for (int k = 0; k < rows; ++k)
                    for (int ww = wl; ww <= wh; ++ww) F[cr + k * colR][ww] &= ~span_mask(y0, len, ww);
                if (FILL && n < room)
                    out[off + n] = quad_word(cr & 15, y0, cr >> 4, d, colR == 1 ? rows - 1 : 0, len - 1, colR == 1 ? 0 : rows - 1, chunk[y0 + 384 * cr]);
                ++n;
            }
        }
    }
    if (!FILL) s_grp[g] = n;
}

// The y planes: three per lane.  Rows z of 16 bits (x); F rows are consumed, the equality rows are shared by the two directions of a level.
template <bool FILL>
MM_DEV void y_planes(TopBuf& Y, int t, uint32_t* s_grp, uint64_t* __restrict__ out, const uint8_t* __restrict__ chunk)
{
    uint16_t* R = (uint16_t*)Y.rows;
    const int lane = t & 63, wave = t >> 6;
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        const int m = lane + 64 * k, e = m >= 96 ? 1 : 0, y = 4 * (m - 96 * e) + wave;
        const int g = 64 + 384 * e + y;
        const uint64_t* F64 = Y.rows[y][e];
        uint32_t n = 0;
        if ((F64[0] | F64[1] | F64[2] | F64[3]) != 0) {
            uint16_t* Fr = R + (4 * y + e) * 16;
            const uint16_t* ex = R + (4 * y + 2) * 16;
            const uint16_t* ez = R + (4 * y + 3) * 16;
            const uint32_t off = FILL ? s_grp[g] : 0u, room = FILL ? s_grp[g + 1] - off : 0u;
#pragma unroll 1
            for (int r = 0; r < 16; ++r) {
                uint32_t row;
                while ((row = Fr[r]) != 0) {
                    const int q0 = __builtin_ctz(row);
                    const uint32_t cont = (row & ex[r]) >> (q0 + 1);                // < 2^15: the inverse is never zero
                    const int len = 1 + __builtin_ctz(~cont);
                    const uint32_t mk = ((1u << len) - 1u) << q0;
                    int rows = 1;
                    while (r + rows < 16 && (((uint32_t)Fr[r + rows] & ez[r + rows]) & mk) == mk) ++rows;
                    for (int j = 0; j < rows; ++j) Fr[r + j] = (uint16_t)(Fr[r + j] & ~mk);
                    if (FILL && n < room) out[off + n] = quad_word(q0, y, r, 4 + e, len - 1, 0, rows - 1, chunk[y + 384 * (q0 + 16 * r)]);
                    ++n;
                }
            }
        }
        if (!FILL) s_grp[g] = n;
    }
}

#define QUAD_SCAN 836      // 833 group counts / offsets, the total behind them, padded to whole lanes of four
template <bool FILL>
__global__ void __launch_bounds__(256, 3)      // three waves per SIMD = the three workgroups per CU that the LDS allows: at most 168 VGPRs
k_quads(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ chunkIdx, const int32_t* __restrict__ neighborIdx, const uint32_t* __restrict__ groupIn,
        uint32_t* __restrict__ groupOut, uint32_t* __restrict__ chunkQuads, const uint64_t* __restrict__ quadOffset, unsigned long long capacity,
        uint64_t* __restrict__ quads)
{
    __shared__ QuadWork W;
    __shared__ uint32_t s_grp[QUAD_SCAN];      // count: quads per group; fill: exclusive offsets, [833] = the chunk's total
    __shared__ uint32_t s_wsum[4];
    const int o = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int c = chunkIdx ? chunkIdx[o] : o;      // o = position in the work list (outputs), c = chunk in the block array
    uint64_t* out = nullptr;
    if (FILL) {
        uint32_t v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = 4 * t + k < MMGEN_QUAD_GROUPS ? groupIn[(size_t)MMGEN_QUAD_GROUPS * o + 4 * t + k] : 0u; sum += v[k]; }
        uint32_t total;
        uint32_t run = block_incl_scan(sum, t, s_wsum, &total) - sum;
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (4 * t + k < QUAD_SCAN) s_grp[4 * t + k] = run; run += v[k]; }
        __syncthreads();
        const uint64_t base = quadOffset[o];
        if (total == 0 || base + total > capacity) return;      // (workgroup-uniform)
        out = quads + base;
    }
    const uint8_t* chunk = blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * c;

    // 1: classes -> this column's face masks, 64 voxels per word, in registers
    int nbSlot[4]; bool nbPresent[4];
    mesh_classify(blocks, neighborIdx, o, c, W.c.cls, W.c.P, nbSlot, nbPresent);
    uint64_t F[6][6] = {}, X[6] = {};
#pragma unroll 1
    for (int w6 = 0; w6 < 6; ++w6) {
        uint64_t f64[6] = {0, 0, 0, 0, 0, 0}, x64 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int w = 4 * w6 + j;
            if ((W.c.P.p0[t][w] | W.c.P.p1[t][w] | W.c.P.p2[t][w]) == 0) continue;      // a word of AIR shows nothing
            const WordFaces f = word_faces(W.c.P, t, w, nbSlot, nbPresent);
#pragma unroll
            for (int d = 0; d < 6; ++d) f64[d] |= (uint64_t)f.f[d] << (16 * j);
            x64 |= (uint64_t)f.xsh << (16 * j);
        }
#pragma unroll
        for (int d = 0; d < 6; ++d) push_word(F[d], f64[d]);
        push_word(X, x64);
    }

    // 2: the X-shaped blocks first (their masks are dead afterwards), ascending voxel index = column after column.  The scan's barriers
    // also end the reading of the class planes: the work area is free from here on.
    {
        uint32_t nx = 0;
#pragma unroll
        for (int w = 0; w < 6; ++w) nx += (uint32_t)__popcll(X[w]);
        uint32_t totalX;
        uint32_t n = block_incl_scan(nx, t, s_wsum, &totalX) - nx;
        if (FILL) {
            const uint32_t off = s_grp[MMGEN_QUAD_GROUPS - 1], room = s_grp[MMGEN_QUAD_GROUPS] - off;
#pragma unroll
            for (int w = 0; w < 6; ++w)
                for (uint64_t m = X[w]; m; m &= m - 1) {
                    const int y = 64 * w + __builtin_ctzll(m);
                    if (n < room) out[off + n] = quad_word(t & 15, y, t >> 4, 6, 0, 0, 0, chunk[y + 384 * t]);
                    ++n;
                }
        } else if (t == 0) s_grp[MMGEN_QUAD_GROUPS - 1] = totalX;
    }

    // 3C: the y planes.  Ballot transposition of 64 levels at a time: lane i keeps the ballot of bit i and stores level 64 w + i.  A word in
    // which none of the wave's 64 columns has a +-y face stores zero rows and skips the equality ballots (equality rows are only ever ANDed
    // with F rows).  The equality masks are taken from whole words of block ids only after F(+y), F(-y) have left the registers.
    const uint4* me = (const uint4*)(chunk + 384 * t);
    const bool hasX = (t & 15) > 0, hasZ = t >= 16;
    bool any[6];
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        any[w] = __ballot((F[4][w] | F[5][w]) != 0) != 0;
        uint64_t up = 0, dn = 0;
        if (any[w])
#pragma unroll 1
            for (int i = 0; i < 64; ++i) {
                const uint64_t b4 = __ballot((F[4][w] >> i) & 1), b5 = __ballot((F[5][w] >> i) & 1);
                if (lane == i) { up = b4; dn = b5; }
            }
        W.y.rows[64 * w + lane][0][wave] = up; W.y.rows[64 * w + lane][1][wave] = dn;
    }
    uint64_t eqX[6] = {}, eqZ[6] = {};
    column_equal(me, (const uint4*)(chunk + 384 * (hasX ? t - 1 : t)), hasX, eqX);      // the columns at x - 1 and z - 1 lie 384 and 6 144 bytes before
    column_equal(me, (const uint4*)(chunk + 384 * (hasZ ? t - 16 : t)), hasZ, eqZ);
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        if (!any[w]) continue;
        uint64_t ex = 0, ez = 0;
#pragma unroll 1
        for (int i = 0; i < 64; ++i) {
            const uint64_t bx = __ballot((eqX[w] >> i) & 1), bz = __ballot((eqZ[w] >> i) & 1);
            if (lane == i) { ex = bx; ez = bz; }
        }
        W.y.rows[64 * w + lane][2][wave] = ex; W.y.rows[64 * w + lane][3][wave] = ez;
    }
    __syncthreads();
    y_planes<FILL>(W.y, t, s_grp, out, chunk);
    __syncthreads();

    // 3A: planes z = p, rows x: F(+z), F(-z), equality along y and x
    uint64_t eqY[6] = {};
    column_equal_below(me, eqY);
#pragma unroll
    for (int w = 0; w < 6; ++w) { W.s.fa[t][w] = F[0][w]; W.s.fb[t][w] = F[2][w]; W.s.eqq[t][w] = eqY[w]; W.s.eqr[t][w] = eqX[w]; }
    __syncthreads();
    side_planes<FILL>(W.s, t, 0, 2, 16, 1, s_grp, out, chunk);
    __syncthreads();
    // 3B: planes x = p, rows z: F(+x), F(-x), equality along y and z
#pragma unroll
    for (int w = 0; w < 6; ++w) { W.s.fa[t][w] = F[1][w]; W.s.fb[t][w] = F[3][w]; W.s.eqq[t][w] = eqY[w]; W.s.eqr[t][w] = eqZ[w]; }
    __syncthreads();
    side_planes<FILL>(W.s, t, 1, 3, 1, 16, s_grp, out, chunk);
    if (FILL) return;
    __syncthreads();
    uint32_t sum = 0;
    for (int g = t; g < MMGEN_QUAD_GROUPS; g += 256) { const uint32_t v = s_grp[g]; groupOut[(size_t)MMGEN_QUAD_GROUPS * o + g] = v; sum += v; }
    uint32_t all;
    block_incl_scan(sum, t, s_wsum, &all);
    if (t == 0) chunkQuads[o] = all;
}

}  // namespace mm

extern "C" {

int mmgen_mesh_quads_count(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n, uint32_t* d_group_quads,
                           uint32_t* d_chunk_quads, void* stream)
{
    if (n < 0 || (n > 0 && (!d_blocks || !d_group_quads || !d_chunk_quads))) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_QUADS_COUNT, mm::k_quads<false>, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_chunk_idx, d_neighbor_idx,
                     (const uint32_t*)nullptr, d_group_quads, d_chunk_quads, (const uint64_t*)nullptr, 0ull, (uint64_t*)nullptr);
    return (int)hipGetLastError();
}

int mmgen_mesh_quads_fill(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n, const uint32_t* d_group_quads,
                          const uint64_t* d_quad_offset, uint64_t capacity_quads, uint64_t* d_quads, void* stream)
{
    if (n < 0 || capacity_quads == 0 || (n > 0 && (!d_blocks || !d_group_quads || !d_quad_offset || !d_quads))) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_QUADS_FILL, mm::k_quads<true>, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_chunk_idx, d_neighbor_idx, d_group_quads,
                     (uint32_t*)nullptr, (uint32_t*)nullptr, d_quad_offset, (unsigned long long)capacity_quads, d_quads);
    return (int)hipGetLastError();
}

}  // extern "C"
