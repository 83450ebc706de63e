// mmgen voxel lighting for gfx950: a 4-bit sky light and a 4-bit block light per voxel over blocks that stay in HBM (contract: include/mmgen.h
// "voxel lighting", design: DESIGN.md section 6.7).  The reference lights its world with an OptiX path tracer; this is the classic flood fill,
// restated as 15 dilations of bit masks: S_L = {source >= L} | (T & dilate6(S_L+1)), light = number of L with v in S_L.
//
//   k_light_masks   one workgroup per chunk, one lane per column (the mesher's 16-byte loads): the column's 384-bit mask T of voxels that pass
//                   light, its open height, its emission as four bit-sliced planes per 64-voxel word and, per word, the OR of the emission
//                   values in it (0 = no emitter in this word; also an upper bound of the level).  A dense record: no emitter capacity.
//   k_light<SW>     one workgroup per (chunk, slab of SW words of y).  Its window is the chunk's 256 columns and the 1 260 columns of the eight
//                   neighbours within Manhattan distance 14 of the footprint, SW + 2 words high.  S lives in LDS, [word][column]; a lane owns
//                   up to four window columns and keeps their T words in registers, so the vertical neighbours are shifts in registers with
//                   carries between the words, and the four horizontal ones are LDS reads.  A level is a Jacobi step (read, barrier, write,
//                   barrier) over the columns within distance L - 1 of the footprint only: column ring r needs S_L only for L <= 15 - r.  The
//                   footprint's lanes count level membership in bit-sliced 4-bit counters and expand them to bytes at the end.
// No global atomics, no data-dependent loop besides the levels, no matrix instructions: there is no contraction here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mm_math.cuh"
#include "mm_blockdata.cuh"
#include "mm_meshclass.cuh"
#include "../../include/mmgen.h"
#include "mmgen_prof.h"

namespace mm {

// the mask record of a chunk slot (MMGEN_LIGHT_MASK_BYTES), c = x + 16 z, w = y / 64, bit y % 64
#define LM_T 0              // u64 [256][6]      voxel passes light (class not OPAQUE)
#define LM_E 12288          // u64 [256][6][4]   bit k of the emission value
#define LM_OPEN 61440       // u16 [256]         lowest y from which the column is AIR / X_SHAPED up to y = 383; 384 = none
#define LM_FLAG 61952       // u32 [256]         nibble w = OR of the emission values of word w
static_assert(LM_FLAG + 1024 == MMGEN_LIGHT_MASK_BYTES, "mask record layout");

__host__ __device__ inline uint8_t light_default_emission(int id)
{
    switch (id) {
    case MMB_LAVA: case MMB_GLOWSTONE: case MMB_SHROOMLIGHT: case MMB_SEA_LANTERN: return 15;
    case MMB_CAVE_VINES_GLOW_MAIN: case MMB_CAVE_VINES_GLOW_END: return 14;
    case MMB_MAGENTA_CRYSTAL: case MMB_CYAN_CRYSTAL: case MMB_GREEN_CRYSTAL: return 10;
    case MMB_SMALL_MAGENTA_CRYSTAL: case MMB_SMALL_CYAN_CRYSTAL: case MMB_SMALL_GREEN_CRYSTAL:
    case MMB_HANGING_SMALL_MAGENTA_CRYSTAL: case MMB_HANGING_SMALL_CYAN_CRYSTAL: case MMB_HANGING_SMALL_GREEN_CRYSTAL: return 6;
    default: return 0;
    }
}

// ---------------------------------------------------------------------------------------------------------
// masks
// ---------------------------------------------------------------------------------------------------------
#define LT_PASS 16u         // s_tab[id]: bits 0-3 emission, bit 4 passes light, bit 5 AIR or X_SHAPED
#define LT_AIRX 32u

// 16 voxels of a column -> 16 bits each of: passes light, AIR / X_SHAPED, emission planes 0..3; returns the OR of the emission values
MM_DEV uint32_t light_word(const uint4& v, const uint8_t* s_tab, uint32_t& pass, uint32_t& airx, uint32_t e[4])
{
    // terrain is long vertical runs: most words hold one block id 16 times - one lookup instead of 16
    if (v.x == v.y && v.x == v.z && v.x == v.w && v.x == ((v.x << 8) | (v.x >> 24))) {
        const uint32_t c = s_tab[v.x & 255u];
        pass = (c & LT_PASS) ? 0xffffu : 0u; airx = (c & LT_AIRX) ? 0xffffu : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = ((c >> k) & 1u) ? 0xffffu : 0u;
        return c & 15u;
    }
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    uint32_t any = 0;
    pass = airx = e[0] = e[1] = e[2] = e[3] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t c = s_tab[(q[k] >> (8 * j)) & 255u];
            const int i = 4 * k + j;
            pass |= ((c >> 4) & 1u) << i; airx |= ((c >> 5) & 1u) << i;
            e[0] |= (c & 1u) << i; e[1] |= ((c >> 1) & 1u) << i; e[2] |= ((c >> 2) & 1u) << i; e[3] |= ((c >> 3) & 1u) << i;
            any |= c & 15u;
        }
    return any;
}

__global__ void __launch_bounds__(256)
k_light_masks(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ chunkIdx, const uint8_t* __restrict__ emission, uint8_t* __restrict__ masks)
{
    __shared__ uint8_t s_tab[256];
    const int t = threadIdx.x;
    const int c = chunkIdx ? chunkIdx[blockIdx.x] : (int)blockIdx.x;
    {
        const int tr = t < MMB_NUM_BLOCKS ? (int)MESH_TRANS(kBlockData[t]) : T_OPAQUE;      // ids beyond the enum are OPAQUE, as in the mesher
        const bool air = t == MMB_AIR, pass = air || tr != T_OPAQUE, airx = air || tr == T_XSHAPED;
        const uint32_t e = emission ? min((uint32_t)emission[t], 15u) : (uint32_t)light_default_emission(t);
        s_tab[t] = (uint8_t)(e | (pass ? LT_PASS : 0u) | (airx ? LT_AIRX : 0u));
    }
    __syncthreads();
    const uint4* col = (const uint4*)(blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * c + 384 * t);
    uint8_t* rec = masks + (size_t)MMGEN_LIGHT_MASK_BYTES * c;
    uint64_t* outT = (uint64_t*)(rec + LM_T) + 6 * t;
    uint64_t* outE = (uint64_t*)(rec + LM_E) + 24 * t;
    // open: start of the run of AIR / X_SHAPED voxels that reaches the top of what has been read so far
    uint32_t open = 0, flags = 0;
#pragma unroll 1
    for (int w0 = 0; w0 < 24; w0 += 8) {                  // 8 independent 16-byte loads in flight per lane, as the mesher: two 64-voxel words
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = col[w0 + k];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint64_t pass = 0, airx = 0, e[4] = {0, 0, 0, 0};
            uint32_t any = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t p16, a16, e16[4];
                any |= light_word(v[4 * h + k], s_tab, p16, a16, e16);
                pass |= (uint64_t)p16 << (16 * k); airx |= (uint64_t)a16 << (16 * k);
#pragma unroll
                for (int b = 0; b < 4; ++b) e[b] |= (uint64_t)e16[b] << (16 * k);
            }
            const int w = w0 / 4 + h;
            outT[w] = pass;
#pragma unroll
            for (int b = 0; b < 4; ++b) outE[4 * w + b] = e[b];
            flags |= any << (4 * w);
            if (~airx) open = 64 * w + 64 - __builtin_clzll(~airx);      // just above the highest voxel that closes the column
        }
    }
    ((uint16_t*)(rec + LM_OPEN))[t] = (uint16_t)open;
    ((uint32_t*)(rec + LM_FLAG))[t] = flags;
}

// ---------------------------------------------------------------------------------------------------------
// light
// ---------------------------------------------------------------------------------------------------------
// The window in coordinates xi = x + 14, zi = z + 14 of a 44 x 44 square; the footprint is 14..29.  A column's ring is its Manhattan
// distance from the footprint; the window is the 1 516 columns of ring <= 14, stored row after row (row zi holds xi in [cut, 44 - cut)).
#ifndef MMGEN_LIGHT_SLAB
#define MMGEN_LIGHT_SLAB 2  // words of y per workgroup (1, 2, 3 or 6; 3 and 6 spill): DESIGN.md section 6.7 has the measurements behind the choice
#endif
#ifndef MMGEN_LIGHT_WAVES
#define MMGEN_LIGHT_WAVES 2 // waves per SIMD the register allocation aims at: one workgroup of 512 lanes per CU (4 would spill)
#endif
#define LW_SIDE 44
#define LW_COLS 1516
#define LIGHT_NT 512
#define LIGHT_K 4           // window slots per lane: 44 x 44 = 1 936 <= 4 x 512
static_assert(LIGHT_K * LIGHT_NT >= LW_SIDE * LW_SIDE, "every window slot has a lane");

MM_DEV int lw_cut(int i) { return max(0, max(14 - i, i - 29)); }
MM_DEV int lw_rowstart(int zi)
{
    if (zi <= 14) return 16 * zi + zi * (zi - 1);          // rows of 16, 18, .. 42 columns
    if (zi <= 30) return 406 + 44 * (zi - 14);
    const int m = zi - 30;
    return 1110 + 42 * m - m * (m - 1);                    // rows of 42, 40, .. 16 columns
}
MM_DEV int lw_col(int xi, int zi) { return lw_rowstart(zi) + xi - lw_cut(zi); }

// bits of `e >= L` from the four planes of e (L in 1..15)
MM_DEV uint64_t planes_ge(const uint64_t p[4], int L)
{
    uint64_t gt = 0, eq = ~0ull;
#pragma unroll
    for (int b = 3; b >= 0; --b) {
        if ((L >> b) & 1) eq &= p[b];
        else { gt |= eq & p[b]; eq &= ~p[b]; }
    }
    return gt | eq;
}

// bit i of the result's byte i = bit i of b8 (b8 < 256), every byte 0 or 1
MM_DEV uint64_t spread_bits(uint64_t b8)
{
    const uint64_t x = (b8 * 0x0101010101010101ull) & 0x8040201008040201ull;
    return ((x + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}

// adds the bits of m to the bit-sliced 4-bit counters c (a voxel is counted at most 15 times)
MM_DEV void count_bits(uint64_t c[4], uint64_t m)
{
#pragma unroll
    for (int b = 0; b < 4; ++b) { const uint64_t carry = c[b] & m; c[b] ^= m; m = carry; }
}

template <int WW>
struct LightCols {                                         // a lane's window columns
    int col[LIGHT_K];                                      // index into S, -1 = no column in this slot
    int up[LIGHT_K], dn[LIGHT_K];                          // the columns at z + 1 and z - 1 (valid for ring <= 13)
    int ring[LIGHT_K];                                     // 99 = never updated: no column, or nothing passes light and nothing emits
    int slot[LIGHT_K], ccol[LIGHT_K];                      // chunk slot (-1 absent) and column in it
    int open[LIGHT_K];                                     // open height, 384 = none (also for an absent chunk)
    uint32_t flag[LIGHT_K];                                // nibble j = OR of the emission values of window word j
    uint64_t T[LIGHT_K][WW];
};

// source bits of level L in window word j of slot k
template <bool SKY, int WW>
MM_DEV uint64_t light_source(const LightCols<WW>& C, const uint8_t* __restrict__ masks, int wb, int k, int j, int L)
{
    if (SKY) {                                             // an open voxel is a source of 15: a member of every level
        const int o = C.open[k] - 64 * (wb + j);
        if ((unsigned)(wb + j) > 5u) return 0ull;          // nothing below y = 0 or above y = 383
        return o <= 0 ? ~0ull : (o >= 64 ? 0ull : ~0ull << o);
    }
    if ((int)((C.flag[k] >> (4 * j)) & 15u) < L) return 0ull;      // the OR of the word's emission values bounds every one of them
    const uint64_t* e = (const uint64_t*)(masks + (size_t)MMGEN_LIGHT_MASK_BYTES * C.slot[k] + LM_E) + 4 * (6 * C.ccol[k] + wb + j);
    const uint64_t p[4] = {e[0], e[1], e[2], e[3]};
    return planes_ge(p, L);
}

// One channel over the window: levels L0 .. 1 (every level above L0 is empty).  cnt: the footprint column of lanes 0..255, slab words only.
template <bool SKY, int SW>
MM_DEV void light_channel(const LightCols<SW + 2>& C, uint64_t (*S)[LW_COLS], const uint8_t* __restrict__ masks, int wb, int L0, int fcol, uint64_t cnt[SW][4])
{
    constexpr int WW = SW + 2;
    const int t = threadIdx.x;
    __syncthreads();                                       // the previous channel's counting reads are done
    // S_L0 = its sources: nothing above it to dilate
#pragma unroll
    for (int k = 0; k < LIGHT_K; ++k)
        if (C.col[k] >= 0)
#pragma unroll
            for (int j = 0; j < WW; ++j) S[j][C.col[k]] = C.ring[k] < 99 ? light_source<SKY, WW>(C, masks, wb, k, j, L0) : 0ull;
    __syncthreads();
    if (t < 256)
#pragma unroll
        for (int j = 0; j < SW; ++j) count_bits(cnt[j], S[1 + j][fcol]);
#pragma unroll 1
    for (int L = L0 - 1; L >= 1; --L) {
        uint64_t nw[LIGHT_K][WW];
#pragma unroll
        for (int k = 0; k < LIGHT_K; ++k) {
            if (C.ring[k] >= L) continue;                  // S_L is needed within distance L - 1 of the footprint only
            const int c = C.col[k];
            uint64_t s[WW];
#pragma unroll
            for (int j = 0; j < WW; ++j) s[j] = S[j][c];
#pragma unroll
            for (int j = 0; j < WW; ++j) {
                uint64_t a = S[j][c - 1] | S[j][c + 1] | S[j][C.up[k]] | S[j][C.dn[k]] | (s[j] << 1) | (s[j] >> 1);
                if (j > 0) a |= s[j - 1] >> 63;
                if (j < WW - 1) a |= s[j + 1] << 63;
                nw[k][j] = light_source<SKY, WW>(C, masks, wb, k, j, L) | (C.T[k][j] & a);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LIGHT_K; ++k) {
            if (C.ring[k] >= L) continue;
#pragma unroll
            for (int j = 0; j < WW; ++j) S[j][C.col[k]] = nw[k][j];
        }
        __syncthreads();
        if (t < 256)
#pragma unroll
            for (int j = 0; j < SW; ++j) count_bits(cnt[j], S[1 + j][fcol]);
    }
}

template <int SW>
__global__ void __launch_bounds__(LIGHT_NT, MMGEN_LIGHT_WAVES)
k_light(const uint8_t* __restrict__ masks, const int32_t* __restrict__ grid, int gw, int gh, const int32_t* __restrict__ cells, uint8_t* __restrict__ light)
{
    constexpr int WW = SW + 2, NSLAB = 6 / SW;
    static_assert(6 % SW == 0, "slabs tile the column");
    __shared__ uint64_t S[WW][LW_COLS];
    __shared__ uint32_t s_red[LIGHT_NT / 64];
    const int t = threadIdx.x;
    const int item = blockIdx.x / NSLAB, slab = blockIdx.x % NSLAB;
    const int cell = cells ? cells[item] : item;
    if (cell < 0 || cell >= gw * gh) return;               // (workgroup-uniform, as is the next)
    const int home = grid[cell];
    if (home < 0) return;
    const int cx = cell % gw, cz = cell / gw;
    const int wb = slab * SW - 1;                          // the column word of window word 0; words outside 0..5 pass nothing and emit nothing

    LightCols<WW> C;
    uint32_t red = 0;       // bits 0-3: OR of the window's emission values; 16: a footprint voxel of the slab is not open; 32: an open voxel in the window
#pragma unroll
    for (int k = 0; k < LIGHT_K; ++k) {
        const int s = t + LIGHT_NT * k, zi = s / LW_SIDE, xi = s % LW_SIDE;
        const int ring = lw_cut(xi) + lw_cut(zi);
        const bool valid = s < LW_SIDE * LW_SIDE && ring <= 14;
        C.col[k] = valid ? lw_col(xi, zi) : -1;
        C.up[k] = lw_col(xi, zi + 1); C.dn[k] = lw_col(xi, zi - 1);      // read for ring <= 13 only: both rows exist and hold xi
        const int x = xi - 14, z = zi - 14, gx = cx + (x >> 4), gz = cz + (z >> 4);
        int slot = -1;
        if (valid && gx >= 0 && gx < gw && gz >= 0 && gz < gh) slot = grid[gz * gw + gx];
        C.slot[k] = slot; C.ccol[k] = (x & 15) + 16 * (z & 15);
        C.flag[k] = 0;
        int open = 384;
        uint64_t anyT = 0;
#pragma unroll
        for (int j = 0; j < WW; ++j) C.T[k][j] = 0;
        if (slot >= 0) {
            const uint8_t* rec = masks + (size_t)MMGEN_LIGHT_MASK_BYTES * slot;
            open = ((const uint16_t*)(rec + LM_OPEN))[C.ccol[k]];
            const uint32_t f = ((const uint32_t*)(rec + LM_FLAG))[C.ccol[k]];
#pragma unroll
            for (int j = 0; j < WW; ++j) {
                const int w = wb + j;
                if (w < 0 || w > 5) continue;
                C.T[k][j] = ((const uint64_t*)(rec + LM_T))[6 * C.ccol[k] + w];
                anyT |= C.T[k][j];
                C.flag[k] |= ((f >> (4 * w)) & 15u) << (4 * j);
            }
        }
        C.open[k] = open;
        // a column through which nothing passes and that emits nothing keeps S = 0 at every level: it is never updated
        C.ring[k] = (valid && (anyT | C.flag[k])) ? ring : 99;
#pragma unroll
        for (int j = 0; j < WW; ++j) red |= (C.flag[k] >> (4 * j)) & 15u;
        if (valid && ring == 0 && open > 64 * SW * slab) red |= 16u;
        if (valid && open < 64 * min(wb + WW, 6)) red |= 32u;
    }
    {
        uint32_t r = 0;
#pragma unroll
        for (int b = 0; b < 6; ++b) r |= __ballot((red >> b) & 1u) ? 1u << b : 0u;
        if ((t & 63) == 0) s_red[t >> 6] = r;
        __syncthreads();
        red = 0;
#pragma unroll
        for (int i = 0; i < LIGHT_NT / 64; ++i) red |= s_red[i];
    }

    const int fcol = lw_col(14 + (t & 15), 14 + ((t >> 4) & 15));
    uint64_t sky[SW][4], blk[SW][4];
#pragma unroll
    for (int j = 0; j < SW; ++j)
#pragma unroll
        for (int b = 0; b < 4; ++b) { sky[j][b] = 0; blk[j][b] = 0; }
    // Shortcuts (workgroup-uniform), each with the same result as the level loop:
    //   every voxel of the slab's footprint is open: open(v) gives sky(v) = 15 by definition, no neighbour is looked at;
    //   no open voxel in the window: every source set is empty there, so by induction from S_16 = {} every S_L is empty on the rings it is
    //   needed on, and the sky light of the footprint is 0;
    //   block light: levels above the OR of the window's emission values have no source, so they are empty by the same induction and the
    //   loop starts at that level; when the OR is 0 there is no emitter at all and the block light of the footprint is 0.
    if (!(red & 16u)) {
#pragma unroll
        for (int j = 0; j < SW; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) sky[j][b] = ~0ull;
    } else if (red & 32u) light_channel<true, SW>(C, S, masks, wb, 15, fcol, sky);
    if (red & 15u) light_channel<false, SW>(C, S, masks, wb, (int)(red & 15u), fcol, blk);

    if (t < 256) {
        uint4* out = (uint4*)(light + (size_t)MMGEN_BLOCKS_PER_CHUNK * home + 384 * t + 64 * SW * slab);
#pragma unroll
        for (int j = 0; j < SW; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {                  // 16 voxels = one 16-byte store of (sky << 4) | block
                uint64_t q[2] = {0, 0};
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        q[h] |= (spread_bits((blk[j][b] >> (16 * g + 8 * h)) & 255ull) << b) | (spread_bits((sky[j][b] >> (16 * g + 8 * h)) & 255ull) << (4 + b));
                out[4 * j + g] = make_uint4((uint32_t)q[0], (uint32_t)(q[0] >> 32), (uint32_t)q[1], (uint32_t)(q[1] >> 32));
            }
    }
}

}  // namespace mm

extern "C" {

int mmgen_light_default_emission(uint8_t* h_out)
{
    if (!h_out) return (int)hipErrorInvalidValue;
    for (int i = 0; i < 256; ++i) h_out[i] = mm::light_default_emission(i);
    return 0;
}

int mmgen_light_masks(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, const uint8_t* d_emission, uint8_t* d_masks, void* stream)
{
    if (n < 0 || (n > 0 && (!d_blocks || !d_masks))) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_LIGHT_MASKS, mm::k_light_masks, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_chunk_idx, d_emission, d_masks);
    return (int)hipGetLastError();
}

int mmgen_light(const uint8_t* d_masks, const int32_t* d_grid, int grid_w, int grid_h, const int32_t* d_cells, int n, uint8_t* d_light, void* stream)
{
    if (n < 0 || grid_w < 1 || grid_h < 1 || grid_w > 16384 || grid_h > 16384) return (int)hipErrorInvalidValue;
    if (!d_cells && n > grid_w * grid_h) return (int)hipErrorInvalidValue;
    if (n > 0 && (!d_masks || !d_grid || !d_light)) return (int)hipErrorInvalidValue;
    constexpr int slabs = 6 / MMGEN_LIGHT_SLAB;
    if (n > 0x7fffffff / slabs) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_LIGHT, mm::k_light<MMGEN_LIGHT_SLAB>, dim3(n * slabs), dim3(LIGHT_NT), (hipStream_t)stream, d_masks, d_grid, grid_w, grid_h,
                     d_cells, d_light);
    return (int)hipGetLastError();
}

}  // extern "C"
