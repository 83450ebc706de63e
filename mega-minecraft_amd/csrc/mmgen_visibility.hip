// mmgen section visibility for gfx950: which 16^3 sections of a world of device-resident chunks a consumer has to draw from a given eye
// (contract: include/mmgen.h "section visibility", design: DESIGN.md section 6.8).  The reference leaves this to OptiX; here it is the
// voxel engines' two-part answer in software.
//
//   k_section_conn       one workgroup per chunk, one lane per column (the occupancy / mask kernels' 16-byte loads).  A lane keeps its
//                        column's see-through mask T as 6 x u64 (4 sections of 16 bits per word) and five floods of all 24 sections at once,
//                        5 x 6 u64 in registers: flood f starts from face layer f (connectivity is symmetric, the sixth is redundant).
//                        A round is one horizontal step (+-x: DPP row shifts inside the row of 16 lanes, +-z: lane +- 16 through LDS) and
//                        then the whole vertical run within the lane by the carry of one addition per direction, masked so that nothing
//                        crosses a 16-bit section boundary.  Rounds repeat, per 64-voxel word, until a workgroup-wide OR of "changed" is 0.
//   k_visible_sections   one workgroup of 1 024 lanes, a lane owns up to 5 window columns.  Sections are processed level by level of
//                        Manhattan distance from the eye section; at level k a column holds at most two sections (dy = +-m).  A finished
//                        section publishes its EXIT mask X (6 bits: the faces some entry face connects to) in LDS, double-buffered by
//                        level parity; a section of the next level pulls X from its up to three predecessors (one per axis): no atomics,
//                        one barrier per level, 17 KB of LDS at the largest radius.  A column's record of the next level is prefetched.
// No floating point, no global atomics, no matrix instructions: there is no contraction here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mm_math.cuh"
#include "mm_blockdata.cuh"
#include "mm_meshclass.cuh"
#include "../../include/mmgen.h"
#include "mmgen_prof.h"

namespace mm {

// ---------------------------------------------------------------------------------------------------------
// connectivity
// ---------------------------------------------------------------------------------------------------------
#define CONN_FLOODS 5
#define CONN_MAX_ROUNDS 2048
#define CONN_GROUPS_EVEN 0x0000ffff0000ffffull             // sections 0 and 2 of a word: 16 zero bits above each stop a carry
#define CONN_TOP 0x8000800080008000ull                     // the y = 15 layer of the 4 sections of a word
#define CONN_BOTTOM 0x0001000100010001ull                  // the y = 0 layer

// 16 voxels of a column -> 16 bits "sees through"
MM_DEV uint32_t conn_word(const uint4& v, const uint8_t* s_tab)
{
    // terrain is long vertical runs: most words hold one block id 16 times - one lookup instead of 16
    if (v.x == v.y && v.x == v.z && v.x == v.w && v.x == ((v.x << 8) | (v.x >> 24))) return s_tab[v.x & 255u] ? 0xffffu : 0u;
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) m |= (uint32_t)s_tab[(q[k] >> (8 * j)) & 255u] << (4 * k + j);
    return m;
}

// s subset of t.  In every run of t, the bits from the run's lowest seed up to its top, never across a 16-bit boundary: adding the seeds to
// the run carries through its ones and stops in the zero above it; the even and the odd sections are added apart, so that zero always exists.
MM_DEV uint64_t conn_fill_up(uint64_t t, uint64_t s)
{
    const uint64_t te = t & CONN_GROUPS_EVEN, to = t & ~CONN_GROUPS_EVEN, se = s & CONN_GROUPS_EVEN, so = s & ~CONN_GROUPS_EVEN;
    return (((((te + se) ^ te) | se) & te) | ((((to + so) ^ to) | so) & to));      // a seed above another one keeps its bit under the carry: | s
}
// every run of t (trev = its bit reversal) that holds a bit of s, whole
MM_DEV uint64_t conn_fill_runs(uint64_t t, uint64_t trev, uint64_t s) { return conn_fill_up(t, s) | __brevll(conn_fill_up(trev, __brevll(s))); }

// the lanes at x - 1 and x + 1 of the row of 16 (zero beyond the row's ends), OR-ed
MM_DEV uint32_t conn_row_nbrs32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101 /*row_shl:1*/, 0xf, 0xf, true) |
           (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /*row_shr:1*/, 0xf, 0xf, true);
}
MM_DEV uint64_t conn_row_nbrs(uint64_t v) { return (uint64_t)conn_row_nbrs32((uint32_t)v) | ((uint64_t)conn_row_nbrs32((uint32_t)(v >> 32)) << 32); }

// bit j = the 16-bit group j of m is not zero
MM_DEV uint32_t conn_groups_nz(uint64_t m)
{
    return ((m & 0xffffull) ? 1u : 0u) | ((m & 0xffff0000ull) ? 2u : 0u) | ((m & 0xffff00000000ull) ? 4u : 0u) | ((m & 0xffff000000000000ull) ? 8u : 0u);
}
MM_DEV uint32_t conn_groups_full(uint64_t m) { return conn_groups_nz(~m) ^ 15u; }
// 0xffff in every group whose bit is set
MM_DEV uint64_t conn_groups_expand(uint32_t g) { return (((uint64_t)(g & 1u)) | ((uint64_t)(g & 2u) << 15) | ((uint64_t)(g & 4u) << 30) | ((uint64_t)(g & 8u) << 45)) * 0xffffull; }

MM_DEV uint32_t wave_or(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o);
    return v;
}

__global__ void __launch_bounds__(256)
k_section_conn(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ chunkIdx, uint8_t* __restrict__ conn, uint32_t* __restrict__ rounds)
{
    __shared__ uint64_t s_R[CONN_FLOODS][6][256];         // 61 440 bytes: what the lanes at z +- 1 read
    __shared__ uint8_t s_tab[256];
    __shared__ uint32_t s_chg[4], s_notfull[4], s_any[4];
    __shared__ uint32_t s_res[15];                         // per face pair: bit sy = connected in section sy
    const int t = threadIdx.x, x = t & 15, z = t >> 4, wave = t >> 6;
    const int c = chunkIdx ? chunkIdx[blockIdx.x] : (int)blockIdx.x;
    {
        const int tr = t < MMB_NUM_BLOCKS ? (int)MESH_TRANS(kBlockData[t]) : T_OPAQUE;      // ids beyond the enum are OPAQUE, as in the lighting
        s_tab[t] = (t == MMB_AIR || tr != T_OPAQUE) ? 1 : 0;
        if (t < 15) s_res[t] = 0;
    }
    __syncthreads();
    const uint4* col = (const uint4*)(blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * c + 384 * t);
    uint64_t T[6], Trev[6];
#pragma unroll
    for (int w0 = 0; w0 < 24; w0 += 8) {                  // 8 independent 16-byte loads in flight per lane: two 64-voxel words
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = col[w0 + k];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint64_t m = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) m |= (uint64_t)conn_word(v[4 * h + k], s_tab) << (16 * k);
            T[w0 / 4 + h] = m; Trev[w0 / 4 + h] = __brevll(m);
        }
    }
    // sections that are all T are connected through and through, sections without T have no path: neither needs a round
    uint32_t notfull = 0, any = 0;
#pragma unroll
    for (int w = 0; w < 6; ++w) { notfull |= (conn_groups_full(T[w]) ^ 15u) << (4 * w); any |= conn_groups_nz(T[w]) << (4 * w); }
    notfull = wave_or(notfull); any = wave_or(any);
    if ((t & 63) == 0) { s_notfull[wave] = notfull; s_any[wave] = any; }
    __syncthreads();
    notfull = s_notfull[0] | s_notfull[1] | s_notfull[2] | s_notfull[3];
    any = s_any[0] | s_any[1] | s_any[2] | s_any[3];
    const uint32_t full = ~notfull & 0xffffffu, mixed = notfull & any;

    // layer f of this lane's column: the whole column on a side face, one voxel per section on the top and the bottom one
    const uint64_t layer[6] = {z == 15 ? ~0ull : 0ull, x == 15 ? ~0ull : 0ull, z == 0 ? ~0ull : 0ull, x == 0 ? ~0ull : 0ull, CONN_TOP, CONN_BOTTOM};
    uint64_t R[CONN_FLOODS][6];
    uint32_t active = 0;                                   // words with a section that has to be flooded
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        const uint64_t fullw = conn_groups_expand((full >> (4 * w)) & 15u);
#pragma unroll
        for (int f = 0; f < CONN_FLOODS; ++f) {
            R[f][w] = conn_fill_runs(T[w], Trev[w], layer[f] & T[w]) | fullw;
            s_R[f][w][t] = R[f][w];
        }
        if ((mixed >> (4 * w)) & 15u) active |= 1u << w;
    }
    active = __builtin_amdgcn_readfirstlane(active);
    __syncthreads();

    // Jacobi rounds.  A round takes every flood one horizontal step and then to the ends of the vertical runs it has reached.  A shortest path
    // enters a vertical run once, and a section has at most 256 x 8 runs, so a flood is complete after at most CONN_MAX_ROUNDS rounds: the loop ends.
    uint32_t nrounds = 0;
    while (active && nrounds < CONN_MAX_ROUNDS) {
        uint32_t chg = 0;
#pragma unroll
        for (int w = 0; w < 6; ++w) {
            if (!((active >> w) & 1u)) continue;           // (workgroup-uniform)
#pragma unroll
            for (int f = 0; f < CONN_FLOODS; ++f) {
                const uint64_t r = R[f][w];
                uint64_t n = r | conn_row_nbrs(r);
                if (z < 15) n |= s_R[f][w][t + 16];
                if (z > 0) n |= s_R[f][w][t - 16];
                n &= T[w];
                if (n != r) { R[f][w] = conn_fill_runs(T[w], Trev[w], n); chg |= 1u << w; }
            }
        }
        __syncthreads();                                   // every read of this round is done
#pragma unroll
        for (int w = 0; w < 6; ++w)
            if ((chg >> w) & 1u)
#pragma unroll
                for (int f = 0; f < CONN_FLOODS; ++f) s_R[f][w][t] = R[f][w];
        chg = wave_or(chg);
        if ((t & 63) == 0) s_chg[wave] = chg;
        __syncthreads();
        active = __builtin_amdgcn_readfirstlane(s_chg[0] | s_chg[1] | s_chg[2] | s_chg[3]);      // words are independent: one that did not change is done
        ++nrounds;
    }

    // pair (a, b), a < b: flood a meets layer b
    int p = 0;
#pragma unroll
    for (int a = 0; a < CONN_FLOODS; ++a)
#pragma unroll
        for (int b = a + 1; b < 6; ++b, ++p) {
            uint32_t hit = 0;
#pragma unroll
            for (int w = 0; w < 6; ++w) hit |= conn_groups_nz(R[a][w] & layer[b]) << (4 * w);
            if (hit) atomicOr(&s_res[p], hit);
        }
    __syncthreads();
    if (t < 24) {
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 15; ++q) v |= ((s_res[q] >> t) & 1u) << q;
        ((uint16_t*)(conn + (size_t)MMGEN_SECTION_CONN_BYTES * c))[t] = (uint16_t)v;
    }
    if (rounds && t == 0) rounds[c] = nrounds;
}

// ---------------------------------------------------------------------------------------------------------
// visible set
// ---------------------------------------------------------------------------------------------------------
#define VIS_NT 1024
#define VIS_MAXW (2 * MMGEN_VISIBLE_MAX_RADIUS + 1)
#define VIS_K 5                                            // window columns per lane: 65 x 65 = 4 225 <= 5 x 1 024
static_assert(VIS_K * VIS_NT >= VIS_MAXW * VIS_MAXW, "every window column has a lane");

// the faces that some face of E is connected to in the record
MM_DEV uint32_t vis_exits(uint32_t E, uint32_t rec)
{
    uint32_t X = 0;
    int p = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = a + 1; b < 6; ++b, ++p)
            if ((rec >> p) & 1u) X |= (((E >> a) & 1u) << b) | (((E >> b) & 1u) << a);
    return X;
}

struct VisColumn {
    int s;                  // window column wx + W wz, -1 = this slot has none
    int dx, dz, start;      // offset from the eye's column; the level of its first section
    int px, pz;             // the window columns of the predecessors on x and z (valid where dx, dz != 0)
    bool ingrid;            // the cell exists
    const uint16_t* rec;    // its 24 records, NULL = absent (or outside the grid)
    uint32_t recUp, recDn;  // the records of the sections of the coming level (prefetched)
    uint32_t vis;
};

// the record of section sy of the column: virtual layers and absent cells are transparent
MM_DEV uint32_t vis_record(const VisColumn& C, int sy)
{
    if (!C.ingrid || sy < -1 || sy > 24) return 0u;       // no such section: never used
    if (!C.rec || sy < 0 || sy > 23) return 0x7fffu;
    return C.rec[sy];
}

// One section: pulls its entry set from the predecessors' exit masks of the previous level, reports itself, returns its own exit mask.
// sign: 0 = at or above the eye's layer (reads the up buffer), 1 = below.
MM_DEV uint32_t vis_section(VisColumn& C, const uint8_t* Xprev /*[2][W2]*/, int W2, int sign, int sy, int m, uint32_t rec)
{
    if (!C.ingrid || sy < -1 || sy > 24) return 0u;       // the section does not exist: nothing steps into it, nothing leaves it
    const uint8_t* Xp = Xprev + sign * W2;
    uint32_t E = 0;
    if (C.dx > 0 && (Xp[C.px] & 2u)) E |= 8u;              // the predecessor leaves through +x (1): entered through -x (3)
    if (C.dx < 0 && (Xp[C.px] & 8u)) E |= 2u;
    if (C.dz > 0 && (Xp[C.pz] & 1u)) E |= 4u;              // +z (0) -> -z (2)
    if (C.dz < 0 && (Xp[C.pz] & 4u)) E |= 1u;
    if (m > 0 && sign == 0 && (Xp[C.s] & 16u)) E |= 32u;   // +y (4) -> -y (5)
    if (m > 0 && sign == 1 && (Xp[C.s] & 32u)) E |= 16u;
    const bool eye = C.start == 0 && m == 0;
    if (C.rec && (E || eye) && sy >= 0 && sy <= 23) C.vis |= 1u << sy;
    return eye ? 63u : vis_exits(E, rec);
}

__global__ void __launch_bounds__(VIS_NT)
k_visible_sections(const uint8_t* __restrict__ conn, const int32_t* __restrict__ grid, int gw, int gh, int ecx, int esy, int ecz, int radius,
                   uint32_t* __restrict__ visible)
{
    __shared__ uint8_t s_X[2][2][VIS_MAXW * VIS_MAXW];    // [level parity][up / down][window column]: exit masks, 16 900 bytes
    const int t = threadIdx.x, W = 2 * radius + 1, W2 = W * W;
    VisColumn C[VIS_K];
#pragma unroll
    for (int k = 0; k < VIS_K; ++k) {
        const int s = t + VIS_NT * k;
        const bool valid = s < W2;
        const int dx = s % W - radius, dz = s / W - radius, cx = ecx + dx, cz = ecz + dz;
        C[k].s = valid ? s : -1;
        C[k].dx = dx; C[k].dz = dz; C[k].start = abs(dx) + abs(dz);
        C[k].px = s - (dx > 0 ? 1 : -1); C[k].pz = s - (dz > 0 ? W : -W);
        C[k].ingrid = valid && cx >= 0 && cx < gw && cz >= 0 && cz < gh;
        const int slot = C[k].ingrid ? grid[cz * gw + cx] : -1;
        C[k].rec = slot >= 0 ? (const uint16_t*)(conn + (size_t)MMGEN_SECTION_CONN_BYTES * slot) : nullptr;
        C[k].recUp = C[k].recDn = vis_record(C[k], esy);
        C[k].vis = 0;
    }
    // the farthest section that exists: 2 radius in the plane, then up to layer 24 or down to layer -1
    const int levels = 2 * radius + max(24 - esy, esy + 1);
#pragma unroll 1
    for (int lv = 0; lv <= levels; ++lv) {
        uint8_t* Xcur = &s_X[lv & 1][0][0];
        const uint8_t* Xprev = &s_X[(lv & 1) ^ 1][0][0];
#pragma unroll
        for (int k = 0; k < VIS_K; ++k) {
            const int m = lv - C[k].start;
            if (C[k].s < 0 || m < 0) continue;
            // every column of the window writes both entries at every level from its first one on: what the next level reads is never stale
            const uint32_t up = vis_section(C[k], Xprev, VIS_MAXW * VIS_MAXW, 0, esy + m, m, C[k].recUp);
            const uint32_t dn = m == 0 ? up : vis_section(C[k], Xprev, VIS_MAXW * VIS_MAXW, 1, esy - m, m, C[k].recDn);
            Xcur[C[k].s] = (uint8_t)up; Xcur[VIS_MAXW * VIS_MAXW + C[k].s] = (uint8_t)dn;
            C[k].recUp = vis_record(C[k], esy + m + 1); C[k].recDn = vis_record(C[k], esy - m - 1);
        }
        __syncthreads();                                   // level lv is published; its reads of level lv - 1 are done before lv + 1 overwrites them
    }
#pragma unroll
    for (int k = 0; k < VIS_K; ++k)
        if (C[k].s >= 0) visible[C[k].s] = C[k].vis;
}

}  // namespace mm

extern "C" {

static int section_connectivity(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, uint8_t* d_conn, uint32_t* d_rounds, void* stream)
{
    if (n < 0 || !d_blocks || !d_conn) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_SECTION_CONN, mm::k_section_conn, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_chunk_idx, d_conn, d_rounds);
    return (int)hipGetLastError();
}

int mmgen_section_connectivity(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, uint8_t* d_conn, void* stream)
{
    return section_connectivity(d_blocks, d_chunk_idx, n, d_conn, nullptr, stream);
}

int mmgen_debug_section_rounds(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, uint8_t* d_conn, uint32_t* d_rounds, void* stream)
{
    if (!d_rounds) return (int)hipErrorInvalidValue;
    return section_connectivity(d_blocks, d_chunk_idx, n, d_conn, d_rounds, stream);
}

int mmgen_visible_sections(const uint8_t* d_conn, const int32_t* d_grid, int grid_w, int grid_h, int eye_cx, int eye_sy, int eye_cz, int radius,
                           uint32_t* d_visible, void* stream)
{
    if (!d_conn || !d_grid || !d_visible) return (int)hipErrorInvalidValue;
    if (grid_w < 1 || grid_h < 1 || grid_w > 16384 || grid_h > 16384) return (int)hipErrorInvalidValue;
    if (eye_cx < 0 || eye_cx >= grid_w || eye_cz < 0 || eye_cz >= grid_h || eye_sy < -1 || eye_sy > 24) return (int)hipErrorInvalidValue;
    if (radius < 0 || radius > MMGEN_VISIBLE_MAX_RADIUS) return (int)hipErrorInvalidValue;
    MMK_LAUNCH_NORET(mmk::KID_VISIBLE_SECTIONS, mm::k_visible_sections, dim3(1), dim3(VIS_NT), (hipStream_t)stream, d_conn, d_grid, grid_w, grid_h,
                     eye_cx, eye_sy, eye_cz, radius, d_visible);
    return (int)hipGetLastError();
}

}  // extern "C"
