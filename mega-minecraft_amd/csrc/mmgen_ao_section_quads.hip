// mmgen section quad mesher with per-corner ambient occlusion for gfx950: the lit stream of mmgen_lit_section_quads.hip with a face AO byte in the
// greedy key and in a second parallel byte stream (contract: include/mmgen.h "section quad mesh with ambient occlusion", design: DESIGN.md
// section 6.11).  Two faces share a quad only if they share the block id, the light in front of them AND all four corner values.
//
// k_ao_section_quads<FILL>: one workgroup (4 waves) per chunk.
//   1  as in k_lit_section_quads: class bit planes in LDS, lane = column keeps F, X and the three id equality masks in registers.  Before the
//      planes die, their OPAQUE bit is copied into an OCCLUDER HALO u16 [18 x 18 columns][24 words] that lives for the whole kernel: the 256
//      own columns, the 4 x 16 facing columns of the present side neighbours, and the four corner columns of the present DIAGONAL chunks
//      (classified here, 96 lanes x one 16-byte word).  Absent chunks and everything outside the world stay zero.
//   2  six passes as in k_lit_section_quads.  Staging a word in which the lane has a face also bit-slices the face AO of all its 16 voxels from
//      occluder words - eight bit planes (hi, lo per corner) of the face's column in the low half of a u32, of its predecessor's in the high half -
//      and ANDs "all eight planes equal to the predecessor along q / along r" into the id-and-light equality word as it is stored.  +-x / +-z:
//      four 18-bit windows (y - 1 .. y + 16) of the columns f - 2 e_r .. f + e_r; +-y: the layer y +- 1 of the columns around the lane's and
//      around its two predecessors.  All of it is LDS; no global load is added.  The plane walk is k_section_quads', line for line.
//   3  count / fill exactly as in k_lit_section_quads.  The emitting pass computes a record's AO byte at the run's origin cell from the
//      occluder bits of the eight voxels around its front voxel, the three offsets built from uniform integers per direction.
// No floating point, no matrix instructions: there is no contraction here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mm_math.cuh"
#include "mm_blockdata.cuh"
#include "mm_meshclass.cuh"
#include "mm_quadbits.cuh"
#include "../../include/mmgen.h"
#include "mmgen_prof.h"

namespace mm {

#define AQ_GROUPS 97                                      // per section: 16 d + p, then the kind-6 records
#define AQ_ALL (MMGEN_SECTIONS_PER_CHUNK * AQ_GROUPS)     // 2 328 per chunk
#define AQ_SCAN 2560                                      // ten per lane, zero behind AQ_ALL
#define AQ_SY_STRIDE (3 * 256 + 16)                       // u16 per section of the work area, 32 bytes of padding as in k_section_quads
#define AQ_HALO 18                                        // columns per side of the occluder halo: x, z = -1 .. 16 at index x + 1, z + 1
#define AQ_HALO_COLS (AQ_HALO * AQ_HALO)

struct AoClassBuf { Planes P; uint8_t cls[256]; };
union AoWork { AoClassBuf c; uint16_t rows[MMGEN_SECTIONS_PER_CHUNK * AQ_SY_STRIDE]; };      // 46 336 bytes (the class planes)
typedef uint16_t OccCol[24];                              // bit y & 15 of word y >> 4: the voxel is OPAQUE

// 16 x 16 bit transposition over the 16 lanes of a row, two matrices at once (the halves of v): lane x bit y <- lane y bit x
MM_DEV uint32_t aq_transpose(uint32_t v, int x)
{
#pragma unroll
    for (int j = 8; j >= 1; j >>= 1) {
        const uint32_t m = j == 8 ? 0x00ff00ffu : j == 4 ? 0x0f0f0f0fu : j == 2 ? 0x33333333u : 0x55555555u;
        const uint32_t p = (uint32_t)__shfl_xor((int)v, j);
        v = (x & j) ? ((v & ~m) | ((p >> j) & m)) : ((v & m) | ((p & m) << j));
    }
    return v;
}

// ---- occluder words.  Every column index below stays inside the 18 x 18 halo: a face's front column is at most one step outside the chunk and
// its row neighbours run along the border; a predecessor two rows back exists whenever the row equality of the ids can be set at all.

// 18-bit window of halo column col: bit i = O(y = 16 k - 1 + i); nothing occludes below y = 0 or above y = 383
MM_DEV uint32_t aq_window(const OccCol* O, int col, int k)
{
    uint32_t w = (uint32_t)O[col][k] << 1;
    if (k > 0) w |= (uint32_t)O[col][k - 1] >> 15;
    if (k < 23) w |= ((uint32_t)O[col][k + 1] & 1u) << 17;
    return w;
}

// the 16 bits O(y = 16 k + i + 1) (UP) or O(y = 16 k + i - 1) of halo columns a (low half) and b (high half)
MM_DEV uint32_t aq_layer2(const OccCol* O, int a, int b, int k, const bool UP)
{
    const bool in = UP ? k < 23 : k > 0;
    const int k2 = in ? (UP ? k + 1 : k - 1) : k;
    const uint32_t m = (uint32_t)O[a][k] | ((uint32_t)O[b][k] << 16), adj = in ? (uint32_t)O[a][k2] | ((uint32_t)O[b][k2] << 16) : 0u;
    return UP ? ((m >> 1) & 0x7fff7fffu) | ((adj & 0x00010001u) << 15) : ((m << 1) & 0xfffefffeu) | ((adj >> 15) & 0x00010001u);
}

// The AO bit planes of one corner for 2 x 16 faces at once: each u32 holds two columns, the face's in the low half, a predecessor's in the high
// half.  With s = s1 | s2:  .x = hi = ~(s1 & s2) & ~(s & c),  .y = lo = ~(s1 & s2) & ~(s ^ c)  (3 - the number of occluders, 0 when both sides are set)
MM_DEV uint2 aq_corner(uint32_t s1, uint32_t s2, uint32_t c)
{
    const uint32_t s = s1 | s2, n = ~(s1 & s2);
    return make_uint2(n & ~(s & c), n & ~(s ^ c));
}
// bit i set: face i differs from face i - 1 of its own column (bit 0 is never read: no quad crosses a word) / from face i of the predecessor column
MM_DEV uint32_t aq_diff_q(uint2 p) { return (p.x ^ (p.x << 1)) | (p.y ^ (p.y << 1)); }
MM_DEV uint32_t aq_diff_r(uint2 p) { return (p.x ^ (p.x >> 16)) | (p.y ^ (p.y >> 16)); }

// +-x / +-z, word k: the face's front column f, its row neighbours f -+ rc, and the same around the predecessor f - rc (p2 = f - 2 rc, or any column
// where there is no predecessor: the row equality of the ids is zero there).  .x: bit i = face i has the AO of face i - 1, .y: of the predecessor's face i
MM_DEV uint2 aq_equal_side(const OccCol* O, int f, int rc, int p2, int k)
{
    const uint32_t w0 = aq_window(O, f, k), wm = aq_window(O, f - rc, k), wp = aq_window(O, f + rc, k), wmm = aq_window(O, p2, k);
    const uint32_t dn0 = w0 & 0xffffu, dnm = wm & 0xffffu, dnp = wp & 0xffffu, dnmm = wmm & 0xffffu;
    const uint32_t md0 = (w0 >> 1) & 0xffffu, mdm = (wm >> 1) & 0xffffu, mdp = (wp >> 1) & 0xffffu, mdmm = (wmm >> 1) & 0xffffu;
    const uint32_t up0 = w0 >> 2, upm = wm >> 2, upp = wp >> 2, upmm = wmm >> 2;
    const uint32_t s1m = mdm | (mdmm << 16), s1p = mdp | (md0 << 16), s2m = dn0 | (dnm << 16), s2p = up0 | (upm << 16);
    const uint2 c0 = aq_corner(s1m, s2m, dnm | (dnmm << 16)), c1 = aq_corner(s1m, s2p, upm | (upmm << 16)),
                c2 = aq_corner(s1p, s2m, dnp | (dn0 << 16)), c3 = aq_corner(s1p, s2p, upp | (up0 << 16));
    return make_uint2(~(aq_diff_q(c0) | aq_diff_q(c1) | aq_diff_q(c2) | aq_diff_q(c3)) & 0xffffu,
                      ~(aq_diff_r(c0) | aq_diff_r(c1) | aq_diff_r(c2) | aq_diff_r(c3)) & 0xffffu);
}

// +-y, word k: the faces of the lane's halo column hc against those of hx (x - 1, along q) and hz (z - 1, along r), occluders in the layer above /
// below; rows along z (18 columns apart), fast axis along x.  Rolled over (predecessor, row side): unrolled, the 64 loads are hoisted and spill.
MM_DEV uint2 aq_equal_y(const OccCol* O, int hc, int hx, int hz, int k, const bool UP)
{
    uint32_t dx = 0, dz = 0;
#pragma unroll 1
    for (int it = 0; it < 4; ++it) {
        const int b = it < 2 ? hx : hz, dr = (it & 1) ? AQ_HALO : -AQ_HALO;
        const uint32_t s1 = aq_layer2(O, hc + dr, b + dr, k, UP);
        const uint32_t df = aq_diff_r(aq_corner(s1, aq_layer2(O, hc - 1, b - 1, k, UP), aq_layer2(O, hc + dr - 1, b + dr - 1, k, UP))) |
                            aq_diff_r(aq_corner(s1, aq_layer2(O, hc + 1, b + 1, k, UP), aq_layer2(O, hc + dr + 1, b + dr + 1, k, UP)));
        if (it < 2) dx |= df; else dz |= df;
    }
    return make_uint2(~dx & 0xffffu, ~dz & 0xffffu);
}

MM_DEV uint32_t aq_bit(const OccCol* O, int col, int y) { return (uint32_t)y < 384u ? ((uint32_t)O[col][y >> 4] >> (y & 15)) & 1u : 0u; }

// the AO byte of the face whose front voxel is (halo column f, y): e_r = rc columns, e_q = qc columns and qy voxels (uniform integers per direction)
MM_DEV uint32_t aq_face_ao(const OccCol* O, int f, int y, int rc, int qc, int qy)
{
    uint32_t ao = 0;
#pragma unroll
    for (int kr = 0; kr < 2; ++kr)
#pragma unroll
        for (int kq = 0; kq < 2; ++kq) {
            const int cr = kr ? rc : -rc, cq = kq ? qc : -qc, yq = y + (kq ? qy : -qy);
            const uint32_t s1 = aq_bit(O, f + cr, y), s2 = aq_bit(O, f + cq, yq), c = aq_bit(O, f + cr + cq, yq);
            ao |= ((s1 & s2) ? 0u : 3u - (s1 + s2 + c)) << (2 * (2 * kr + kq));
        }
    return ao;
}

// ---- light, as in k_lit_section_quads: the light column one step along d (0..3) from column t and that column's predecessor along the plane's rows
struct AoLitCols { const uint8_t* at; const uint8_t* pred; };
MM_DEV AoLitCols aq_shifted(const uint8_t* __restrict__ light, const uint8_t* own, const int32_t* nb, int t, int d)
{
    const int x = t & 15, z = t >> 4;
    const bool inside = d == 0 ? z < 15 : d == 1 ? x < 15 : d == 2 ? z > 0 : x > 0;
    const int step = d == 0 ? 16 : d == 1 ? 1 : d == 2 ? -16 : -1;
    AoLitCols c;
    c.at = own + 384 * (inside ? t + step : t);
    if (!inside) {
        const int n = nb[d];
        const int facing = d == 0 ? x : d == 1 ? 16 * z : d == 2 ? x + 240 : 15 + 16 * z;
        if (n >= 0) c.at = light + (size_t)MMGEN_BLOCKS_PER_CHUNK * n + 384 * facing;
    }
    const bool hasPred = (d & 1) ? z > 0 : x > 0;
    c.pred = hasPred ? c.at - ((d & 1) ? 16 * 384 : 384) : c.at;
    return c;
}

// a side direction: F; id equality along y AND light equality along y of the shifted column AND AO equality along y; id equality along the rows AND
// light equality of the shifted column with its predecessor AND AO equality with the predecessor's face.  Rolled over the six u64 as in lq_stage_side.
MM_DEV void aq_stage_side(uint16_t* rows, const OccCol* O, uint64_t a[6], uint64_t q[6], uint64_t r[6], const AoLitCols lc, int f, int rc, int p2, uint64_t m8,
                          int inner)
{
#pragma unroll 1
    for (int w = 0; w < 6; ++w) {
        const uint64_t a0 = a[0], q0 = q[0], r0 = r[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t fm = (uint32_t)(a0 >> (16 * j)) & 0xffffu;
            uint16_t* dst = rows + (4 * w + j) * AQ_SY_STRIDE + inner;
            if (__ballot(fm != 0) == 0) { dst[0] = 0; continue; }      // (wave-uniform)
            uint32_t qq = 0, rr = 0;
            if (fm != 0) {
                const int k = 4 * w + j;
                const uint4 A = ((const uint4*)lc.at)[k], B = ((const uint4*)lc.pred)[k];
                const uint32_t below = k > 0 ? lc.at[16 * k - 1] : 0u;
                const uint2 e = aq_equal_side(O, f, rc, p2, k);
                qq = (uint32_t)(q0 >> (16 * j)) & eq_bytes16_below_masked(A, below, m8) & e.x;
                rr = (uint32_t)(r0 >> (16 * j)) & eq_bytes16_masked(A, B, m8) & e.y;
            }
            dst[0] = (uint16_t)fm; dst[256] = (uint16_t)qq; dst[512] = (uint16_t)rr;
        }
        push_word(a, a0); push_word(q, q0); push_word(r, r0);
    }
}

// +y (UP, wave-uniform) or -y, as lq_stage_y; the AO of the lane's faces against those of column x - 1 (along q) and z - 1 (along r).  hc = the
// lane's halo column, hx / hz = that of its predecessors (hc itself where there is none: the id equality is zero there).
MM_DEV void aq_stage_y(uint16_t* rows, const OccCol* O, uint64_t a[6], uint64_t q[6], uint64_t r[6], const uint8_t* me, const uint8_t* mx, const uint8_t* mz,
                       int hc, int hx, int hz, uint64_t m8, const bool UP, int x, int inner)
{
    const uint32_t m1 = (uint32_t)m8 & 0xffu;
#pragma unroll 1
    for (int w = 0; w < 6; ++w) {
        const uint64_t a0 = a[0], q0 = q[0], r0 = r[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t fm = (uint32_t)(a0 >> (16 * j)) & 0xffffu;
            uint16_t* dst = rows + (4 * w + j) * AQ_SY_STRIDE + inner;
            if (__ballot(fm != 0) == 0) { dst[0] = 0; continue; }      // (wave-uniform: the transposition exchanges lanes)
            uint32_t qq = 0, rr = 0;
            if (fm != 0) {
                const int k = 4 * w + j;
                const uint4 A = ((const uint4*)me)[k];
                uint32_t ex = eq_bytes16_masked(A, ((const uint4*)mx)[k], m8), ez = eq_bytes16_masked(A, ((const uint4*)mz)[k], m8);
                const bool in = UP ? k < 23 : k > 0;
                const int e = in ? (UP ? 16 * k + 16 : 16 * k - 1) : 0;
                const uint32_t v = me[e], bx = (!in || ((v ^ mx[e]) & m1) == 0) ? 1u : 0u, bz = (!in || ((v ^ mz[e]) & m1) == 0) ? 1u : 0u;
                if (UP) { ex = (ex >> 1) | (bx << 15); ez = (ez >> 1) | (bz << 15); }
                else { ex = ((ex << 1) & 0xffffu) | bx; ez = ((ez << 1) & 0xffffu) | bz; }
                const uint2 ea = aq_equal_y(O, hc, hx, hz, k, UP);
                qq = (uint32_t)(q0 >> (16 * j)) & 0xffffu & ex & ea.x;
                rr = (uint32_t)(r0 >> (16 * j)) & 0xffffu & ez & ea.y;
            }
            const uint32_t fq = aq_transpose(fm | (qq << 16), x), r2 = aq_transpose(rr, x);
            dst[0] = (uint16_t)fq; dst[256] = (uint16_t)(fq >> 16); dst[512] = (uint16_t)r2;
        }
        push_word(a, a0); push_word(q, q0); push_word(r, r0);
    }
}

// see lq_opaque in mmgen_lit_section_quads.hip: lane predicates are recomputed where they are used instead of living in two SGPRs each
MM_DEV int aq_opaque(int v) { asm volatile("" : "+v"(v)); return v; }
MM_DEV int aq_uniform(int v) { asm volatile("" : "+s"(v)); return v; }

// the plane's 16 rows, two per u32: row 0 leaves at the bottom, zeros enter at the top
MM_DEV void aq_next_row(uint32_t m[8])
{
#pragma unroll
    for (int i = 0; i < 7; ++i) m[i] = __funnelshift_r(m[i], m[i + 1], 16);
    m[7] >>= 16;
}

// FL of a face of voxel (vx, y, vz): the light one step (dx, dy, dz) along its normal (lq_face_light)
MM_DEV uint32_t aq_face_light(const uint8_t* __restrict__ light, const uint8_t* own, int nbd, int dx, int dy, int dz, int vx, int y, int vz)
{
    const int nx = vx + dx, ny = y + dy, nz = vz + dz;
    if (ny > 383) return (uint32_t)MMGEN_LIGHT_ABOVE;
    if (ny < 0) return 0u;
    if (((nx | nz) & ~15) == 0) return own[ny + 384 * (nx + 16 * nz)];
    if (nbd < 0) return 0u;                                // (a face towards an absent neighbour is not in F)
    return light[(size_t)MMGEN_BLOCKS_PER_CHUNK * nbd + ny + 384 * ((nx & 15) + 16 * (nz & 15))];
}

// where a group's records go: the section's range as counted by mmgen_mesh_ao_section_quads_count, the group's offset in it from this launch's own counts
struct AoOut { uint32_t* at; uint8_t* lt; uint8_t* ao; uint32_t rel, room; };
MM_DEV void aq_put(const AoOut& o, uint32_t n, uint32_t rec, uint32_t fl, uint32_t ao)
{
    if (o.rel + n < o.room) { o.at[o.rel + n] = rec; o.lt[o.rel + n] = (uint8_t)fl; o.ao[o.rel + n] = (uint8_t)ao; }
}

template <bool FILL>
__global__ void __launch_bounds__(256, 2)      // two workgroups per CU by LDS (2 x 72 KB of 160): up to 256 VGPRs
k_ao_section_quads(const uint8_t* __restrict__ blocks, const uint8_t* __restrict__ light, const int32_t* __restrict__ chunkIdx,
                   const int32_t* __restrict__ neighborIdx8, uint32_t lightMask, const uint32_t* __restrict__ secIn, uint32_t* __restrict__ secOut,
                   uint32_t* __restrict__ chunkQuads, const uint64_t* __restrict__ quadOffset, unsigned long long capacity, uint32_t* __restrict__ quads,
                   uint8_t* __restrict__ quadLight, uint8_t* __restrict__ quadAo)
{
    __shared__ __attribute__((aligned(16))) AoWork W;
    __shared__ OccCol s_occ[AQ_HALO_COLS];     // the occluder halo: lives from the prologue to the last record
    __shared__ uint32_t s_grp[AQ_SCAN];        // counting: records per group; writing: exclusive offsets over the chunk
    __shared__ uint32_t s_wsum[4];
    __shared__ uint32_t s_secoff[MMGEN_SECTIONS_PER_CHUNK], s_secn[MMGEN_SECTIONS_PER_CHUNK];
    __shared__ int32_t s_nb[8];                // the neighbours' slots, -1 = absent
    const int o = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, x = t & 15;
    const int c = chunkIdx ? chunkIdx[o] : o;      // o = position in the work list (outputs), c = chunk in the block and light arrays
    uint32_t* out = nullptr;
    uint8_t* outL = nullptr;
    uint8_t* outA = nullptr;
    if (FILL) {
        if (t < MMGEN_SECTIONS_PER_CHUNK) s_secn[t] = secIn[(size_t)MMGEN_SECTIONS_PER_CHUNK * o + t];
        __syncthreads();
        if (t == 0) {
            uint32_t run = 0;
            for (int k = 0; k < MMGEN_SECTIONS_PER_CHUNK; ++k) { s_secoff[k] = run; run += s_secn[k]; }
            s_wsum[0] = run;
        }
        __syncthreads();
        const uint32_t total = s_wsum[0];
        const uint64_t base = quadOffset[o];
        __syncthreads();
        if (total == 0 || base + total > capacity) return;      // (workgroup-uniform) none of the three arrays is written
        out = quads + base; outL = quadLight + base; outA = quadAo + base;
    }
    for (int g = AQ_ALL + t; g < AQ_SCAN; g += 256) s_grp[g] = 0;
    if (t < 8) s_nb[t] = neighborIdx8 ? neighborIdx8[8 * (size_t)o + t] : -1;      // (mesh_classify has barriers)
    const uint8_t* chunk = blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * c;
    // without light (light_mask == 0, d_light may be NULL) the light reads go to the block ids: under the zero mask every byte compares equal and
    // every light byte is 0, and the light volume is never touched
    if (lightMask == 0) light = blocks;
    const uint8_t* lchunk = light + (size_t)MMGEN_BLOCKS_PER_CHUNK * c;
    const uint64_t m8 = mask_bytes8(lightMask);

    // 1: classes -> this column's face masks, 64 voxels per word, in registers; then the id equality masks from whole words of ids.
    // mesh_classify reads neighborIdx[4 o + d]: handed the list moved by 4 o entries, it finds entries 0..3 of this chunk's eight.
    int nbSlot[4]; bool nbPresent[4];
    mesh_classify(blocks, neighborIdx8 ? neighborIdx8 + 4 * (size_t)o : nullptr, o, c, W.c.cls, W.c.P, nbSlot, nbPresent);
    uint64_t F[6][6] = {}, X[6] = {};
#pragma unroll 1
    for (int w6 = 0; w6 < 6; ++w6) {
        uint64_t f64[6] = {0, 0, 0, 0, 0, 0}, x64 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int w = 4 * w6 + j;
            s_occ[AQ_HALO * ((t >> 4) + 1) + x + 1][w] = (uint16_t)word_masks(W.c.P, t, w).opq;
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
    // the halo's ring.  Lanes 0..63: border slot 256 + t of the class planes = side d = t >> 4, position t & 15 along the edge (classified only
    // when the neighbour is present).  Lanes 64..159: word (t - 64) % 24 of the corner column of diagonal (t - 64) / 24, straight from its ids.
    if (t < 64) {
        const int d = t >> 4, al = (t & 15) + 1;
        const int col = d == 0 ? AQ_HALO * 17 + al : d == 1 ? AQ_HALO * al + 17 : d == 2 ? al : AQ_HALO * al;
        const bool present = s_nb[d] >= 0;
        for (int w = 0; w < 24; ++w) s_occ[col][w] = present ? (uint16_t)word_masks(W.c.P, 256 + t, w).opq : (uint16_t)0;
    } else if (t < 64 + 4 * 24) {
        const int k = (t - 64) / 24, w = (t - 64) % 24, n = s_nb[4 + k];
        // (+x,+z) shows its column (0, 0) at halo (17, 17); (+x,-z) its (0, 15) at (17, 0); (-x,-z) its (15, 15) at (0, 0); (-x,+z) its (15, 0) at (0, 17)
        const int src = k == 0 ? 0 : k == 1 ? 240 : k == 2 ? 255 : 15;
        const int col = k == 0 ? AQ_HALO * 17 + 17 : k == 1 ? 17 : k == 2 ? 0 : AQ_HALO * 17;
        uint32_t m = 0;
        if (n >= 0) {
            const uint4 v = ((const uint4*)(blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * n + 384 * src))[w];
            const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 16; ++i) m |= (W.c.cls[(q[i >> 2] >> (8 * (i & 3))) & 255u] == C_OPAQUE ? 1u : 0u) << i;
        }
        s_occ[col][w] = (uint16_t)m;
    }
    const uint4* me = (const uint4*)(chunk + 384 * t);
    const bool hasX = x > 0, hasZ = t >= 16;
    uint64_t eqY[6] = {}, eqX[6] = {}, eqZ[6] = {};
    column_equal_below(me, eqY);
    column_equal(me, (const uint4*)(chunk + 384 * (hasX ? t - 1 : t)), hasX, eqX);
    column_equal(me, (const uint4*)(chunk + 384 * (hasZ ? t - 16 : t)), hasZ, eqZ);
    __syncthreads();                                       // the class planes are dead: their LDS is the work area; the halo is complete

    // 2: the traversal; the fill runs it twice (count into LDS, scan, write)
#pragma unroll 1
    for (int pass = 0; pass < (FILL ? 2 : 1); ++pass) {
        const bool emit = FILL && pass == 1;

        // phase X: ascending voxel index inside a section = column after column; a kind-6 record has its own voxel's light and no occlusion
#pragma unroll 1
        for (int w = 0; w < 6; ++w) {
            const uint64_t x0 = X[0];
#pragma unroll
            for (int j = 0; j < 4; ++j) W.rows[(4 * w + j) * 256 + t] = (uint16_t)(x0 >> (16 * j));
            push_word(X, x0);
        }
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < 6; ++i) {
            const int sy = wave + 4 * i, g = sy * AQ_GROUPS + 96, ln = aq_opaque(lane);
            const uint64_t v = ((const uint64_t*)W.rows)[sy * 64 + lane];      // the words of columns 4 lane .. 4 lane + 3
            const uint32_t cnt = (uint32_t)__popcll(v);
            if (__ballot(cnt != 0) == 0) { if (!emit && ln == 0) s_grp[g] = 0; continue; }      // (wave-uniform)
            const uint32_t incl = wave_incl_scan(cnt, ln);
            if (!emit) { if (ln == 63) s_grp[g] = incl; continue; }
            const AoOut so = {out + s_secoff[sy], outL + s_secoff[sy], outA + s_secoff[sy], s_grp[g] - s_grp[sy * AQ_GROUPS], s_secn[sy]};
            uint32_t n = incl - cnt;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                for (uint32_t m = (uint32_t)(v >> (16 * k)) & 0xffffu; m; m &= m - 1) {
                    const int col = 4 * lane + k, yl = __builtin_ctz(m), at = 16 * sy + yl + 384 * col;
                    aq_put(so, n++, (uint32_t)((col & 15) | (yl << 4) | ((col >> 4) << 8) | (MMGEN_QUAD_KIND_XSHAPED << 12)) | ((uint32_t)chunk[at] << 23),
                           lchunk[at] & lightMask, (uint32_t)MMGEN_AO_NONE);
                }
        }
        __syncthreads();

        // the six directions: stage F and the two combined equality masks, then three planes per two lanes
#pragma unroll 1
        for (int d = 0; d < 6; ++d) {
            const int tl = aq_opaque(t), xl = tl & 15, zl = tl >> 4;
            uint64_t a[6], er[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                a[i] = d == 0 ? F[0][i] : d == 1 ? F[1][i] : d == 2 ? F[2][i] : d == 3 ? F[3][i] : d == 4 ? F[4][i] : F[5][i];
                er[i] = (d >= 4 || (d & 1)) ? eqZ[i] : eqX[i];
            }
            const int rc = (d >= 4 || (d & 1)) ? AQ_HALO : 1;      // e_r as halo columns
            const int hc = AQ_HALO * (zl + 1) + xl + 1;    // the lane's own halo column
            if (d < 4) {    // planes z = p, rows x, stored as they are; planes x = p, rows z, stored [x][z]
                const int f = hc + AQ_HALO * ((d == 0) - (d == 2)) + (d == 1) - (d == 3);
                const bool hasPred = (d & 1) ? zl > 0 : xl > 0;
                aq_stage_side(W.rows, s_occ, a, eqY, er, aq_shifted(light, lchunk, s_nb, tl, d), f, rc, hasPred ? f - 2 * rc : f, m8,
                              (d & 1) ? 16 * xl + zl : tl);
            } else
                aq_stage_y(W.rows, s_occ, a, eqX, er, lchunk + 384 * tl, lchunk + 384 * (xl > 0 ? tl - 1 : tl), lchunk + 384 * (tl >= 16 ? tl - 16 : tl), hc,
                           xl > 0 ? hc - 1 : hc, zl > 0 ? hc - AQ_HALO : hc, m8, d == 4, xl, 16 * xl + zl);
            __syncthreads();
            const int nbd = s_nb[d & 3];
            // where the run's column c0, the plane p and the row r go in x | y << 4 | z << 8
            const int shC = d >= 4 ? 0 : 4, shP = d >= 4 ? 4 : (d & 1) ? 0 : 8, shR = (d >= 4 || (d & 1)) ? 8 : 0;
#pragma unroll 1
            for (int k = 0; k < 2; ++k) {
                const int j = lane + 64 * k, sy = j >> 2, p = 4 * (j & 3) + wave;
                if (sy >= MMGEN_SECTIONS_PER_CHUNK) continue;
                const int g = sy * AQ_GROUPS + 16 * d + p;
                const uint4* src = (const uint4*)(W.rows + sy * AQ_SY_STRIDE + 16 * p);      // 32-byte rows: [kind][p][16 r]
                const uint4 f0 = src[0], f1 = src[1];
                uint32_t n = 0;
                if ((f0.x | f0.y | f0.z | f0.w | f1.x | f1.y | f1.z | f1.w) != 0) {
                    const uint4 q0 = src[32], q1 = src[33], r0 = src[64], r1 = src[65];
                    // the walk of k_section_quads: the CURRENT row at the bottom of the registers, nothing indexed by a variable
                    uint32_t Fp[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w}, Qp[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w},
                             Rp[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
                    AoOut so = {nullptr, nullptr, nullptr, 0u, 0u};
                    if (emit) so = AoOut{out + s_secoff[sy], outL + s_secoff[sy], outA + s_secoff[sy], s_grp[g] - s_grp[sy * AQ_GROUPS], s_secn[sy]};
#pragma unroll 1
                    for (int r = 0; r < 16; ++r) {
                        uint32_t row;
                        while ((row = Fp[0] & 0xffffu) != 0) {
                            const int c0 = __builtin_ctz(row);
                            const uint32_t cont = (row & Qp[0]) >> (c0 + 1);      // < 2^15: the inverse is never zero
                            const int len = 1 + __builtin_ctz(~cont);
                            const uint32_t mk = ((1u << len) - 1u) << c0;
                            int nrows = 1;
                            bool go = true;
#pragma unroll
                            for (int kk = 1; kk < 16; ++kk) {
                                go = go && ((((Fp[kk >> 1] & Rp[kk >> 1]) >> (16 * (kk & 1))) & mk) == mk);
                                if (go) { Fp[kk >> 1] &= ~(mk << (16 * (kk & 1))); ++nrows; }
                            }
                            Fp[0] &= ~mk;
                            if (emit) {
                                // the step along the normal and e_r / e_q as halo columns and voxels along y: uniform integers of the direction,
                                // rebuilt here from an opaque copy of d (kept live across the walk they cost the fill nine more SGPRs than it has)
                                const int de = aq_uniform(d);
                                const int ndx = (de == 1) - (de == 3), ndy = (de == 4) - (de == 5), ndz = (de == 0) - (de == 2);
                                const int erc = (de >= 4 || (de & 1)) ? AQ_HALO : 1, qc = de >= 4 ? 1 : 0, qy = de >= 4 ? 0 : 1;
                                const int xyz = (c0 << shC) | (p << shP) | (r << shR), vx = xyz & 15, vz = xyz >> 8, y = 16 * sy + ((xyz >> 4) & 15);
                                aq_put(so, n, (uint32_t)(xyz | (d << 12) | ((nrows - 1) << 15) | ((len - 1) << 19)) | ((uint32_t)chunk[y + 384 * (vx + 16 * vz)] << 23),
                                       aq_face_light(light, lchunk, nbd, ndx, ndy, ndz, vx, y, vz) & lightMask,
                                       aq_face_ao(s_occ, AQ_HALO * (vz + 1 + ndz) + vx + 1 + ndx, y + ndy, erc, qc, qy));
                            }
                            ++n;
                        }
                        aq_next_row(Fp); aq_next_row(Qp); aq_next_row(Rp);
                        if ((Fp[0] | Fp[1] | Fp[2] | Fp[3] | Fp[4] | Fp[5] | Fp[6] | Fp[7]) == 0) break;
                    }
                }
                if (!emit) s_grp[g] = n;
            }
            __syncthreads();
        }

        if (FILL && pass == 0) {
            // exclusive scan of the chunk's 2 328 group counts, ten per lane
            uint32_t v[10], sum = 0;
#pragma unroll
            for (int k = 0; k < 10; ++k) { v[k] = s_grp[10 * t + k]; sum += v[k]; }
            uint32_t all;
            uint32_t run = block_incl_scan(sum, aq_opaque(t), s_wsum, &all) - sum;
#pragma unroll
            for (int k = 0; k < 10; ++k) { s_grp[10 * t + k] = run; run += v[k]; }
            __syncthreads();
        }
    }
    if (FILL) return;

    // 3 (count): lanes 8 sy .. 8 sy + 7 sum the 97 groups of section sy
    uint32_t sum = 0;
    if (t < 8 * MMGEN_SECTIONS_PER_CHUNK)
        for (int g = t & 7; g < AQ_GROUPS; g += 8) sum += s_grp[(t >> 3) * AQ_GROUPS + g];
    sum += (uint32_t)__shfl_xor((int)sum, 1); sum += (uint32_t)__shfl_xor((int)sum, 2); sum += (uint32_t)__shfl_xor((int)sum, 4);
    const bool first = (t & 7) == 0 && t < 8 * MMGEN_SECTIONS_PER_CHUNK;
    if (first) secOut[(size_t)MMGEN_SECTIONS_PER_CHUNK * o + (t >> 3)] = sum;
    uint32_t all;
    block_incl_scan(first ? sum : 0u, t, s_wsum, &all);
    if (t == 0) chunkQuads[o] = all;
}

}  // namespace mm

extern "C" {

int mmgen_mesh_ao_section_quads_count(const uint8_t* d_blocks, const uint8_t* d_light, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx8, int n,
                                      uint8_t light_mask, uint32_t* d_section_quads, uint32_t* d_chunk_quads, void* stream)
{
    if (n < 0 || (n > 0 && (!d_blocks || (!d_light && light_mask != 0) || !d_section_quads || !d_chunk_quads))) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_AO_SECTION_QUADS_COUNT, mm::k_ao_section_quads<false>, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_light, d_chunk_idx,
                     d_neighbor_idx8, (uint32_t)light_mask, (const uint32_t*)nullptr, d_section_quads, d_chunk_quads, (const uint64_t*)nullptr, 0ull,
                     (uint32_t*)nullptr, (uint8_t*)nullptr, (uint8_t*)nullptr);
    return (int)hipGetLastError();
}

int mmgen_mesh_ao_section_quads_fill(const uint8_t* d_blocks, const uint8_t* d_light, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx8, int n,
                                     uint8_t light_mask, const uint32_t* d_section_quads, const uint64_t* d_quad_offset, uint64_t capacity_quads,
                                     uint32_t* d_quads, uint8_t* d_quad_light, uint8_t* d_quad_ao, void* stream)
{
    if (n < 0 || capacity_quads == 0 ||
        (n > 0 && (!d_blocks || (!d_light && light_mask != 0) || !d_section_quads || !d_quad_offset || !d_quads || !d_quad_light || !d_quad_ao)))
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_AO_SECTION_QUADS_FILL, mm::k_ao_section_quads<true>, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_light, d_chunk_idx,
                     d_neighbor_idx8, (uint32_t)light_mask, d_section_quads, (uint32_t*)nullptr, (uint32_t*)nullptr, d_quad_offset,
                     (unsigned long long)capacity_quads, d_quads, d_quad_light, d_quad_ao);
    return (int)hipGetLastError();
}

}  // extern "C"
