// mmgen section-bucketed quad mesher for gfx950: the faces of a chunk merged into rectangles INSIDE each 16^3 section, one 32-bit record per
// quad, a section's records contiguous, and the device-built list of draw ranges that joins the stream to mmgen_visible_sections (contract:
// include/mmgen.h "section-bucketed quad mesh", records: include/mmgen_types.h, design: DESIGN.md section 6.9).
//
// k_section_quads<FILL>: one workgroup (4 waves) per chunk.
//   1  classify the columns into class bit planes (LDS, mm_meshclass.cuh); lane = column keeps its six face masks, its X mask and the three
//      equality masks (same id as the block at y-1 / x-1 / z-1, from whole 8-byte words of ids) as 6 x u64 each, IN REGISTERS, for the whole
//      kernel.  The planes' LDS is the work area from then on.
//   2  cut at section borders every plane of every direction is the same object: 16 rows of 16 bits.  Per section 96 of them + the X group.
//      Four phases over one work area u16 [24 sy][F a, F b, eq along q, eq along r][16 p][16 r]:
//        X  the X words as they are; a wave takes six sections, a lane four columns, one wave scan per section that has any;
//        Y  F(+y), F(-y) and eqX, eqZ, transposed by a 16 x 16 bit butterfly over the 16 lanes of a row of columns (4 lane exchanges for two
//           masks packed in a u32): lane (x, z) ends up with row z of plane y = x;
//        A  planes z = p: F(+z), F(-z), eqY, eqX, stored as they are;      B  planes x = p: F(+x), F(-x), eqY, eqZ, stored [x][z].
//      A word of a wave without a face stores zeros and skips its equality words (they are only ever ANDed with face rows).
//      Then lane = PLANE, three per lane and phase: the 16 rows are loaded into registers by two 16-byte LDS reads per mask, a run is a ctz
//      of a 16-bit row, "covered" is a cleared register bit, the rows shift down through the registers as the walk advances.  Section sy is walked by lanes 8 (sy & 7) .. + 7 of ALL four waves, so the
//      few sections that carry the surface are spread over the four SIMDs; a plane without a face costs two LDS reads.
//   3  count: the 97 group counts of a section are summed.  Fill: the SAME traversal runs twice, first counting into LDS, then - after one
//      scan of the 2 328 counts - writing every group's records at its scanned offset in emission order.  No global atomics, no sort.  A
//      section never writes beyond the records counted for it by mmgen_mesh_section_quads_count.
// k_section_draws: one workgroup; a lane takes up to five consecutive window cells, popcount(visible & nonempty) per cell, one scan over the
// lanes, then every lane writes its cells' draws in order.
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

#define SQ_GROUPS 97                                      // per section: 16 d + p, then the kind-6 records
#define SQ_ALL (MMGEN_SECTIONS_PER_CHUNK * SQ_GROUPS)     // 2 328 per chunk
#define SQ_SCAN 2560                                      // ten per lane, zero behind SQ_ALL
#define SQ_SY_STRIDE (4 * 256 + 16)                       // u16 per section of the work area; + 32 bytes: the 8 sections a wave reads at once fall on different banks

struct SecClassBuf { Planes P; uint8_t cls[256]; };
union SecWork { SecClassBuf c; uint16_t rows[MMGEN_SECTIONS_PER_CHUNK * SQ_SY_STRIDE]; };      // 49 920 bytes

// 16 x 16 bit transposition over the 16 lanes of a row, two matrices at once (the halves of v): lane x bit y <- lane y bit x
MM_DEV uint32_t sq_transpose(uint32_t v, int x)
{
#pragma unroll
    for (int j = 8; j >= 1; j >>= 1) {
        const uint32_t m = j == 8 ? 0x00ff00ffu : j == 4 ? 0x0f0f0f0fu : j == 2 ? 0x33333333u : 0x55555555u;
        const uint32_t p = (uint32_t)__shfl_xor((int)v, j);
        v = (x & j) ? ((v & ~m) | ((p >> j) & m)) : ((v & m) | ((p & m) << j));
    }
    return v;
}

// the lane's 24 words of two face masks and two equality masks into the work area at [sy][kind][inner].  The loop over the six u64 is ROLLED and
// the register arrays rotate once around (push_word): unrolled, the compiler computes the words of all phases ahead of the pass loop and spills.
template <bool TRANSPOSE>
MM_DEV void sq_stage(uint16_t* rows, uint64_t a[6], uint64_t b[6], uint64_t q[6], uint64_t r[6], int x, int inner)
{
#pragma unroll 1
    for (int w = 0; w < 6; ++w) {
        const uint64_t a0 = a[0], b0 = b[0], q0 = q[0], r0 = r[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t ab = ((uint32_t)(a0 >> (16 * j)) & 0xffffu) | ((uint32_t)(b0 >> (16 * j)) << 16);
            uint16_t* dst = rows + (4 * w + j) * SQ_SY_STRIDE + inner;
            if (__ballot(ab != 0) == 0) { dst[0] = 0; dst[256] = 0; continue; }      // (wave-uniform)
            uint32_t qr = ((uint32_t)(q0 >> (16 * j)) & 0xffffu) | ((uint32_t)(r0 >> (16 * j)) << 16);
            if (TRANSPOSE) { ab = sq_transpose(ab, x); qr = sq_transpose(qr, x); }
            dst[0] = (uint16_t)ab; dst[256] = (uint16_t)(ab >> 16); dst[512] = (uint16_t)qr; dst[768] = (uint16_t)(qr >> 16);
        }
        push_word(a, a0); push_word(b, b0); push_word(q, q0); push_word(r, r0);
    }
}

// the plane's 16 rows, two per u32: row 0 leaves at the bottom, zeros enter at the top
MM_DEV void sq_next_row(uint32_t m[8])
{
#pragma unroll
    for (int i = 0; i < 7; ++i) m[i] = __funnelshift_r(m[i], m[i + 1], 16);
    m[7] >>= 16;
}

// where a group's records go: the section's range as counted by mmgen_mesh_section_quads_count, the group's offset in it from this launch's own counts
struct SecOut { uint32_t* at; uint32_t rel, room; };
MM_DEV void sq_put(const SecOut& o, uint32_t n, uint32_t rec) { if (o.rel + n < o.room) o.at[o.rel + n] = rec; }

template <bool FILL>
__global__ void __launch_bounds__(256, 2)      // two workgroups per CU by LDS (2 x 60 KB of 160): up to 256 VGPRs
k_section_quads(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ chunkIdx, const int32_t* __restrict__ neighborIdx, const uint32_t* __restrict__ secIn,
                uint32_t* __restrict__ secOut, uint32_t* __restrict__ chunkQuads, const uint64_t* __restrict__ quadOffset, unsigned long long capacity,
                uint32_t* __restrict__ quads)
{
    __shared__ __attribute__((aligned(16))) SecWork W;
    __shared__ uint32_t s_grp[SQ_SCAN];        // counting: records per group; writing: exclusive offsets over the chunk
    __shared__ uint32_t s_wsum[4];
    __shared__ uint32_t s_secoff[MMGEN_SECTIONS_PER_CHUNK], s_secn[MMGEN_SECTIONS_PER_CHUNK];
    const int o = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, x = t & 15;
    const int c = chunkIdx ? chunkIdx[o] : o;      // o = position in the work list (outputs), c = chunk in the block array
    uint32_t* out = nullptr;
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
        if (total == 0 || base + total > capacity) return;      // (workgroup-uniform)
        out = quads + base;
    }
    for (int g = SQ_ALL + t; g < SQ_SCAN; g += 256) s_grp[g] = 0;
    const uint8_t* chunk = blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * c;

    // 1: classes -> this column's face masks, 64 voxels per word, in registers; then the equality masks from whole words of ids
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
    const uint4* me = (const uint4*)(chunk + 384 * t);
    const bool hasX = x > 0, hasZ = t >= 16;
    uint64_t eqY[6] = {}, eqX[6] = {}, eqZ[6] = {};
    column_equal_below(me, eqY);
    column_equal(me, (const uint4*)(chunk + 384 * (hasX ? t - 1 : t)), hasX, eqX);      // the columns at x - 1 and z - 1 lie 384 and 6 144 bytes before
    column_equal(me, (const uint4*)(chunk + 384 * (hasZ ? t - 16 : t)), hasZ, eqZ);
    __syncthreads();                                       // the class planes are dead: their LDS is the work area

    // 2: the traversal; the fill runs it twice (count into LDS, scan, write)
#pragma unroll 1
    for (int pass = 0; pass < (FILL ? 2 : 1); ++pass) {
        const bool emit = FILL && pass == 1;

        // phase X: ascending voxel index inside a section = column after column
#pragma unroll 1
        for (int w = 0; w < 6; ++w) {                      // (rolled, the array rotates once around: see sq_stage)
            const uint64_t x0 = X[0];
#pragma unroll
            for (int j = 0; j < 4; ++j) W.rows[(4 * w + j) * 256 + t] = (uint16_t)(x0 >> (16 * j));
            push_word(X, x0);
        }
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < 6; ++i) {
            const int sy = wave + 4 * i, g = sy * SQ_GROUPS + 96;
            const uint64_t v = ((const uint64_t*)W.rows)[sy * 64 + lane];      // the words of columns 4 lane .. 4 lane + 3
            const uint32_t cnt = (uint32_t)__popcll(v);
            if (__ballot(cnt != 0) == 0) { if (!emit && lane == 0) s_grp[g] = 0; continue; }      // (wave-uniform)
            const uint32_t incl = wave_incl_scan(cnt, lane);
            if (!emit) { if (lane == 63) s_grp[g] = incl; continue; }
            const SecOut so = {out + s_secoff[sy], s_grp[g] - s_grp[sy * SQ_GROUPS], s_secn[sy]};
            uint32_t n = incl - cnt;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                for (uint32_t m = (uint32_t)(v >> (16 * k)) & 0xffffu; m; m &= m - 1) {
                    const int col = 4 * lane + k, yl = __builtin_ctz(m);
                    sq_put(so, n++, (uint32_t)((col & 15) | (yl << 4) | ((col >> 4) << 8) | (MMGEN_QUAD_KIND_XSHAPED << 12)) |
                                        ((uint32_t)chunk[16 * sy + yl + 384 * col] << 23));
                }
        }
        __syncthreads();

        // phases Y, A, B: stage the masks, then three planes per lane
#pragma unroll 1
        for (int ph = 0; ph < 3; ++ph) {
            if (ph == 0) sq_stage<true>(W.rows, F[4], F[5], eqX, eqZ, x, 16 * x + (t >> 4));
            else if (ph == 1) sq_stage<false>(W.rows, F[0], F[2], eqY, eqX, x, t);
            else sq_stage<false>(W.rows, F[1], F[3], eqY, eqZ, x, 16 * x + (t >> 4));
            __syncthreads();
#pragma unroll 1
            for (int k = 0; k < 3; ++k) {
                const int j = lane + 64 * k, sy = j >> 3, pe = 4 * (j & 7) + wave, e = pe >> 4, p = pe & 15;
                const int d = ph == 0 ? 4 + e : 2 * e + ph - 1;
                const int g = sy * SQ_GROUPS + 16 * d + p;
                const uint4* src = (const uint4*)(W.rows + sy * SQ_SY_STRIDE + 16 * p);      // 32-byte rows: [kind][p][16 r]
                const uint4 f0 = src[32 * e], f1 = src[32 * e + 1];
                uint32_t n = 0;
                if ((f0.x | f0.y | f0.z | f0.w | f1.x | f1.y | f1.z | f1.w) != 0) {
                    const uint4 q0 = src[64], q1 = src[65], r0 = src[96], r1 = src[97];
                    // the walk keeps the CURRENT row at the bottom of the registers (row k above it is a constant position): no register is
                    // ever indexed by a variable, and the rows behind the plane's last one are zeros, which end every extension
                    uint32_t Fp[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w}, Qp[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w},
                             Rp[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
                    SecOut so = {nullptr, 0u, 0u};
                    if (emit) so = SecOut{out + s_secoff[sy], s_grp[g] - s_grp[sy * SQ_GROUPS], s_secn[sy]};
#pragma unroll 1
                    for (int r = 0; r < 16; ++r) {
                        uint32_t row;
                        while ((row = Fp[0] & 0xffffu) != 0) {
                            const int c0 = __builtin_ctz(row);
                            const uint32_t cont = (row & Qp[0]) >> (c0 + 1);      // < 2^15: the inverse is never zero
                            const int len = 1 + __builtin_ctz(~cont);
                            const uint32_t mk = ((1u << len) - 1u) << c0;
                            int rows = 1;
                            bool go = true;
#pragma unroll
                            for (int k = 1; k < 16; ++k) {
                                go = go && ((((Fp[k >> 1] & Rp[k >> 1]) >> (16 * (k & 1))) & mk) == mk);
                                if (go) { Fp[k >> 1] &= ~(mk << (16 * (k & 1))); ++rows; }
                            }
                            Fp[0] &= ~mk;
                            if (emit) {
                                const int vx = ph == 0 ? c0 : ph == 1 ? r : p, vy = ph == 0 ? p : c0, vz = ph == 1 ? p : r;
                                sq_put(so, n, (uint32_t)(vx | (vy << 4) | (vz << 8) | (d << 12) | ((rows - 1) << 15) | ((len - 1) << 19)) |
                                                  ((uint32_t)chunk[16 * sy + vy + 384 * (vx + 16 * vz)] << 23));
                            }
                            ++n;
                        }
                        sq_next_row(Fp); sq_next_row(Qp); sq_next_row(Rp);
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
            uint32_t run = block_incl_scan(sum, t, s_wsum, &all) - sum;
#pragma unroll
            for (int k = 0; k < 10; ++k) { s_grp[10 * t + k] = run; run += v[k]; }
            __syncthreads();
        }
    }
    if (FILL) return;

    // 3 (count): lanes 8 sy .. 8 sy + 7 sum the 97 groups of section sy
    uint32_t sum = 0;
    if (t < 8 * MMGEN_SECTIONS_PER_CHUNK)
        for (int g = t & 7; g < SQ_GROUPS; g += 8) sum += s_grp[(t >> 3) * SQ_GROUPS + g];
    sum += (uint32_t)__shfl_xor((int)sum, 1); sum += (uint32_t)__shfl_xor((int)sum, 2); sum += (uint32_t)__shfl_xor((int)sum, 4);
    const bool first = (t & 7) == 0 && t < 8 * MMGEN_SECTIONS_PER_CHUNK;
    if (first) secOut[(size_t)MMGEN_SECTIONS_PER_CHUNK * o + (t >> 3)] = sum;
    uint32_t all;
    block_incl_scan(first ? sum : 0u, t, s_wsum, &all);
    if (t == 0) chunkQuads[o] = all;
}

// ---------------------------------------------------------------------------------------------------------
// draw list
// ---------------------------------------------------------------------------------------------------------
#define DRAW_NT 1024
#define DRAW_K 5                                           // window cells per lane: 65 x 65 = 4 225 <= 5 x 1 024
static_assert(DRAW_K * DRAW_NT >= (2 * MMGEN_VISIBLE_MAX_RADIUS + 1) * (2 * MMGEN_VISIBLE_MAX_RADIUS + 1), "every window cell has a lane");

__global__ void __launch_bounds__(DRAW_NT)
k_section_draws(const uint32_t* __restrict__ visible, const int32_t* __restrict__ grid, int gw, int gh, int ecx, int ecz, int radius,
                const int32_t* __restrict__ meshPos, const uint32_t* __restrict__ secQuads, const uint64_t* __restrict__ quadOffset, int n, uint32_t capacity,
                mmgen_section_draw* __restrict__ draws, unsigned long long* __restrict__ totals)
{
    __shared__ uint32_t s_draws[DRAW_NT / 64];
    __shared__ unsigned long long s_quads[DRAW_NT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, Wd = 2 * radius + 1, W2 = Wd * Wd;
    const int per = (W2 + DRAW_NT - 1) / DRAW_NT;         // consecutive cells per lane: the draws of lane t precede those of lane t + 1
    int mesh[DRAW_K];
    uint32_t mask[DRAW_K], cnt = 0;
    unsigned long long nq = 0;
#pragma unroll
    for (int k = 0; k < DRAW_K; ++k) {
        const int s = t * per + k;
        mesh[k] = -1; mask[k] = 0;
        if (k >= per || s >= W2) continue;
        const int cx = ecx + s % Wd - radius, cz = ecz + s / Wd - radius;
        if (cx < 0 || cx >= gw || cz < 0 || cz >= gh) continue;
        const int slot = grid[(size_t)cz * gw + cx];
        if (slot < 0) continue;
        const int m = meshPos ? meshPos[slot] : slot;
        if (m < 0 || m >= n) continue;
        const uint32_t vis = visible[s] & 0xffffffu;
        const uint32_t* q = secQuads + (size_t)MMGEN_SECTIONS_PER_CHUNK * m;
        uint32_t ne = 0;
        if (vis)
            for (int sy = 0; sy < MMGEN_SECTIONS_PER_CHUNK; ++sy) {
                const uint32_t v = q[sy];
                if (v != 0 && ((vis >> sy) & 1u)) { ne |= 1u << sy; nq += v; }
            }
        mesh[k] = m; mask[k] = ne; cnt += (uint32_t)__popc(ne);
    }
    // exclusive scan of the draws over the 1 024 lanes, sum of the quads
    const uint32_t incl = wave_incl_scan(cnt, lane);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nq += (unsigned long long)__shfl_xor((long long)nq, d);
    if (lane == 63) { s_draws[wave] = incl; s_quads[wave] = nq; }
    __syncthreads();
    uint32_t at = incl - cnt, allDraws = 0;
    unsigned long long allQuads = 0;
#pragma unroll
    for (int w = 0; w < DRAW_NT / 64; ++w) { if (w < wave) at += s_draws[w]; allDraws += s_draws[w]; allQuads += s_quads[w]; }
    if (t == 0) { totals[0] = allDraws; totals[1] = allQuads; }
#pragma unroll
    for (int k = 0; k < DRAW_K; ++k) {
        if (mask[k] == 0) continue;
        const int s = t * per + k;
        const uint32_t* q = secQuads + (size_t)MMGEN_SECTIONS_PER_CHUNK * mesh[k];
        uint64_t first = quadOffset[mesh[k]];
        const uint32_t top = 32u - (uint32_t)__clz(mask[k]);
        for (uint32_t sy = 0; sy < top; ++sy) {
            const uint32_t v = q[sy];
            if ((mask[k] >> sy) & 1u) {
                if (at < capacity) {
                    mmgen_section_draw dr;
                    dr.first = first; dr.count = v; dr.origin = (uint32_t)(s % Wd) | ((uint32_t)(s / Wd) << 7) | (sy << 14);
                    draws[at] = dr;
                }
                ++at;
            }
            first += v;
        }
    }
}

}  // namespace mm

extern "C" {

int mmgen_mesh_section_quads_count(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n, uint32_t* d_section_quads,
                                   uint32_t* d_chunk_quads, void* stream)
{
    if (n < 0 || (n > 0 && (!d_blocks || !d_section_quads || !d_chunk_quads))) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_SECTION_QUADS_COUNT, mm::k_section_quads<false>, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_chunk_idx, d_neighbor_idx,
                     (const uint32_t*)nullptr, d_section_quads, d_chunk_quads, (const uint64_t*)nullptr, 0ull, (uint32_t*)nullptr);
    return (int)hipGetLastError();
}

int mmgen_mesh_section_quads_fill(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n, const uint32_t* d_section_quads,
                                  const uint64_t* d_quad_offset, uint64_t capacity_quads, uint32_t* d_quads, void* stream)
{
    if (n < 0 || capacity_quads == 0 || (n > 0 && (!d_blocks || !d_section_quads || !d_quad_offset || !d_quads))) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_SECTION_QUADS_FILL, mm::k_section_quads<true>, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_chunk_idx, d_neighbor_idx,
                     d_section_quads, (uint32_t*)nullptr, (uint32_t*)nullptr, d_quad_offset, (unsigned long long)capacity_quads, d_quads);
    return (int)hipGetLastError();
}

int mmgen_section_draws(const uint32_t* d_visible, const int32_t* d_grid, int grid_w, int grid_h, int eye_cx, int eye_cz, int radius, const int32_t* d_mesh_pos,
                        const uint32_t* d_section_quads, const uint64_t* d_quad_offset, int n, uint32_t capacity_draws, mmgen_section_draw* d_draws,
                        uint64_t* d_totals, void* stream)
{
    if (!d_visible || !d_grid || !d_section_quads || !d_quad_offset || !d_totals || (!d_draws && capacity_draws > 0) || n < 0) return (int)hipErrorInvalidValue;
    if (grid_w < 1 || grid_h < 1 || grid_w > 16384 || grid_h > 16384) return (int)hipErrorInvalidValue;
    if (eye_cx < 0 || eye_cx >= grid_w || eye_cz < 0 || eye_cz >= grid_h) return (int)hipErrorInvalidValue;
    if (radius < 0 || radius > MMGEN_VISIBLE_MAX_RADIUS) return (int)hipErrorInvalidValue;
    MMK_LAUNCH_NORET(mmk::KID_SECTION_DRAWS, mm::k_section_draws, dim3(1), dim3(DRAW_NT), (hipStream_t)stream, d_visible, d_grid, grid_w, grid_h, eye_cx, eye_cz,
                     radius, d_mesh_pos, d_section_quads, d_quad_offset, n, capacity_draws, d_draws, (unsigned long long*)d_totals);
    return (int)hipGetLastError();
}

}  // extern "C"
