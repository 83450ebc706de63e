// mmgen lit section-bucketed quad mesher for gfx950: the stream of mmgen_section_quads.hip with flat per-face light.  The light of a face is the
// light of the voxel in front of it, two faces share a quad only if they share the block id AND that light, and every record has its light byte
// in a parallel stream (contract: include/mmgen.h "lit section quad mesh", design: DESIGN.md section 6.10).
//
// k_lit_section_quads<FILL>: one workgroup (4 waves) per chunk.
//   1  as in k_section_quads: class bit planes in LDS (mm_meshclass.cuh); lane = column keeps its six face masks, its X mask and the three id
//      equality masks as 6 x u64 each in registers for the whole kernel.  No light equality is kept: 120 VGPRs are taken, and a face needs the
//      equality of the column one step along its normal, not of its own.
//   2  SIX passes, one per direction d, over one work area u16 [24 sy][F, eq along q, eq along r][16 p][16 r] (37 632 bytes, under the dead class
//      planes).  Staging a direction ANDs the id equality words with the LIGHT equality words of the shifted column, recomputed from its light
//      bytes: for a 16-voxel word in which the lane has a face, one 16-byte load of the shifted column, one of that column's predecessor along
//      the plane's rows, one byte below.  +-x / +-z: the shifted column is a neighbouring column of the chunk or the facing column of the
//      neighbour slot; +-y: the lane's own column against x - 1 and z - 1, the 16 equality bits moved by one voxel along y with the bit of the
//      adjacent word carried in (beyond the world both lights are the same constant: "equal").  Words without a face load nothing - most of a
//      chunk is rock or air.  The staged words are what k_section_quads stages, so the plane walk is that kernel's, line for line.
//   3  lane = plane: 384 planes per pass; section sy is walked by lanes 4 (sy & 15) .. + 3 of all four waves.
//   4  count / fill exactly as in k_section_quads (the traversal twice, one scan of the 2 328 group counts).  Only the emitting pass reads a
//      light byte per record: the voxel in front of the run's origin cell.
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

#define LQ_GROUPS 97                                      // per section: 16 d + p, then the kind-6 records
#define LQ_ALL (MMGEN_SECTIONS_PER_CHUNK * LQ_GROUPS)     // 2 328 per chunk
#define LQ_SCAN 2560                                      // ten per lane, zero behind LQ_ALL
#define LQ_SY_STRIDE (3 * 256 + 16)                       // u16 per section of the work area, 32 bytes of padding as in k_section_quads

struct LitClassBuf { Planes P; uint8_t cls[256]; };
union LitWork { LitClassBuf c; uint16_t rows[MMGEN_SECTIONS_PER_CHUNK * LQ_SY_STRIDE]; };      // 46 336 bytes (the class planes)

// 16 x 16 bit transposition over the 16 lanes of a row, two matrices at once (the halves of v): lane x bit y <- lane y bit x
MM_DEV uint32_t lq_transpose(uint32_t v, int x)
{
#pragma unroll
    for (int j = 8; j >= 1; j >>= 1) {
        const uint32_t m = j == 8 ? 0x00ff00ffu : j == 4 ? 0x0f0f0f0fu : j == 2 ? 0x33333333u : 0x55555555u;
        const uint32_t p = (uint32_t)__shfl_xor((int)v, j);
        v = (x & j) ? ((v & ~m) | ((p >> j) & m)) : ((v & m) | ((p & m) << j));
    }
    return v;
}

// the light column one step along d (0..3) from column t - inside the chunk, or the facing column of the neighbour slot - and that column's
// predecessor along the plane's rows (x for the +-z planes, z for the +-x planes).  Without a predecessor, or towards an absent neighbour
// (whose faces are not in F), any column of the chunk serves: the words are only ever ANDed with face rows and with id equality, both zero there.
struct LitCols { const uint8_t* at; const uint8_t* pred; };
MM_DEV LitCols lq_shifted(const uint8_t* __restrict__ light, const uint8_t* own, const int32_t* nb, int t, int d)
{
    const int x = t & 15, z = t >> 4;
    const bool inside = d == 0 ? z < 15 : d == 1 ? x < 15 : d == 2 ? z > 0 : x > 0;
    const int step = d == 0 ? 16 : d == 1 ? 1 : d == 2 ? -16 : -1;
    LitCols c;
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

// a side direction: F, id equality along y AND light equality along y of the shifted column, id equality along the rows AND light equality of
// the shifted column with its predecessor.  Rolled over the six u64, the register arrays rotate once around (see sq_stage in mmgen_section_quads.hip).
MM_DEV void lq_stage_side(uint16_t* rows, uint64_t a[6], uint64_t q[6], uint64_t r[6], const LitCols lc, uint64_t m8, int inner)
{
#pragma unroll 1
    for (int w = 0; w < 6; ++w) {
        const uint64_t a0 = a[0], q0 = q[0], r0 = r[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t f = (uint32_t)(a0 >> (16 * j)) & 0xffffu;
            uint16_t* dst = rows + (4 * w + j) * LQ_SY_STRIDE + inner;
            if (__ballot(f != 0) == 0) { dst[0] = 0; continue; }      // (wave-uniform)
            uint32_t qq = 0, rr = 0;
            if (f != 0) {
                const int k = 4 * w + j;
                const uint4 A = ((const uint4*)lc.at)[k], B = ((const uint4*)lc.pred)[k];
                const uint32_t below = k > 0 ? lc.at[16 * k - 1] : 0u;      // bit 0 of eqY is zero at y = 0
                qq = (uint32_t)(q0 >> (16 * j)) & eq_bytes16_below_masked(A, below, m8);
                rr = (uint32_t)(r0 >> (16 * j)) & eq_bytes16_masked(A, B, m8);
            }
            dst[0] = (uint16_t)f; dst[256] = (uint16_t)qq; dst[512] = (uint16_t)rr;
        }
        push_word(a, a0); push_word(q, q0); push_word(r, r0);
    }
}

// +y (UP, wave-uniform) or -y: the light one voxel above / below, own column against x - 1 (along q) and z - 1 (along r): the 16 equality bits of the aligned
// word move by one voxel, the bit of the adjacent word (or "equal" beyond the world) enters.  Then the 16 x 16 transposition of k_section_quads.
MM_DEV void lq_stage_y(uint16_t* rows, uint64_t a[6], uint64_t q[6], uint64_t r[6], const uint8_t* me, const uint8_t* mx, const uint8_t* mz, uint64_t m8,
                       const bool UP, int x, int inner)
{
    const uint32_t m1 = (uint32_t)m8 & 0xffu;
#pragma unroll 1
    for (int w = 0; w < 6; ++w) {
        const uint64_t a0 = a[0], q0 = q[0], r0 = r[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t f = (uint32_t)(a0 >> (16 * j)) & 0xffffu;
            uint16_t* dst = rows + (4 * w + j) * LQ_SY_STRIDE + inner;
            if (__ballot(f != 0) == 0) { dst[0] = 0; continue; }      // (wave-uniform: the transposition exchanges lanes)
            uint32_t qq = 0, rr = 0;
            if (f != 0) {
                const int k = 4 * w + j;
                const uint4 A = ((const uint4*)me)[k];
                uint32_t ex = eq_bytes16_masked(A, ((const uint4*)mx)[k], m8), ez = eq_bytes16_masked(A, ((const uint4*)mz)[k], m8);
                const bool in = UP ? k < 23 : k > 0;
                const int e = in ? (UP ? 16 * k + 16 : 16 * k - 1) : 0;
                const uint32_t v = me[e], bx = (!in || ((v ^ mx[e]) & m1) == 0) ? 1u : 0u, bz = (!in || ((v ^ mz[e]) & m1) == 0) ? 1u : 0u;
                if (UP) { ex = (ex >> 1) | (bx << 15); ez = (ez >> 1) | (bz << 15); }
                else { ex = ((ex << 1) & 0xffffu) | bx; ez = ((ez << 1) & 0xffffu) | bz; }
                qq = (uint32_t)(q0 >> (16 * j)) & 0xffffu & ex;
                rr = (uint32_t)(r0 >> (16 * j)) & 0xffffu & ez;
            }
            const uint32_t fq = lq_transpose(f | (qq << 16), x), r2 = lq_transpose(rr, x);
            dst[0] = (uint16_t)fq; dst[256] = (uint16_t)(fq >> 16); dst[512] = (uint16_t)r2;
        }
        push_word(a, a0); push_word(q, q0); push_word(r, r0);
    }
}

// A lane predicate (lane == 63, x > 0, lane >= 8 ..) that the compiler hoists out of the pass loop lives in TWO SGPRs for the whole kernel;
// the fill has some twenty of them and ran out of SGPRs.  A lane index that went through here is opaque, so its predicates are recomputed
// where they are used (one v_cmp each).
MM_DEV int lq_opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// the plane's 16 rows, two per u32: row 0 leaves at the bottom, zeros enter at the top
MM_DEV void lq_next_row(uint32_t m[8])
{
#pragma unroll
    for (int i = 0; i < 7; ++i) m[i] = __funnelshift_r(m[i], m[i + 1], 16);
    m[7] >>= 16;
}

// FL of a face of voxel (vx, y, vz): the light one step (dx, dy, dz) along its normal - own slot, neighbour slot nbd, or the constants beyond
// the world.  The step is three uniform integers, not a chain of conditions on d: every such condition is a lane mask in two SGPRs.
MM_DEV uint32_t lq_face_light(const uint8_t* __restrict__ light, const uint8_t* own, int nbd, int dx, int dy, int dz, int vx, int y, int vz)
{
    const int nx = vx + dx, ny = y + dy, nz = vz + dz;
    if (ny > 383) return (uint32_t)MMGEN_LIGHT_ABOVE;
    if (ny < 0) return 0u;
    if (((nx | nz) & ~15) == 0) return own[ny + 384 * (nx + 16 * nz)];
    if (nbd < 0) return 0u;                                // (a face towards an absent neighbour is not in F)
    return light[(size_t)MMGEN_BLOCKS_PER_CHUNK * nbd + ny + 384 * ((nx & 15) + 16 * (nz & 15))];
}

// where a group's records go: the section's range as counted by mmgen_mesh_lit_section_quads_count, the group's offset in it from this launch's own counts
struct LitOut { uint32_t* at; uint8_t* lt; uint32_t rel, room; };
MM_DEV void lq_put(const LitOut& o, uint32_t n, uint32_t rec, uint32_t fl)
{
    if (o.rel + n < o.room) { o.at[o.rel + n] = rec; o.lt[o.rel + n] = (uint8_t)fl; }
}

template <bool FILL>
__global__ void __launch_bounds__(256, 2)      // two workgroups per CU by LDS (2 x 57 KB of 160): up to 256 VGPRs
k_lit_section_quads(const uint8_t* __restrict__ blocks, const uint8_t* __restrict__ light, const int32_t* __restrict__ chunkIdx,
                    const int32_t* __restrict__ neighborIdx, uint32_t lightMask, const uint32_t* __restrict__ secIn, uint32_t* __restrict__ secOut,
                    uint32_t* __restrict__ chunkQuads, const uint64_t* __restrict__ quadOffset, unsigned long long capacity, uint32_t* __restrict__ quads,
                    uint8_t* __restrict__ quadLight)
{
    __shared__ __attribute__((aligned(16))) LitWork W;
    __shared__ uint32_t s_grp[LQ_SCAN];        // counting: records per group; writing: exclusive offsets over the chunk
    __shared__ uint32_t s_wsum[4];
    __shared__ uint32_t s_secoff[MMGEN_SECTIONS_PER_CHUNK], s_secn[MMGEN_SECTIONS_PER_CHUNK];
    __shared__ int32_t s_nb[4];                // the neighbours' slots, -1 = absent: read in every pass, the pointer dies after the prologue
    const int o = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, x = t & 15;
    const int c = chunkIdx ? chunkIdx[o] : o;      // o = position in the work list (outputs), c = chunk in the block and light arrays
    uint32_t* out = nullptr;
    uint8_t* outL = nullptr;
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
        if (total == 0 || base + total > capacity) return;      // (workgroup-uniform) neither array is written
        out = quads + base; outL = quadLight + base;
    }
    for (int g = LQ_ALL + t; g < LQ_SCAN; g += 256) s_grp[g] = 0;
    if (t < 4) s_nb[t] = neighborIdx ? neighborIdx[4 * o + t] : -1;      // (mesh_classify ends with a barrier)
    const uint8_t* chunk = blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * c;
    const uint8_t* lchunk = light + (size_t)MMGEN_BLOCKS_PER_CHUNK * c;
    const uint64_t m8 = mask_bytes8(lightMask);

    // 1: classes -> this column's face masks, 64 voxels per word, in registers; then the id equality masks from whole words of ids
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
    column_equal(me, (const uint4*)(chunk + 384 * (hasX ? t - 1 : t)), hasX, eqX);
    column_equal(me, (const uint4*)(chunk + 384 * (hasZ ? t - 16 : t)), hasZ, eqZ);
    __syncthreads();                                       // the class planes are dead: their LDS is the work area

    // 2: the traversal; the fill runs it twice (count into LDS, scan, write)
#pragma unroll 1
    for (int pass = 0; pass < (FILL ? 2 : 1); ++pass) {
        const bool emit = FILL && pass == 1;

        // phase X: ascending voxel index inside a section = column after column; the light of a kind-6 record is the voxel's own
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
            const int sy = wave + 4 * i, g = sy * LQ_GROUPS + 96, ln = lq_opaque(lane);
            const uint64_t v = ((const uint64_t*)W.rows)[sy * 64 + lane];      // the words of columns 4 lane .. 4 lane + 3
            const uint32_t cnt = (uint32_t)__popcll(v);
            if (__ballot(cnt != 0) == 0) { if (!emit && ln == 0) s_grp[g] = 0; continue; }      // (wave-uniform)
            const uint32_t incl = wave_incl_scan(cnt, ln);
            if (!emit) { if (ln == 63) s_grp[g] = incl; continue; }
            const LitOut so = {out + s_secoff[sy], outL + s_secoff[sy], s_grp[g] - s_grp[sy * LQ_GROUPS], s_secn[sy]};
            uint32_t n = incl - cnt;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                for (uint32_t m = (uint32_t)(v >> (16 * k)) & 0xffffu; m; m &= m - 1) {
                    const int col = 4 * lane + k, yl = __builtin_ctz(m), at = 16 * sy + yl + 384 * col;
                    lq_put(so, n++, (uint32_t)((col & 15) | (yl << 4) | ((col >> 4) << 8) | (MMGEN_QUAD_KIND_XSHAPED << 12)) | ((uint32_t)chunk[at] << 23),
                           lchunk[at] & lightMask);
                }
        }
        __syncthreads();

        // the six directions: stage F and the two combined equality masks, then three planes per two lanes
#pragma unroll 1
        for (int d = 0; d < 6; ++d) {
            // the direction's face mask and its row equality as copies chosen by the (uniform) d: ONE instance of each staging loop; the copies
            // rotate inside it and are dropped
            const int tl = lq_opaque(t), xl = tl & 15;
            uint64_t a[6], er[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                a[i] = d == 0 ? F[0][i] : d == 1 ? F[1][i] : d == 2 ? F[2][i] : d == 3 ? F[3][i] : d == 4 ? F[4][i] : F[5][i];
                er[i] = (d >= 4 || (d & 1)) ? eqZ[i] : eqX[i];
            }
            if (d < 4)      // planes z = p, rows x, stored as they are; planes x = p, rows z, stored [x][z]
                lq_stage_side(W.rows, a, eqY, er, lq_shifted(light, lchunk, s_nb, tl, d), m8, (d & 1) ? 16 * xl + (tl >> 4) : tl);
            else
                lq_stage_y(W.rows, a, eqX, er, lchunk + 384 * tl, lchunk + 384 * (xl > 0 ? tl - 1 : tl), lchunk + 384 * (tl >= 16 ? tl - 16 : tl), m8, d == 4, xl,
                           16 * xl + (tl >> 4));
            __syncthreads();
            const int nbd = s_nb[d & 3];
            // where the run's column c0, the plane p and the row r go in x | y << 4 | z << 8, and the step along the normal (all uniform)
            const int shC = d >= 4 ? 0 : 4, shP = d >= 4 ? 4 : (d & 1) ? 0 : 8, shR = (d >= 4 || (d & 1)) ? 8 : 0;
            const int ndx = (d == 1) - (d == 3), ndy = (d == 4) - (d == 5), ndz = (d == 0) - (d == 2);
#pragma unroll 1
            for (int k = 0; k < 2; ++k) {
                const int j = lane + 64 * k, sy = j >> 2, p = 4 * (j & 3) + wave;
                if (sy >= MMGEN_SECTIONS_PER_CHUNK) continue;
                const int g = sy * LQ_GROUPS + 16 * d + p;
                const uint4* src = (const uint4*)(W.rows + sy * LQ_SY_STRIDE + 16 * p);      // 32-byte rows: [kind][p][16 r]
                const uint4 f0 = src[0], f1 = src[1];
                uint32_t n = 0;
                if ((f0.x | f0.y | f0.z | f0.w | f1.x | f1.y | f1.z | f1.w) != 0) {
                    const uint4 q0 = src[32], q1 = src[33], r0 = src[64], r1 = src[65];
                    // the walk of k_section_quads: the CURRENT row at the bottom of the registers, nothing indexed by a variable
                    uint32_t Fp[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w}, Qp[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w},
                             Rp[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
                    LitOut so = {nullptr, nullptr, 0u, 0u};
                    if (emit) so = LitOut{out + s_secoff[sy], outL + s_secoff[sy], s_grp[g] - s_grp[sy * LQ_GROUPS], s_secn[sy]};
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
                                const int xyz = (c0 << shC) | (p << shP) | (r << shR), vx = xyz & 15, vz = xyz >> 8, y = 16 * sy + ((xyz >> 4) & 15);
                                lq_put(so, n, (uint32_t)(xyz | (d << 12) | ((nrows - 1) << 15) | ((len - 1) << 19)) | ((uint32_t)chunk[y + 384 * (vx + 16 * vz)] << 23),
                                       lq_face_light(light, lchunk, nbd, ndx, ndy, ndz, vx, y, vz) & lightMask);
                            }
                            ++n;
                        }
                        lq_next_row(Fp); lq_next_row(Qp); lq_next_row(Rp);
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
            uint32_t run = block_incl_scan(sum, lq_opaque(t), s_wsum, &all) - sum;
#pragma unroll
            for (int k = 0; k < 10; ++k) { s_grp[10 * t + k] = run; run += v[k]; }
            __syncthreads();
        }
    }
    if (FILL) return;

    // 3 (count): lanes 8 sy .. 8 sy + 7 sum the 97 groups of section sy
    uint32_t sum = 0;
    if (t < 8 * MMGEN_SECTIONS_PER_CHUNK)
        for (int g = t & 7; g < LQ_GROUPS; g += 8) sum += s_grp[(t >> 3) * LQ_GROUPS + g];
    sum += (uint32_t)__shfl_xor((int)sum, 1); sum += (uint32_t)__shfl_xor((int)sum, 2); sum += (uint32_t)__shfl_xor((int)sum, 4);
    const bool first = (t & 7) == 0 && t < 8 * MMGEN_SECTIONS_PER_CHUNK;
    if (first) secOut[(size_t)MMGEN_SECTIONS_PER_CHUNK * o + (t >> 3)] = sum;
    uint32_t all;
    block_incl_scan(first ? sum : 0u, t, s_wsum, &all);
    if (t == 0) chunkQuads[o] = all;
}

}  // namespace mm

extern "C" {

int mmgen_mesh_lit_section_quads_count(const uint8_t* d_blocks, const uint8_t* d_light, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n,
                                       uint8_t light_mask, uint32_t* d_section_quads, uint32_t* d_chunk_quads, void* stream)
{
    if (n < 0 || (n > 0 && (!d_blocks || !d_light || !d_section_quads || !d_chunk_quads))) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_LIT_SECTION_QUADS_COUNT, mm::k_lit_section_quads<false>, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_light, d_chunk_idx,
                     d_neighbor_idx, (uint32_t)light_mask, (const uint32_t*)nullptr, d_section_quads, d_chunk_quads, (const uint64_t*)nullptr, 0ull,
                     (uint32_t*)nullptr, (uint8_t*)nullptr);
    return (int)hipGetLastError();
}

int mmgen_mesh_lit_section_quads_fill(const uint8_t* d_blocks, const uint8_t* d_light, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n,
                                      uint8_t light_mask, const uint32_t* d_section_quads, const uint64_t* d_quad_offset, uint64_t capacity_quads,
                                      uint32_t* d_quads, uint8_t* d_quad_light, void* stream)
{
    if (n < 0 || capacity_quads == 0 || (n > 0 && (!d_blocks || !d_light || !d_section_quads || !d_quad_offset || !d_quads || !d_quad_light)))
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_LIT_SECTION_QUADS_FILL, mm::k_lit_section_quads<true>, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_light, d_chunk_idx,
                     d_neighbor_idx, (uint32_t)light_mask, d_section_quads, (uint32_t*)nullptr, (uint32_t*)nullptr, d_quad_offset,
                     (unsigned long long)capacity_quads, d_quads, d_quad_light);
    return (int)hipGetLastError();
}

}  // extern "C"
