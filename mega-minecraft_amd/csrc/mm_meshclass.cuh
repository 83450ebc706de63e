// Block classes and face visibility as bit arithmetic, shared by the two meshers (mmgen_mesh.hip: the reference-exact vertex stream,
// mmgen_quads.hip: the greedy-merged quad stream).  Moved verbatim out of mmgen_mesh.hip; the mesher's byte-exact tests pin it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mm_math.cuh"
#include "mm_blockdata.cuh"
#include "../../include/mmgen.h"

namespace mm {

#define MESH_TRANS(d) ((d) >> 30)
enum { T_OPAQUE = 0, T_SEMI = 1, T_TRANSPARENT = 2, T_XSHAPED = 3 };

// ---------------------------------------------------------------------------------------------------------
// Face visibility as bit arithmetic.  Every block belongs to one of five classes (AIR, OPAQUE, SEMI_TRANSPARENT, TRANSPARENT,
// X_SHAPED) and the display rule of chunk.cu:1912-1928 only looks at classes:
//     opaque / semi-transparent block : face shows  <=>  neighbour is not OPAQUE
//     transparent block               : face shows  <=>  neighbour is AIR or SEMI_TRANSPARENT
// So each column is classified ONCE into three bit planes of its class code per 16-voxel word (LDS, 3 x 16 bits per word), the
// facing border column of a present neighbour chunk likewise, and the six face masks of a word are a handful of AND / OR / shifts
// on 16-bit masks - instead of 98 304 x 6 table lookups and branches per chunk.  Only voxels that really emit a quad are visited.
// ---------------------------------------------------------------------------------------------------------
enum { C_AIR = 0, C_OPAQUE = 1, C_SEMI = 2, C_TRANS = 3, C_XSHAPED = 4 };
#define MESH_COLS 320                                     // 256 own columns + 4 x 16 facing border columns of the neighbour chunks
struct Planes { uint16_t p0[MESH_COLS][24], p1[MESH_COLS][24], p2[MESH_COLS][24]; };      // 46 080 bytes

MM_DEV void classify_word(const uint4& v, const uint8_t* s_cls, Planes& P, int slot, int w)
{
    // terrain is long vertical runs: most words hold one block id 16 times - one lookup instead of 16
    if (v.x == v.y && v.x == v.z && v.x == v.w && v.x == ((v.x << 8) | (v.x >> 24))) {
        const uint32_t cls = s_cls[v.x & 255u];
        P.p0[slot][w] = (cls & 1u) ? 0xffffu : 0u; P.p1[slot][w] = (cls & 2u) ? 0xffffu : 0u; P.p2[slot][w] = (cls & 4u) ? 0xffffu : 0u;
        return;
    }
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    uint32_t a = 0, b = 0, c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t cls = s_cls[(q[k] >> (8 * j)) & 255u];
            const int i = 4 * k + j;
            a |= (cls & 1u) << i; b |= ((cls >> 1) & 1u) << i; c |= (cls >> 2) << i;
        }
    P.p0[slot][w] = (uint16_t)a; P.p1[slot][w] = (uint16_t)b; P.p2[slot][w] = (uint16_t)c;
}

MM_DEV void classify_column(const uint8_t* __restrict__ col, const uint8_t* s_cls, Planes& P, int slot)
{
    // 8 independent 16-byte loads in flight per lane (a load-use-load chain would cost 24 memory latencies per column)
    for (int w0 = 0; w0 < 24; w0 += 8) {
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = ((const uint4*)col)[w0 + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) classify_word(v[k], s_cls, P, slot, w0 + k);
    }
}

struct WordMasks { uint32_t opq, semi, air, trn, xsh; };
MM_DEV WordMasks word_masks(const Planes& P, int slot, int w)
{
    const uint32_t a = P.p0[slot][w], b = P.p1[slot][w], c = P.p2[slot][w];
    WordMasks m;
    m.opq = a & ~b & ~c; m.semi = ~a & b & ~c & 0xffffu; m.air = ~(a | b | c) & 0xffffu; m.trn = a & b; m.xsh = c;
    return m;
}

// the six face masks (dirVecs order: +z, +x, -z, -x, +y, -y) and the X mask of word w of column t
struct WordFaces { uint32_t f[6], xsh; };
MM_DEV WordFaces word_faces(const Planes& P, int t, int w, const int nbSlot[4], const bool nbPresent[4])
{
    const WordMasks me = word_masks(P, t, w);
    const uint32_t solidish = me.opq | me.semi;
    WordFaces r;
    r.xsh = me.xsh;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (!nbPresent[d]) { r.f[d] = 0; continue; }      // neighbouring chunk absent: the face is skipped (chunk.cu:1906-1909)
        const WordMasks nb = word_masks(P, nbSlot[d], w);
        r.f[d] = (solidish & ~nb.opq) | (me.trn & (nb.air | nb.semi));
    }
    // vertical neighbours: the column itself shifted by one voxel; beyond the world (y = -1, 384) the face always shows, which is
    // what a virtual AIR neighbour gives under both rules
    uint32_t upOpq = me.opq >> 1, upAir = me.air >> 1, upSemi = me.semi >> 1;
    if (w < 23) { const WordMasks n = word_masks(P, t, w + 1); upOpq |= (n.opq & 1u) << 15; upAir |= (n.air & 1u) << 15; upSemi |= (n.semi & 1u) << 15; }
    else upAir |= 1u << 15;
    uint32_t dnOpq = (me.opq << 1) & 0xffffu, dnAir = (me.air << 1) & 0xffffu, dnSemi = (me.semi << 1) & 0xffffu;
    if (w > 0) { const WordMasks n = word_masks(P, t, w - 1); dnOpq |= n.opq >> 15; dnAir |= n.air >> 15; dnSemi |= n.semi >> 15; }
    else dnAir |= 1u;
    r.f[4] = (solidish & ~upOpq) | (me.trn & (upAir | upSemi));
    r.f[5] = (solidish & ~dnOpq) | (me.trn & (dnAir | dnSemi));
    return r;
}

// workgroup-wide: block class table, own columns, facing border columns of the present neighbour chunks.  Ends with a barrier.
MM_DEV void mesh_classify(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ neighborIdx, int o, int c, uint8_t* s_cls, Planes& P,
                          int nbSlot[4], bool nbPresent[4])
{
    const int t = threadIdx.x, x = t & 15, z = t >> 4;
    if (t < MMB_NUM_BLOCKS) {
        const int tr = MESH_TRANS(kBlockData[t]);
        s_cls[t] = (uint8_t)(t == MMB_AIR ? C_AIR : (tr == T_OPAQUE ? C_OPAQUE : (tr == T_SEMI ? C_SEMI : (tr == T_TRANSPARENT ? C_TRANS : C_XSHAPED))));
    }
    if (t >= MMB_NUM_BLOCKS) s_cls[t] = C_OPAQUE;         // ids beyond the enum never occur; BlockData{} default is OPAQUE (block.hpp)
    __syncthreads();
    const uint8_t* base = blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * c;
    classify_column(base + 384 * t, s_cls, P, t);
    // neighbour of (x, z) in direction d: inside the chunk, or border slot 256 + 16 d + (position along the edge)
    const int inside[4] = {z < 15, x < 15, z > 0, x > 0};
    const int insideSlot[4] = {t + 16, t + 1, t - 16, t - 1};
    const int along[4] = {x, z, x, z};
    const int facing[4] = {x + 16 * 0, 0 + 16 * z, x + 16 * 15, 15 + 16 * z};      // the neighbour chunk's column that touches this one
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (inside[d]) { nbSlot[d] = insideSlot[d]; nbPresent[d] = true; continue; }
        const int n = neighborIdx ? neighborIdx[4 * o + d] : -1;
        nbSlot[d] = 256 + 16 * d + along[d];
        nbPresent[d] = n >= 0;
        if (n >= 0) classify_column(blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * n + 384 * facing[d], s_cls, P, nbSlot[d]);
    }
    __syncthreads();
}

}  // namespace mm
