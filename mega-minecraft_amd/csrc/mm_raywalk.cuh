// The contract walk of include/mmgen.h ("THE TRAVERSAL CONTRACT") with its three-level skip structure, its LDS tables and the host-side
// argument checks: shared by the ray caster (mmgen_ray.hip) and the shaded camera render (mmgen_render.hip).  DESIGN.md section 6.5.
//
// The walk: classify the voxel the ray is in - outside the grid / absent chunk / stopping block end it - and otherwise name the largest
// known-empty box around it: the slab above or below the world, the vertical RUN of empty sections of its chunk, its empty 4^3 brick, or
// the voxel itself.  Leave that box through the face whose plane has the smallest ((float)plane - o) * inv (the expression the contract
// evaluates at that very plane), and on the two other axes count the planes the contract would have crossed before it (land()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "mm_math.cuh"
#include "mm_blockdata.cuh"
#include "../../include/mmgen.h"

namespace mm {

#define RAY_FAR (1 << 22)      // y extent of the slabs above / below the world: beyond any origin (|y| < 1 408 + steps), exact in f32
#define RAY_LDS_CELLS 4096     // grids of up to 64 x 64 chunks are staged in LDS

struct RayScene {
    const uint8_t* blocks; const int32_t* grid; const uint8_t* occ;
    int gw, gh; uint32_t stopMask, flags; float tMax;
};
struct CamBasis { float eye[3], f[3], r[3], u[3]; float sx2, sy2; int width, height; };

// block class bit (mmgen.h MMGEN_RAY_*): AIR none; else 1 << transparency of mm_blockdata.cuh; ids beyond the enum are OPAQUE like the mesher's
MM_DEV uint32_t ray_class_bit(int id) { return id == MMB_AIR ? 0u : (id < MMB_NUM_BLOCKS ? 1u << (kBlockData[id] >> 30) : 1u); }

// s_stop: 256 bits, bit id = "block id stops the ray".  Workgroup of 256 lanes, lane t classifies id t; no barrier here.
MM_DEV void build_stop_table(uint32_t stopMask, uint32_t* s_stop)
{
    const int t = threadIdx.x;
    const unsigned long long b = __ballot((ray_class_bit(t) & stopMask) != 0u);
    if ((t & 63) == 0) { s_stop[2 * (t >> 6)] = (uint32_t)b; s_stop[2 * (t >> 6) + 1] = (uint32_t)(b >> 32); }
}
MM_DEV uint32_t stops(const uint32_t* s_stop, uint32_t id) { return (s_stop[id >> 5] >> (id & 31u)) & 1u; }

MM_DEV bool ray_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

MM_DEV void write_hit(uint32_t* out, int vx, int vy, int vz, float t, uint32_t block, uint32_t face, uint32_t status)
{
    out[0] = (uint32_t)vx; out[1] = (uint32_t)vy; out[2] = (uint32_t)vz; out[3] = __float_as_uint(t);
    out[4] = block | (face << 8) | (status << 16);
}

// Where the contract's walk stands on axis b (sign sb != 0) once it has crossed every plane of the box [lo, hi) whose
// t = ((float)p - ob) * invb lies below T (incl: at or below): the expression is monotone in p along the direction of travel, so the
// float estimate floor(ob + T db) only has to be corrected until the exact predicate flips - one step in practice, never past the box.
MM_DEV int land(float ob, float db, float invb, int sb, int vb, int lo, int hi, float T, bool incl)
{
    auto crossed = [&](int p) { const float tp = ((float)p - ob) * invb; return incl ? tp <= T : tp < T; };
    const float est = floorf(ob + T * db);
    if (sb > 0) {                                          // voxel c > vb is reached iff plane c is crossed
        int c = (int)fminf(fmaxf(est, (float)vb), (float)(hi - 1));
        while (c < hi - 1 && crossed(c + 1)) ++c;
        while (c > vb && !crossed(c)) --c;
        return c;
    }
    int c = (int)fminf(fmaxf(est, (float)lo), (float)vb);  // voxel c < vb is reached iff plane c + 1 is crossed
    while (c > lo && crossed(c)) --c;
    while (c < vb && !crossed(c + 1)) ++c;
    return c;
}

template <bool STAGED>
MM_DEV void trace(const RayScene& sc, const int32_t* s_grid, const uint32_t* s_sec, const uint32_t* s_stop, const float o[3], const float d[3],
                  uint32_t* out)
{
    const int W = 16 * sc.gw, H = 16 * sc.gh;
    const bool noSkip = sc.flags & MMGEN_RAY_NO_SKIP, count = sc.flags & MMGEN_RAY_COUNT_VISITS;
    float inv[3];
    int s[3], v[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        s[a] = d[a] > 0.f ? 1 : (d[a] < 0.f ? -1 : 0);
        inv[a] = s[a] ? 1.0f / d[a] : 0.f;
        ok = ok && ray_finite(o[a]) && ray_finite(d[a]) && ray_finite(inv[a]);
    }
    ok = ok && (s[0] | s[1] | s[2]) && o[0] >= 0.f && o[0] < (float)W && o[2] >= 0.f && o[2] < (float)H && o[1] >= -1024.f && o[1] < 1408.f;
    if (!ok) { write_hit(out, 0, 0, 0, 0.f, 0u, MMGEN_RAY_FACE_NONE, MMGEN_RAY_INVALID); return; }
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = (int)floorf(o[a]);
    float t = 0.f;
    uint32_t face = MMGEN_RAY_FACE_NONE, nVoxel = 0, nBrick = 0;
    // every iteration moves at least one voxel along the ray and the walk ends outside the grid: W + H + 1 409 steps at most
    const int maxIter = W + H + 4096;
    for (int it = 0; it < maxIter; ++it) {
        // ---- classify the voxel: a status ends the ray, otherwise [lo, hi) is a box around it that holds nothing that stops it
        int lo[3], hi[3], status = -1;
        uint32_t block = 0;
        bool fine = false;                                 // the box is the voxel itself
        if (v[0] < 0 || v[0] >= W || v[2] < 0 || v[2] >= H) status = MMGEN_RAY_LEFT_GRID;
        else if ((v[1] < 0 && s[1] <= 0) || (v[1] >= MMGEN_CHUNK_HEIGHT && s[1] >= 0)) status = MMGEN_RAY_LEFT_GRID;
        else if (v[1] < 0 || v[1] >= MMGEN_CHUNK_HEIGHT) {
            lo[0] = 0; hi[0] = W; lo[2] = 0; hi[2] = H;
            lo[1] = v[1] < 0 ? -RAY_FAR : MMGEN_CHUNK_HEIGHT; hi[1] = v[1] < 0 ? 0 : RAY_FAR;
            fine = noSkip;
        } else {
            const int cell = (v[2] >> 4) * sc.gw + (v[0] >> 4);
            const int g = STAGED ? s_grid[cell] : sc.grid[cell];
            if (g < 0) status = MMGEN_RAY_ABSENT_CHUNK;
            else {
                const uint8_t* chunkOcc = sc.occ + (size_t)MMGEN_RAY_OCCUPANCY_BYTES * g;
                const int sy = v[1] >> 4;
                bool read = noSkip;
                if (!noSkip) {
                    const uint32_t sec = STAGED ? s_sec[cell] : *(const uint32_t*)chunkOcc;
                    if (!((sec >> sy) & 1u)) {             // the run of empty sections around sy, in this chunk's 16 x 16 footprint
                        const uint32_t below = sec & ((1u << sy) - 1u), above = sec >> sy;
                        lo[0] = v[0] & ~15; hi[0] = lo[0] + 16; lo[2] = v[2] & ~15; hi[2] = lo[2] + 16;
                        lo[1] = below ? 16 * (32 - __clz((int)below)) : 0;
                        hi[1] = above ? 16 * (sy + __ffs((int)above) - 1) : MMGEN_CHUNK_HEIGHT;
                    } else {
                        const unsigned long long brick = ((const unsigned long long*)chunkOcc)[1 + sy];
                        ++nBrick;
                        const int bit = ((v[1] >> 2) & 3) + 4 * (((v[0] >> 2) & 3) + 4 * ((v[2] >> 2) & 3));
                        if (!((brick >> bit) & 1ull)) {
#pragma unroll
                            for (int a = 0; a < 3; ++a) { lo[a] = v[a] & ~3; hi[a] = lo[a] + 4; }
                        } else read = true;
                    }
                }
                if (read) {
                    block = sc.blocks[(size_t)MMGEN_BLOCKS_PER_CHUNK * g + v[1] + MMGEN_CHUNK_HEIGHT * ((v[0] & 15) + 16 * (v[2] & 15))];
                    ++nVoxel;
                    if (stops(s_stop, block)) status = MMGEN_RAY_HIT;
                    fine = true;
                }
            }
        }
        if (status >= 0) {
            if (status != MMGEN_RAY_HIT) block = 0;
            if (count) write_hit(out, (int)nVoxel, it, (int)nBrick, t, block, face, (uint32_t)status);
            else write_hit(out, v[0], v[1], v[2], t, block, face, (uint32_t)status);
            return;
        }
        if (fine) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = v[a]; hi[a] = v[a] + 1; }
        }
        // ---- leave the box: the exit plane is the contract's next plane of that axis once the walk has reached it
        float tE = 0.f;
        int aE = -1;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (s[a]) {
                const float ta = ((float)(s[a] > 0 ? hi[a] : lo[a]) - o[a]) * inv[a];
                if (aE < 0 || ta < tE) { tE = ta; aE = a; }
            }
        const bool miss = tE > sc.tMax;                    // the contract stops in front of the first plane beyond t_max
        const float T = miss ? sc.tMax : tE;
        const int aX = miss ? 3 : aE;                      // planes of a lower axis win ties against the exit plane, planes of a higher one lose
        if (!fine) {
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (s[b] && b != aX) v[b] = land(o[b], d[b], inv[b], s[b], v[b], lo[b], hi[b], T, b < aX);
        }
        if (miss) {
            if (count) write_hit(out, (int)nVoxel, it + 1, (int)nBrick, sc.tMax, 0u, MMGEN_RAY_FACE_NONE, MMGEN_RAY_MISS_TMAX);
            else write_hit(out, v[0], v[1], v[2], sc.tMax, 0u, MMGEN_RAY_FACE_NONE, MMGEN_RAY_MISS_TMAX);
            return;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (a == aE) v[a] = s[a] > 0 ? hi[a] : lo[a] - 1;
        t = tE;
        // dirVecs index of the outward normal of the face entered: stepping +x enters through -x (3), -x through +x (1), ...
        face = aE == 0 ? (s[0] > 0 ? 3u : 1u) : (aE == 1 ? (s[1] > 0 ? 5u : 4u) : (s[2] > 0 ? 2u : 0u));
    }
    write_hit(out, 0, 0, 0, 0.f, 0u, MMGEN_RAY_FACE_NONE, MMGEN_RAY_INVALID);      // not reachable (see maxIter)
}

// chunk-grid table + the grid's section masks -> LDS (STAGED), stop table; ends with a barrier
template <bool STAGED>
MM_DEV void stage_tables(const RayScene& sc, int32_t* s_grid, uint32_t* s_sec, uint32_t* s_stop)
{
    build_stop_table(sc.stopMask, s_stop);
    if (STAGED)
        for (int c = threadIdx.x; c < sc.gw * sc.gh; c += 256) {
            const int g = sc.grid[c];
            s_grid[c] = g;
            s_sec[c] = g >= 0 ? *(const uint32_t*)(sc.occ + (size_t)MMGEN_RAY_OCCUPANCY_BYTES * g) : 0u;
        }
    __syncthreads();
}

// ---- host side: what every ray entry point rejects, and the camera's basis
inline int ray_scene(RayScene& sc, const uint8_t* d_blocks, const int32_t* d_grid, int grid_w, int grid_h, const uint8_t* d_occupancy, unsigned stop_mask,
                     unsigned flags, float t_max)
{
    if (!d_blocks || !d_grid || !d_occupancy || grid_w < 1 || grid_h < 1 || grid_w > 16384 || grid_h > 16384) return (int)hipErrorInvalidValue;
    if (stop_mask == 0u || stop_mask > 15u || (flags & ~(MMGEN_RAY_NO_SKIP | MMGEN_RAY_COUNT_VISITS)) || !(t_max >= 0.f) || !(t_max <= 3.4028234e38f))
        return (int)hipErrorInvalidValue;
    sc = RayScene{d_blocks, d_grid, d_occupancy, grid_w, grid_h, (uint32_t)stop_mask, (uint32_t)flags, t_max};
    return 0;
}

inline int cam_basis(CamBasis& cb, const mmgen_camera* cam)
{
    if (!cam || cam->width < 1 || cam->height < 1 || cam->width > 16384 || cam->height > 16384) return (int)hipErrorInvalidValue;
    // the basis in double, rounded once (mmgen.h): f = forward / |forward|, r = f x up / |f x up|, u = r x f
    const double fw[3] = {cam->forward[0], cam->forward[1], cam->forward[2]}, up[3] = {cam->up[0], cam->up[1], cam->up[2]};
    const double fl = sqrt(fw[0] * fw[0] + fw[1] * fw[1] + fw[2] * fw[2]);
    if (!(fl > 0.0) || !(fl < INFINITY) || !(cam->fov_y > 0.f) || !(cam->fov_y < 3.1415925f)) return (int)hipErrorInvalidValue;
    const double f[3] = {fw[0] / fl, fw[1] / fl, fw[2] / fl};
    const double r0[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    const double rl = sqrt(r0[0] * r0[0] + r0[1] * r0[1] + r0[2] * r0[2]);
    if (!(rl > 0.0) || !(rl < INFINITY)) return (int)hipErrorInvalidValue;
    const double r[3] = {r0[0] / rl, r0[1] / rl, r0[2] / rl};
    const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
    const double th = tan(0.5 * (double)cam->fov_y), tha = th * ((double)cam->width / (double)cam->height);
    for (int a = 0; a < 3; ++a) { cb.eye[a] = cam->eye[a]; cb.f[a] = (float)f[a]; cb.r[a] = (float)(r[a] * tha); cb.u[a] = (float)(u[a] * th); }
    cb.sx2 = 2.0f / (float)cam->width; cb.sy2 = 2.0f / (float)cam->height; cb.width = cam->width; cb.height = cam->height;
    return 0;
}

// direction of pixel (i, j): the header's formula, no contraction
MM_DEV void cam_dir(const CamBasis& cb, int i, int j, float d[3])
{
    const float fx = ((float)i + 0.5f) * cb.sx2 - 1.0f, fy = 1.0f - ((float)j + 0.5f) * cb.sy2;
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = (cb.f[a] + fx * cb.r[a]) + fy * cb.u[a];
}

}  // namespace mm
