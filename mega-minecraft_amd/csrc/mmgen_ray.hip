// mmgen ray caster for gfx950: line of sight, block picking and a headless camera over blocks that stay in HBM (a region's output or
// RegionTerrain's pool).  The reference's only consumer of a chunk is OptixRenderer::buildChunkAccel (RT cores); an MI355X has none, so
// this is a software traversal whose RESULT is fixed by the one-voxel-at-a-time contract of include/mmgen.h and whose SPEED comes from a
// three-level skip structure that provably returns the same records.
//
//   k_ray_occupancy    one workgroup per chunk, one lane per column (as the mesher): a column's 24 16-byte words are its 24 sections,
//                      a word's 4 dwords its 4 y-bricks.  A wave holds 16 x 4 columns = the 4 x-bricks of ONE z-brick, so a brick's
//                      16 columns are a lane mask of one ballot: 4 ballots per section and wave give 16 brick bits, the 4 waves' parts
//                      meet in LDS.  200 bytes per chunk: u64 section mask (24 bits used), 24 x u64 brick masks, bit = by + 4 (bx + 4 bz).
//   k_raycast          one ray per lane from a [n][6] batch;  k_raycast_camera: a wave owns an 8 x 8 pixel tile (coherent rays: the lanes
//                      of a wave descend into the same sections and bricks), a workgroup a 16 x 16 block.  Both stage the chunk-grid table
//                      and the grid's section masks in LDS (32 KB for 64 x 64 chunks; larger grids read them from global memory) together
//                      with a 256-bit "does this block id stop the ray" table; brick masks (8 bytes) and block bytes come from global memory.
//
// The walk itself (trace, land, the LDS tables) lives in mm_raywalk.cuh, shared with the shaded camera render (mmgen_render.hip).
#include "mm_raywalk.cuh"
#include "mmgen_prof.h"

namespace mm {

// ---------------------------------------------------------------------------------------------------------
// occupancy
// ---------------------------------------------------------------------------------------------------------
// bit k = y-brick k (dword k: voxels 4k .. 4k+3 of the section) of this column holds a stopping block
MM_DEV uint32_t word_stop_nibble(const uint4& v, const uint32_t* s_stop)
{
    // terrain is long vertical runs: most words hold one block id 16 times - one lookup instead of 16
    if (v.x == v.y && v.x == v.z && v.x == v.w && v.x == ((v.x << 8) | (v.x >> 24))) return stops(s_stop, v.x & 255u) ? 15u : 0u;
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    uint32_t nib = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t any = stops(s_stop, q[k] & 255u) | stops(s_stop, (q[k] >> 8) & 255u) | stops(s_stop, (q[k] >> 16) & 255u) | stops(s_stop, q[k] >> 24);
        nib |= any << k;
    }
    return nib;
}

__global__ void __launch_bounds__(256)
k_ray_occupancy(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ chunkIdx, uint32_t stopMask, uint8_t* __restrict__ occ)
{
    __shared__ uint32_t s_stop[8];
    __shared__ uint16_t s_part[24][4];                    // [section][z-brick = wave]: 16 bits by + 4 bx
    const int t = threadIdx.x, wave = t >> 6;
    const int c = chunkIdx ? chunkIdx[blockIdx.x] : (int)blockIdx.x;
    build_stop_table(stopMask, s_stop);
    __syncthreads();
    const uint4* col = (const uint4*)(blocks + (size_t)MMGEN_BLOCKS_PER_CHUNK * c + 384 * t);
    for (int w0 = 0; w0 < 24; w0 += 8) {                  // 8 independent 16-byte loads in flight per lane, as the mesher
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = col[w0 + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t nib = word_stop_nibble(v[k], s_stop);
            uint32_t part = 0;
#pragma unroll
            for (int by = 0; by < 4; ++by) {
                const unsigned long long b = __ballot((nib >> by) & 1u);
#pragma unroll
                for (int bx = 0; bx < 4; ++bx)            // x-brick bx = lanes with ((lane & 15) >> 2) == bx, all four z rows of the wave
                    if (b & (0x000F000F000F000Full << (4 * bx))) part |= 1u << (by + 4 * bx);
            }
            if ((t & 63) == 0) s_part[w0 + k][wave] = (uint16_t)part;
        }
    }
    __syncthreads();
    if (t < 64) {
        unsigned long long m = 0;
        if (t < 24) m = (unsigned long long)s_part[t][0] | ((unsigned long long)s_part[t][1] << 16) | ((unsigned long long)s_part[t][2] << 32) | ((unsigned long long)s_part[t][3] << 48);
        unsigned long long* out = (unsigned long long*)(occ + (size_t)MMGEN_RAY_OCCUPANCY_BYTES * c);
        if (t < 24) out[1 + t] = m;
        const unsigned long long sec = __ballot(m != 0ull);
        if (t == 0) out[0] = sec;
    }
}

template <bool STAGED>
__global__ void __launch_bounds__(256)
k_raycast(RayScene sc, const float* __restrict__ rays, int n, mmgen_ray_hit* __restrict__ hits)
{
    __shared__ int32_t s_grid[STAGED ? RAY_LDS_CELLS : 1];
    __shared__ uint32_t s_sec[STAGED ? RAY_LDS_CELLS : 1];
    __shared__ uint32_t s_stop[8];
    stage_tables<STAGED>(sc, s_grid, s_sec, s_stop);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float2* r = (const float2*)(rays + 6 * i);
        const float2 a = r[0], b = r[1], c = r[2];
        const float o[3] = {a.x, a.y, b.x}, d[3] = {b.y, c.x, c.y};
        trace<STAGED>(sc, s_grid, s_sec, s_stop, o, d, (uint32_t*)(hits + i));
    }
}

template <bool STAGED>
__global__ void __launch_bounds__(256)
k_raycast_camera(RayScene sc, CamBasis cb, mmgen_ray_hit* __restrict__ hits)
{
    __shared__ int32_t s_grid[STAGED ? RAY_LDS_CELLS : 1];
    __shared__ uint32_t s_sec[STAGED ? RAY_LDS_CELLS : 1];
    __shared__ uint32_t s_stop[8];
    stage_tables<STAGED>(sc, s_grid, s_sec, s_stop);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = 16 * (int)blockIdx.x + 8 * (wave & 1) + (lane & 7), j = 16 * (int)blockIdx.y + 8 * (wave >> 1) + (lane >> 3);
    if (i >= cb.width || j >= cb.height) return;
    float d[3];
    cam_dir(cb, i, j, d);
    trace<STAGED>(sc, s_grid, s_sec, s_stop, cb.eye, d, (uint32_t*)(hits + (size_t)j * cb.width + i));
}

}  // namespace mm

extern "C" {

int mmgen_ray_occupancy(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, unsigned stop_mask, uint8_t* d_occupancy, void* stream)
{
    if (n < 0 || stop_mask == 0u || stop_mask > 15u || (n > 0 && (!d_blocks || !d_occupancy))) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    MMK_LAUNCH_NORET(mmk::KID_RAY_OCCUPANCY, mm::k_ray_occupancy, dim3(n), dim3(256), (hipStream_t)stream, d_blocks, d_chunk_idx, (uint32_t)stop_mask, d_occupancy);
    return (int)hipGetLastError();
}

int mmgen_raycast(const uint8_t* d_blocks, const int32_t* d_grid, int grid_w, int grid_h, const uint8_t* d_occupancy, unsigned stop_mask, unsigned flags,
                  const float* d_rays, int n, float t_max, mmgen_ray_hit* d_hits, void* stream)
{
    mm::RayScene sc;
    if (int e = mm::ray_scene(sc, d_blocks, d_grid, grid_w, grid_h, d_occupancy, stop_mask, flags, t_max)) return e;
    if (n < 0 || (n > 0 && (!d_rays || !d_hits))) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const int cus = mmk::device_cus();
    int wgs = (n + 255) / 256;
    if (cus > 0 && wgs > 8 * cus) wgs = 8 * cus;          // a workgroup stages the tables once and strides over the batch
    if (grid_w * grid_h <= RAY_LDS_CELLS)
        MMK_LAUNCH_NORET(mmk::KID_RAYCAST, mm::k_raycast<true>, dim3(wgs), dim3(256), (hipStream_t)stream, sc, d_rays, n, d_hits);
    else
        MMK_LAUNCH_NORET(mmk::KID_RAYCAST, mm::k_raycast<false>, dim3(wgs), dim3(256), (hipStream_t)stream, sc, d_rays, n, d_hits);
    return (int)hipGetLastError();
}

int mmgen_raycast_camera(const uint8_t* d_blocks, const int32_t* d_grid, int grid_w, int grid_h, const uint8_t* d_occupancy, unsigned stop_mask, unsigned flags,
                         const mmgen_camera* cam, float t_max, mmgen_ray_hit* d_hits, void* stream)
{
    mm::RayScene sc;
    if (int e = mm::ray_scene(sc, d_blocks, d_grid, grid_w, grid_h, d_occupancy, stop_mask, flags, t_max)) return e;
    mm::CamBasis cb;
    if (!d_hits) return (int)hipErrorInvalidValue;
    if (int e = mm::cam_basis(cb, cam)) return e;
    const dim3 grid((cam->width + 15) / 16, (cam->height + 15) / 16);
    if (grid_w * grid_h <= RAY_LDS_CELLS)
        MMK_LAUNCH_NORET(mmk::KID_RAYCAST_CAMERA, mm::k_raycast_camera<true>, grid, dim3(256), (hipStream_t)stream, sc, cb, d_hits);
    else
        MMK_LAUNCH_NORET(mmk::KID_RAYCAST_CAMERA, mm::k_raycast_camera<false>, grid, dim3(256), (hipStream_t)stream, sc, cb, d_hits);
    return (int)hipGetLastError();
}

}  // extern "C"
