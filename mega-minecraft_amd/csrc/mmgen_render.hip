// mmgen shaded camera render for gfx950: camera -> RGBA8 in one launch, over blocks, light and occupancy that stay in HBM.  The contract
// (walks A, B, S; integer shading; the AO factor; the pixel) is in include/mmgen.h "shaded camera render"; DESIGN.md section 6.13.
//
//   k_render_camera    the tiling of k_raycast_camera: a workgroup is a 16 x 16 pixel tile, a wave an 8 x 8 tile, lane = pixel.
//     1  walk A: every lane traces its camera ray (mm_raywalk.cuh, grid table and section masks of occ_first staged in LDS) and keeps
//        the record in registers; d_hits gets it as mmgen_raycast_camera would write it.
//     2  secondary rays - walk B of a pixel that hit a TRANSPARENT block, walk S of a pixel that hit a face - are needed by SOME lanes,
//        scattered over the tile.  They are not walked under that divergent mask: each lane appends (pixel, kind, front voxel) to a
//        workgroup queue in LDS, 8 bytes per entry.  The slot is two ballots and a popcount below the lane inside the wave plus the
//        totals of the lower waves, which meet in four LDS words: no atomics of any kind.
//     3  after a barrier the workgroup drains the queue densely, lane q takes entry q (at most two rounds of 256): it rebuilds the ray
//        (B: the owner pixel's direction from the camera formula, the same f32 operations; S: the front voxel's centre towards the sun),
//        walks it with stop mask OPAQUE | SEMI over occ_second, and leaves a finished result in the owner's LDS slot: B the shaded
//        colour behind the water (or the sky), S one shadow byte.  These walks read the grid table and section masks from global
//        memory (trace<false>): a second staged section table would cost 16 KB and the fourth workgroup of a CU.
//     4  after a barrier every lane composites its pixel from registers and its two slots: light of the front voxel, ramp, face factor,
//        AO from 8 occluder bytes around the front voxel weighted by the hit point inside the face, shadow, blend, fog.  One 4-byte store.
//   Palette, class table, RAMP / FACE / AOW and both stop tables live in LDS.  Shading is integer only; the two f32 expressions of the
//   contract (hit point, fog) are built without contraction like the walk.
#include "mm_raywalk.cuh"
#include "mmgen_prof.h"

namespace mm {

#define RENDER_QUEUE 512       // a pixel queues at most one walk B and one walk S

// tools/render_view.py:palette() rounded to u8, r | g << 8 | b << 16 | alpha << 24; alpha 150 for the TRANSPARENT class (1, 92 - 94, 103)
#define MM_DEFAULT_PALETTE \
    0xff5a646eu, 0x96c85a28u, 0xff145ae6u, 0xff61a9a1u, 0xff7eac8au, 0xff73af73u, 0xff68b298u, 0xff5db581u, \
    0xff7ab8a6u, 0xff6fbb8fu, 0xff64be78u, 0xff81c19du, 0xff76c486u, 0xff6bc76fu, 0xff60ca94u, 0xff7dcd7du, \
    0xff72d0a2u, 0xff67a18bu, 0xff5ca474u, 0xff79a799u, 0xff6eaa82u, 0xff63ada7u, 0xff80b090u, 0xff75b379u, \
    0xff6ab69eu, 0xff5fb987u, 0xff7cbc70u, 0xff71bf95u, 0xff66c27eu, 0xff5bc5a3u, 0xff78c88cu, 0xff6dcb75u, \
    0xff62ce9au, 0xff7fd183u, 0xff74a2a8u, 0xff69a591u, 0xff5ea87au, 0xff7bab9fu, 0xff70ae88u, 0xff65b171u, \
    0xff5ab496u, 0xff77b77fu, 0xff6cbaa4u, 0xff61bd8du, 0xff7ec076u, 0xff73c39bu, 0xff68c684u, 0xff5dc9a9u, \
    0xff7acc92u, 0xff6fcf7bu, 0xff64a0a0u, 0xff81a389u, 0xff76a672u, 0xff6ba997u, 0xff60ac80u, 0xff7dafa5u, \
    0xff72768eu, 0xff7d7d7du, 0xff3c5578u, 0xff46a05au, 0xff96cddcu, 0xff82878cu, 0xff80887cu, 0xfffaf5f0u, \
    0xfff0ebe1u, 0xff5f9173u, 0xff7c9498u, 0xff716581u, 0xff6668a6u, 0xff5b6b8fu, 0xff786e78u, 0xff6d719du, \
    0xff627486u, 0xff7f776fu, 0xff747a94u, 0xff697d7du, 0xff5e80a2u, 0xff7b838bu, 0xff3c6ec8u, 0xff658999u, \
    0xff5a8c82u, 0xff329646u, 0xff6c9290u, 0xff619579u, 0xff7e669eu, 0xff736987u, 0xff686c70u, 0xff287828u, \
    0xff28823cu, 0xff6f75a3u, 0xff64788cu, 0xff817b75u, 0x96767e9au, 0x966b8183u, 0x966084a8u, 0xff7d8791u, \
    0xff728a7au, 0xff678d9fu, 0xff5c9088u, 0xff799371u, 0xff6e6496u, 0xff63677fu, 0xff806aa4u, 0x96f5d2aau, \
    0xff6a7076u, 0xff5f739bu, 0xff50a5aau, 0xff7179a9u, 0xff50a064u, 0xff5b7f7bu, 0xff7882a0u, 0xff6d8589u, \
    0xff628872u, 0xff7f8b97u, 0xff748e80u, 0xff3c5a28u, 0xff5e948eu, 0xff7b6577u, 0xff70689cu, 0xff656b85u, \
    0xff5a6e6eu, 0xff78dcfau, 0xff6c747cu, 0xff6177a1u, 0xff7e7a8au, 0xff737d73u, 0xff688098u, 0xff5d8381u, \
    0xff7a86a6u, 0xff6f898fu, 0xff648c78u, 0xff818f9du, 0xff769286u, 0xff6b956fu, 0xff606694u, 0xff7d697du, \
    0xff726ca2u, 0xff676f8bu, 0xff5c7274u, 0xff797599u, 0xff6e7882u, 0xff637ba7u, 0xff807e90u, 0xff758179u, \
    0xff6a849eu, 0xff5f8787u, 0xff7c8a70u, 0xff718d95u, 0xff66907eu, 0xff5b93a3u, 0xff78648cu, 0xff6d6775u, \
    0xff626a9au, 0xff7f6d83u, 0xff7470a8u, 0xff697391u, 0xff5e767au, 0xff7b799fu, 0xff707c88u, 0xff657f71u, \
    0xff5a8296u, 0xff77857fu, 0xff6c88a4u, 0xff618b8du, 0xff7e8e76u, 0xff73919bu, 0xff689484u, 0xff5d65a9u, \
    0xff7a6892u, 0xff6f6b7bu, 0xff646ea0u, 0xff817189u, 0xff767472u, 0xff6b7797u, 0xff607a80u, 0xff7d7da5u, \
    0xff72808eu, 0xff678377u, 0xff5c869cu, 0xff798985u, 0xff6e8c6eu, 0xff638f93u, 0xff80927cu, 0xff7595a1u, \
    0xff6a668au, 0xff5f6973u, 0xff7c6c98u, 0xff716f81u, 0xff6672a6u, 0xff5b758fu, 0xff787878u, 0xff6d7b9du, \
    0xff627e86u, 0xff7f816fu, 0xff748494u, 0xff69877du, 0xff5e8aa2u, 0xff7b8d8bu, 0xff709074u, 0xff659399u, \
    0xff5a6482u, 0xff7767a7u, 0xff6c6a90u, 0xff616d79u, 0xff7e709eu, 0xff737387u, 0xff687670u, 0xff5d7995u, \
    0xff7a7c7eu, 0xff6f7fa3u, 0xff64828cu, 0xff818575u, 0xff76889au, 0xff6b8b83u, 0xff608ea8u, 0xff7d9191u, \
    0xff72947au, 0xff67659fu, 0xff5c6888u, 0xff796b71u, 0xff6e6e96u, 0xff63717fu, 0xff8074a4u, 0xff75778du, \
    0xff6a7a76u, 0xff5f7d9bu, 0xff7c8084u, 0xff7183a9u, 0xff668692u, 0xff5b897bu, 0xff788ca0u, 0xff6d8f89u, \
    0xff629272u, 0xff7f9597u, 0xff746680u, 0xff6969a5u, 0xff5e6c8eu, 0xff7b6f77u, 0xff70729cu, 0xff657585u, \
    0xff5a786eu, 0xff777b93u, 0xff6c7e7cu, 0xff6181a1u, 0xff7e848au, 0xff738773u, 0xff688a98u, 0xff5d8d81u, \
    0xff7a90a6u, 0xff6f938fu, 0xff646478u, 0xff81679du, 0xff766a86u, 0xff6b6d6fu, 0xff607094u, 0xff7d737du
__device__ const uint32_t kDefaultPalette[256] = {MM_DEFAULT_PALETTE};
static const uint32_t kDefaultPaletteHost[256] = {MM_DEFAULT_PALETTE};

// RAMP at 0, FACE at 16, AOW at 24 (mmgen.h)
#define TAB_FACE 16
#define TAB_AOW 24
__device__ const uint8_t kShadeTables[32] = {9, 11, 14, 18, 22, 27, 34, 43, 53, 67, 84, 104, 131, 163, 204, 255,
                                             204, 179, 153, 179, 255, 115, 255, 0, 115, 153, 204, 255, 0, 0, 0, 0};

struct RenderArgs {
    const uint8_t* occ2; const uint8_t* light; const uint32_t* palette; uint32_t* rgba; mmgen_ray_hit* hits;
    uint32_t flags, sky, sunLevel, shadowDim;
    float sun[3], fogStart, fogScale;                      // fogScale = 1.0f / (fog_end - fog_start), rounded once on the host
};

MM_DEV uint32_t mul8(uint32_t a, uint32_t b) { return (a * b + 127u) / 255u; }
MM_DEV uint32_t rgb_scale(uint32_t c, uint32_t k)
{
    return mul8(c & 255u, k) | mul8((c >> 8) & 255u, k) << 8 | mul8((c >> 16) & 255u, k) << 16;
}
// per channel (c w + other (255 - w) + 127) / 255
MM_DEV uint32_t rgb_mix(uint32_t c, uint32_t other, uint32_t w)
{
    uint32_t out = 0;
#pragma unroll
    for (int sh = 0; sh < 24; sh += 8) out |= ((((c >> sh) & 255u) * w + ((other >> sh) & 255u) * (255u - w) + 127u) / 255u) << sh;
    return out;
}

// chunk slot of the cell that holds column (x, z); -1 outside the grid or absent
template <bool STAGED>
MM_DEV int grid_slot(const RayScene& sc, const int32_t* s_grid, int x, int z)
{
    if (x < 0 || x >= 16 * sc.gw || z < 0 || z >= 16 * sc.gh) return -1;
    const int cell = (z >> 4) * sc.gw + (x >> 4);
    return STAGED ? s_grid[cell] : sc.grid[cell];
}
MM_DEV size_t voxel_index(int g, int x, int y, int z) { return (size_t)MMGEN_BLOCKS_PER_CHUNK * g + y + MMGEN_CHUNK_HEIGHT * ((x & 15) + 16 * (z & 15)); }

MM_DEV void front_voxel(const uint32_t* rec, int f[3])
{
    const uint32_t face = (rec[4] >> 8) & 255u;
    f[0] = (int)rec[0] + (face == 1u) - (face == 3u);
    f[1] = (int)rec[1] + (face == 4u) - (face == 5u);
    f[2] = (int)rec[2] + (face == 0u) - (face == 2u);
}

// shade(hit) of mmgen.h for a HIT record: palette x RAMP[level of the front voxel's light] x FACE
template <bool STAGED>
MM_DEV uint32_t shade(const RayScene& sc, const int32_t* s_grid, const RenderArgs& ra, const uint32_t* s_pal, const uint8_t* s_tab, const uint32_t* rec)
{
    int f[3];
    front_voxel(rec, f);
    uint32_t L = MMGEN_LIGHT_ABOVE;
    if (ra.light && f[1] < 0) L = 0u;
    else if (ra.light && f[1] < MMGEN_CHUNK_HEIGHT) {
        const int g = grid_slot<STAGED>(sc, s_grid, f[0], f[2]);      // present by the walk; a slot that is not reads as dark
        L = g >= 0 ? ra.light[voxel_index(g, f[0], f[1], f[2])] : 0u;
    }
    const uint32_t lv = max((L >> 4) * ra.sunLevel / 15u, L & 15u);
    return rgb_scale(rgb_scale(s_pal[rec[4] & 255u] & 0xffffffu, s_tab[lv]), s_tab[TAB_FACE + ((rec[4] >> 8) & 255u)]);
}

// the AO factor A of mmgen.h for walk A's hit on face 0..5: four corner values around the front voxel, weighted by where the ray met the face
template <bool STAGED>
MM_DEV uint32_t ao_factor(const RayScene& sc, const int32_t* s_grid, const uint8_t* s_cls, const uint8_t* s_tab, const uint32_t* rec,
                          const float o[3], const float d[3])
{
    const uint32_t face = (rec[4] >> 8) & 255u;
    const bool nz = face == 0u || face == 2u, ny = face >= 4u;          // the face's normal; rows r: x (nz) or z, fast axis q: x (ny) or y
    int f[3];
    front_voxel(rec, f);
    auto O = [&](int sr, int sq) -> uint32_t {
        const int x = f[0] + (nz ? sr : 0) + (ny ? sq : 0), y = f[1] + (ny ? 0 : sq), z = f[2] + (nz ? 0 : sr);
        if (y < 0 || y >= MMGEN_CHUNK_HEIGHT) return 0u;
        const int g = grid_slot<STAGED>(sc, s_grid, x, z);
        return g >= 0 && s_cls[sc.blocks[voxel_index(g, x, y, z)]] == MMGEN_RAY_OPAQUE ? 1u : 0u;
    };
    const uint32_t rm = O(-1, 0), rp = O(1, 0), qm = O(0, -1), qp = O(0, 1), c0 = O(-1, -1), c1 = O(-1, 1), c2 = O(1, -1), c3 = O(1, 1);
    auto aow = [&](uint32_t s1, uint32_t s2, uint32_t c) -> uint32_t { return s_tab[TAB_AOW + ((s1 & s2) ? 0u : 3u - (s1 + s2 + c))]; };
    const float t = __uint_as_float(rec[3]);
    auto sub = [&](float oa, float da, int va) -> int {                  // h = o + t d: one multiply, one add; 16ths of the voxel, clamped
        const float h = oa + t * da;
        return (int)fminf(fmaxf(floorf((h - (float)va) * 16.0f), 0.f), 15.f);
    };
    const int ur = nz ? sub(o[0], d[0], (int)rec[0]) : sub(o[2], d[2], (int)rec[2]);
    const int uq = ny ? sub(o[0], d[0], (int)rec[0]) : sub(o[1], d[1], (int)rec[1]);
    const uint32_t wrp = 2 * ur + 1, wrm = 31 - 2 * ur, wqp = 2 * uq + 1, wqm = 31 - 2 * uq;
    return (wrm * wqm * aow(rm, qm, c0) + wrm * wqp * aow(rm, qp, c1) + wrp * wqm * aow(rp, qm, c2) + wrp * wqp * aow(rp, qp, c3) + 512u) >> 10;
}

template <bool STAGED>
__global__ void __launch_bounds__(256)
k_render_camera(RayScene sc, CamBasis cbArg, RenderArgs raArg)
{
    // camera and parameters are read from LDS where they are used: as kernel arguments they would sit in scalar registers through all
    // three walks (50 of them), and the walk has none to spare
    __shared__ CamBasis s_cb;
    __shared__ RenderArgs s_ra;
    const CamBasis& cb = s_cb;
    const RenderArgs& ra = s_ra;
    __shared__ int32_t s_grid[STAGED ? RAY_LDS_CELLS : 1];
    __shared__ uint32_t s_sec[STAGED ? RAY_LDS_CELLS : 1];
    __shared__ uint32_t s_stop[8], s_stop2[8], s_pal[256], s_back[256], s_count[4];
    __shared__ uint2 s_queue[RENDER_QUEUE];
    __shared__ uint8_t s_cls[256], s_tab[32], s_shadow[256];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (t == 0) { s_cb = cbArg; s_ra = raArg; }
    sc.flags = 0u;                                         // a constant: the walk's debug paths fold away
    s_pal[t] = raArg.palette ? raArg.palette[t] : kDefaultPalette[t];
    s_cls[t] = (uint8_t)ray_class_bit(t);
    if (t < 32) s_tab[t] = kShadeTables[t];
    build_stop_table(MMGEN_RAY_OPAQUE | MMGEN_RAY_SEMI, s_stop2);
    stage_tables<STAGED>(sc, s_grid, s_sec, s_stop);       // ends with the barrier that covers all of the above

    auto pixel = [&](int p, int& i, int& j) {              // pixel of the tile's lane p
        i = 16 * (int)blockIdx.x + 8 * ((p >> 6) & 1) + (p & 7); j = 16 * (int)blockIdx.y + 8 * (p >> 7) + ((p & 63) >> 3);
    };
    // ---- 1: walk A
    int i, j;
    pixel(t, i, j);
    const bool live = i < cb.width && j < cb.height;
    const size_t px = (size_t)j * cb.width + i;
    const float eye[3] = {cb.eye[0], cb.eye[1], cb.eye[2]};
    float d[3];
    cam_dir(cb, i, j, d);
    uint32_t A[5] = {0u, 0u, 0u, 0u, MMGEN_RAY_FACE_NONE << 8 | MMGEN_RAY_INVALID << 16};
    if (live) {
        trace<STAGED>(sc, s_grid, s_sec, s_stop, eye, d, A);
        if (ra.hits) {
            uint32_t* h = (uint32_t*)(ra.hits + px);
#pragma unroll
            for (int k = 0; k < 5; ++k) h[k] = A[k];
        }
    }
    const uint32_t blockA = A[4] & 255u, faceA = (A[4] >> 8) & 255u;
    const bool hitA = live && (A[4] >> 16) == MMGEN_RAY_HIT;
    const bool needB = hitA && (ra.flags & MMGEN_RENDER_TRANSLUCENT) && s_cls[blockA] == MMGEN_RAY_TRANSPARENT;
    const bool needS = hitA && (ra.flags & MMGEN_RENDER_SUN_SHADOW) && faceA != MMGEN_RAY_FACE_NONE;

    const uint32_t flags = __builtin_amdgcn_readfirstlane(ra.flags);
    if (flags & (MMGEN_RENDER_TRANSLUCENT | MMGEN_RENDER_SUN_SHADOW)) {         // uniform over the launch
        // ---- 2: queue the secondary rays; a wave's entries are its B rays in lane order, then its S rays
        const unsigned long long bB = __ballot(needB), bS = __ballot(needS), below = (1ull << lane) - 1ull;
        if (lane == 0) s_count[wave] = (uint32_t)(__popcll(bB) + __popcll(bS));
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int c = (int)s_count[w]; base += w < wave ? c : 0; total += c; }
        if (needB) s_queue[base + __popcll(bB & below)] = make_uint2((uint32_t)t, 0u);
        if (needS) {                                       // front voxel: x, z < 2^18, y + 1 in 0 .. 385
            int f[3];
            front_voxel(A, f);
            s_queue[base + __popcll(bB) + __popcll(bS & below)] =
                make_uint2((uint32_t)t | 1u << 8 | (uint32_t)(f[1] + 1) << 9 | ((uint32_t)f[2] >> 14) << 18, (uint32_t)f[0] | ((uint32_t)f[2] & 0x3fffu) << 18);
        }
        __syncthreads();
        // ---- 3: drain it densely
        RayScene sc2 = sc;
        sc2.occ = ra.occ2;
#pragma unroll 1
        for (int q = t; q < total; q += 256) {
            const uint2 e = s_queue[q];
            const int p = (int)(e.x & 255u);
            const bool isS = (e.x >> 8) & 1u;
            int pi, pj;
            pixel(p, pi, pj);
            float o2[3], d2[3];
            cam_dir(cb, pi, pj, d2);
            const int f[3] = {(int)(e.y & 0x3ffffu), (int)((e.x >> 9) & 511u) - 1, (int)((e.x >> 18) << 14 | e.y >> 18)};
#pragma unroll
            for (int a = 0; a < 3; ++a) { o2[a] = isS ? (float)f[a] + 0.5f : eye[a]; d2[a] = isS ? ra.sun[a] : d2[a]; }
            uint32_t R[5];
            trace<false>(sc2, nullptr, nullptr, s_stop2, o2, d2, R);
            const bool hit = (R[4] >> 16) == MMGEN_RAY_HIT;
            if (isS) s_shadow[p] = hit;
            else s_back[p] = hit ? shade<STAGED>(sc, s_grid, ra, s_pal, s_tab, R) : ra.sky;
        }
        __syncthreads();
    }
    // ---- 4: the pixel
    if (!live) return;
    uint32_t C = ra.sky, alpha = 0u;
    if (hitA) {
        C = shade<STAGED>(sc, s_grid, ra, s_pal, s_tab, A);
        alpha = 255u;
        if ((flags & MMGEN_RENDER_AO) && faceA != MMGEN_RAY_FACE_NONE && (s_cls[blockA] & (MMGEN_RAY_OPAQUE | MMGEN_RAY_SEMI)))
            C = rgb_scale(C, ao_factor<STAGED>(sc, s_grid, s_cls, s_tab, A, eye, d));
        if (needS && s_shadow[t]) C = rgb_scale(C, ra.shadowDim);
        if (needB) C = rgb_mix(C, s_back[t], s_pal[blockA] >> 24);
        if (flags & MMGEN_RENDER_FOG) {
            const float x = (__uint_as_float(A[3]) - ra.fogStart) * ra.fogScale;
            const uint32_t g = (uint32_t)(int)(fminf(fmaxf(x, 0.f), 1.f) * 255.0f + 0.5f);
            C = rgb_mix(C, ra.sky, 255u - g);
        }
    }
    ra.rgba[px] = C | alpha << 24;
}

}  // namespace mm

extern "C" {

int mmgen_render_default_palette(uint32_t* h_out)
{
    if (!h_out) return (int)hipErrorInvalidValue;
    for (int i = 0; i < 256; ++i) h_out[i] = mm::kDefaultPaletteHost[i];
    return 0;
}

int mmgen_render_camera(const uint8_t* d_blocks, const int32_t* d_grid, int grid_w, int grid_h, const uint8_t* d_occ_first, const uint8_t* d_occ_second,
                        const uint8_t* d_light, const uint32_t* d_palette, const mmgen_camera* cam, const mmgen_render_params* p, uint32_t* d_rgba,
                        mmgen_ray_hit* d_hits, void* stream)
{
    if (!p || !d_rgba) return (int)hipErrorInvalidValue;
    mm::RayScene sc;
    if (int e = mm::ray_scene(sc, d_blocks, d_grid, grid_w, grid_h, d_occ_first, p->first_mask, 0u, p->t_max)) return e;
    mm::CamBasis cb;
    if (int e = mm::cam_basis(cb, cam)) return e;
    const auto finite = [](float x) { return x - x == 0.f; };
    const unsigned all = MMGEN_RENDER_AO | MMGEN_RENDER_TRANSLUCENT | MMGEN_RENDER_SUN_SHADOW | MMGEN_RENDER_FOG;
    if (!(p->first_mask & MMGEN_RAY_OPAQUE) || (p->flags & ~all) || p->sun_level > 15) return (int)hipErrorInvalidValue;
    if ((p->flags & (MMGEN_RENDER_TRANSLUCENT | MMGEN_RENDER_SUN_SHADOW)) && !d_occ_second) return (int)hipErrorInvalidValue;
    if ((p->flags & MMGEN_RENDER_FOG) && !(finite(p->fog_start) && finite(p->fog_end) && p->fog_end > p->fog_start)) return (int)hipErrorInvalidValue;
    if ((p->flags & MMGEN_RENDER_SUN_SHADOW) &&
        !(finite(p->sun_dir[0]) && finite(p->sun_dir[1]) && finite(p->sun_dir[2]) && (p->sun_dir[0] != 0.f || p->sun_dir[1] != 0.f || p->sun_dir[2] != 0.f)))
        return (int)hipErrorInvalidValue;
    mm::RenderArgs ra{d_occ_second, d_light, d_palette, d_rgba, d_hits, p->flags,
                      (uint32_t)p->sky_rgb[0] | (uint32_t)p->sky_rgb[1] << 8 | (uint32_t)p->sky_rgb[2] << 16, p->sun_level, p->shadow_dim,
                      {p->sun_dir[0], p->sun_dir[1], p->sun_dir[2]}, p->fog_start, (p->flags & MMGEN_RENDER_FOG) ? 1.0f / (p->fog_end - p->fog_start) : 0.f};
    const dim3 grid((cam->width + 15) / 16, (cam->height + 15) / 16);
    if (grid_w * grid_h <= RAY_LDS_CELLS)
        MMK_LAUNCH_NORET(mmk::KID_RENDER_CAMERA, mm::k_render_camera<true>, grid, dim3(256), (hipStream_t)stream, sc, cb, ra);
    else
        MMK_LAUNCH_NORET(mmk::KID_RENDER_CAMERA, mm::k_render_camera<false>, grid, dim3(256), (hipStream_t)stream, sc, cb, ra);
    return (int)hipGetLastError();
}

}  // extern "C"
