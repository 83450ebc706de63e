/* mmgen — wire types of the chunk-generation path (C ABI, no C++ / torch types).
 *
 * These PODs and enumerations are the layout contract between stages and with the caller.  They replace, value for
 * value and byte for byte, the reference's
 *   enum Block              src/terrain/block.hpp:5-154      (uint8 block ids written to Chunk::blocks)
 *   enum Biome/CaveBiome/Material/Feature/CaveFeature        src/terrain/biome.hpp:13-167
 *   struct CaveLayer (12 B)                                   src/terrain/biome.hpp:106-115
 *   struct FeaturePlacement (20 B), CaveFeaturePlacement (24 B)  src/terrain/biome.hpp:195-245
 * and the staging sizes of src/terrain/terrain.hpp:17-50.
 */
#ifndef MMGEN_TYPES_H
#define MMGEN_TYPES_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMGEN_CHUNK_COLS 256                 /* 16 x 16 columns, idx2d = x + 16 z          (biomeFuncs.hpp:11-23) */
#define MMGEN_CHUNK_HEIGHT 384
#define MMGEN_BLOCKS_PER_CHUNK 98304         /* idx = y + 384 (x + 16 z)                    (terrain.hpp:37)       */
#define MMGEN_NUM_BIOMES 24
#define MMGEN_NUM_CAVE_BIOMES 5
#define MMGEN_NUM_MATERIALS 20
#define MMGEN_NUM_FORWARD_MATERIALS 10
#define MMGEN_NUM_STRATIFIED_MATERIALS 12
#define MMGEN_NUM_ERODED_MATERIALS 8
#define MMGEN_NUM_FEATURES 21
#define MMGEN_NUM_CAVE_FEATURES 10
#define MMGEN_HEIGHTFIELD_SIZE 256
#define MMGEN_GATHERED_HEIGHTFIELD_SIZE 324  /* 18 x 18, devHeightfieldSize                 (terrain.hpp:41)       */
#define MMGEN_BIOME_WEIGHTS_SIZE 6144        /* devBiomeWeightsSize = 256 * 24, biome-major (terrain.hpp:42)       */
#define MMGEN_LAYERS_SIZE 5120               /* devLayersSize = 256 * 20, layer-major       (terrain.hpp:44)       */
#define MMGEN_MAX_CAVE_LAYERS_PER_COLUMN 32  /*                                              (biome.hpp:6)          */
#define MMGEN_CAVE_LAYERS_SIZE 8192          /* devCaveLayersSize = 256 * 32, column-major  (terrain.hpp:45)       */
#define MMGEN_MAX_GATHERED_FEATURES_PER_CHUNK 2048        /* biome.hpp:7 */
#define MMGEN_MAX_GATHERED_CAVE_FEATURES_PER_CHUNK 4096   /* biome.hpp:8 */
#define MMGEN_FP_CAP 256                     /* per-chunk surface placements: at most one per column (chunk.cu:1136-1141) */
#define MMGEN_CFP_CAP 1024                   /* per-chunk cave placements kept on device (typ. < 80, biome.hpp:8 comment)  */
#define MMGEN_SEA_LEVEL 128
#define MMGEN_LAVA_LEVEL 8
#define MMGEN_ZONE_SIZE 12                   /* chunks per zone side                         (terrain.hpp:17)       */
#define MMGEN_EROSION_GRID_SIDE 384          /* EROSION_GRID_SIDE_LENGTH_BLOCKS             (terrain.hpp:18)       */
#define MMGEN_EROSION_GRID_NUM_COLS 147456   /* EROSION_GRID_NUM_COLS                        (terrain.hpp:19)       */
#define MMGEN_GATHERED_LAYERS_SIZE 1327105   /* devGatheredLayersSize = 147456 * 9 + 1 flag (terrain.hpp:47)       */

typedef struct mmgen_cave_layer {            /* biome.hpp:106-115 */
    int32_t start;                           /* exclusive (is not air); 384 = unused slot */
    int32_t end;                             /* inclusive (is air); 384 = open to the sky */
    uint8_t bottom_biome;                    /* cave biome of block y = start   */
    uint8_t top_biome;                       /* cave biome of block y = end + 1 */
    uint8_t padding[2];
} mmgen_cave_layer;

typedef struct mmgen_vertex {                /* Vertex, src/rendering/structs.hpp:25-31 (vec3, vec3, vec2, Mats : size_t) */
    float pos[3];                            /* chunk-local block coordinates */
    float nor[3];
    float uv[2];                             /* texture-atlas coordinates, tile = 1/16 */
    uint64_t material;                       /* Mats: 0 DIFFUSE, 1 WATER, 2 CRYSTAL, 3 SMOOTH_MICRO, 4 MICRO, 5 ROUGH_MICRO */
} mmgen_vertex;

/* ---- quad record of the greedy mesher (mmgen.h "greedy-merged compact quad mesh"): one uint64_t per quad ----
 *   bits  0- 3  x of the min-corner voxel          bits 20-23  dx
 *   bits  4-12  y of the min-corner voxel          bits 24-32  dy
 *   bits 13-16  z of the min-corner voxel          bits 33-36  dz
 *   bits 17-19  kind: 0-5 = direction d            bits 37-44  block id
 *               (+z +x -z -x +y -y), 6 = X-shaped  bits 45-63  zero
 * dx, dy, dz are extents minus one; the extent along the normal is 0; a kind-6 record has all extents 0.  The quad is the face, on side d,
 * of the box [x, x+dx+1) x [y, y+dy+1) x [z, z+dz+1). */
#define MMGEN_QUAD_KIND_XSHAPED 6

/* ---- ray casting (mmgen.h "ray casting over device-resident chunks"; the reference has none: its chunks go to RT cores) ---- */
typedef struct mmgen_ray_hit {               /* 20 bytes */
    int32_t voxel[3];                        /* grid-local block x, world y, grid-local block z */
    float t;                                 /* ray parameter of the plane crossed last (o + t d); 0 at the start voxel; t_max for MISS_TMAX */
    uint8_t block;                           /* block id for HIT, else 0 */
    uint8_t face;                            /* dirVecs index (+z, +x, -z, -x, +y, -y) of the outward normal of the face entered; 6 = none */
    uint8_t status;                          /* MMGEN_RAY_HIT ... */
    uint8_t pad;                             /* 0 */
} mmgen_ray_hit;
enum { MMGEN_RAY_HIT, MMGEN_RAY_MISS_TMAX, MMGEN_RAY_LEFT_GRID, MMGEN_RAY_ABSENT_CHUNK, MMGEN_RAY_INVALID };
#define MMGEN_RAY_FACE_NONE 6
/* stop_mask bits = the mesher's block classes (transparency of mm_blockdata.cuh); AIR belongs to none; 15 = any non-air block */
#define MMGEN_RAY_OPAQUE 1u
#define MMGEN_RAY_SEMI 2u
#define MMGEN_RAY_TRANSPARENT 4u
#define MMGEN_RAY_XSHAPED 8u
/* flags (debug): walk voxel by voxel without the skip structure; report visit counts in place of the voxel */
#define MMGEN_RAY_NO_SKIP 1u
#define MMGEN_RAY_COUNT_VISITS 2u
#define MMGEN_RAY_OCCUPANCY_BYTES 200        /* per chunk: u64 section mask (bit sy, 24 used), then 24 x u64 brick masks, bit = by + 4 (bx + 4 bz) */
typedef struct mmgen_camera {                /* pinhole camera in the rays' coordinates */
    float eye[3];
    float forward[3];                        /* need not be normalised */
    float up[3];                             /* not parallel to forward */
    float fov_y;                             /* vertical field of view, radians, in (0, pi) */
    int32_t width, height;                   /* pixels */
} mmgen_camera;

/* ---- shaded camera render (mmgen_render_camera, include/mmgen.h) ---- */
#define MMGEN_RENDER_AO 1u                   /* corner occlusion on walk A's hit */
#define MMGEN_RENDER_TRANSLUCENT 2u          /* walk B behind a TRANSPARENT-class hit, blended by the palette alpha */
#define MMGEN_RENDER_SUN_SHADOW 4u           /* walk S from the front voxel towards the sun */
#define MMGEN_RENDER_FOG 8u                  /* blend towards sky_rgb by t */
typedef struct mmgen_render_params {         /* 40 bytes */
    uint32_t flags;                          /* MMGEN_RENDER_* */
    uint32_t first_mask;                     /* stop_mask of walk A; must contain MMGEN_RAY_OPAQUE */
    float t_max;                             /* of all three walks */
    float sun_dir[3];                        /* points towards the sun; need not be normalised */
    float fog_start, fog_end;                /* in t; fog_end > fog_start */
    uint8_t sky_rgb[3];
    uint8_t sun_level;                       /* 0..15: what sky light 15 is worth (15 = noon) */
    uint8_t shadow_dim;                      /* mul8 factor of a shadowed pixel */
    uint8_t pad[3];
} mmgen_render_params;

/* ---- voxel lighting (mmgen_light_masks / mmgen_light, include/mmgen.h) ----
 * The mask record of a chunk slot, c = x + 16 z, word w = y / 64, bit y % 64:
 *   u64 [256][6]     at     0   the voxel passes light (its class is not OPAQUE)
 *   u64 [256][6][4]  at 12288   bit k of the voxel's emission value, k = 0..3
 *   u16 [256]        at 61440   open height: the lowest y from which the column is AIR / X_SHAPED up to y = 383, 384 = none
 *   u32 [256]        at 61952   nibble w = OR of the emission values of the column's word w (0 = no emitter in that word) */
#define MMGEN_LIGHT_MASK_BYTES 62976
#define MMGEN_LIGHT_MAX 15
#define MMGEN_LIGHT_ABOVE 0xF0u               /* the light above y = 383: sky 15, block 0 (mmgen_mesh_lit_section_quads_*) */

/* ---- section visibility (mmgen_section_connectivity / mmgen_visible_sections, include/mmgen.h) ----
 * The connectivity record of a chunk slot: u16 [24], one per 16^3 section sy = y >> 4; bit a (11 - a) / 2 + b - a - 1 = faces a < b (dirVecs
 * order) are connected through see-through voxels inside the section; bit 15 is 0. */
#define MMGEN_SECTION_CONN_BYTES 48
#define MMGEN_VISIBLE_MAX_RADIUS 32

/* ---- section quad record (mmgen.h "section-bucketed quad mesh"): one uint32_t per quad, coordinates local to the 16^3 section ----
 *   bits  0- 3  x of the min-corner voxel          bits 15-18  W - 1, the extent along the plane's rows r
 *   bits  4- 7  y & 15 of the min-corner voxel     bits 19-22  L - 1, the extent along the plane's fast axis q
 *   bits  8-11  z of the min-corner voxel          bits 23-30  block id
 *   bits 12-14  kind: 0-5 = direction d            bit  31     zero
 *               (+z +x -z -x +y -y), 6 = X-shaped
 * Rows and fast axis per direction: d in {0, 2}: r = x, q = y;  d in {1, 3}: r = z, q = y;  d in {4, 5}: r = z, q = x.  A kind-6 record has
 * W - 1 = L - 1 = 0.  The section (chunk, sy) is not in the record: it follows from the record's position (mmgen_section_draw.origin). */
#define MMGEN_SECTIONS_PER_CHUNK 24
/* ---- face AO byte (mmgen.h "section quad mesh with ambient occlusion"): one uint8_t per record, parallel to the records ----
 *   bits 2k, 2k+1 = ao of corner k = 2 [row side is +] + [fast-axis side is +] of every cell of the quad (rows r and fast axis q as above):
 *   3 = open, 2 / 1 = one / two of {side, side, corner} opaque, 0 = both sides opaque.  0xFF = unoccluded; every kind-6 record has 0xFF. */
#define MMGEN_AO_NONE 0xFFu
/* one contiguous range of section quad records = one section that has to be drawn (mmgen_section_draws) */
typedef struct mmgen_section_draw {          /* 16 bytes */
    uint64_t first;                          /* index of the section's first record in d_quads */
    uint32_t count;                          /* its records, > 0 */
    uint32_t origin;                         /* wx | wz << 7 | sy << 14: window cell (cx - eye_cx + radius, cz - eye_cz + radius) and section */
} mmgen_section_draw;

typedef struct mmgen_feature_placement {     /* biome.hpp:195-200: feature@0, pos@4, canReplaceBlocks@16 */
    uint8_t feature;
    uint8_t pad0[3];
    int32_t pos[3];
    uint8_t can_replace_blocks;
    uint8_t pad1[3];
} mmgen_feature_placement;

typedef struct mmgen_cave_feature_placement { /* biome.hpp:239-245: feature@0, pos@4, layerHeight@16, canReplaceBlocks@20 */
    uint8_t feature;
    uint8_t pad0[3];
    int32_t pos[3];                          /* lowest air block of the cave layer */
    int32_t layer_height;
    uint8_t can_replace_blocks;
    uint8_t pad1[3];
} mmgen_cave_feature_placement;

/* enum Block (block.hpp:5-154): the first 56 ids (AIR .. KELP_END) are non-solid */
enum {
    MMB_AIR, MMB_WATER, MMB_LAVA, MMB_CAVE_VINES_MAIN, MMB_CAVE_VINES_GLOW_MAIN, MMB_CAVE_VINES_END, MMB_CAVE_VINES_GLOW_END,
    MMB_GRASS, MMB_JUNGLE_GRASS, MMB_SAVANNA_GRASS, MMB_WARPED_MUSHROOM, MMB_WARPED_ROOTS, MMB_NETHER_SPROUTS,
    MMB_INFECTED_MUSHROOM, MMB_AMBER_ROOTS, MMB_DANDELION, MMB_POPPY, MMB_PITCHER_BOTTOM, MMB_PITCHER_TOP, MMB_CORNFLOWER,
    MMB_BLUE_ORCHID, MMB_ALLIUM, MMB_RED_TULIP, MMB_ORANGE_TULIP, MMB_WHITE_TULIP, MMB_PINK_TULIP, MMB_LILAC_BOTTOM,
    MMB_LILAC_TOP, MMB_PEONY_BOTTOM, MMB_PEONY_TOP, MMB_OXEYE_DAISY, MMB_LILY_OF_THE_VALLEY, MMB_JUNGLE_FERN,
    MMB_SMALL_MAGENTA_CRYSTAL, MMB_SMALL_CYAN_CRYSTAL, MMB_SMALL_GREEN_CRYSTAL, MMB_SMALL_PURPLE_MUSHROOM, MMB_DEAD_BUSH,
    MMB_HANGING_SMALL_MAGENTA_CRYSTAL, MMB_HANGING_SMALL_CYAN_CRYSTAL, MMB_HANGING_SMALL_GREEN_CRYSTAL, MMB_TALL_GRASS_BOTTOM,
    MMB_TALL_GRASS_TOP, MMB_TALL_JUNGLE_GRASS_BOTTOM, MMB_TALL_JUNGLE_GRASS_TOP, MMB_TORCHFLOWER, MMB_BRAIN_CORAL,
    MMB_BUBBLE_CORAL, MMB_FIRE_CORAL, MMB_HORN_CORAL, MMB_TUBE_CORAL, MMB_SEAGRASS, MMB_TALL_SEAGRASS_BOTTOM,
    MMB_TALL_SEAGRASS_TOP, MMB_KELP_MAIN, MMB_KELP_END,
    MMB_BEDROCK,
    MMB_STONE, MMB_DIRT, MMB_GRASS_BLOCK, MMB_SAND, MMB_GRAVEL, MMB_MYCELIUM, MMB_SNOW, MMB_SNOWY_GRASS_BLOCK, MMB_MUSHROOM_STEM,
    MMB_MUSHROOM_UNDERSIDE, MMB_PURPLE_MUSHROOM_CAP, MMB_MARBLE, MMB_ANDESITE, MMB_CALCITE, MMB_BLACKSTONE, MMB_TUFF,
    MMB_DEEPSLATE, MMB_GRANITE, MMB_SLATE, MMB_SANDSTONE, MMB_CLAY, MMB_RED_SAND, MMB_RED_SANDSTONE, MMB_MUD,
    MMB_JUNGLE_GRASS_BLOCK, MMB_RAFFLESIA_PETAL, MMB_RAFFLESIA_CENTER, MMB_RAFFLESIA_SPIKES, MMB_RAFFLESIA_STEM, MMB_JUNGLE_WOOD,
    MMB_JUNGLE_LEAVES_PLAIN, MMB_JUNGLE_LEAVES_FRUITS, MMB_CACTUS, MMB_PALM_WOOD, MMB_PALM_LEAVES, MMB_MAGENTA_CRYSTAL,
    MMB_CYAN_CRYSTAL, MMB_GREEN_CRYSTAL, MMB_SMOOTH_SAND, MMB_TERRACOTTA, MMB_YELLOW_TERRACOTTA, MMB_ORANGE_TERRACOTTA,
    MMB_PURPLE_TERRACOTTA, MMB_RED_TERRACOTTA, MMB_WHITE_TERRACOTTA, MMB_QUARTZ, MMB_ICE, MMB_PACKED_ICE, MMB_BLUE_ICE,
    MMB_SAVANNA_GRASS_BLOCK, MMB_BIRCH_WOOD, MMB_BIRCH_LEAVES, MMB_YELLOW_BIRCH_LEAVES, MMB_ORANGE_BIRCH_LEAVES, MMB_ACACIA_WOOD,
    MMB_ACACIA_LEAVES, MMB_SMOOTH_SANDSTONE, MMB_PINE_WOOD, MMB_PINE_LEAVES_1, MMB_PINE_LEAVES_2, MMB_REDWOOD_WOOD,
    MMB_REDWOOD_LEAVES, MMB_CYPRESS_WOOD, MMB_CYPRESS_LEAVES, MMB_GLOWSTONE, MMB_SHROOMLIGHT, MMB_WARPED_DEEPSLATE,
    MMB_WARPED_BLACKSTONE, MMB_MOSS, MMB_AMBER_DEEPSLATE, MMB_AMBER_BLACKSTONE, MMB_WARPED_STEM, MMB_WARPED_WART, MMB_AMBER_STEM,
    MMB_AMBER_WART, MMB_COBBLESTONE, MMB_COBBLED_DEEPSLATE, MMB_BRAIN_CORAL_BLOCK, MMB_BUBBLE_CORAL_BLOCK, MMB_FIRE_CORAL_BLOCK,
    MMB_HORN_CORAL_BLOCK, MMB_TUBE_CORAL_BLOCK, MMB_SEA_LANTERN,
    MMB_NUM_BLOCKS
};
#define MMB_NUM_NON_SOLID_BLOCKS (MMB_KELP_END + 1)

/* enum Biome (biome.hpp:13-44) */
enum {
    MMBIO_CORAL_REEF, MMBIO_ARCHIPELAGO, MMBIO_WARM_OCEAN, MMBIO_ICEBERGS, MMBIO_COOL_OCEAN,
    MMBIO_ROCKY_BEACH, MMBIO_TROPICAL_BEACH, MMBIO_BEACH,
    MMBIO_SAVANNA, MMBIO_MESA, MMBIO_FROZEN_WASTELAND, MMBIO_REDWOOD_FOREST, MMBIO_SHREKS_SWAMP, MMBIO_SPARSE_DESERT,
    MMBIO_LUSH_BIRCH_FOREST, MMBIO_TIANZI_MOUNTAINS,
    MMBIO_JUNGLE, MMBIO_RED_DESERT, MMBIO_PURPLE_MUSHROOMS, MMBIO_CRYSTALS, MMBIO_OASIS, MMBIO_DESERT, MMBIO_PLAINS, MMBIO_MOUNTAINS
};
#define MMGEN_NUM_OCEAN_BIOMES 5
#define MMGEN_NUM_OCEAN_AND_BEACH_BIOMES 8

/* enum CaveBiome (biome.hpp:50-59) */
enum { MMCB_NONE, MMCB_CRYSTAL_CAVES, MMCB_LUSH_CAVES, MMCB_WARPED_FOREST, MMCB_AMBER_FOREST };

/* enum Material (biome.hpp:65-93): 0-9 forward stratified, 10-11 backward stratified, 12-19 eroded */
enum {
    MMM_BLACKSTONE, MMM_DEEPSLATE, MMM_SLATE, MMM_STONE, MMM_TUFF, MMM_CALCITE, MMM_GRANITE, MMM_TERRACOTTA, MMM_MARBLE, MMM_ANDESITE,
    MMM_RED_SANDSTONE, MMM_SANDSTONE,
    MMM_GRAVEL, MMM_CLAY, MMM_MUD, MMM_DIRT, MMM_RED_SAND, MMM_SAND, MMM_SMOOTH_SAND, MMM_SNOW
};

/* enum Feature (biome.hpp:117-158) */
enum {
    MMF_NONE, MMF_SPHERE, MMF_CORAL, MMF_KELP, MMF_ICEBERG, MMF_ACACIA_TREE, MMF_REDWOOD_TREE, MMF_CYPRESS_TREE, MMF_BIRCH_TREE,
    MMF_PINE_TREE, MMF_PINE_SHRUB, MMF_RAFFLESIA, MMF_LARGE_JUNGLE_TREE, MMF_SMALL_JUNGLE_TREE, MMF_TINY_JUNGLE_TREE,
    MMF_MEDIUM_PURPLE_MUSHROOM, MMF_PURPLE_MUSHROOM, MMF_MEDIUM_CRYSTAL, MMF_CRYSTAL, MMF_PALM_TREE, MMF_CACTUS
};

/* enum CaveFeature (biome.hpp:162-177) */
enum {
    MMCF_NONE, MMCF_TEST_GLOWSTONE_PILLAR, MMCF_TEST_SHROOMLIGHT_PILLAR, MMCF_CAVE_VINE, MMCF_GLOWSTONE_CLUSTER,
    MMCF_STORMLIGHT_SPHERE, MMCF_CEILING_STORMLIGHT_SPHERE, MMCF_CRYSTAL_PILLAR, MMCF_WARPED_FUNGUS, MMCF_AMBER_FUNGUS
};

/* mmgen_debug_probe function selectors (test-only entry point: one device math function per item) */
enum {
    MMGEN_PROBE_SIN, MMGEN_PROBE_COS, MMGEN_PROBE_POW, MMGEN_PROBE_ATAN2, MMGEN_PROBE_ACOS, MMGEN_PROBE_SIMPLEX2, MMGEN_PROBE_SIMPLEX3,
    MMGEN_PROBE_FBM2_5, MMGEN_PROBE_FBM3_4, MMGEN_PROBE_RAND3FROM3, MMGEN_PROBE_WORLEY2, MMGEN_PROBE_WORLEY3,
    MMGEN_PROBE_SPECIAL_CAVE_NOISE, MMGEN_PROBE_BIOME_HEIGHT, MMGEN_PROBE_CAVE_BIOME, MMGEN_PROBE_HASH, MMGEN_PROBE_RNG4_U01,
    MMGEN_PROBE_SIMPLEX3_SPLIT   /* simplex3 regrouped at the lattice (part1 -> corner gradients -> part3), as k_cave_voxels evaluates it */
};

#ifdef __cplusplus
}
#endif
#endif /* MMGEN_TYPES_H */
