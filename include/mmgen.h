/* mmgen — C ABI of the MI355X chunk-generation path (libmmgen.so).
 *
 * Drop-in boundary for the GPU stages of the reference's `Chunk` class (src/terrain/chunk.hpp:99-172, called only from
 * Terrain::tick, src/terrain/terrain.cpp:643-937).  Each entry point replaces the device part of one reference stage;
 * the reference's host part (pack / H2D / D2H / unpack) stays with the caller (see INTEGRATION.md and the C++ mirror in
 * mega-minecraft_amd/host/).  Conventions:
 *   - every pointer prefixed d_ is a DEVICE pointer owned by the caller, laid out exactly like the reference's staging
 *     buffers (sizes in mmgen_types.h); nothing is allocated or freed across the boundary;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on it;
 *   - return value: 0 on success, otherwise the hipError_t value (mmgen_error_string() names it).  The reference's
 *     convention "print + exit(EXIT_FAILURE)" (src/cuda/cuda_utils.cpp:5-17) is kept by the C++ wrapper, not here;
 *   - the library is stateless with respect to ChunkState (src/terrain/chunk.hpp:18-32): the caller advances it.
 */
#ifndef MMGEN_H
#define MMGEN_H
#include <stddef.h>
#include "mmgen_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* BiomeUtils::init() (src/terrain/biome.hpp:299-305, biomeFuncs.hpp:725-1256) + cudaSetDevice (src/main.cpp:31).
 * Rule tables are compile-time constants of the code object; this selects the device, checks it is gfx950 and builds the per-device
 * simplex-noise lookup image (one tiny launch + wait), so that no later call synchronises or allocates behind the caller's back.
 * Threading contract: calls may come from several host threads, streams and devices; the library-owned scratch of the per-stage
 * calls (mmgen_generate_caves, mmgen_erode_zone(s), mmgen_fill) is keyed by (device, stream), so calls on different streams never
 * share a buffer; calls that use the SAME stream from several threads must be serialised by the caller (the reference is
 * single-threaded, terrain.cpp:587-960).  A mmgen_region owns its scratch. */
int mmgen_init(int device);
const char* mmgen_error_string(int code);
/* pre-size the library-internal scratch of the per-stage calls on `stream` (per-column cave info, fill's voxel lists: 393 KB per chunk, at most 8 192 chunks' worth = 3.2 GB per (device, stream) for a full reserve) so that later
 * calls on that stream allocate nothing (graph capture).  Scratch is keyed by (device, stream). */
int mmgen_reserve(int max_chunks_per_call, void* stream);
/* frees the library-internal scratch kept for `stream` on the current device (synchronises it first): call before destroying a stream,
 * so that the entry does not outlive it and a recycled handle does not inherit its buffers.  mmgen_release_all: every stream, every
 * device entry (synchronises the current device).  Threading: per-stage calls on ONE (device, stream) and a release of that stream must
 * not run concurrently (a stage call launches with pointers into the entry the release frees); different streams are independent. */
int mmgen_release(void* stream);
int mmgen_release_all(void);

/* Chunk::generateHeightfields, device part (chunk.cu:150-185,207-213): kernGenerateHeightfield.
 * in : d_chunk_world_block_pos [n][2] int32 (x, z) world block position of each chunk's (0,0) column
 * out: d_heightfields [n][256] f32, d_biome_weights [n][24][256] f32 */
int mmgen_generate_heightfields(const int32_t* d_chunk_world_block_pos, int num_chunks, float* d_heightfields, float* d_biome_weights,
                                void* stream);

/* Same, fused with Chunk::gatherHeightfield (chunk.cu:231-302): additionally writes the 18x18 gathered heightfield
 * d_gathered [n][324] (ring columns recomputed from position — identical values to the neighbours' heightfields). */
int mmgen_generate_heightfields_gathered(const int32_t* d_chunk_world_block_pos, int num_chunks, float* d_heightfields, float* d_biome_weights,
                                         float* d_gathered, void* stream);

/* Chunk::generateLayers, device part (chunk.cu:308-415,448-455): kernGenerateLayers.
 * in : d_gathered_heightfields [n][324], d_biome_weights [n][24][256], positions; out: d_layers [n][20][256] */
int mmgen_generate_layers(const float* d_gathered_heightfields, const float* d_biome_weights, const int32_t* d_chunk_world_block_pos,
                          int num_chunks, float* d_layers, void* stream);

/* Chunk::fixBackwardStratifiedLayers (chunk.cu:725-749), run by Chunk::erodeZone after (or instead of) erosion. */
int mmgen_fix_backward_layers(float* d_layers, int num_chunks, void* stream);

/* Chunk::erodeZone, device part (chunk.cu:477-601 kernDoErosion + the relaxation loop :672-705).
 * d_gathered_layers: the packed zone buffer of copyLayers(..., true) (chunk.cu:603-656): 8 eroded-layer start planes + the heightfield
 * plane over the 384x384 zone grid (+1 trailing flag word, unused here), MMGEN_GATHERED_LAYERS_SIZE floats; eroded IN PLACE.
 * d_accumulated_heights: 147456 floats, overwritten with the accumulated lift (may be NULL).  Synchronous on return, like the reference.
 * Canonical semantics: synchronous Jacobi passes; the reference's in-place update races between thread blocks. */
int mmgen_erode_zone(float* d_gathered_layers, float* d_accumulated_heights, void* stream);
/* The relaxation loop runs on the device as one persistent launch whose workgroups wait for each other; no wait is unbounded.  If a zone's
 * workgroups do not meet within MMGEN_EROSION_TIMEOUT_MS (environment; default 2 000 ms, a thousand times the longest healthy wait) the
 * launch ends itself - starvation is the realistic cause: persistent kernels of other processes, or of this one on other streams, holding
 * its slots - and the RESCUE PASS enqueued right behind it relaxes every zone that is not done (abandoned, or never drawn because the
 * device handed the launch's workgroups to its XCDs differently than assumed) with single workgroups that wait for nobody: same planes,
 * same pass counts, only slower.  Like the reference's host loop (chunk.cu:682-705) the relaxation therefore cannot fail; a launch that
 * gave up is reported on stderr and counted (mmgen_erosion_stalls).  The code below is kept for ABI stability; no call returns it. */
#define MMGEN_ERROR_EROSION_STALL 20002
/* Batched form: num_zones buffers of MMGEN_GATHERED_LAYERS_SIZE floats back to back (ONE persistent launch relaxes all zones to
 * convergence: the host loop of chunk.cu:682-705 runs on the device, a zone's workgroups meet at a barrier after every block of passes);
 * *max_passes (nullable) receives the largest number of relaxation passes any zone needed. */
int mmgen_erode_zones(float* d_gathered_layers, int num_zones, float* d_accumulated_heights, int* max_passes, void* stream);

/* Chunk::generateCaves, device part (chunk.cu:755-937,970-981): default-fill + kernGenerateCaves.
 * out: d_cave_layers [n][256][32] mmgen_cave_layer */
int mmgen_generate_caves(const float* d_heightfields, const float* d_biome_weights, const int32_t* d_chunk_world_block_pos, int num_chunks,
                         mmgen_cave_layer* d_cave_layers, void* stream);

/* Chunk::generateFeaturePlacements (chunk.cu:999-1156; CPU in the reference, a device kernel here) for a batch of chunks.
 * in : heightfields, biome weights, (eroded, fixed-up) layers, cave layers, positions
 * out: d_feature_placements [n][MMGEN_FP_CAP], d_cave_feature_placements [n][MMGEN_CFP_CAP] in the reference's emission order
 *      (columns z-major, then emission order inside a column), d_counts [n][2] int32 = list lengths (cave count may exceed the cap:
 *      the surplus is dropped and reported by the count). */
int mmgen_generate_feature_placements(const float* d_heightfields, const float* d_biome_weights, const float* d_layers,
                                      const mmgen_cave_layer* d_cave_layers, const int32_t* d_chunk_world_block_pos, int num_chunks,
                                      mmgen_feature_placement* d_feature_placements, mmgen_cave_feature_placement* d_cave_feature_placements,
                                      int32_t* d_counts, void* stream);

/* Chunk::gatherFeaturePlacements (chunk.cu:1158-1196) + the host part of Chunk::fill (chunk.cu:1555-1601) on a rectangular chunk grid:
 * the per-chunk lists above are indexed by grid cell (cell = cx + grid_w * cz); for each of the num_targets cells named by
 * d_target_cells the 49 neighbour lists are concatenated in the reference's fixed offset order, truncated to 2048 / 4096 entries and
 * NONE-terminated; d_feature_bounds [num_targets][4] receives {allFeaturesHeightBounds, allCaveFeaturesHeightBounds} of the
 * un-truncated lists.  Neighbours outside the grid contribute nothing (the reference never fills such a chunk). */
int mmgen_gather_feature_placements(const mmgen_feature_placement* d_feature_placements, const mmgen_cave_feature_placement* d_cave_feature_placements,
                                    const int32_t* d_counts, const int32_t* d_target_cells, int num_targets, int grid_w, int grid_h,
                                    mmgen_feature_placement* d_gathered, mmgen_cave_feature_placement* d_gathered_cave, int32_t* d_feature_bounds,
                                    void* stream);

/* Chunk::placeDecorators (chunk.cu:1634-1747; CPU in the reference, after the D2H of the blocks), in place on d_blocks. */
int mmgen_place_decorators(uint8_t* d_blocks, const float* d_heightfields, const float* d_biome_weights, const mmgen_cave_layer* d_cave_layers,
                           const int32_t* d_chunk_world_block_pos, int num_chunks, void* stream);

/* Chunk::fill, device part (chunk.cu:1202-1510,1603-1616): kernFill for every chunk of the batch in ONE launch.
 * d_feature_placements / d_cave_feature_placements: [n][2048] / [n][4096] NONE-terminated gathered lists (may be NULL = empty),
 * d_feature_bounds [n][4] int32 = {allFeaturesHeightBounds.xy, allCaveFeaturesHeightBounds.xy} (chunk.cu:1555-1570; NULL with NULL lists).
 * out: d_blocks [n][98304] u8 */
int mmgen_fill(const float* d_heightfields, const float* d_biome_weights, const float* d_layers, const mmgen_cave_layer* d_cave_layers,
               const int32_t* d_chunk_world_block_pos, int num_chunks, const mmgen_feature_placement* d_feature_placements,
               const mmgen_cave_feature_placement* d_cave_feature_placements, const int32_t* d_feature_bounds, uint8_t* d_blocks, void* stream);

/* ---- Region fast path: a rectangle of chunks through ALL stages without leaving the device between stages -------------------
 * Replaces, for a batch world, the per-tick stage dispatch of Terrain::tick (src/terrain/terrain.cpp:643-937) and its host round
 * trips.  The region owns its scratch (grow-only device buffers); results go to caller-owned device buffers.
 * Chunks are ordered z-major: index = (cx - cx0) + nx * (cz - cz0).  flags select the stages that are optional in the reference
 * (DEBUG_SKIP_EROSION chunk.cu:12,665-715; features / decorators).  Canonical region semantics: DESIGN.md. */
#define MMGEN_REGION_EROSION 1u
#define MMGEN_REGION_FEATURES 2u
#define MMGEN_REGION_DECORATORS 4u
/* mmgen_region_generate only: compute the 3-chunk ring's placement lists in full (mask 1 below) instead of lazily (mask 2).  The blocks
 * are the same unless a chunk's gathered list exceeds the reference's truncation (2 048 surface / 4 096 cave entries, chunk.cu:1573-1601):
 * the reference truncates the FULL list, a lazy ring can only truncate its shortened one, so entries the reference drops could be kept.
 * The full lengths cannot be known without the work the lazy ring saves; mmgen_region_max_gathered reports what a run has seen. */
#define MMGEN_REGION_EXACT_RING 256u
typedef struct mmgen_region mmgen_region;
int mmgen_region_create(mmgen_region** out);
void mmgen_region_destroy(mmgen_region* region);
/* one call: begin + finish */
int mmgen_region_generate(mmgen_region* region, int cx0, int cz0, int nx, int nz, unsigned flags, uint8_t* d_blocks /*[nx*nz][98304]*/,
                          float* d_heightfields /*[nx*nz][256], nullable*/, void* stream);
/* two-phase form for spatial multi-GPU tiling: begin runs heightfield .. feature placements on the tile plus its 3-chunk ring;
 * h_local_mask (host, [(nx+6)*(nz+6)] bytes over the ring-extended grid, nullable = all 1) says for every RING cell who provides its
 * placement lists (cells of the rectangle itself are always computed in full):
 *   0  the caller writes them into the placement buffers before finish (RCCL halo exchange with the neighbouring tiles, a cache);
 *   1  computed here, complete (the lists may be kept and re-used as ring cells of later regions);
 *   2  computed here LAZILY: only the placements that can reach the rectangle are generated, and only the columns that can produce one
 *      get cave noise (a cave feature reaches <= 8 blocks; a surface feature only stands on its gen's jittered grid point, chunk.cu:999-1008,
 *      which is known before the caves are) - about 1/5 of the ring's cave work.  The blocks of the rectangle are identical; the
 *      ring's lists are a subset of the complete ones and must not be re-used elsewhere.  mmgen_region_generate uses 2 throughout. */
int mmgen_region_begin(mmgen_region* region, int cx0, int cz0, int nx, int nz, unsigned flags, const uint8_t* h_local_mask, void* stream);
int mmgen_region_placement_buffers(mmgen_region* region, mmgen_feature_placement** d_fp /*[grid][MMGEN_FP_CAP]*/,
                                   mmgen_cave_feature_placement** d_cfp /*[grid][MMGEN_CFP_CAP]*/, int32_t** d_counts /*[grid][2]*/,
                                   int* grid_cx0, int* grid_cz0, int* grid_w, int* grid_h);
/* optional middle step: the base blocks of the rectangle (kernFill without feature lists, chunk.cu:1202-1510).  It needs nothing from the
 * placement ring, so a tiling caller issues it while the ring exchange is in flight; finish (same d_blocks) then skips it. */
int mmgen_region_fill(mmgen_region* region, uint8_t* d_blocks, void* stream);
/* optional, BEFORE a begin: names the block buffer the region is going to be finished into, which lets that begin issue the base fill
 * itself as soon as the caves' extents and the eroded layers exist - beside the cave biomes and the placement stages, which only the
 * rasterisers wait for - instead of when mmgen_region_fill / _finish is called (then a no-op for the same pointer).  The fill is ordered
 * behind what the stream held when begin was CALLED: the caller promises that nothing it enqueues between that begin and the finish
 * reads or writes d_blocks.  One-shot (cleared by the begin); ignored in the serial schedule.  mmgen_region_generate does this itself. */
int mmgen_region_set_output(mmgen_region* region, uint8_t* d_blocks);
int mmgen_region_finish(mmgen_region* region, uint8_t* d_blocks, float* d_heightfields /*nullable*/, float* d_layers /*[n][20][256], nullable*/,
                        mmgen_cave_layer* d_cave_layers /*[n][256][32], nullable*/, void* stream);
/* waits for the erosion branch of the last begin and returns the largest pass count of its zones (-1: the wait itself failed) */
int mmgen_region_last_erosion_passes(const mmgen_region* region);
/* The longest gathered (un-truncated) surface / cave placement list any chunk had in the finishes since the last call (synchronises the
 * stream; clears the record).  With a full ring (mask 1 or peer-provided lists) these are the lengths the reference's Chunk::fill truncates
 * at MMGEN_MAX_GATHERED_FEATURES_PER_CHUNK / MMGEN_MAX_GATHERED_CAVE_FEATURES_PER_CHUNK; below them nothing is truncated and the lazy ring
 * gives the same blocks.  (A generated world stays below a third of either limit: tests/test_gpu_features.py.) */
int mmgen_region_max_gathered(mmgen_region* region, int* out_surface, int* out_cave, void* stream);
/* The one capacity of this library that the reference does not have: a chunk's cave placement list holds MMGEN_CFP_CAP entries (the
 * reference pushes into an unbounded vector, chunk.cu:1028-1038; a chunk of a generated world carries < 100, the worst case the
 * algorithm allows is 16 384).  Entries beyond the capacity are dropped, which would change blocks - so it is reported, not hidden:
 * mmgen_region_finish checks every list length it is about to gather (its own and the ones that arrived from other GPUs) on the device
 * and records the largest in host-visible memory; from then on mmgen_region_begin / _finish return MMGEN_ERROR_PLACEMENT_OVERFLOW
 * until the caller acknowledges it.  mmgen_region_max_cave_placements synchronises `stream`, returns the largest cave list length seen
 * since the last call (<= MMGEN_CFP_CAP means nothing was dropped) and clears the record.  (Surface lists cannot overflow: at most one
 * placement per column, MMGEN_FP_CAP = 256.  The per-stage call mmgen_generate_feature_placements returns the raw counts to its caller.) */
#define MMGEN_ERROR_PLACEMENT_OVERFLOW 20001
int mmgen_region_max_cave_placements(mmgen_region* region, int* out_max, void* stream);
/* How the region schedules its stages.  Default (serial = 0): a stage DAG over the caller's stream and three
 * internal ones - the erosion branch (one persistent relaxation launch per zone batch, no host read-backs, finish, fix-up) beside the
 * caves, which need none of it (the reference rotates five streams over its stages, terrain.cpp:129,179-182); the base fill on its own
 * stream, ordered behind whatever the caller's stream holds when d_blocks is first passed in - or, after mmgen_region_set_output, behind
 * what it held when begin was called, and then started by begin itself; the rectangle optionally cut into `slices` z slices (0 =
 * automatic = 1) with the rasterisers / decorators of slice i beside the fill of slice i + 1.  Every internal stream is joined into the
 * caller's stream before mmgen_region_finish returns, so callers order against that one stream only; no region call blocks the host
 * except the three queries (last_erosion_passes, max_cave_placements, max_gathered) and set_serial, which waits for the internal streams.
 * serial = 1: every kernel on the caller's stream in the reference's stage order (what per-kernel timing and the counters want); also
 * selected by MMGEN_REGION_SERIAL=1 in the environment.  Results are identical. */
int mmgen_region_set_serial(mmgen_region* region, int serial, int slices);
/* Streaming callers (host/region_terrain.cpp): keep the eroded layers of up to max_zones whole zones (1.18 MB each, device memory of the
 * region) across calls; 0 = off (the default) and frees them.  A region call then relaxes only the covering zones it has not seen, and
 * runs K1 / K2 on their gathered areas only - a thin strip of new chunks touches up to ten zones, each a 24 x 24-chunk gather and a full
 * relaxation in the reference (terrain.cpp:471-522, chunk.cu:658-723).  Results are identical: with the canonical raw padding (DESIGN.md
 * section 4) a zone's eroded layers are a pure function of its position.  Least recently used zones make room.  Synchronises the device.
 * Not for throughput measurements of a fixed rectangle (every call after the first would skip the erosion).
 * mmgen_region_zone_cache_stats: zones served from the cache / relaxed since the last set_zone_cache. */
int mmgen_region_set_zone_cache(mmgen_region* region, int max_zones);
int mmgen_region_zone_cache_stats(const mmgen_region* region, long long* hits, long long* misses);
/* Copies the placement lists of n whole cells between two placement grids with the per-cell layout of mmgen_region_placement_buffers
 * (fp [cells][MMGEN_FP_CAP], cfp [cells][MMGEN_CFP_CAP], counts [cells][2]): cell d_dst_idx[i] of dst <- cell d_src_idx[i] of src.  A streaming
 * caller keeps the lists of chunks it has generated in its own grid and feeds them back as ring cells of later regions (mask 0 in
 * mmgen_region_begin) instead of having their caves and placements recomputed. */
int mmgen_copy_placements(const mmgen_feature_placement* d_src_fp, const mmgen_cave_feature_placement* d_src_cfp, const int32_t* d_src_counts,
                          const int32_t* d_src_idx, mmgen_feature_placement* d_dst_fp, mmgen_cave_feature_placement* d_dst_cfp, int32_t* d_dst_counts,
                          const int32_t* d_dst_idx, int n, void* stream);

/* Compact wire form of placement-grid cells for the ring exchange between spatial tiles (SURVEY 8e "counts, then payload"; the reference
 * has no multi-GPU path, the lists are those of chunk.cu:1158-1196).  For a list of n grid cells d_cells:
 *   mmgen_ring_header : d_header [n][2] = the cells' two list lengths (as counted, a cave count may exceed MMGEN_CFP_CAP);
 *   mmgen_ring_offsets: d_offsets [n+1] = exclusive scan of the cells' payload words 5 min(c0, FP_CAP) + 6 min(c1, CFP_CAP)
 *                       (both sides run it: the receiver sizes its payload buffer from the received header);
 *   mmgen_ring_pack   : payload words of cell i at d_payload + d_offsets[i]: its surface entries (5 words each), then its cave entries (6);
 *   mmgen_ring_unpack : the inverse, into the placement grid of the receiver, lengths included.
 * Cells of several peers are handled in one call: concatenate the peers' cell lists, the peers' messages are contiguous slices. */
int mmgen_ring_header(const int32_t* d_counts, const int32_t* d_cells, int n, int32_t* d_header, void* stream);
int mmgen_ring_offsets(const int32_t* d_header, int n, int32_t* d_offsets, void* stream);
int mmgen_ring_pack(const mmgen_feature_placement* d_fp, const mmgen_cave_feature_placement* d_cfp, const int32_t* d_cells, const int32_t* d_header,
                    const int32_t* d_offsets, int n, int32_t* d_payload, void* stream);
int mmgen_ring_unpack(const int32_t* d_payload, const int32_t* d_header, const int32_t* d_offsets, const int32_t* d_cells, int n,
                      mmgen_feature_placement* d_fp, mmgen_cave_feature_placement* d_cfp, int32_t* d_counts, void* stream);

/* The same exchange in ONE phase, with no host read between counting and sending (what a host that must never synchronise mid-step
 * wants: nothing it needs to know depends on the lists).  The cells of each peer form one message whose size follows from the layout alone:
 *   [2 words per cell: its two raw list lengths][the cells' entries packed back to back, as above][slack up to the message's capacity].
 * d_slots [n][4] (built once per layout by the host): word index of the cell's two lengths in d_messages, first payload word of its
 * peer's message, index (into d_cells) of that peer's first cell, the message's payload capacity in words.  A typical cell carries
 * 250 - 750 words; 5 * MMGEN_FP_CAP + 6 * MMGEN_CFP_CAP = 7 424 words per cell can never overflow.  If a message's entries do not fit,
 * sender and receiver both see it from the lengths: *d_overflow (device, cleared by the caller) is raised to the number of payload words
 * that message needed and the cells that did not fit arrive EMPTY - check it before trusting the step, and retry with more slack.
 * d_scratch: 3 n + 1 words.  Same kernels on both sides; cells of several peers in one call. */
int mmgen_ring_pack_messages(const mmgen_feature_placement* d_fp, const mmgen_cave_feature_placement* d_cfp, const int32_t* d_counts, const int32_t* d_cells,
                             const int32_t* d_slots, int n, int32_t* d_scratch, int32_t* d_messages, int32_t* d_overflow, void* stream);
int mmgen_ring_unpack_messages(const int32_t* d_messages, const int32_t* d_cells, const int32_t* d_slots, int n, int32_t* d_scratch,
                               mmgen_feature_placement* d_fp, mmgen_cave_feature_placement* d_cfp, int32_t* d_counts, int32_t* d_overflow, void* stream);

/* Measurement hooks (not part of the reference's interface): when enabled every kernel launch is bracketed by HIP events on its
 * launch stream; mmgen_profile_collect() waits for them and returns total milliseconds and launch counts per kernel id
 * (arrays of mmgen_profile_num_kernels() entries), then clears the records. */
void mmgen_profile_enable(int on);
int mmgen_profile_num_kernels(void);
const char* mmgen_profile_kernel_name(int id);
int mmgen_profile_collect(double* total_ms, long long* counts);

/* ---- mesh build that follows the path ------------------------------------------------------
 * Replaces Chunk::createVBOs (src/terrain/chunk.cu:1778-2003), the host loop over 98 304 voxels x 6 neighbours per chunk.
 * d_blocks: [*][98304] block ids (a batch, a whole region grid or a pool of chunk slots); d_chunk_idx: [n] which chunks of
 * d_blocks to mesh (NULL = chunks 0 .. n-1); every other per-chunk array is indexed by the position in that work list.
 * d_neighbor_idx: [n][4] index into d_blocks of the N (+z), E (+x), S (-z), W (-x) neighbour chunk, -1 = absent (faces towards an
 * absent chunk are not emitted, chunk.cu:1906), NULL = all absent.  Vertices are the reference's Vertex (40 bytes), indices are local to their chunk, order is the reference's
 * (z, x, y; faces in DirectionEnums::dirVecs order); a chunk with V vertices has exactly 3 V / 2 indices.
 *   mmgen_mesh_count: d_column_verts [n][256] and d_chunk_verts [n] receive the vertex counts.
 *   mmgen_mesh_fill : writes chunk c's vertices at d_verts[d_vert_offset[c] ...] and its indices at d_idx[d_vert_offset[c] * 3 / 2 ...]
 *                     (d_vert_offset: exclusive prefix of d_chunk_verts, computed by the caller who also sizes the buffers);
 *                     d_chunk_world_block_pos [n][2] = (x, z) world block origin of each chunk (X-shaped jitter and uv rotation seeds). */
int mmgen_mesh_count(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n, uint32_t* d_column_verts,
                     uint32_t* d_chunk_verts, void* stream);
int mmgen_mesh_fill(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, const int32_t* d_chunk_world_block_pos, int n,
                    const uint32_t* d_column_verts, const uint64_t* d_vert_offset, mmgen_vertex* d_verts, uint32_t* d_idx, void* stream);
/* The same without a host round trip between the count and the fill (a streaming tick: the host neither reads the counts nor uploads the
 * offsets before the fill is enqueued):
 *   mmgen_mesh_offsets      d_vert_offset[c] = exclusive prefix of d_chunk_verts on the device, d_total[0] = their sum;
 *   mmgen_mesh_fill_capped  mmgen_mesh_fill that writes nothing for a chunk whose vertices would end beyond capacity_verts (the caller sized
 *                           d_verts / d_idx for capacity_verts vertices from what earlier ticks needed; it reads d_total afterwards, and when
 *                           that exceeds the capacity it grows the buffers and repeats the three calls);
 *   mmgen_mesh_fill_strip   both in ONE launch for 1 <= n <= 256 chunks (a streaming tick's strip): every workgroup sums the counts of the
 *                           chunks before its own (d_chunk_verts from mmgen_mesh_count), d_vert_offset / d_total are OUTPUTS. */
int mmgen_mesh_offsets(const uint32_t* d_chunk_verts, int n, uint64_t* d_vert_offset, uint64_t* d_total, void* stream);
int mmgen_mesh_fill_strip(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, const int32_t* d_chunk_world_block_pos, int n,
                          const uint32_t* d_column_verts, const uint32_t* d_chunk_verts, uint64_t* d_vert_offset, uint64_t* d_total, uint64_t capacity_verts,
                          mmgen_vertex* d_verts, uint32_t* d_idx, void* stream);
int mmgen_mesh_fill_capped(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, const int32_t* d_chunk_world_block_pos, int n,
                           const uint32_t* d_column_verts, const uint64_t* d_vert_offset, uint64_t capacity_verts, mmgen_vertex* d_verts, uint32_t* d_idx,
                           void* stream);

/* ---- greedy-merged compact quad mesh -----------------------------------------------------------------------------------
 * A second mesher with its own contract: coplanar, adjacent faces of ONE block id merged into rectangles, one 64-bit record per quad
 * (mmgen_types.h "quad record") for vertex pulling.  d_blocks / d_chunk_idx / d_neighbor_idx exactly as in mmgen_mesh_count.  The quad
 * stream of a chunk is a pure function of its blocks, its four neighbours' blocks and which neighbours are present; the kernels return
 * exactly this stream, in this order.
 *
 * FACE SET F = the display rule of mmgen_mesh_* (chunk.cu:1906-1928) over the block table's classes AIR, OPAQUE, SEMI, TRANSPARENT,
 * X_SHAPED (ids >= MMB_NUM_BLOCKS count as OPAQUE); directions in dirVecs order +z 0, +x 1, -z 2, -x 3, +y 4, -y 5:
 *   an X-shaped block has no faces, it emits one record of kind 6;
 *   opaque or semi-transparent block: face d is in F iff the neighbour's class is not OPAQUE;
 *   transparent block: face d is in F iff the neighbour is AIR or SEMI;
 *   a horizontal neighbour outside the chunk is read from the neighbour chunk when present; when it is absent the face is NOT in F;
 *   below y = 0 and above y = 383 the neighbour is AIR.
 * PLANES: a face belongs to plane (d, p) with rows r and fast axis q:
 *   d in {0, 2}: p = z, r = x, q = y;     d in {1, 3}: p = x, r = z, q = y;     d in {4, 5}: p = y, r = z, q = x.
 * GREEDY RULE per plane: visit the cells with r ascending, then q ascending.  At the first cell (r0, q0) in F and not yet covered, of block
 * id b: L = the largest length such that every cell (r0, q0 .. q0+L-1) is in F, uncovered and of id b; W = the largest count such that for
 * every row r0 .. r0+W-1 all cells (r, q0 .. q0+L-1) are in F, uncovered and of id b; emit one quad of W rows x L cells and mark them
 * covered.  Faces of different block ids never share a quad, even within one class.  Nothing merges across a chunk border.
 * ORDER of a chunk's records: the planes with d ascending, then p ascending, each in emission order; then the kind-6 records in ascending
 * voxel index y + 384 (x + 16 z).  Each (d, p) is one group and the kind-6 records one more: 64 + 768 + 1 = MMGEN_QUAD_GROUPS, group index
 * 16 d + p for d < 4, 64 + 384 (d - 4) + p for d >= 4, 832 for kind 6.
 * NOT REPRESENTED: the per-face random uv rotation and flip of the reference's Vertex stream.  A consumer tiles the block's texture over the
 * quad; the material follows from the block id as in the vertex mesher (mesh_material, chunk.cu:1797-1829).
 *
 *   mmgen_mesh_quads_count: d_group_quads [n][MMGEN_QUAD_GROUPS] and d_chunk_quads [n] receive the record counts.
 *   mmgen_mesh_quads_fill : writes chunk i's records at d_quads[d_quad_offset[i] ...]; d_quad_offset = exclusive prefix of d_chunk_quads
 *                           (mmgen_mesh_offsets computes it on the device unchanged: count -> offsets -> fill needs no host read).  A chunk
 *                           whose records would end beyond capacity_quads writes nothing; UINT64_MAX = uncapped, 0 is hipErrorInvalidValue.
 * Nothing is allocated; all calls are asynchronous on `stream`. */
#define MMGEN_QUAD_GROUPS 833
int mmgen_mesh_quads_count(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n,
                           uint32_t* d_group_quads /*[n][MMGEN_QUAD_GROUPS]*/, uint32_t* d_chunk_quads /*[n]*/, void* stream);
int mmgen_mesh_quads_fill(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n,
                          const uint32_t* d_group_quads, const uint64_t* d_quad_offset, uint64_t capacity_quads,
                          uint64_t* d_quads, void* stream);

/* ---- ray casting over device-resident chunks -------------------------------------------------------------------------------
 * The reference's only consumer of a generated chunk is OptixRenderer::buildChunkAccel (RT-core hardware).  Here line of sight, block
 * picking and a headless camera run against the blocks where they lie: d_blocks [*][98304] (a region's output, a pool of chunk slots),
 * d_grid [grid_h][grid_w] = index into d_blocks of the chunk at grid cell (cx, cz), -1 = absent.
 *
 * THE TRAVERSAL CONTRACT (results are a pure function of the inputs; the kernels' skip structure returns exactly this):
 *   A ray is (o, d), six f32, in GRID-LOCAL block coordinates: x in [0, 16 grid_w), z in [0, 16 grid_h), y = world y (f32 stays exact at
 *   far world positions).  d need not be normalised.  The ray is INVALID (voxel 0, t 0, face 6) unless every component is finite, o lies in
 *   the grid's xz rectangle, o.y in [-1024, 1408), d is not all zero and 1.0f / d_a is finite for every d_a != 0.
 *   Setup: inv_a = 1.0f / d_a (correctly rounded) for d_a != 0; an axis with d_a == 0 never steps.  v = floor(o), t = 0, face = 6 (none).
 *   EXAMINE v, in this order:
 *     v outside the xz rectangle                                   -> LEFT_GRID
 *     v.y < 0 with d_y <= 0, or v.y >= 384 with d_y >= 0           -> LEFT_GRID
 *     any other v.y outside [0, 384)                               -> air
 *     d_grid[v.z >> 4][v.x >> 4] == -1                             -> ABSENT_CHUNK (at the first voxel inside that cell)
 *     block = d_blocks[chunk][v.y + 384 ((v.x & 15) + 16 (v.z & 15))]; its class in stop_mask -> HIT (block reported), else air
 *   A status ends the ray and reports v, t, face (block = 0 unless HIT).  So a ray that starts inside a stopping block is a HIT with
 *   t = 0, face = 6.  On air, STEP - non-incremental, from the integer voxel, nothing accumulated:
 *     for every axis with d_a != 0: p_a = v_a + (d_a > 0), t_a = ((float)p_a - o_a) * inv_a      (two roundings, no fused multiply-add)
 *     a = the axis with the smallest t_a, ties to the lowest axis index (x, y, z)
 *     t_a > t_max -> MISS_TMAX, reporting the voxel the ray stands in, t = t_max, face = 6
 *     otherwise v_a += sign(d_a), t = t_a, face = the dirVecs index (+z 0, +x 1, -z 2, -x 3, +y 4, -y 5) of the outward normal of the
 *     face entered (a step towards +x enters through the -x face: 3), and EXAMINE again.
 *   stop_mask: bit set over the mesher's block classes (MMGEN_RAY_OPAQUE 1, _SEMI 2, _TRANSPARENT 4, _XSHAPED 8); 0 or > 15 is
 *   hipErrorInvalidValue, as are a t_max that is negative or not finite, null pointers and grid sides outside [1, 16384].
 *   flags: MMGEN_RAY_NO_SKIP walks exactly as written above, one voxel per step (testing, and pricing the skip structure);
 *   MMGEN_RAY_COUNT_VISITS replaces hit.voxel by {blocks read, boxes classified, brick masks read} (status, t, face, block unchanged).
 *
 * mmgen_ray_occupancy builds the skip structure of n chunks for ONE stop_mask: d_occupancy [*][MMGEN_RAY_OCCUPANCY_BYTES], indexed like
 * d_blocks (chunk d_chunk_idx[i], or i when d_chunk_idx is NULL, writes its own 200 bytes: a pool refreshes only the slots that changed).
 * Per chunk: u64 whose bit sy says that 16^3 section sy holds a stopping block, then per section a u64 over its 4^3 bricks, bit
 * by + 4 (bx + 4 bz).  mmgen_raycast / _camera must be given the occupancy of the same blocks and the same stop_mask; every chunk the grid
 * names must have been built.  Nothing is allocated; all calls are asynchronous on `stream`.
 *
 * mmgen_raycast: d_rays [n][6] (o, d), d_hits [n].
 * mmgen_raycast_camera: d_hits [height][width]; pixel (i, j) (column i, row j, row 0 on top) casts the ray o = eye,
 *     d_a = (F_a + sx * R_a) + sy * U_a,    sx = ((float)i + 0.5f) * (2.0f / (float)width) - 1.0f,   sy = 1.0f - ((float)j + 0.5f) * (2.0f / (float)height)
 * in f32 without fused multiply-add, where the basis is computed ONCE on the host in double and rounded to f32:
 *     f = forward / sqrt(forward . forward),  r = f x up,  r /= sqrt(r . r),  u = r x f   (dot products summed x, y, z)
 *     F = (float)f,  R = (float)(r * (tan(0.5 * fov_y) * ((double)width / (double)height))),  U = (float)(u * tan(0.5 * fov_y))
 * so a camera image equals mmgen_raycast on rays built from this formula, record for record. */
int mmgen_ray_occupancy(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, unsigned stop_mask, uint8_t* d_occupancy, void* stream);
int mmgen_raycast(const uint8_t* d_blocks, const int32_t* d_grid, int grid_w, int grid_h, const uint8_t* d_occupancy, unsigned stop_mask, unsigned flags,
                  const float* d_rays, int n, float t_max, mmgen_ray_hit* d_hits, void* stream);
int mmgen_raycast_camera(const uint8_t* d_blocks, const int32_t* d_grid, int grid_w, int grid_h, const uint8_t* d_occupancy, unsigned stop_mask, unsigned flags,
                         const mmgen_camera* cam, float t_max, mmgen_ray_hit* d_hits, void* stream);

/* ---- shaded camera render: camera -> RGBA8 in one launch (light, AO, water, sun shadow, fog) ---------------------------------
 * The reference's product is an image.  mmgen_render_camera turns what this header keeps on the device - blocks, the light volume, the
 * occluder rule of the AO mesher - into pixels without a host round trip.  d_blocks, d_grid, cam and the pixel-to-ray formula are exactly
 * those of mmgen_raycast_camera; d_rgba [height][width] = r | g << 8 | b << 16 | alpha << 24.  The image is a pure function of the inputs.
 *
 * WALKS, all three THE TRAVERSAL CONTRACT above, unchanged, with p->t_max:
 *   A  the pixel's camera ray, stop_mask = p->first_mask (must contain MMGEN_RAY_OPAQUE), occupancy d_occ_first.  d_hits, when given,
 *      receives exactly what mmgen_raycast_camera writes for that mask.
 *   B  only with MMGEN_RENDER_TRANSLUCENT when A is a HIT on a TRANSPARENT-class block: the same ray (o, d), stop_mask = OPAQUE | SEMI,
 *      occupancy d_occ_second; its result is that of a fresh walk.
 *   S  only with MMGEN_RENDER_SUN_SHADOW when A is a HIT with face != 6: o = the centre of the front voxel f = v + dirVec(face)
 *      (f_a + 0.5f, exact in f32), d = p->sun_dir, stop_mask = OPAQUE | SEMI, occupancy d_occ_second.  The pixel is SHADOWED iff S is a HIT
 *      (an INVALID S does not shadow).
 *   d_occ_second may be NULL iff neither of the two flags is set.
 * SHADING is integer only.  mul8(a, b) = (a * b + 127) / 255.
 *     RAMP[0..15] = 9, 11, 14, 18, 22, 27, 34, 43, 53, 67, 84, 104, 131, 163, 204, 255
 *     FACE[0..6]  = 204, 179, 153, 179, 255, 115, 255          AOW[0..3] = 115, 153, 204, 255
 *   shade(hit) for a HIT with voxel v, face, block id:  f = v + dirVec(face) (f = v when face == 6);  L = d_light at f when 0 <= f.y <= 383
 *   (indexed like d_blocks through d_grid; the walk guarantees that f's chunk is present), 0xF0 above the world, 0x00 below it, 0xF0
 *   everywhere when d_light is NULL;  lv = max((L >> 4) * sun_level / 15, L & 15);  per channel c of palette[id]:
 *   x = mul8(mul8(c, RAMP[lv]), FACE[face]).
 *   Walk A's hit takes two more factors: with MMGEN_RENDER_AO, face != 6 and a block of class OPAQUE or SEMI, x = mul8(x, A); if the pixel
 *   is shadowed, x = mul8(x, shadow_dim).
 * AO FACTOR A: the occluder is that of the AO mesher taken over the whole grid: O(u) = 1 iff u lies in a present chunk, 0 <= u.y <= 383 and
 *   its class is OPAQUE.  ao_k, k = 0..3, around f is the FACE AO formula below with its axes r and q.  The hit point on a tangential axis
 *   a is h_a = o_a + t * d_a (one f32 multiply, one f32 add, not fused);  u_a = clamp((int)floorf((h_a - (float)v_a) * 16.0f), 0, 15);  the
 *   weight of the + side of an axis is 2 u_a + 1, of the - side 31 - 2 u_a;  A = (sum over k of w_r(k) w_q(k) AOW[ao_k] + 512) >> 10.
 * THE PIXEL
 *   1  A is not a HIT: rgb = sky_rgb, alpha 0.          2  A is a HIT: C = shade(A) with its factors, alpha 255.
 *   3  walk B was taken: back = shade(B) when B is a HIT (no AO, no shadow factor), else sky_rgb;
 *      C = (C * al + back * (255 - al) + 127) / 255 per channel, al = the palette alpha of A's block.
 *   4  MMGEN_RENDER_FOG and A is a HIT: g = (int)(fminf(fmaxf((t_A - fog_start) * (1.0f / (fog_end - fog_start)), 0.f), 1.f) * 255.0f + 0.5f),
 *      every operation in f32;  C = (C * (255 - g) + sky_rgb * g + 127) / 255 per channel.
 * d_palette [256] on the device, r | g << 8 | b << 16 | alpha << 24; NULL = the default table (mmgen_render_default_palette returns it: a
 * colour per block id, alpha 255 except 150 for the TRANSPARENT-class ids).
 * hipErrorInvalidValue: what mmgen_raycast_camera rejects; a first_mask without OPAQUE or above 15; unknown flag bits; sun_level > 15; with
 * _FOG a fog_end that is not greater than fog_start or a fog value that is not finite; with _SUN_SHADOW a sun_dir that is zero or not
 * finite; a NULL d_occ_second under the rule above; a NULL d_rgba, cam or p.  Nothing is allocated; the call is asynchronous on `stream`. */
int mmgen_render_default_palette(uint32_t* h_out /*[256], host*/);
int mmgen_render_camera(const uint8_t* d_blocks, const int32_t* d_grid, int grid_w, int grid_h,
                        const uint8_t* d_occ_first, const uint8_t* d_occ_second /*nullable, see above*/,
                        const uint8_t* d_light /*[*][98304], nullable = full bright (0xF0 everywhere)*/,
                        const uint32_t* d_palette /*[256] device, NULL = default*/,
                        const mmgen_camera* cam, const mmgen_render_params* p,
                        uint32_t* d_rgba /*[height][width]*/, mmgen_ray_hit* d_hits /*[height][width], nullable*/, void* stream);

/* ---- voxel lighting: sky and block light over device-resident chunks --------------------------------------------------------
 * The reference gets its illumination from an OptiX path tracer and an emissive texture.  Here every voxel gets the classic pair of
 * 4-bit values, each dropping by one per step through voxels that are not opaque.  d_blocks, d_grid [grid_h][grid_w] (index into the
 * chunk slots, -1 = absent) exactly as in mmgen_raycast.  The light is a pure function of the grid's blocks and the emission table.
 *
 * THE LIGHT CONTRACT
 *   Block classes are the mesher's: AIR, OPAQUE, SEMI, TRANSPARENT, X_SHAPED; ids >= MMB_NUM_BLOCKS count as OPAQUE.  e[256] is the
 *   emission table, values 0..15 (a larger value is taken as 15); NULL selects the default table:
 *     LAVA, GLOWSTONE, SHROOMLIGHT, SEA_LANTERN 15;  CAVE_VINES_GLOW_MAIN, CAVE_VINES_GLOW_END 14;  MAGENTA_, CYAN_, GREEN_CRYSTAL 10;
 *     SMALL_ and HANGING_SMALL_ MAGENTA_, CYAN_, GREEN_CRYSTAL 6;  every other id 0     (mmgen_light_default_emission returns it).
 *   The domain is the voxels of the grid's present chunks.  Everything else - absent cells, cells outside the grid, y < 0, y > 383 - has
 *   T = 0, emits nothing, is not open and has light 0.
 *     T(v)     the class of v is not OPAQUE: light passes AIR, SEMI, TRANSPARENT and X_SHAPED alike, at a cost of 1 per step;
 *     open(v)  v and every voxel above it in its column, up to y = 383, is AIR or X_SHAPED;
 *     block(v) = max(e[id(v)], T(v) ? max over the 6 face neighbours n of block(n) - 1 : 0), never below 0: an opaque emitter carries its
 *                own emission and lights its neighbours, an opaque non-emitter is 0;
 *     sky(v)   = 15 if open(v), else T(v) ? max over the 6 face neighbours n of sky(n) - 1 : 0: water, ice and leaves under the open sky
 *                get 14, 13, ...
 *   Both fields are the unique solutions of these equations.  Equivalently, with S_16 = {} and dilate6 = the union of the six shifts:
 *     S_L = {source >= L} | (T & dilate6(S_L+1)) for L = 15 .. 1 (source = e[id] for block light, 15 on open voxels and 0 elsewhere for sky
 *     light), and the light of v is the number of L with v in S_L.
 *   Output: d_light[slot][y + 384 (x + 16 z)] = (sky << 4) | block, laid out and indexed like d_blocks.
 *   EXACTNESS: the light of a voxel depends only on the blocks within Manhattan distance 14 of it and on the column above it.  So a chunk
 *   whose 8 neighbours are present has the light of the unbounded world; a chunk next to an absent cell is darker towards it, absent cells
 *   behave as dark rock.
 *
 * mmgen_light_masks derives, per chunk slot, what the lighting reads instead of the blocks (to lighting what mmgen_ray_occupancy is to
 * rays): d_masks [*][MMGEN_LIGHT_MASK_BYTES], indexed like d_blocks; chunk d_chunk_idx[i] (i when NULL) writes its own record, so a pool
 * refreshes only the slots whose blocks changed.  d_emission: e[256] on the device, NULL = the default table.  The record has no
 * capacity on the number of emitters: a lava lake, or a table that makes STONE glow, is legal input.
 * mmgen_light lights the chunks of the listed grid cells (d_cells [n] = cz * grid_w + cx on the device, NULL = cells 0 .. n-1).  It must be
 * given the masks of EVERY present chunk of the grid, built with one emission table.  Only the slots of listed cells that are present are
 * written; every other slot of d_light stays untouched.
 * Nothing is allocated; all calls are asynchronous on `stream`; n == 0 succeeds without a launch.  Null pointers, grid sides outside
 * [1, 16384], n < 0, and n beyond grid_w * grid_h when d_cells is NULL are hipErrorInvalidValue.  A d_cells entry outside the grid lives on
 * the device, where an asynchronous call cannot report it: such an entry is skipped, nothing is written for it. */
int mmgen_light_default_emission(uint8_t* h_out /*[256], host*/);
int mmgen_light_masks(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, const uint8_t* d_emission /*[256] device, NULL = default*/,
                      uint8_t* d_masks /*[*][MMGEN_LIGHT_MASK_BYTES], indexed like d_blocks*/, void* stream);
int mmgen_light(const uint8_t* d_masks, const int32_t* d_grid, int grid_w, int grid_h, const int32_t* d_cells /*[n] grid cells to light, NULL = cells 0..n-1*/,
                int n, uint8_t* d_light /*[*][98304], indexed like d_blocks*/, void* stream);

/* ---- section visibility: face connectivity per 16^3 section and the occlusion-culled set of sections an eye can see -----------
 * The reference culls with OptiX.  Here: per section, which of its six faces are connected through see-through voxels (15 bits), and a
 * walk of the section graph outward from the eye's section through connected faces that never turns back.  d_blocks, d_chunk_idx exactly
 * as in mmgen_ray_occupancy and mmgen_light_masks; d_grid as in mmgen_raycast.  Faces are numbered in dirVecs order.
 *
 * THE CONNECTIVITY CONTRACT (mmgen_section_connectivity)
 *   d_conn [*][MMGEN_SECTION_CONN_BYTES], indexed like d_blocks: per chunk slot u16 [24], section sy = y >> 4.  Chunk d_chunk_idx[i] (i when
 *   NULL) writes its own 48 bytes, every other slot stays untouched.
 *   A voxel SEES THROUGH iff its class is not OPAQUE: AIR, SEMI, TRANSPARENT and X_SHAPED do, ids >= MMB_NUM_BLOCKS are OPAQUE (the T of
 *   the lighting).  Face d of a section is the layer of its 256 voxels at local z = 15 (d = 0), x = 15 (1), z = 0 (2), x = 0 (3), y = 15 (4),
 *   y = 0 (5); an edge voxel belongs to two faces, a corner voxel to three.
 *   Faces a < b are CONNECTED iff a 6-connected path of see-through voxels, all of them inside the section, has a voxel in layer a and a
 *   voxel in layer b.  One voxel is a path.  A path that leaves the section and comes back does not count; nothing is read from
 *   neighbouring chunks.
 *   The pair (a, b) is bit a (11 - a) / 2 + b - a - 1 of the section's u16: bits 0..14 are (0,1), (0,2) .. (0,5), (1,2) .. (4,5); bit 15 is 0.
 *   A section without an opaque voxel gives 0x7fff, one without a see-through voxel 0.
 *   Null d_blocks or d_conn and n < 0 are hipErrorInvalidValue; n == 0 succeeds without a launch.
 *
 * THE VISIBLE-SET CONTRACT (mmgen_visible_sections)
 *   d_conn must hold the record of every present chunk of the window.  The window is the cells with |cx - eye_cx| <= radius and
 *   |cz - eye_cz| <= radius.  A section is (cx, sy, cz), sy in [-1, 24]; the layers sy = -1 and sy = 24 are virtual.  A window cell outside
 *   the grid does not exist: nothing steps into it.  A window cell inside the grid that is absent, and every virtual-layer section of a window
 *   cell inside the grid, is TRANSPARENT: its record reads 0x7fff and it is never reported.
 *   Let s0 = (eye_cx, eye_sy, eye_cz), E(s) a set of faces of s.  A step from s through its face d to n = s + dirVec(d) is taken iff
 *     n exists,  the step moves away from the eye on its axis: (n_a - s0_a) * sign(d) > 0 for the axis a of d,  and
 *     s = s0, or some f in E(s) has the pair (f, d) set in the record of s.
 *   A taken step puts opposite(d) into E(n) (d ^ 2 for d < 4; 4 and 5 are each other's opposite).  The E are the least sets closed under this
 *   rule; every step increases the Manhattan distance from s0 by one, so E at distance k depends on E at distance k - 1 only: they are unique.
 *   d_visible [2 radius + 1][2 radius + 1]: entry (cz - eye_cz + radius)(2 radius + 1) + (cx - eye_cx + radius) has bit sy (0..23) set iff the
 *   cell is present and E((cx, sy, cz)) is not empty or the section is s0.  Every entry is written; cells outside the grid or absent get 0.
 *   There is no frustum test (the consumer's), and the eye's section exits through all six faces (no flood from the eye voxel): conservative.
 *   Null pointers, grid sides outside [1, 16384], an eye cell outside the grid, eye_sy outside [-1, 24] and a radius outside
 *   [0, MMGEN_VISIBLE_MAX_RADIUS] are hipErrorInvalidValue.
 *   CONSERVATIVE: a contract ray of mmgen_raycast with stop_mask = MMGEN_RAY_OPAQUE whose origin lies in section s0 with y in [0, 384) walks
 *   voxels that are 6-connected, monotone on every axis and see-through up to the HIT voxel.  Cut at section borders, that walk is a chain of
 *   taken steps, so the section of every HIT voxel inside the window is reported.  An eye above y = 383 passes eye_sy = 24, one below 0
 *   passes -1: both layers see through everywhere and the ray is monotone, so the set stays conservative.
 * Both calls are asynchronous on `stream` and allocate nothing. */
int mmgen_section_connectivity(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, uint8_t* d_conn /*[*][48], indexed like d_blocks*/,
                               void* stream);
int mmgen_visible_sections(const uint8_t* d_conn, const int32_t* d_grid, int grid_w, int grid_h, int eye_cx, int eye_sy, int eye_cz, int radius,
                           uint32_t* d_visible /*[2 radius + 1][2 radius + 1]*/, void* stream);

/* ---- section-bucketed quad mesh and its draw list -------------------------------------------------------------------------
 * A third mesher: the greedy quad stream cut at the borders of the 16^3 sections, one 32-bit record per quad (mmgen_types.h "section quad
 * record"), every section's records one contiguous range - the stream that mmgen_visible_sections can cull.  (Culling the 64-bit stream of
 * mmgen_mesh_quads_* by the section of a quad's origin is not conservative: its side faces merge along y over the whole column.)
 * d_blocks / d_chunk_idx / d_neighbor_idx exactly as in mmgen_mesh_quads_count.  The stream of a chunk is a pure function of its blocks, its
 * four neighbours' blocks and which neighbours are present; the kernels return exactly this stream, in this order.
 *
 * FACE SET F: that of mmgen_mesh_quads_*, word for word - the display rule of mmgen_mesh_* (chunk.cu:1906-1928) over the classes AIR,
 * OPAQUE, SEMI, TRANSPARENT, X_SHAPED (ids >= MMB_NUM_BLOCKS count as OPAQUE); directions in dirVecs order +z 0, +x 1, -z 2, -x 3, +y 4, -y 5:
 *   an X-shaped block has no faces, it emits one record of kind 6;
 *   opaque or semi-transparent block: face d is in F iff the neighbour's class is not OPAQUE;
 *   transparent block: face d is in F iff the neighbour is AIR or SEMI;
 *   a horizontal neighbour outside the chunk is read from the neighbour chunk when present; when it is absent the face is NOT in F;
 *   below y = 0 and above y = 383 the neighbour is AIR.
 * SECTIONS AND PLANES: a section is (chunk, sy), sy = y >> 4.  Per section 96 planes (d, p), p in 0..15, of 16 rows r x 16 cells q:
 *   d in {0, 2}: p = z, r = x, q = y & 15;     d in {1, 3}: p = x, r = z, q = y & 15;     d in {4, 5}: p = y & 15, r = z, q = x.
 * GREEDY RULE: that of mmgen_mesh_quads_*, applied to each 16 x 16 plane: visit the cells with r ascending, then q ascending.  At the first
 * cell (r0, q0) in F and not yet covered, of block id b: L = the largest length such that every cell (r0, q0 .. q0+L-1) is in F, uncovered and
 * of id b; W = the largest count such that for every row r0 .. r0+W-1 all cells (r, q0 .. q0+L-1) are in F, uncovered and of id b; emit one
 * quad of W rows x L cells and mark them covered.  Faces of different ids never share a quad.  Nothing merges across a section border or a
 * chunk border.
 * ORDER of a chunk's records: sy ascending; inside a section the planes with d ascending, then p ascending, each in emission order; then that
 * section's kind-6 records in ascending voxel index y + 384 (x + 16 z).  A section's records are therefore one contiguous range.
 *
 *   mmgen_mesh_section_quads_count: d_section_quads [n][24] and d_chunk_quads [n] receive the record counts.
 *   mmgen_mesh_section_quads_fill : d_quad_offset = exclusive prefix of d_chunk_quads (mmgen_mesh_offsets computes it on the device unchanged:
 *                           count -> offsets -> fill needs no host read).  Section sy of chunk i starts at d_quad_offset[i] + the sum of
 *                           d_section_quads[i][k], k < sy.  A chunk whose records would end beyond capacity_quads writes nothing; UINT64_MAX =
 *                           uncapped, 0 is hipErrorInvalidValue.  A section never writes more records than were counted for it: blocks that
 *                           changed between the two calls cannot make it write outside its range.
 * n == 0 succeeds without a launch; null pointers and n < 0 are hipErrorInvalidValue.  Nothing is allocated; both calls are asynchronous on
 * `stream`.
 *
 * THE DRAW LIST (mmgen_section_draws): the visible sections that have records, as ranges of d_quads, built on the device.
 *   d_visible, d_grid, grid_w, grid_h, eye_cx, eye_cz, radius: the output and the arguments of mmgen_visible_sections.  d_mesh_pos [slots]:
 *   position of a chunk slot in the work list that was meshed (d_section_quads and d_quad_offset are indexed by it, n entries), -1 = not
 *   meshed; NULL = the slot itself.
 *   Walk the window entries of d_visible in their stored order (wz major, then wx).  Take each entry whose cell lies in the grid, is present
 *   with slot s, and has m = d_mesh_pos ? d_mesh_pos[s] : s in [0, n).  For that entry take each sy ascending whose bit is set in the entry
 *   and whose d_section_quads[m][sy] > 0.  Each such (entry, sy) is one draw: first = the section's start as defined above, count =
 *   d_section_quads[m][sy], origin = wx | wz << 7 | sy << 14 with wx = cx - eye_cx + radius, wz = cz - eye_cz + radius.
 *   Draw k is written iff k < capacity_draws.  d_totals[0] = the number of draws, d_totals[1] = the sum of their counts, both over ALL draws,
 *   not only the written ones: a caller grows the buffer and repeats.  d_draws may be NULL when capacity_draws is 0.
 *   Other null pointers, n < 0, grid sides outside [1, 16384], an eye cell outside the grid and a radius outside
 *   [0, MMGEN_VISIBLE_MAX_RADIUS] are hipErrorInvalidValue.  Nothing is allocated; the call is asynchronous on `stream`. */
int mmgen_mesh_section_quads_count(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n,
                                   uint32_t* d_section_quads /*[n][24]*/, uint32_t* d_chunk_quads /*[n]*/, void* stream);
int mmgen_mesh_section_quads_fill(const uint8_t* d_blocks, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n,
                                  const uint32_t* d_section_quads, const uint64_t* d_quad_offset, uint64_t capacity_quads,
                                  uint32_t* d_quads, void* stream);
int mmgen_section_draws(const uint32_t* d_visible, const int32_t* d_grid, int grid_w, int grid_h, int eye_cx, int eye_cz, int radius,
                        const int32_t* d_mesh_pos /*[slots], NULL = identity*/, const uint32_t* d_section_quads, const uint64_t* d_quad_offset, int n,
                        uint32_t capacity_draws, mmgen_section_draw* d_draws, uint64_t* d_totals /*[2]*/, void* stream);

/* ---- lit section quad mesh: per-quad light, light-aware greedy merge ------------------------------------------------------
 * The section-bucketed stream with flat lighting: the light of a face is the light of the voxel in front of it, two faces share a quad only if
 * they share the block id AND that light, and every record carries its light in a parallel byte stream.  With it the dense light volume
 * (98 304 bytes per chunk) is a transient like the class planes: the draw list of mmgen_section_draws delivers lit geometry as it stands.
 * d_blocks / d_chunk_idx / d_neighbor_idx exactly as in mmgen_mesh_section_quads_count.  d_light [*][98304] is indexed and laid out like
 * d_blocks - normally the output of mmgen_light, but any bytes are legal input.  The caller must have lit every listed chunk and every
 * present neighbour.
 *
 * FACE LIGHT: F, directions, sections and planes are exactly those of mmgen_mesh_section_quads_*.  For a face (v, d) of F
 *     FL(v, d) = L(v + dirVec(d)) & light_mask
 *   L inside the chunk is read from the chunk's own slot of d_light;
 *   a horizontal neighbour outside the chunk is read from the slot d_neighbor_idx names (a face towards an absent neighbour is not in F, so
 *   that light is never needed);
 *   above y = 383 L is MMGEN_LIGHT_ABOVE = 0xF0 (sky 15, block 0); below y = 0 L is 0x00;
 *   for a kind-6 record (X-shaped block) FL = L(v) & light_mask, the voxel's own light.
 * GREEDY RULE: that of mmgen_mesh_section_quads_*, applied to each 16 x 16 plane: visit the cells with r ascending, then q ascending.  At the
 * first cell (r0, q0) in F and not yet covered, of block id b and face light FL(r0, q0): L = the largest length such that every cell
 * (r0, q0 .. q0+L-1) is in F, uncovered, of id b and of that face light; W = the largest count such that for every row r0 .. r0+W-1 all
 * cells (r, q0 .. q0+L-1) are in F, uncovered, of id b and of that face light; emit one quad of W rows x L cells and mark them covered.
 * Nothing merges across a section border or a chunk border.  ORDER, the section ranges, the record format, count -> mmgen_mesh_offsets -> fill,
 * the capacity rule and "a section never writes more records than were counted for it" are those of mmgen_mesh_section_quads_*.
 * The stream of a chunk is a pure function of its blocks and light, its four neighbours' blocks and light, which neighbours are present,
 * and light_mask.  With light_mask == 0 the records equal those of mmgen_mesh_section_quads_fill exactly and every light byte is 0; 0xF0 merges
 * by sky light alone, 0x0F by block light alone.
 *
 *   mmgen_mesh_lit_section_quads_count: d_section_quads [n][24] and d_chunk_quads [n] receive the record counts.
 *   mmgen_mesh_lit_section_quads_fill : d_quads holds the section quad record of mmgen_types.h, bit for bit; d_quad_light[k] is the face light
 *                           of record k, a parallel byte stream over the same indices.  Offsets, mmgen_section_draws and a vertex puller's
 *                           decode work on these counts and offsets unchanged.  A chunk whose records would end beyond capacity_quads
 *                           writes NEITHER array.  Blocks, light and light_mask must be those of the count.
 * n == 0 succeeds without a launch; null pointers (d_light among them) and n < 0 are hipErrorInvalidValue, as is capacity_quads == 0.
 * Nothing is allocated; both calls are asynchronous on `stream`. */
int mmgen_mesh_lit_section_quads_count(const uint8_t* d_blocks, const uint8_t* d_light, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n,
                                       uint8_t light_mask, uint32_t* d_section_quads /*[n][24]*/, uint32_t* d_chunk_quads /*[n]*/, void* stream);
int mmgen_mesh_lit_section_quads_fill(const uint8_t* d_blocks, const uint8_t* d_light, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx, int n,
                                      uint8_t light_mask, const uint32_t* d_section_quads, const uint64_t* d_quad_offset, uint64_t capacity_quads,
                                      uint32_t* d_quads, uint8_t* d_quad_light, void* stream);

/* ---- section quad mesh with ambient occlusion: per-corner AO in the greedy key ----------------------------------------------
 * The lit section stream with the shading a voxel world is expected to have: every face carries the darkening of its four corners by the
 * opaque blocks that touch them, two faces share a quad only if they share the block id, the face light AND the four corner values, and every
 * record has its AO byte (mmgen_types.h "face AO byte") in a second parallel byte stream.
 * d_blocks / d_light / d_chunk_idx / light_mask exactly as in mmgen_mesh_lit_section_quads_*, but d_light may be NULL iff light_mask == 0: then
 * every light byte is 0 and the light volume is not read.
 * d_neighbor_idx8 [n][8]: entries 0..3 = N (+z), E (+x), S (-z), W (-x) as in d_neighbor_idx; entries 4..7 = the diagonals (+x,+z), (+x,-z),
 * (-x,-z), (-x,+z); -1 = absent, NULL = all absent.
 *
 * UNCHANGED: the face set F is that of mmgen_mesh_section_quads_*, word for word, and uses entries 0..3 only; directions, sections, planes,
 * the face light FL, the record format, the ORDER, the section ranges, count -> mmgen_mesh_offsets -> fill and "a section never writes more
 * records than were counted for it" are those of mmgen_mesh_lit_section_quads_*.
 * OCCLUDER: O(u) = 1 iff u lies in the chunk or in one of its eight PRESENT neighbour chunks, 0 <= u.y <= 383, and the class of u is OPAQUE
 * (ids >= MMB_NUM_BLOCKS count as OPAQUE).  Everything else - absent chunks, voxels beyond the 18 x 18 column halo, below or above the world -
 * does not occlude.
 * FACE AO: for a face (v, d) of F let f = v + dirVec(d) and e_r, e_q the unit steps of the plane's row axis and fast axis (d in {0, 2}: r = x,
 * q = y;  d in {1, 3}: r = z, q = y;  d in {4, 5}: r = z, q = x).  Corner k = 2 [r side is +] + [q side is +], k = 0..3, has the signs (s_r, s_q):
 *     s1 = O(f + s_r e_r),  s2 = O(f + s_q e_q),  c = O(f + s_r e_r + s_q e_q);   ao_k = 0 if s1 and s2, else 3 - (s1 + s2 + c);
 *     AO(v, d) = sum of ao_k << 2k.   An unoccluded face has MMGEN_AO_NONE = 0xFF.
 *   A kind-6 record (X-shaped block) has AO 0xFF and its own voxel's light.
 * GREEDY RULE: that of mmgen_mesh_section_quads_* with "of id b" replaced by "of id b, of face light FL(r0, q0) and of face AO AO(r0, q0)",
 * for L and for W alike.  Nothing merges across a section border or a chunk border.
 * FOR THE CONSUMER: the four corner values are interpolated bilinearly inside each CELL of the quad, by the fractional part of the tiled
 * coordinate that already tiles the block's texture; every cell of a quad has the same AO byte, so the merged quad shades exactly like its
 * unmerged faces.
 * The stream of a chunk is a pure function of its blocks and light, its eight neighbours' blocks, its four side neighbours' light, which
 * neighbours are present, and light_mask.
 *
 *   mmgen_mesh_ao_section_quads_count: d_section_quads [n][24] and d_chunk_quads [n] receive the record counts.
 *   mmgen_mesh_ao_section_quads_fill : d_quads, d_quad_light as in mmgen_mesh_lit_section_quads_fill; d_quad_ao[k] is the AO byte of record k.
 *                           A chunk whose records would end beyond capacity_quads writes NONE of the three arrays; UINT64_MAX = uncapped.
 *                           Blocks, light, neighbours and light_mask must be those of the count.
 * n == 0 succeeds without a launch; capacity_quads == 0, null pointers (d_light under the rule above) and n < 0 are hipErrorInvalidValue.
 * Nothing is allocated; both calls are asynchronous on `stream`. */
int mmgen_mesh_ao_section_quads_count(const uint8_t* d_blocks, const uint8_t* d_light, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx8, int n,
                                      uint8_t light_mask, uint32_t* d_section_quads /*[n][24]*/, uint32_t* d_chunk_quads /*[n]*/, void* stream);
int mmgen_mesh_ao_section_quads_fill(const uint8_t* d_blocks, const uint8_t* d_light, const int32_t* d_chunk_idx, const int32_t* d_neighbor_idx8, int n,
                                     uint8_t light_mask, const uint32_t* d_section_quads, const uint64_t* d_quad_offset, uint64_t capacity_quads,
                                     uint32_t* d_quads, uint8_t* d_quad_light, uint8_t* d_quad_ao, void* stream);

/* ---- level-of-detail chunks: s x s source chunks reduced to one chunk-shaped volume of s^3-block cells ------------------------
 * The far field for every consumer above: the output is a chunk slot in the standard layout, AIR above its content, so a grid of level-k
 * slots is lit, culled, meshed and ray cast by the calls of this header unchanged; the consumer multiplies positions by s.  The reference
 * has nothing like it.
 *
 * THE CONTRACT (mmgen_lod_reduce)
 *   level is 1, 2 or 3 and s = 1 << level.  LOD chunk i covers the s x s source chunks d_src_idx[i][qx + s qz], qx, qz in 0..s-1 along +x and
 *   +z: slots of d_blocks, -1 = absent (reads as all AIR); a slot may appear in several lists.  LOD chunk i is written to slot d_dst_idx[i]
 *   of d_lod_blocks (slot i when NULL): all 98 304 bytes, index Y + 384 (X + 16 Z); every other slot stays untouched.  d_lod_blocks must not
 *   overlap a source slot that is read, and the destination slots must be distinct.
 *   Coarse voxel (X, Y, Z), X, Z in 0..15, Y in 0..384/s - 1, has the cube C of the s^3 source voxels at footprint columns (s X + i, s Z + j)
 *   and y in [s Y, s Y + s); footprint column gx belongs to source chunk qx = gx >> 4 at local x = gx & 15, and so for z.  Y >= 384/s is AIR.
 *   Classes are the mesher's; ids >= MMB_NUM_BLOCKS are OPAQUE.  A voxel is CONTENT iff its class is OPAQUE, SEMI or TRANSPARENT: AIR and
 *   X_SHAPED are not, so flowers and grass tufts vanish with distance.
 *   SOLIDITY: with N the number of content voxels of C, the cell is AIR (0) iff 2 N < s^3: the surface is rounded to the nearest cell, and
 *   exactly half counts as solid.
 *   BLOCK ID of a solid cell: every column of C that holds a content voxel gives one sample.  y1 is its highest content voxel inside C, y2
 *   the largest y with y1 <= y2 <= min(s Y + 2 s - 1, 383) such that every voxel y1..y2 of that source column is content; the sample is the
 *   id at y2.  (The look-ahead of at most s voxels into the cube above keeps a grass or water skin on a cell whose own top voxel is dirt.)
 *   The cell's id is the id with the most samples, ties to the lowest id.
 *   The output is a pure function of the listed source chunks and level.  It is NOT a cascade: level k is defined from level 0.
 *   Null d_blocks, d_src_idx or d_lod_blocks, n < 0 and a level outside [1, 3] are hipErrorInvalidValue; n == 0 succeeds without a launch.
 * Nothing is allocated; the call is asynchronous on `stream`. */
int mmgen_lod_reduce(const uint8_t* d_blocks, const int32_t* d_src_idx /*[n][s*s]*/, int n, int level,
                     uint8_t* d_lod_blocks /*[*][98304]*/, const int32_t* d_dst_idx /*[n], NULL = 0..n-1*/, void* stream);

/* ---- region wire format (the reference has none) ---------------------------------------------
 * A chunk's 98 304 block ids as per-column run-length pairs: u16 runsOfColumn[256], then for each column (x + 16 z, the blocks[]
 * order) its runs as (u8 blockId, u8 length - 1), 1 .. 256 voxels per pair.  512 + 2 R bytes per chunk (typically 5 - 9 KB).
 * d_chunk_idx as in the mesher (NULL = chunks 0 .. n-1 of d_blocks); d_chunk_offset = exclusive prefix of d_chunk_bytes, by the
 * caller, who also sizes d_out.  mmgen_unpack is the device inverse (d_blocks [n][98304] dense) for streams this library produced
 * (it never writes outside a chunk, but it trusts the run counts of the header when reading); mmgen_unpack_chunk_host decodes one
 * chunk on the host (plain C, no device), validates every count and length against packed_bytes and returns -1 on a malformed stream:
 * use it for data of unknown origin. */
int mmgen_pack_count(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, uint16_t* d_col_runs /*[n][256]*/, uint32_t* d_chunk_bytes /*[n]*/, void* stream);
int mmgen_pack_fill(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, const uint16_t* d_col_runs, const uint64_t* d_chunk_offset, uint8_t* d_out,
                    void* stream);
int mmgen_unpack(const uint8_t* d_packed, const uint64_t* d_chunk_offset, int n, uint8_t* d_blocks, void* stream);
int mmgen_unpack_chunk_host(const uint8_t* packed, size_t packed_bytes, uint8_t* blocks);

/* Test-only: evaluates device math function `fn` (MMGEN_PROBE_*) on n packed fp32 items (ints bit-cast); used by the parity
 * tests to pin the device math against golden vectors.  Not part of the reference's interface. */
int mmgen_debug_probe(int fn, const float* d_in, int n, float* d_out, void* stream);
/* Test-only: caps the queue of deferred clay / moss voxels of mmgen_fill / the region path at `entries` (0 = the library's own size, 2 048 per
 * chunk), so that a test can drive the path that evaluates them in place when a reservation does not fit.  Process-wide. */
int mmgen_debug_set_lush_queue_cap(int entries);
/* Test-only: the following persistent relaxation launches wait for `missing_workgroups` more workgroups than they have, so that the wait
 * can never complete, and give up after timeout_ms: drives the give-up + rescue path.  (0, 0) restores the defaults.  Process-wide. */
int mmgen_debug_erosion_stall(int missing_workgroups, int timeout_ms);
/* process-wide counters (either pointer may be NULL): persistent relaxations that gave up, as far as the host has learnt of them (the
 * synchronous per-stage calls at once, a region at its next call), and zones the rescue pass had to relax (synchronous calls only) */
int mmgen_erosion_stalls(long long* stalls, long long* zones_rescued);
/* Test-only: the library's constant rule tables (BiomeUtils::init, biomeFuncs.hpp:725-1256) as floats in the layout of
 * tools/extract_ref_tables.py, so that a test can hold them to the reference's literals.  d_out == NULL: returns the number of floats. */
int mmgen_debug_tables(float* d_out, int capacity_floats, void* stream);
/* Test-only: rasterises ONE (cave) feature placement into a box of voxels (placeFeature / placeCaveFeature per voxel,
 * featurePlacement.hpp:147,1110); d_out[box_size x*y*z] in z, x, y order (y fastest), 255 = voxel not claimed. */
int mmgen_debug_feature_box(int is_cave, int feature, const int32_t* h_feature_pos, int layer_height, const int32_t* h_box_min,
                            const int32_t* h_box_size, uint8_t* d_out, void* stream);
/* Measuring only: mmgen_section_connectivity that also reports, per chunk slot it writes, the flood rounds it took: d_rounds [*], indexed
 * like d_blocks. */
int mmgen_debug_section_rounds(const uint8_t* d_blocks, const int32_t* d_chunk_idx, int n, uint8_t* d_conn, uint32_t* d_rounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGEN_H */
