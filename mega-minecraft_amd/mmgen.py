"""ctypes binding of libmmgen.so (include/mmgen.h) + a thin torch-tensor convenience layer.

Mirrors the static stage functions of the reference's ``Chunk`` class (src/terrain/chunk.hpp:99-172): same stage names,
same per-chunk staging layouts, same error convention at this level (a failing stage raises; the C++ wrapper in host/
prints and exits like src/cuda/cuda_utils.cpp:5-17).  There is NO CPU fallback: if the HIP library is missing or the
device is not gfx950 every call fails loudly.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMGEN_LIB", os.path.join(_HERE, "libmmgen.so"))   # MMGEN_LIB: A/B builds of the same ABI

HF, GHF, BW, LAYERS, CAVE, BLOCKS = 256, 324, 6144, 5120, 8192, 98304


def build(verbose=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("libmmgen build failed:\n" + r.stdout + r.stderr)
    if verbose:
        print(r.stdout)


def load_library():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: build it with `make -C mega-minecraft_amd/csrc` (no CPU fallback exists)")
    # torch first: libmmgen.so needs libamdhip64.so.N, and the loader gives it whichever copy is in the process already.  Loaded before
    # torch it binds /opt/rocm's runtime, torch then brings its own bundled copy, and the process ends up with two HIP runtimes of which
    # ours sees no device (hipErrorNoDevice from mmgen_init: found with build() followed by smoke() in one process, round 6).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.mmgen_init.argtypes = [i32]
    lib.mmgen_error_string.restype = ctypes.c_char_p
    lib.mmgen_error_string.argtypes = [i32]
    lib.mmgen_reserve.argtypes = [i32, vp]
    lib.mmgen_generate_heightfields.argtypes = [vp, i32, vp, vp, vp]
    lib.mmgen_generate_heightfields_gathered.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.mmgen_generate_layers.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.mmgen_fix_backward_layers.argtypes = [vp, i32, vp]
    lib.mmgen_generate_caves.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.mmgen_fill.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    return lib


class MMGen:
    """Stage-level access to libmmgen on one GPU.  All tensors are torch CUDA tensors in the reference's layouts."""

    def __init__(self, device=0):
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("mmgen needs a GPU (gfx950); no CPU path exists")
        self.lib = load_library()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self._check(self.lib.mmgen_init(device), "mmgen_init")

    # ------------------------------------------------------------------ helpers
    def _check(self, code, what):
        if code != 0:
            raise RuntimeError(f"{what} failed: {self.lib.mmgen_error_string(code).decode()} ({code})")

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def _empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.device)

    @staticmethod
    def _p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def positions(self, chunk_coords):
        """[(cx, cz)] chunk coordinates -> device int32 [n,2] world block positions (Chunk::worldBlockPos, chunk.cu:18-20)."""
        t = self.torch.tensor([[c[0] * 16, c[1] * 16] for c in chunk_coords], dtype=self.torch.int32)
        return t.to(self.device)

    # ------------------------------------------------------------------ stages
    def generate_heightfields(self, pos, gathered=False):
        n = pos.shape[0]
        f32 = self.torch.float32
        hf, bw = self._empty((n, HF), f32), self._empty((n, 24, 256), f32)
        if gathered:
            g = self._empty((n, GHF), f32)
            self._check(self.lib.mmgen_generate_heightfields_gathered(self._p(pos), n, self._p(hf), self._p(bw), self._p(g), self._stream()),
                        "mmgen_generate_heightfields_gathered")
            return hf, bw, g
        self._check(self.lib.mmgen_generate_heightfields(self._p(pos), n, self._p(hf), self._p(bw), self._stream()), "mmgen_generate_heightfields")
        return hf, bw

    def generate_layers(self, gathered, bw, pos):
        n = pos.shape[0]
        layers = self._empty((n, 20, 256), self.torch.float32)
        self._check(self.lib.mmgen_generate_layers(self._p(gathered), self._p(bw), self._p(pos), n, self._p(layers), self._stream()), "mmgen_generate_layers")
        return layers

    def fix_backward_layers(self, layers):
        self._check(self.lib.mmgen_fix_backward_layers(self._p(layers), layers.shape[0], self._stream()), "mmgen_fix_backward_layers")
        return layers

    def erode_zones(self, gathered, want_acc=False):
        """gathered: [zones, MMGEN_GATHERED_LAYERS_SIZE] f32 packed zone planes (copyLayers(to), chunk.cu:603-656), eroded in place.
        Returns (gathered, max_passes[, accumulated])."""
        zones = gathered.shape[0]
        assert gathered.shape[1] == 1327105 and gathered.is_contiguous()
        acc = self._empty((zones, 147456), self.torch.float32) if want_acc else None
        mp = ctypes.c_int(0)
        self.lib.mmgen_erode_zones.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
        self._check(self.lib.mmgen_erode_zones(self._p(gathered), zones, self._p(acc), ctypes.byref(mp), self._stream()), "mmgen_erode_zones")
        return (gathered, mp.value, acc) if want_acc else (gathered, mp.value)

    def erosion_stalls(self):
        """(persistent relaxations that gave up, zones the rescue pass relaxed) - process-wide counters (mmgen_erosion_stalls)."""
        a, b = ctypes.c_longlong(0), ctypes.c_longlong(0)
        self.lib.mmgen_erosion_stalls.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
        self._check(self.lib.mmgen_erosion_stalls(ctypes.byref(a), ctypes.byref(b)), "mmgen_erosion_stalls")
        return a.value, b.value

    def debug_erosion_stall(self, missing_workgroups, timeout_ms):
        """Test hook (mmgen_debug_erosion_stall): the next persistent relaxations are launched short; (0, 0) restores the defaults."""
        self.lib.mmgen_debug_erosion_stall.argtypes = [ctypes.c_int, ctypes.c_int]
        self._check(self.lib.mmgen_debug_erosion_stall(missing_workgroups, timeout_ms), "mmgen_debug_erosion_stall")

    @staticmethod
    def zone_area_coords(zone_cx, zone_cz):
        """The 24x24 chunks a zone gathers for erosion: own 12x12 + 6-chunk padding (terrain.cpp:471-522), z-major."""
        return [(zone_cx - 6 + x, zone_cz - 6 + z) for z in range(24) for x in range(24)]

    def pack_zone_planes(self, layers, hf):
        """copyLayers(..., true) on device tensors: layers [576,20,256], hf [576,256] of zone_area_coords order -> [1, 1327105]."""
        t = self.torch
        planes = t.cat([layers[:, 12:20, :], hf.unsqueeze(1)], dim=1)              # [576, 9, 256]
        planes = planes.view(24, 24, 9, 16, 16).permute(2, 0, 3, 1, 4).reshape(9, 384 * 384)   # [plane][cz,z][cx,x]
        out = t.zeros((1, 1327105), dtype=t.float32, device=self.device)
        out[0, : 9 * 147456] = planes.reshape(-1)
        return out

    def generate_caves(self, hf, bw, pos):
        n = pos.shape[0]
        cave = self._empty((n, 256, 32, 3), self.torch.int32)      # 12-byte mmgen_cave_layer viewed as 3 int32
        self._check(self.lib.mmgen_generate_caves(self._p(hf), self._p(bw), self._p(pos), n, self._p(cave), self._stream()), "mmgen_generate_caves")
        return cave

    def fill(self, hf, bw, layers, cave, pos, features=None, cave_features=None, bounds=None):
        n = pos.shape[0]
        blocks = self._empty((n, BLOCKS), self.torch.uint8)
        self._check(self.lib.mmgen_fill(self._p(hf), self._p(bw), self._p(layers), self._p(cave), self._p(pos), n, self._p(features),
                                        self._p(cave_features), self._p(bounds), self._p(blocks), self._stream()), "mmgen_fill")
        return blocks

    # ------------------------------------------------------------------ feature stages
    def generate_feature_placements(self, hf, bw, layers, cave, pos):
        """-> (fp [n,256,5] int32 view of 20-byte records, cfp [n,1024,6] int32 view of 24-byte records, counts [n,2])."""
        n = pos.shape[0]
        i32 = self.torch.int32
        fp = self.torch.zeros((n, 256, 5), dtype=i32, device=self.device)
        cfp = self.torch.zeros((n, 1024, 6), dtype=i32, device=self.device)
        counts = self.torch.zeros((n, 2), dtype=i32, device=self.device)
        self.lib.mmgen_generate_feature_placements.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] + [ctypes.c_void_p] * 4
        self._check(self.lib.mmgen_generate_feature_placements(self._p(hf), self._p(bw), self._p(layers), self._p(cave), self._p(pos), n,
                                                               self._p(fp), self._p(cfp), self._p(counts), self._stream()),
                    "mmgen_generate_feature_placements")
        return fp, cfp, counts

    def gather_feature_placements(self, fp, cfp, counts, targets, grid_w, grid_h):
        nt = targets.shape[0]
        i32 = self.torch.int32
        gfp = self.torch.zeros((nt, 2048, 5), dtype=i32, device=self.device)
        gcfp = self.torch.zeros((nt, 4096, 6), dtype=i32, device=self.device)
        bounds = self.torch.zeros((nt, 4), dtype=i32, device=self.device)
        self.lib.mmgen_gather_feature_placements.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
        self._check(self.lib.mmgen_gather_feature_placements(self._p(fp), self._p(cfp), self._p(counts), self._p(targets), nt, grid_w, grid_h,
                                                             self._p(gfp), self._p(gcfp), self._p(bounds), self._stream()),
                    "mmgen_gather_feature_placements")
        return gfp, gcfp, bounds

    def place_decorators(self, blocks, hf, bw, cave, pos):
        self.lib.mmgen_place_decorators.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p]
        self._check(self.lib.mmgen_place_decorators(self._p(blocks), self._p(hf), self._p(bw), self._p(cave), self._p(pos), pos.shape[0],
                                                    self._stream()), "mmgen_place_decorators")
        return blocks

    # ------------------------------------------------------------------ mesh build (Chunk::createVBOs, chunk.cu:1778-2003)
    def create_vbos(self, blocks, world_block_pos, nx=None, nz=None, neighbor_idx=None):
        """blocks: uint8 [n, 98304] on the device.  Either `neighbor_idx` (int32 [n, 4]: N(+z), E(+x), S(-z), W(-x) index into the
        batch, -1 = absent) or a z-major nx x nz grid shape (neighbours = grid neighbours, absent beyond the grid) or neither (every
        chunk alone).  world_block_pos: int32 [n, 2] (x, z) world block origins.  Returns dict(verts float32 view [V, 10] (pos 3, nor 3,
        uv 2, material as 2 x 32-bit), idx int32 [3 V / 2], chunk_verts int32 [n], vert_offset int64 [n])."""
        t = self.torch
        n = blocks.shape[0]
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        self.lib.mmgen_mesh_count.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        self.lib.mmgen_mesh_fill.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
        if neighbor_idx is None and nx is not None:
            c = t.arange(n, dtype=t.int32, device=blocks.device)
            x, z = c % nx, c // nx
            neg = t.full_like(c, -1)
            neighbor_idx = t.stack([t.where(z < nz - 1, c + nx, neg), t.where(x < nx - 1, c + 1, neg), t.where(z > 0, c - nx, neg),
                                    t.where(x > 0, c - 1, neg)], dim=1).contiguous()
        colv = self._empty((n, 256), t.int32)
        chv = self._empty((n,), t.int32)
        self._check(self.lib.mmgen_mesh_count(self._p(blocks), None, self._p(neighbor_idx), n, self._p(colv), self._p(chv), self._stream()), "mmgen_mesh_count")
        incl = t.cumsum(chv.to(t.int64), 0)
        off = (incl - chv).contiguous()
        total = int(incl[-1].item()) if n else 0
        verts = self._empty((max(total, 1), 10), t.float32)
        idx = self._empty((max(total * 3 // 2, 1),), t.int32)
        if total:
            self._check(self.lib.mmgen_mesh_fill(self._p(blocks), None, self._p(neighbor_idx), self._p(world_block_pos), n, self._p(colv), self._p(off),
                                                 self._p(verts), self._p(idx), self._stream()), "mmgen_mesh_fill")
        return dict(verts=verts[:total], idx=idx[:total * 3 // 2], chunk_verts=chv, vert_offset=off)

    def create_vbos_capped(self, blocks, world_block_pos, nx, nz, capacity_verts, strip=False):
        """The round-trip-free form (mmgen_mesh_count -> mmgen_mesh_offsets -> mmgen_mesh_fill_capped): offsets scanned on the device, buffers
        sized for `capacity_verts` vertices and pre-filled with a sentinel.  Returns dict(verts [capacity, 10], idx, chunk_verts, vert_offset,
        total) - chunks that would end beyond the capacity are left untouched.  strip=True: mmgen_mesh_fill_strip, the offsets summed inside
        the fill (at most 256 chunks)."""
        t = self.torch
        n = blocks.shape[0]
        vp, i32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
        self.lib.mmgen_mesh_count.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        self.lib.mmgen_mesh_offsets.argtypes = [vp, i32, vp, vp, vp]
        self.lib.mmgen_mesh_fill_capped.argtypes = [vp, vp, vp, vp, i32, vp, vp, u64, vp, vp, vp]
        c = t.arange(n, dtype=t.int32, device=blocks.device)
        x, z = c % nx, c // nx
        neg = t.full_like(c, -1)
        nb = t.stack([t.where(z < nz - 1, c + nx, neg), t.where(x < nx - 1, c + 1, neg), t.where(z > 0, c - nx, neg), t.where(x > 0, c - 1, neg)], dim=1).contiguous()
        colv = self._empty((n, 256), t.int32)
        chv = self._empty((n,), t.int32)
        off = self._empty((n,), t.int64)
        total = self._empty((1,), t.int64)
        verts = t.full((capacity_verts, 10), -7.0, dtype=t.float32, device=blocks.device)
        idx = t.full((capacity_verts * 3 // 2,), -7, dtype=t.int32, device=blocks.device)
        self._check(self.lib.mmgen_mesh_count(self._p(blocks), None, self._p(nb), n, self._p(colv), self._p(chv), self._stream()), "mmgen_mesh_count")
        if strip:
            self.lib.mmgen_mesh_fill_strip.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, u64, vp, vp, vp]
            off.fill_(-1); total.fill_(-1)
            self._check(self.lib.mmgen_mesh_fill_strip(self._p(blocks), None, self._p(nb), self._p(world_block_pos), n, self._p(colv), self._p(chv), self._p(off),
                                                       self._p(total), capacity_verts, self._p(verts), self._p(idx), self._stream()), "mmgen_mesh_fill_strip")
            return dict(verts=verts, idx=idx, chunk_verts=chv, vert_offset=off, total=int(total.item()))
        self._check(self.lib.mmgen_mesh_offsets(self._p(chv), n, self._p(off), self._p(total), self._stream()), "mmgen_mesh_offsets")
        self._check(self.lib.mmgen_mesh_fill_capped(self._p(blocks), None, self._p(nb), self._p(world_block_pos), n, self._p(colv), self._p(off), capacity_verts,
                                                    self._p(verts), self._p(idx), self._stream()), "mmgen_mesh_fill_capped")
        return dict(verts=verts, idx=idx, chunk_verts=chv, vert_offset=off, total=int(total.item()))

    # ------------------------------------------------------------------ greedy-merged quad mesh (include/mmgen.h)
    QUAD_GROUPS = 833

    def mesh_quads(self, blocks, nx=None, nz=None, neighbor_idx=None, chunk_idx=None, capacity_quads=None):
        """blocks: uint8 [slots, 98304] on the device; chunk_idx (int32 device tensor) picks the chunks to mesh (None = all, in order).
        Neighbours as in create_vbos: `neighbor_idx` (int32 [n, 4] N E S W index into blocks, -1 = absent), or a z-major nx x nz grid shape
        (without chunk_idx), or neither (every chunk alone).  capacity_quads=None sizes the buffer from the counts; a given capacity runs
        count -> mmgen_mesh_offsets -> fill without a host read into a buffer pre-filled with -7, and chunks that would end beyond it are left
        untouched.  Returns dict(quads int64 [Q or capacity], chunk_quads int32 [n], quad_offset int64 [n], total)."""
        t = self.torch
        n = blocks.shape[0] if chunk_idx is None else chunk_idx.shape[0]
        vp, i32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
        self.lib.mmgen_mesh_quads_count.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        self.lib.mmgen_mesh_quads_fill.argtypes = [vp, vp, vp, i32, vp, vp, u64, vp, vp]
        self.lib.mmgen_mesh_offsets.argtypes = [vp, i32, vp, vp, vp]
        if neighbor_idx is None and nx is not None:
            assert chunk_idx is None, "a grid shape names the neighbours of chunks 0 .. n-1; give neighbor_idx with chunk_idx"
            c = t.arange(n, dtype=t.int32, device=blocks.device)
            x, z = c % nx, c // nx
            neg = t.full_like(c, -1)
            neighbor_idx = t.stack([t.where(z < nz - 1, c + nx, neg), t.where(x < nx - 1, c + 1, neg), t.where(z > 0, c - nx, neg),
                                    t.where(x > 0, c - 1, neg)], dim=1).contiguous()
        groups = self._empty((max(n, 1), self.QUAD_GROUPS), t.int32)
        chq = self._empty((n,), t.int32)
        self._check(self.lib.mmgen_mesh_quads_count(self._p(blocks), self._p(chunk_idx), self._p(neighbor_idx), n, self._p(groups), self._p(chq), self._stream()),
                    "mmgen_mesh_quads_count")
        if capacity_quads is None:
            incl = t.cumsum(chq.to(t.int64), 0)
            off = (incl - chq).contiguous()
            total = int(incl[-1].item()) if n else 0
            quads = self._empty((max(total, 1),), t.int64)
            capacity = 2 ** 64 - 1
        else:
            off = self._empty((max(n, 1),), t.int64)[:n]
            tot = self._empty((1,), t.int64)
            quads = t.full((capacity_quads,), -7, dtype=t.int64, device=blocks.device)
            self._check(self.lib.mmgen_mesh_offsets(self._p(chq), n, self._p(off), self._p(tot), self._stream()), "mmgen_mesh_offsets")
            total, capacity = None, capacity_quads
        if n:
            self._check(self.lib.mmgen_mesh_quads_fill(self._p(blocks), self._p(chunk_idx), self._p(neighbor_idx), n, self._p(groups), self._p(off), capacity,
                                                       self._p(quads), self._stream()), "mmgen_mesh_quads_fill")
        if total is None:
            return dict(quads=quads, chunk_quads=chq, quad_offset=off, total=int(tot.item()))
        return dict(quads=quads[:total], chunk_quads=chq, quad_offset=off, total=total)

    @classmethod
    def quad_fields(cls, quads):
        """Decodes quad records (int64 tensor or array) into a dict of numpy fields x, y, z, kind, dx, dy, dz, block (mmgen_types.h)."""
        import numpy as np
        q = (quads.cpu().numpy() if hasattr(quads, "cpu") else np.asarray(quads)).astype(np.int64).view(np.uint64)
        field = lambda shift, bits: ((q >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int32)
        return dict(x=field(0, 4), y=field(4, 9), z=field(13, 4), kind=field(17, 3), dx=field(20, 4), dy=field(24, 9), dz=field(33, 4), block=field(37, 8))

    # ------------------------------------------------------------------ section-bucketed quad mesh and its draw list (include/mmgen.h)
    SECTIONS = 24
    SECTION_DRAW_DTYPE = [("first", "<u8"), ("count", "<u4"), ("origin", "<u4")]      # mmgen_section_draw

    def mesh_section_quads(self, blocks, nx=None, nz=None, neighbor_idx=None, chunk_idx=None, capacity_quads=None):
        """The greedy quad mesh cut at the borders of the 16^3 sections, one 32-bit record per quad, every section's records contiguous.
        Arguments as in mesh_quads, including the capped form (buffer pre-filled with -7, chunks that would end beyond it left untouched).
        Returns dict(quads int32 [Q or capacity], section_quads int32 [n, 24], chunk_quads int32 [n], quad_offset int64 [n], total)."""
        t = self.torch
        n = blocks.shape[0] if chunk_idx is None else chunk_idx.shape[0]
        vp, i32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
        self.lib.mmgen_mesh_section_quads_count.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        self.lib.mmgen_mesh_section_quads_fill.argtypes = [vp, vp, vp, i32, vp, vp, u64, vp, vp]
        self.lib.mmgen_mesh_offsets.argtypes = [vp, i32, vp, vp, vp]
        if neighbor_idx is None and nx is not None:
            assert chunk_idx is None, "a grid shape names the neighbours of chunks 0 .. n-1; give neighbor_idx with chunk_idx"
            c = t.arange(n, dtype=t.int32, device=blocks.device)
            x, z = c % nx, c // nx
            neg = t.full_like(c, -1)
            neighbor_idx = t.stack([t.where(z < nz - 1, c + nx, neg), t.where(x < nx - 1, c + 1, neg), t.where(z > 0, c - nx, neg),
                                    t.where(x > 0, c - 1, neg)], dim=1).contiguous()
        secq = self._empty((max(n, 1), self.SECTIONS), t.int32)[:n]
        chq = self._empty((n,), t.int32)
        self._check(self.lib.mmgen_mesh_section_quads_count(self._p(blocks), self._p(chunk_idx), self._p(neighbor_idx), n, self._p(secq), self._p(chq),
                                                            self._stream()), "mmgen_mesh_section_quads_count")
        if capacity_quads is None:
            incl = t.cumsum(chq.to(t.int64), 0)
            off = (incl - chq).contiguous()
            total = int(incl[-1].item()) if n else 0
            quads = self._empty((max(total, 1),), t.int32)
            capacity = 2 ** 64 - 1
        else:
            off = self._empty((max(n, 1),), t.int64)[:n]
            tot = self._empty((1,), t.int64)
            quads = t.full((capacity_quads,), -7, dtype=t.int32, device=blocks.device)
            self._check(self.lib.mmgen_mesh_offsets(self._p(chq), n, self._p(off), self._p(tot), self._stream()), "mmgen_mesh_offsets")
            total, capacity = None, capacity_quads
        if n:
            self._check(self.lib.mmgen_mesh_section_quads_fill(self._p(blocks), self._p(chunk_idx), self._p(neighbor_idx), n, self._p(secq), self._p(off),
                                                               capacity, self._p(quads), self._stream()), "mmgen_mesh_section_quads_fill")
        if total is None:
            return dict(quads=quads, section_quads=secq, chunk_quads=chq, quad_offset=off, total=int(tot.item()))
        return dict(quads=quads[:total], section_quads=secq, chunk_quads=chq, quad_offset=off, total=total)

    def mesh_lit_section_quads(self, blocks, light, nx=None, nz=None, neighbor_idx=None, chunk_idx=None, capacity_quads=None, light_mask=0xff):
        """mesh_section_quads with flat per-face light (include/mmgen.h "lit section quad mesh"): light uint8 [slots, 98304] indexed like blocks
        (the output of light()); two faces share a quad only if they share the block id and the light of the voxel in front of them under
        light_mask.  Returns the dict of mesh_section_quads plus quad_light uint8 [Q or capacity], the face light of every record (the capped
        form pre-fills it with 0xf9); section_draws accepts the dict as it is."""
        t = self.torch
        n = blocks.shape[0] if chunk_idx is None else chunk_idx.shape[0]
        vp, i32, u64, u8 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint8
        self.lib.mmgen_mesh_lit_section_quads_count.argtypes = [vp, vp, vp, vp, i32, u8, vp, vp, vp]
        self.lib.mmgen_mesh_lit_section_quads_fill.argtypes = [vp, vp, vp, vp, i32, u8, vp, vp, u64, vp, vp, vp]
        self.lib.mmgen_mesh_offsets.argtypes = [vp, i32, vp, vp, vp]
        assert light.dtype == t.uint8 and light.shape == blocks.shape and light.is_contiguous() and 0 <= int(light_mask) <= 0xff
        if neighbor_idx is None and nx is not None:
            assert chunk_idx is None, "a grid shape names the neighbours of chunks 0 .. n-1; give neighbor_idx with chunk_idx"
            c = t.arange(n, dtype=t.int32, device=blocks.device)
            x, z = c % nx, c // nx
            neg = t.full_like(c, -1)
            neighbor_idx = t.stack([t.where(z < nz - 1, c + nx, neg), t.where(x < nx - 1, c + 1, neg), t.where(z > 0, c - nx, neg),
                                    t.where(x > 0, c - 1, neg)], dim=1).contiguous()
        secq = self._empty((max(n, 1), self.SECTIONS), t.int32)[:n]
        chq = self._empty((n,), t.int32)
        self._check(self.lib.mmgen_mesh_lit_section_quads_count(self._p(blocks), self._p(light), self._p(chunk_idx), self._p(neighbor_idx), n, int(light_mask),
                                                                self._p(secq), self._p(chq), self._stream()), "mmgen_mesh_lit_section_quads_count")
        if capacity_quads is None:
            incl = t.cumsum(chq.to(t.int64), 0)
            off = (incl - chq).contiguous()
            total = int(incl[-1].item()) if n else 0
            quads, ql = self._empty((max(total, 1),), t.int32), self._empty((max(total, 1),), t.uint8)
            capacity = 2 ** 64 - 1
        else:
            off = self._empty((max(n, 1),), t.int64)[:n]
            tot = self._empty((1,), t.int64)
            quads = t.full((capacity_quads,), -7, dtype=t.int32, device=blocks.device)
            ql = t.full((capacity_quads,), 0xf9, dtype=t.uint8, device=blocks.device)
            self._check(self.lib.mmgen_mesh_offsets(self._p(chq), n, self._p(off), self._p(tot), self._stream()), "mmgen_mesh_offsets")
            total, capacity = None, capacity_quads
        if n:
            self._check(self.lib.mmgen_mesh_lit_section_quads_fill(self._p(blocks), self._p(light), self._p(chunk_idx), self._p(neighbor_idx), n, int(light_mask),
                                                                   self._p(secq), self._p(off), capacity, self._p(quads), self._p(ql), self._stream()),
                        "mmgen_mesh_lit_section_quads_fill")
        if total is None:
            return dict(quads=quads, quad_light=ql, section_quads=secq, chunk_quads=chq, quad_offset=off, total=int(tot.item()))
        return dict(quads=quads[:total], quad_light=ql[:total], section_quads=secq, chunk_quads=chq, quad_offset=off, total=total)

    def mesh_ao_section_quads(self, blocks, light, nx=None, nz=None, neighbor_idx8=None, chunk_idx=None, capacity_quads=None, light_mask=0xff):
        """mesh_lit_section_quads with per-corner ambient occlusion (include/mmgen.h "section quad mesh with ambient occlusion"): two faces share a
        quad only if they also share the AO byte of mmgen_types.h.  neighbor_idx8 int32 [n, 8]: N E S W, then the diagonals (+x,+z) (+x,-z)
        (-x,-z) (-x,+z), -1 = absent; a grid shape builds all eight.  light may be None iff light_mask == 0.  Returns the dict of
        mesh_lit_section_quads plus quad_ao uint8 [Q or capacity] (the capped form pre-fills it with 0xf9); section_draws accepts the dict as it is."""
        t = self.torch
        n = blocks.shape[0] if chunk_idx is None else chunk_idx.shape[0]
        vp, i32, u64, u8 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint8
        self.lib.mmgen_mesh_ao_section_quads_count.argtypes = [vp, vp, vp, vp, i32, u8, vp, vp, vp]
        self.lib.mmgen_mesh_ao_section_quads_fill.argtypes = [vp, vp, vp, vp, i32, u8, vp, vp, u64, vp, vp, vp, vp]
        self.lib.mmgen_mesh_offsets.argtypes = [vp, i32, vp, vp, vp]
        assert 0 <= int(light_mask) <= 0xff and (light is not None or int(light_mask) == 0)
        assert light is None or (light.dtype == t.uint8 and light.shape == blocks.shape and light.is_contiguous())
        if neighbor_idx8 is None and nx is not None:
            assert chunk_idx is None, "a grid shape names the neighbours of chunks 0 .. n-1; give neighbor_idx8 with chunk_idx"
            c = t.arange(n, dtype=t.int32, device=blocks.device)
            x, z = c % nx, c // nx
            neg = t.full_like(c, -1)
            n_, e_, s_, w_ = z < nz - 1, x < nx - 1, z > 0, x > 0
            neighbor_idx8 = t.stack([t.where(n_, c + nx, neg), t.where(e_, c + 1, neg), t.where(s_, c - nx, neg), t.where(w_, c - 1, neg),
                                     t.where(e_ & n_, c + nx + 1, neg), t.where(e_ & s_, c - nx + 1, neg), t.where(w_ & s_, c - nx - 1, neg),
                                     t.where(w_ & n_, c + nx - 1, neg)], dim=1).contiguous()
        assert neighbor_idx8 is None or (neighbor_idx8.dtype == t.int32 and tuple(neighbor_idx8.shape) == (n, 8) and neighbor_idx8.is_contiguous())
        secq = self._empty((max(n, 1), self.SECTIONS), t.int32)[:n]
        chq = self._empty((n,), t.int32)
        self._check(self.lib.mmgen_mesh_ao_section_quads_count(self._p(blocks), self._p(light), self._p(chunk_idx), self._p(neighbor_idx8), n, int(light_mask),
                                                               self._p(secq), self._p(chq), self._stream()), "mmgen_mesh_ao_section_quads_count")
        if capacity_quads is None:
            incl = t.cumsum(chq.to(t.int64), 0)
            off = (incl - chq).contiguous()
            total = int(incl[-1].item()) if n else 0
            quads, ql, qa = self._empty((max(total, 1),), t.int32), self._empty((max(total, 1),), t.uint8), self._empty((max(total, 1),), t.uint8)
            capacity = 2 ** 64 - 1
        else:
            off = self._empty((max(n, 1),), t.int64)[:n]
            tot = self._empty((1,), t.int64)
            quads = t.full((capacity_quads,), -7, dtype=t.int32, device=blocks.device)
            ql, qa = (t.full((capacity_quads,), 0xf9, dtype=t.uint8, device=blocks.device) for _ in range(2))
            self._check(self.lib.mmgen_mesh_offsets(self._p(chq), n, self._p(off), self._p(tot), self._stream()), "mmgen_mesh_offsets")
            total, capacity = None, capacity_quads
        if n:
            self._check(self.lib.mmgen_mesh_ao_section_quads_fill(self._p(blocks), self._p(light), self._p(chunk_idx), self._p(neighbor_idx8), n, int(light_mask),
                                                                  self._p(secq), self._p(off), capacity, self._p(quads), self._p(ql), self._p(qa), self._stream()),
                        "mmgen_mesh_ao_section_quads_fill")
        if total is None:
            return dict(quads=quads, quad_light=ql, quad_ao=qa, section_quads=secq, chunk_quads=chq, quad_offset=off, total=int(tot.item()))
        return dict(quads=quads[:total], quad_light=ql[:total], quad_ao=qa[:total], section_quads=secq, chunk_quads=chq, quad_offset=off, total=total)

    @classmethod
    def section_quad_fields(cls, quads):
        """Decodes section quad records (int32 tensor or array) into a dict of numpy fields x, y (0..15, local to the section), z, kind,
        w (extent - 1 along the plane's rows), l (extent - 1 along its fast axis), block (mmgen_types.h)."""
        import numpy as np
        q = (quads.cpu().numpy() if hasattr(quads, "cpu") else np.asarray(quads)).astype(np.int64) & 0xffffffff
        field = lambda shift, bits: ((q >> shift) & ((1 << bits) - 1)).astype(np.int32)
        return dict(x=field(0, 4), y=field(4, 4), z=field(8, 4), kind=field(12, 3), w=field(15, 4), l=field(19, 4), block=field(23, 8))

    def section_draws(self, visible, grid, eye_cell, radius, mesh, mesh_pos=None, capacity=None):
        """The draw list of a visible set (visible_sections' output for the same grid, eye cell (cx, cz) and radius) over a section mesh (the
        dict of mesh_section_quads): one (first, count, origin) per visible section that has records, in window order.  mesh_pos: int32
        [slots] device tensor, position of a chunk slot in the mesh's work list, -1 = not meshed; None = the slot itself.  capacity=None
        sizes the buffer for every section of the window; a given capacity receives the first `capacity` draws.  The buffer is pre-filled with 0xff bytes
        and has one guard record behind the capacity.  Returns dict(draws numpy records [min(total, capacity)] of SECTION_DRAW_DTYPE,
        totals (draws, quads) over all draws, buffer = the device tensor uint8 [capacity + 1, 16])."""
        import numpy as np
        t = self.torch
        vp, i32, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
        self.lib.mmgen_section_draws.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, u32, vp, vp, vp]
        assert grid.dtype == t.int32 and grid.dim() == 2 and grid.is_contiguous() and visible.is_contiguous()
        cx, cz = (int(v) for v in eye_cell)
        w = 2 * max(int(radius), 0) + 1
        assert visible.numel() == w * w
        cap = w * w * self.SECTIONS if capacity is None else int(capacity)
        buf = t.full((cap + 1, 16), 0xff, dtype=t.uint8, device=self.device)
        totals = self._empty((2,), t.int64)
        secq, off = mesh["section_quads"], mesh["quad_offset"]
        self._check(self.lib.mmgen_section_draws(self._p(visible), self._p(grid), grid.shape[1], grid.shape[0], cx, cz, int(radius), self._p(mesh_pos),
                                                 self._p(secq), self._p(off), secq.shape[0], cap, self._p(buf), self._p(totals), self._stream()),
                    "mmgen_section_draws")
        tot = tuple(int(v) for v in totals.cpu().numpy())
        draws = np.ascontiguousarray(buf.cpu().numpy()).view(np.dtype(self.SECTION_DRAW_DTYPE)).reshape(-1)
        return dict(draws=draws[:min(tot[0], cap)], totals=tot, buffer=buf)

    # ------------------------------------------------------------------ region wire format (run-length pairs per column)
    def pack(self, blocks):
        """blocks uint8 [n, 98304] on the device -> dict(data uint8 [total], chunk_bytes int32 [n], chunk_offset int64 [n])."""
        t = self.torch
        n = blocks.shape[0]
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        self.lib.mmgen_pack_count.argtypes = [vp, vp, i32, vp, vp, vp]
        self.lib.mmgen_pack_fill.argtypes = [vp, vp, i32, vp, vp, vp, vp]
        runs = self._empty((n, 256), t.int16)
        nbytes = self._empty((n,), t.int32)
        self._check(self.lib.mmgen_pack_count(self._p(blocks), None, n, self._p(runs), self._p(nbytes), self._stream()), "mmgen_pack_count")
        incl = t.cumsum(nbytes.to(t.int64), 0)
        off = (incl - nbytes).contiguous()
        total = int(incl[-1].item()) if n else 0
        data = self._empty((max(total, 1),), t.uint8)
        if n:
            self._check(self.lib.mmgen_pack_fill(self._p(blocks), None, n, self._p(runs), self._p(off), self._p(data), self._stream()), "mmgen_pack_fill")
        return dict(data=data[:total], chunk_bytes=nbytes, chunk_offset=off)

    def unpack(self, data, chunk_offset):
        t = self.torch
        n = chunk_offset.shape[0]
        self.lib.mmgen_unpack.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        blocks = self._empty((n, BLOCKS), t.uint8)
        if n:
            self._check(self.lib.mmgen_unpack(self._p(data), self._p(chunk_offset), n, self._p(blocks), self._stream()), "mmgen_unpack")
        return blocks

    def unpack_chunk_host(self, packed_bytes):
        """Host decoder of one packed chunk (numpy uint8 in, numpy uint8 [98304] out); raises on a malformed stream."""
        import numpy as np
        self.lib.mmgen_unpack_chunk_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        src = np.ascontiguousarray(packed_bytes, dtype=np.uint8)
        out = np.zeros(BLOCKS, np.uint8)
        if self.lib.mmgen_unpack_chunk_host(src.ctypes.data, src.size, out.ctypes.data) != 0:
            raise ValueError("malformed packed chunk")
        return out

    # ------------------------------------------------------------------ ray casting over device-resident chunks (include/mmgen.h)
    RAY_HIT, RAY_MISS_TMAX, RAY_LEFT_GRID, RAY_ABSENT_CHUNK, RAY_INVALID = range(5)
    RAY_NO_SKIP, RAY_COUNT_VISITS = 1, 2
    RAY_HIT_DTYPE = [("voxel", "<i4", 3), ("t", "<f4"), ("block", "u1"), ("face", "u1"), ("status", "u1"), ("pad", "u1")]      # mmgen_ray_hit

    def ray_occupancy(self, blocks, stop_mask=15, chunk_idx=None, out=None):
        """Skip structure of the chunks of `blocks` (uint8 [slots, 98304]) for one stop_mask -> uint8 [slots, 200], indexed like blocks.
        chunk_idx (int32 device tensor): only these slots are (re)built, into `out`."""
        t = self.torch
        vp = ctypes.c_void_p
        self.lib.mmgen_ray_occupancy.argtypes = [vp, vp, ctypes.c_int, ctypes.c_uint, vp, vp]
        occ = out if out is not None else t.zeros((blocks.shape[0], 200), dtype=t.uint8, device=self.device)
        n = blocks.shape[0] if chunk_idx is None else chunk_idx.shape[0]
        self._check(self.lib.mmgen_ray_occupancy(self._p(blocks), self._p(chunk_idx), n, stop_mask, self._p(occ), self._stream()), "mmgen_ray_occupancy")
        return occ

    def raycast(self, blocks, grid, occ, rays, stop_mask=15, t_max=4096.0, flags=0):
        """grid: int32 [grid_h, grid_w] chunk index into blocks or -1; rays: float32 [n, 6] (o, d) in grid-local block coordinates, on the
        device.  Returns the hit records as an int32 [n, 5] device tensor; ray_hits() views them as numpy records."""
        t = self.torch
        vp, i32, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
        self.lib.mmgen_raycast.argtypes = [vp, vp, i32, i32, vp, u32, u32, vp, i32, ctypes.c_float, vp, vp]
        assert grid.dtype == t.int32 and rays.dtype == t.float32 and rays.shape[1] == 6 and grid.is_contiguous() and rays.is_contiguous()
        n = rays.shape[0]
        hits = self._empty((n, 5), t.int32)
        self._check(self.lib.mmgen_raycast(self._p(blocks), self._p(grid), grid.shape[1], grid.shape[0], self._p(occ), stop_mask, flags, self._p(rays), n,
                                           t_max, self._p(hits), self._stream()), "mmgen_raycast")
        return hits

    def render_view(self, blocks, grid, occ, eye, forward, up=(0.0, 1.0, 0.0), fov_y=1.0, width=640, height=360, stop_mask=15, t_max=4096.0, flags=0):
        """One primary ray per pixel of a pinhole camera (mmgen_raycast_camera) -> int32 [height, width, 5] hit records on the device."""
        t = self.torch

        class Camera(ctypes.Structure):
            _fields_ = [("eye", ctypes.c_float * 3), ("forward", ctypes.c_float * 3), ("up", ctypes.c_float * 3), ("fov_y", ctypes.c_float),
                        ("width", ctypes.c_int32), ("height", ctypes.c_int32)]
        f3 = ctypes.c_float * 3
        cam = Camera(f3(*eye), f3(*forward), f3(*up), fov_y, width, height)
        vp, i32, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
        self.lib.mmgen_raycast_camera.argtypes = [vp, vp, i32, i32, vp, u32, u32, ctypes.POINTER(Camera), ctypes.c_float, vp, vp]
        assert grid.dtype == t.int32 and grid.is_contiguous()
        hits = self._empty((height, width, 5), t.int32)
        self._check(self.lib.mmgen_raycast_camera(self._p(blocks), self._p(grid), grid.shape[1], grid.shape[0], self._p(occ), stop_mask, flags,
                                                  ctypes.byref(cam), t_max, self._p(hits), self._stream()), "mmgen_raycast_camera")
        return hits

    # ------------------------------------------------------------------ shaded camera render (include/mmgen.h)
    RENDER_AO, RENDER_TRANSLUCENT, RENDER_SUN_SHADOW, RENDER_FOG = 1, 2, 4, 8

    def render_default_palette(self):
        """The default palette (include/mmgen.h) as a numpy uint32 [256]: r | g << 8 | b << 16 | alpha << 24."""
        import numpy as np
        out = np.zeros(256, np.uint32)
        self.lib.mmgen_render_default_palette.argtypes = [ctypes.c_void_p]
        self._check(self.lib.mmgen_render_default_palette(out.ctypes.data), "mmgen_render_default_palette")
        return out

    def render_camera(self, blocks, grid, occ_first, eye, forward, up=(0.0, 1.0, 0.0), fov_y=1.0, width=640, height=360, occ_second=None, light=None,
                      palette=None, flags=0, first_mask=15, t_max=4096.0, sun_dir=(0.45, 0.8, 0.3), fog_start=0.0, fog_end=4096.0,
                      sky_rgb=(150, 190, 235), sun_level=15, shadow_dim=140, return_hits=False):
        """One shaded pixel per camera ray (mmgen_render_camera) -> uint8 [height, width, 4] RGBA on the device, and with return_hits the
        int32 [height, width, 5] records of walk A.  occ_first: ray_occupancy for first_mask; occ_second: ray_occupancy for stop mask 3
        (OPAQUE | SEMI), needed with RENDER_TRANSLUCENT or RENDER_SUN_SHADOW; light: the volume of light(), None = full bright; palette:
        uint32 [256] device tensor (int32 storage), None = the default."""
        t = self.torch

        class Camera(ctypes.Structure):
            _fields_ = [("eye", ctypes.c_float * 3), ("forward", ctypes.c_float * 3), ("up", ctypes.c_float * 3), ("fov_y", ctypes.c_float),
                        ("width", ctypes.c_int32), ("height", ctypes.c_int32)]

        class Params(ctypes.Structure):
            _fields_ = [("flags", ctypes.c_uint32), ("first_mask", ctypes.c_uint32), ("t_max", ctypes.c_float), ("sun_dir", ctypes.c_float * 3),
                        ("fog_start", ctypes.c_float), ("fog_end", ctypes.c_float), ("sky_rgb", ctypes.c_uint8 * 3), ("sun_level", ctypes.c_uint8),
                        ("shadow_dim", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3)]
        f3, b3 = ctypes.c_float * 3, ctypes.c_uint8 * 3
        cam = Camera(f3(*eye), f3(*forward), f3(*up), fov_y, width, height)
        par = Params(flags, first_mask, t_max, f3(*sun_dir), fog_start, fog_end, b3(*sky_rgb), sun_level, shadow_dim)
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        self.lib.mmgen_render_camera.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, ctypes.POINTER(Camera), ctypes.POINTER(Params), vp, vp, vp]
        assert grid.dtype == t.int32 and grid.is_contiguous()
        assert palette is None or (palette.element_size() == 4 and palette.numel() == 256 and palette.is_contiguous())
        rgba = self._empty((height, width, 4), t.uint8)
        hits = self._empty((height, width, 5), t.int32) if return_hits else None
        self._check(self.lib.mmgen_render_camera(self._p(blocks), self._p(grid), grid.shape[1], grid.shape[0], self._p(occ_first), self._p(occ_second),
                                                 self._p(light), self._p(palette), ctypes.byref(cam), ctypes.byref(par), self._p(rgba), self._p(hits),
                                                 self._stream()), "mmgen_render_camera")
        return (rgba, hits) if return_hits else rgba

    @classmethod
    def ray_hits(cls, hits):
        """The int32 [..., 5] tensor of raycast / render_view as a numpy record array [...] of mmgen_ray_hit."""
        import numpy as np
        a = hits.cpu().numpy()
        return np.ascontiguousarray(a).view(np.dtype(cls.RAY_HIT_DTYPE)).reshape(a.shape[:-1])

    # ------------------------------------------------------------------ voxel lighting over device-resident chunks (include/mmgen.h)
    LIGHT_MASK_BYTES = 62976

    def light_default_emission(self):
        """The default emission table (include/mmgen.h) as a numpy uint8 [256]."""
        import numpy as np
        out = np.zeros(256, np.uint8)
        self.lib.mmgen_light_default_emission.argtypes = [ctypes.c_void_p]
        self._check(self.lib.mmgen_light_default_emission(out.ctypes.data), "mmgen_light_default_emission")
        return out

    def light_masks(self, blocks, chunk_idx=None, emission=None, out=None):
        """What the lighting reads of the chunks of `blocks` (uint8 [slots, 98304]) -> uint8 [slots, LIGHT_MASK_BYTES], indexed like blocks.
        chunk_idx (int32 device tensor): only these slots are (re)built, into `out`.  emission: uint8 [256] device tensor, None = default."""
        t = self.torch
        vp = ctypes.c_void_p
        self.lib.mmgen_light_masks.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
        masks = out if out is not None else t.zeros((blocks.shape[0], self.LIGHT_MASK_BYTES), dtype=t.uint8, device=self.device)
        n = blocks.shape[0] if chunk_idx is None else chunk_idx.shape[0]
        assert emission is None or (emission.dtype == t.uint8 and emission.numel() == 256 and emission.is_contiguous())
        self._check(self.lib.mmgen_light_masks(self._p(blocks), self._p(chunk_idx), n, self._p(emission), self._p(masks), self._stream()), "mmgen_light_masks")
        return masks

    def light(self, masks, grid, cells=None, out=None):
        """grid: int32 [grid_h, grid_w] chunk slot or -1; masks: light_masks of every present chunk.  cells (int32 device tensor of grid cell
        indices cz * grid_w + cx): only these are lit, None = all.  Returns uint8 [slots, 98304] of (sky << 4) | block, indexed like blocks;
        slots that are not lit keep what `out` held (zero when it is allocated here)."""
        t = self.torch
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        self.lib.mmgen_light.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
        assert grid.dtype == t.int32 and grid.dim() == 2 and grid.is_contiguous()
        light = out if out is not None else t.zeros((masks.shape[0], BLOCKS), dtype=t.uint8, device=self.device)
        n = grid.numel() if cells is None else cells.shape[0]
        self._check(self.lib.mmgen_light(self._p(masks), self._p(grid), grid.shape[1], grid.shape[0], self._p(cells), n, self._p(light), self._stream()),
                    "mmgen_light")
        return light

    # ------------------------------------------------------------------ section visibility over device-resident chunks (include/mmgen.h)
    SECTION_CONN_BYTES = 48
    VISIBLE_MAX_RADIUS = 32

    def section_connectivity(self, blocks, chunk_idx=None, out=None, rounds=None):
        """Face connectivity of the 24 sections of the chunks of `blocks` (uint8 [slots, 98304]) -> uint8 [slots, 48] (u16 [24] per slot),
        indexed like blocks.  chunk_idx (int32 device tensor): only these slots are (re)built, into `out`.  rounds (int32 [slots] device
        tensor, measuring only): receives the flood rounds of every chunk built."""
        t = self.torch
        vp = ctypes.c_void_p
        self.lib.mmgen_section_connectivity.argtypes = [vp, vp, ctypes.c_int, vp, vp]
        self.lib.mmgen_debug_section_rounds.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
        conn = out if out is not None else t.zeros((blocks.shape[0], self.SECTION_CONN_BYTES), dtype=t.uint8, device=self.device)
        n = blocks.shape[0] if chunk_idx is None else chunk_idx.shape[0]
        if rounds is not None:
            assert rounds.dtype == t.int32 and rounds.numel() >= blocks.shape[0] and rounds.is_contiguous()
            code = self.lib.mmgen_debug_section_rounds(self._p(blocks), self._p(chunk_idx), n, self._p(conn), self._p(rounds), self._stream())
        else:
            code = self.lib.mmgen_section_connectivity(self._p(blocks), self._p(chunk_idx), n, self._p(conn), self._stream())
        self._check(code, "mmgen_section_connectivity")
        return conn

    def visible_sections(self, conn, grid, eye_section, radius):
        """grid: int32 [grid_h, grid_w] chunk slot or -1; conn: section_connectivity of every present chunk of the window; eye_section:
        (cx, sy, cz) with sy in [-1, 24].  Returns uint32 [2 radius + 1, 2 radius + 1]: entry [cz - eye_cz + radius][cx - eye_cx + radius]
        has bit sy set iff that section has to be drawn."""
        t = self.torch
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        self.lib.mmgen_visible_sections.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
        assert grid.dtype == t.int32 and grid.dim() == 2 and grid.is_contiguous() and conn.dtype == t.uint8 and conn.is_contiguous()
        cx, sy, cz = (int(v) for v in eye_section)
        w = 2 * max(int(radius), 0) + 1
        vis = self._empty((w, w), t.uint32)
        self._check(self.lib.mmgen_visible_sections(self._p(conn), self._p(grid), grid.shape[1], grid.shape[0], cx, sy, cz, int(radius), self._p(vis),
                                                    self._stream()), "mmgen_visible_sections")
        return vis

    # ------------------------------------------------------------------ level-of-detail chunks (include/mmgen.h)
    def lod_reduce(self, blocks, src_idx, level, out=None, dst_idx=None):
        """src_idx: int32 [n, s * s] device tensor, s = 1 << level (1..3): the slots of `blocks` (uint8 [slots, 98304]) under LOD chunk i in
        the order qx + s qz, -1 = absent.  LOD chunk i goes to slot dst_idx[i] of `out` (int32 [n] device tensor, None = slot i); `out` is
        allocated as uint8 [n, 98304] when None and must not share memory with `blocks`.  Returns the output tensor."""
        t = self.torch
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        self.lib.mmgen_lod_reduce.argtypes = [vp, vp, i32, i32, vp, vp, vp]
        assert src_idx.dtype == t.int32 and src_idx.dim() == 2 and src_idx.is_contiguous() and src_idx.shape[1] == 1 << (2 * int(level))
        assert dst_idx is None or (dst_idx.dtype == t.int32 and dst_idx.numel() == src_idx.shape[0] and dst_idx.is_contiguous())
        n = src_idx.shape[0]
        lod = out if out is not None else self._empty((n, BLOCKS), t.uint8)
        self._check(self.lib.mmgen_lod_reduce(self._p(blocks), self._p(src_idx), n, int(level), self._p(lod), self._p(dst_idx), self._stream()),
                    "mmgen_lod_reduce")
        return lod

    # ------------------------------------------------------------------ region fast path (all stages, device resident)
    EROSION, FEATURES, DECORATORS = 1, 2, 4

    def close(self):
        """Destroys the region handle (its device buffers: ~0.4 MB per chunk of the largest region it generated).  Called by __del__; a
        long-lived process that creates many MMGen objects would otherwise hold every handle's memory until it exits."""
        h = getattr(self, "_region_handle", None)
        if h is not None:
            self._region_handle = None
            try:
                self.lib.mmgen_region_destroy.argtypes = [ctypes.c_void_p]
                self.lib.mmgen_region_destroy(h)
            except Exception:                     # (interpreter shutdown: the library may be gone)
                pass

    def __del__(self):
        self.close()

    def _region(self):
        if getattr(self, "_region_handle", None) is None:
            h = ctypes.c_void_p()
            self.lib.mmgen_region_create.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
            self._check(self.lib.mmgen_region_create(ctypes.byref(h)), "mmgen_region_create")
            self._region_handle = h
            vp, i32 = ctypes.c_void_p, ctypes.c_int
            self.lib.mmgen_region_begin.argtypes = [vp, i32, i32, i32, i32, ctypes.c_uint, vp, vp]
            self.lib.mmgen_region_finish.argtypes = [vp, vp, vp, vp, vp, vp]
            self.lib.mmgen_region_fill.argtypes = [vp, vp, vp]
            if hasattr(self.lib, "mmgen_region_set_output"):
                self.lib.mmgen_region_set_output.argtypes = [vp, vp]
            self.lib.mmgen_ring_header.argtypes = [vp, vp, i32, vp, vp]
            self.lib.mmgen_ring_offsets.argtypes = [vp, i32, vp, vp]
            self.lib.mmgen_ring_pack.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp]
            self.lib.mmgen_ring_unpack.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp]
            self.lib.mmgen_region_placement_buffers.argtypes = [vp] + [ctypes.POINTER(vp)] * 3 + [ctypes.POINTER(i32)] * 4
            self.lib.mmgen_region_last_erosion_passes.argtypes = [vp]
        return self._region_handle

    def region_set_zone_cache(self, max_zones):
        """Keep the eroded layers of up to max_zones zones across region calls (include/mmgen.h mmgen_region_set_zone_cache; 0 = off)."""
        self.lib.mmgen_region_set_zone_cache.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self._check(self.lib.mmgen_region_set_zone_cache(self._region(), max_zones), "mmgen_region_set_zone_cache")

    def region_zone_cache_stats(self):
        h, m = ctypes.c_longlong(0), ctypes.c_longlong(0)
        self.lib.mmgen_region_zone_cache_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
        self._check(self.lib.mmgen_region_zone_cache_stats(self._region(), ctypes.byref(h), ctypes.byref(m)), "mmgen_region_zone_cache_stats")
        return h.value, m.value

    def region_set_serial(self, serial, slices=0):
        """serial=True: every kernel of the region path on one stream (per-kernel attribution); False: the stage DAG (include/mmgen.h)."""
        self.lib.mmgen_region_set_serial.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        self._check(self.lib.mmgen_region_set_serial(self._region(), int(bool(serial)), int(slices)), "mmgen_region_set_serial")

    def region_max_cave_placements(self):
        """Largest cave placement list length seen by region_finish since the last call (synchronises); > CFP_CAP (1024) means entries were
        dropped (include/mmgen.h MMGEN_ERROR_PLACEMENT_OVERFLOW).  Clears the record."""
        m = ctypes.c_int(0)
        self.lib.mmgen_region_max_cave_placements.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
        self._check(self.lib.mmgen_region_max_cave_placements(self._region(), ctypes.byref(m), self._stream()), "mmgen_region_max_cave_placements")
        return m.value

    def region_max_gathered(self):
        """(surface, cave): the longest gathered, un-truncated placement lists of the finishes since the last call (synchronises; clears)."""
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        self.lib.mmgen_region_max_gathered.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
        self._check(self.lib.mmgen_region_max_gathered(self._region(), ctypes.byref(a), ctypes.byref(b), self._stream()), "mmgen_region_max_gathered")
        return a.value, b.value

    def region_begin(self, cx0, cz0, nx, nz, flags, local_mask=None):
        mask = None
        if local_mask is not None:
            mask = local_mask if isinstance(local_mask, ctypes.Array) else (ctypes.c_uint8 * len(local_mask))(*[int(m) for m in local_mask])
        # the output buffer is named up front (mmgen_region_set_output): begin then issues the base fill as soon as its inputs exist.  The
        # tensor is fresh from torch's stream-ordered allocator and nothing touches it before region_finish hands it out
        self._region_blocks = self._empty((nx * nz, BLOCKS), self.torch.uint8)
        if hasattr(self.lib, "mmgen_region_set_output"):      # (absent only in the older A/B builds MMGEN_LIB may point at)
            self._check(self.lib.mmgen_region_set_output(self._region(), self._p(self._region_blocks)), "mmgen_region_set_output")
        self._check(self.lib.mmgen_region_begin(self._region(), cx0, cz0, nx, nz, flags, mask, self._stream()), "mmgen_region_begin")

    def region_fill(self, nx, nz):
        """Base blocks of the rectangle (no feature lists needed): issued while the placement-ring exchange is in flight."""
        if getattr(self, "_region_blocks", None) is None:
            self._region_blocks = self._empty((nx * nz, BLOCKS), self.torch.uint8)
        self._check(self.lib.mmgen_region_fill(self._region(), self._p(self._region_blocks), self._stream()), "mmgen_region_fill")

    # compact ring exchange (include/mmgen.h mmgen_ring_*): all tensors int32 on the device
    def ring_header(self, bufs, cells):
        n = cells.shape[0]
        header = self._empty((n, 2), self.torch.int32)
        self._check(self.lib.mmgen_ring_header(self._p(bufs["counts"]), self._p(cells), n, self._p(header), self._stream()), "mmgen_ring_header")
        return header

    def ring_offsets(self, header):
        n = header.shape[0]
        off = self._empty((n + 1,), self.torch.int32)
        self._check(self.lib.mmgen_ring_offsets(self._p(header), n, self._p(off), self._stream()), "mmgen_ring_offsets")
        return off

    def ring_pack(self, bufs, cells, header, offsets, total_words):
        payload = self._empty((max(total_words, 1),), self.torch.int32)
        self._check(self.lib.mmgen_ring_pack(self._p(bufs["fp"]), self._p(bufs["cfp"]), self._p(cells), self._p(header), self._p(offsets),
                                             cells.shape[0], self._p(payload), self._stream()), "mmgen_ring_pack")
        return payload

    def ring_unpack(self, bufs, cells, header, offsets, payload):
        self._check(self.lib.mmgen_ring_unpack(self._p(payload), self._p(header), self._p(offsets), self._p(cells), cells.shape[0],
                                               self._p(bufs["fp"]), self._p(bufs["cfp"]), self._p(bufs["counts"]), self._stream()), "mmgen_ring_unpack")

    # one-phase exchange (include/mmgen.h mmgen_ring_pack_messages / _unpack_messages): fixed-size messages, lengths in-band, no host read
    def ring_pack_messages(self, bufs, cells, slots, scratch, messages, overflow):
        vp = ctypes.c_void_p
        self.lib.mmgen_ring_pack_messages.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp]
        self._check(self.lib.mmgen_ring_pack_messages(self._p(bufs["fp"]), self._p(bufs["cfp"]), self._p(bufs["counts"]), self._p(cells), self._p(slots),
                                                      cells.shape[0], self._p(scratch), self._p(messages), self._p(overflow), self._stream()),
                    "mmgen_ring_pack_messages")

    def ring_unpack_messages(self, bufs, cells, slots, scratch, messages, overflow):
        vp = ctypes.c_void_p
        self.lib.mmgen_ring_unpack_messages.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
        self._check(self.lib.mmgen_ring_unpack_messages(self._p(messages), self._p(cells), self._p(slots), cells.shape[0], self._p(scratch),
                                                        self._p(bufs["fp"]), self._p(bufs["cfp"]), self._p(bufs["counts"]), self._p(overflow), self._stream()),
                    "mmgen_ring_unpack_messages")

    def region_placement_buffers(self):
        """Torch views (no copy) of the region's ring-extended placement grid: fp [cells,256,5], cfp [cells,1024,6], counts [cells,2]."""
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        fp, cfp, cnt = vp(), vp(), vp()
        x0, z0, w, h = i32(), i32(), i32(), i32()
        self._check(self.lib.mmgen_region_placement_buffers(self._region(), ctypes.byref(fp), ctypes.byref(cfp), ctypes.byref(cnt), ctypes.byref(x0),
                                                            ctypes.byref(z0), ctypes.byref(w), ctypes.byref(h)), "mmgen_region_placement_buffers")
        cells = w.value * h.value
        return dict(fp=self._view(fp.value, (cells, 256, 5)), cfp=self._view(cfp.value, (cells, 1024, 6)), counts=self._view(cnt.value, (cells, 2)),
                    x0=x0.value, z0=z0.value, w=w.value, h=h.value)

    def _view(self, ptr, shape):
        """int32 torch tensor aliasing device memory owned by the library (valid until the next region_begin)."""
        import numpy as np
        n = int(np.prod(shape))

        class _Holder:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}
        return self.torch.as_tensor(_Holder(), device=self.device).view(*shape)

    def region_finish(self, nx, nz, want=()):
        n = nx * nz
        t = self.torch
        blocks = self._region_blocks if getattr(self, "_region_blocks", None) is not None else self._empty((n, BLOCKS), t.uint8)
        self._region_blocks = None
        hf = self._empty((n, HF), t.float32)
        layers = self._empty((n, 20, 256), t.float32) if "layers" in want else None
        cave = self._empty((n, 256, 32, 3), t.int32) if "cave" in want else None
        self._check(self.lib.mmgen_region_finish(self._region(), self._p(blocks), self._p(hf), self._p(layers), self._p(cave), self._stream()),
                    "mmgen_region_finish")
        out = dict(blocks=blocks, hf=hf)
        if layers is not None:
            out["layers"] = layers
        if cave is not None:
            out["cave"] = cave
        return out

    def generate_region(self, cx0, cz0, nx, nz, erosion=True, features=True, decorators=True, want=(), lazy_ring=True):
        flags = (self.EROSION if erosion else 0) | (self.FEATURES if features else 0) | (self.DECORATORS if decorators else 0)
        # the ring's placement lists never leave this call: mask value 2 = computed lazily (include/mmgen.h)
        mask = (ctypes.c_uint8 * ((nx + 6) * (nz + 6)))(*([2] * ((nx + 6) * (nz + 6)))) if (features and lazy_ring) else None
        self.region_begin(cx0, cz0, nx, nz, flags, mask)
        out = self.region_finish(nx, nz, want)
        out["erosion_passes"] = self.lib.mmgen_region_last_erosion_passes(self._region())
        return out

    # ------------------------------------------------------------------ config-2 pipeline (no erosion, no features)
    def generate_chunks_no_erosion(self, pos):
        """K1 -> K2 -> E3 fix-up (DEBUG_SKIP_EROSION semantics, chunk.cu:713-720) -> K4 -> K6; everything stays in HBM."""
        hf, bw, g = self.generate_heightfields(pos, gathered=True)
        layers = self.fix_backward_layers(self.generate_layers(g, bw, pos))
        cave = self.generate_caves(hf, bw, pos)
        blocks = self.fill(hf, bw, layers, cave, pos)
        return dict(hf=hf, bw=bw, gathered=g, layers=layers, cave=cave, blocks=blocks)

    # ------------------------------------------------------------------ test-only device math probe
    PROBES = dict(sin=0, cos=1, pow=2, atan2=3, acos=4, simplex2=5, simplex3=6, fbm2_5=7, fbm3_4=8, rand3from3=9, worley2=10, worley3=11,
                  special_cave_noise=12, biome_height=13, cave_biome=14, hash=15, rng4_u01=16, simplex3_split=17)

    def debug_probe(self, name, packed_in, n, out_per_item=1):
        """packed_in: numpy float32/int32/uint32 array (ints are bit-cast); returns numpy float32 [n, out_per_item]."""
        import numpy as np
        t = self.torch.from_numpy(np.ascontiguousarray(packed_in).view(np.float32).copy()).to(self.device)
        out = self._empty((n, out_per_item), self.torch.float32)
        self.lib.mmgen_debug_probe.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.mmgen_debug_probe(self.PROBES[name], self._p(t), n, self._p(out), self._stream()), "mmgen_debug_probe")
        return out.cpu().numpy()

    def debug_tables(self):
        """The library's constant rule tables as numpy arrays in the layout of tools/extract_ref_tables.py (+ its own reach tables)."""
        import numpy as np
        self.lib.mmgen_debug_tables.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        n = self.lib.mmgen_debug_tables(None, 0, None)
        out = self._empty((n,), self.torch.float32)
        self._check(self.lib.mmgen_debug_tables(self._p(out), n, self._stream()), "mmgen_debug_tables")
        a = out.cpu().numpy()
        t, o = {}, 0
        for name, shape, dt in (("biome_rules", (24, 6), np.uint8), ("grass", (24,), np.uint8), ("material_infos", (20, 4), np.float32),
                                ("biome_material_weights", (24, 20), np.float32), ("feature_bounds", (21, 2), np.int32),
                                ("cave_feature_bounds", (10, 2), np.int32), ("surf_gens", (24, 4, 11), np.float32), ("cave_gens", (5, 3, 9), np.float32),
                                ("deco_gens", (24, 7, 10), np.float32), ("cave_deco_gens", (5, 6, 10), np.float32), ("feature_reach", (21,), np.int32),
                                ("cave_feature_reach", (10,), np.int32), ("gather_offsets", (49, 2), np.int32)):
            k = int(np.prod(shape))
            t[name] = a[o:o + k].reshape(shape).astype(dt)
            o += k
        assert o == n
        return t

    def debug_feature_box(self, is_cave, feature, fpos, layer_height, box_min, box_size):
        i3 = ctypes.c_int32 * 3
        n = box_size[0] * box_size[1] * box_size[2]
        out = self._empty((n,), self.torch.uint8)
        self.lib.mmgen_debug_feature_box.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.mmgen_debug_feature_box(int(is_cave), feature, i3(*fpos), layer_height, i3(*box_min), i3(*box_size), self._p(out),
                                                     self._stream()), "mmgen_debug_feature_box")
        return out.cpu().numpy()
