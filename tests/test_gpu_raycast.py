"""GPU tests of the ray caster (include/mmgen.h "ray casting over device-resident chunks"): mmgen_ray_occupancy, mmgen_raycast and
mmgen_raycast_camera against a plain numpy walk of the traversal contract, one voxel per step, bit for bit."""
import functools
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

HIT, MISS, LEFT, ABSENT, INVALID = range(5)
REC = np.dtype([("voxel", "<i4", 3), ("t", "<f4"), ("block", "u1"), ("face", "u1"), ("status", "u1"), ("pad", "u1")])
FACE = np.array([[1, 3], [4, 5], [0, 2]])                 # [axis][d > 0]: dirVecs index of the outward normal of the face entered
T_MAX = 200.0


def block_classes():
    """class bit of every block id: 1 << transparency of the reference's block table (golden), AIR none, ids beyond the enum OPAQUE"""
    cls = np.ones(256, np.uint8)
    cls[:140] = 1 << np.load(os.path.join(GOLDEN, "block_data.npz"))["block_data"][:, 12]
    cls[0] = 0
    return cls


def dda(ft, blocks, grid, stop_mask, rays, t_max=T_MAX):
    """The contract of include/mmgen.h walked one voxel per step, all rays side by side; ft = float type of the plane arithmetic."""
    gh, gw = grid.shape
    stop = (block_classes() & stop_mask) != 0
    o, d = rays[:, :3].astype(ft), rays[:, 3:].astype(ft)
    with np.errstate(all="ignore"):
        inv = np.where(d != 0, ft(1) / d, ft(0)).astype(ft)
        v = np.floor(o).astype(np.int64)
    out = np.zeros(len(rays), REC)
    out["face"], out["status"] = 6, INVALID
    ok = (np.isfinite(o) & np.isfinite(d) & np.isfinite(inv)).all(1) & (d != 0).any(1) & (o[:, 1] >= -1024) & (o[:, 1] < 1408)
    live = np.flatnonzero(ok & (o[:, 0] >= 0) & (o[:, 0] < 16 * gw) & (o[:, 2] >= 0) & (o[:, 2] < 16 * gh))
    t, face = np.zeros(len(rays), ft), np.full(len(rays), 6)
    while live.size:
        (x, y, z), dl = v[live].T, d[live]
        st, blk = np.full(live.size, -1), np.zeros(live.size, np.uint8)
        left = (x < 0) | (x >= 16 * gw) | (z < 0) | (z >= 16 * gh) | ((y < 0) & (dl[:, 1] <= 0)) | ((y >= 384) & (dl[:, 1] >= 0))
        st[left] = LEFT
        inside = ~left & (y >= 0) & (y < 384)
        g = np.full(live.size, -1)
        g[inside] = grid[z[inside] >> 4, x[inside] >> 4]
        st[inside & (g < 0)] = ABSENT
        rd = inside & (g >= 0)
        blk[rd] = blocks[g[rd], y[rd] + 384 * ((x[rd] & 15) + 16 * (z[rd] & 15))]
        st[rd & stop[blk]] = HIT
        blk[st != HIT] = 0
        with np.errstate(all="ignore"):                   # the step: from the integer voxel, nothing accumulated
            ta = np.where(dl != 0, ((v[live] + (dl > 0)).astype(ft) - o[live]) * inv[live], np.inf)
        a = np.argmin(ta, 1)                              # the first minimum: ties go to the lowest axis
        tm = ta[np.arange(live.size), a]
        miss = (st < 0) & (tm > ft(t_max))
        st[miss], t[live[miss]], face[live[miss]] = MISS, ft(t_max), 6
        done = st >= 0
        r = live[done]
        out["voxel"][r], out["t"][r], out["block"][r], out["face"][r], out["status"][r] = v[r], t[r], blk[done], face[r], st[done]
        go, ag = live[~done], a[~done]
        pos = d[go, ag] > 0
        v[go, ag] += np.where(pos, 1, -1)
        t[go], face[go] = tm[~done], FACE[ag, pos.astype(int)]
        live = go
    return out


# ------------------------------------------------------------------ synthetic pools: a 3 x 2 grid, one absent cell, permuted slots
GRID = np.array([[3, 0, -1], [1, 4, 2]], np.int32)
IDS = np.array([57, 68, 87, 91, 1, 103, 7, 16], np.uint8)  # STONE MARBLE (opaque) two LEAVES (semi) WATER ICE (transparent) GRASS POPPY (X)


@functools.lru_cache(None)
def pool(name):
    rng = np.random.default_rng(0)
    b = np.zeros((5, 16, 16, 384), np.uint8)               # [slot][z][x][y]
    if name == "ragged":                                   # solid below a ragged height, with holes, leaves and plants on top
        h = rng.integers(90, 150, (5, 16, 16))
        y = np.arange(384)
        b[y < h[..., None]] = 57
        b[(y == h[..., None]) & (rng.random((5, 16, 16, 1)) < 0.3)] = 87
        b[rng.random(b.shape) < 0.05] = 0
    else:
        b[:] = np.where(rng.random(b.shape) < float(name), rng.choice(IDS, b.shape), 0)
        b[..., 200:300] = 0                                # empty sections between two noisy layers
        b[2] = 0                                           # one chunk of air
    b[3, 9, 9, 101] = 57                                   # the block a hand-listed ray starts in
    return b.reshape(5, 98304)


@functools.lru_cache(None)
def rays():
    rng = np.random.default_rng(0)
    r = np.empty((4096, 6), np.float32)
    r[:, :3] = rng.uniform([0, -8, 0], [48, 392, 32], (4096, 3))
    r[:, 3:] = rng.normal(size=(4096, 3)) * 10.0 ** rng.uniform(-2, 1, (4096, 1))      # some end by t_max, some leave, some hit
    hand = [(8.5, 100.5, 8.5, 1, 0, 0), (8.5, 100.5, 8.5, -1, 0, 0), (8.5, 100.5, 24.5, 0, 0, 1), (8.5, 100.5, 8.5, 0, 0, -1),      # axis aligned
            (8.5, 390.5, 8.5, 0, -1, 0), (8.5, -5.5, 8.5, 0, 1, 0), (40.5, 390.5, 8.5, 0, -1, 0), (8.5, 250.5, 8.5, 0, -0.0, 3),
            (8.5, 100.5, 8.5, 1, 1, 0), (8.5, 100.5, 8.5, 0, -1, 1), (8.5, 100.5, 8.5, 1, 0, -1), (20.5, 250.5, 20.5, 1, 0, -1),    # zero components
            (8, 100, 8, 1, 1, 1), (16, 96, 16, -1, -1, -1), (16, 96, 16, 1, -2, 0.5), (32, 256, 16, -1, 0.25, -1), (16, 208, 16, 1, 1, 1),   # integer origins
            (8.5, 500.25, 8.5, 0.3, -1, 0.2), (8.5, -100.5, 24.5, 0.1, 1, 0.1), (20.5, 384.5, 20.5, 1, -0.001, 0.5),               # above / below the world
            (8.5, -3.5, 8.5, 1, -1, 0), (8.5, 400.5, 8.5, 0, 1, 0), (8.5, 400.5, 8.5, 1, 0, 0),                                    # ... and leaving at once
            (8.5, 250.5, 8.5, 0.001, 0, 0.002), (8.5, 250.5, 8.5, 1e-30, 1e-3, 0), (24.5, 250.5, 8.5, 0.17, 0, 0),                 # end by t_max / absent cell
            (8.5, 250.5, 8.5, -1, 0.1, 0.3), (47.5, 250.5, 31.5, 1, 0, 1), (24.5, 250.5, 8.5, 1, 0.01, 0.01),                      # leave the grid / absent
            (9.5, 101.5, 9.5, 0.3, 0.2, 0.1),                                                                                      # starts inside a block
            (8.5, 100.5, 8.5, 0, 0, 0), (-1, 100.5, 8.5, 1, 0, 0), (8.5, 1408, 8.5, 0, -1, 0), (np.nan, 100.5, 8.5, 1, 0, 0),        # invalid
            (8.5, 100.5, 8.5, 1e-42, 0, 1), (8.5, 100.5, 32, 0, 0, -1)]
    r[:len(hand)] = np.array(hand, np.float32)
    return r


@functools.lru_cache(None)
def expected(name, stop_mask, ft=np.float32):
    return dda(ft, pool(name), GRID, stop_mask, rays())


@functools.lru_cache(None)
def on_device(gen, name, stop_mask):
    blocks = gen.torch.from_numpy(pool(name)).to(gen.device)
    return blocks, gen.torch.from_numpy(GRID).to(gen.device), gen.ray_occupancy(blocks, stop_mask)


def assert_records_equal(got, ref):
    for f in ("status", "voxel", "face", "block"):
        bad = np.flatnonzero((got[f] != ref[f]).reshape(len(ref), -1).any(1))
        assert bad.size == 0, f"{f}: {bad.size} rays differ, first {bad[0]}: {got[bad[0]]} vs {ref[bad[0]]}"
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32)), "bits of t"


@pytest.mark.parametrize("flags", [0, 1], ids=["skip", "no_skip"])
@pytest.mark.parametrize("stop_mask", [15, 1, 3])
@pytest.mark.parametrize("name", ["0.02", "0.1", "ragged"])
def test_rays_equal_the_contract_walk(gen, name, stop_mask, flags):
    blocks, grid, occ = on_device(gen, name, stop_mask)
    got = gen.ray_hits(gen.raycast(blocks, grid, occ, gen.torch.from_numpy(rays()).to(gen.device), stop_mask, T_MAX, flags))
    ref = expected(name, stop_mask)
    assert set(ref["status"]) == {HIT, MISS, LEFT, ABSENT, INVALID}
    assert ref["status"][29] == HIT and ref["t"][29] == 0 and ref["face"][29] == 6      # the ray that starts inside a block
    assert_records_equal(got, ref)


@pytest.mark.parametrize("name", ["0.02", "0.1"])
def test_float64_walk_agrees_except_on_grazed_ties(gen, name):
    blocks, grid, occ = on_device(gen, name, 15)
    got = gen.ray_hits(gen.raycast(blocks, grid, occ, gen.torch.from_numpy(rays()).to(gen.device), 15, T_MAX))
    ref = expected(name, 15, np.float64)
    differ = (got["status"] != ref["status"]) | (got["voxel"] != ref["voxel"]).any(1) | (got["face"] != ref["face"])
    print("rays that differ from the float64 walk:", int(differ.sum()), "of", len(ref))
    assert differ.sum() <= len(ref) // 100


@pytest.mark.parametrize("stop_mask", [15, 1])
def test_occupancy_equals_a_numpy_reduction(gen, stop_mask):
    _, _, occ = on_device(gen, "ragged", stop_mask)
    occ = occ.cpu().numpy().view(np.uint64)                # [slot][1 + 24]
    stop = ((block_classes() & stop_mask) != 0)[pool("ragged")].reshape(5, 4, 4, 4, 4, 24, 4, 4)      # [slot][bz][z][bx][x][sy][by][y]
    brick = stop.any((2, 4, 7)).transpose(0, 3, 1, 2, 4)   # [slot][sy][bz][bx][by]: bit = by + 4 (bx + 4 bz)
    masks = (brick.reshape(5, 24, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(2, dtype=np.uint64)
    assert np.array_equal(occ[:, 1:], masks)
    assert np.array_equal(occ[:, 0], ((masks != 0).astype(np.uint64) << np.arange(24, dtype=np.uint64)).sum(1, dtype=np.uint64))


def camera_rays(eye, forward, up, fov_y, width, height):
    """the formula of include/mmgen.h: the basis in double (python floats), rounded once; the pixel arithmetic in float32"""
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    fw, up = [float(np.float32(c)) for c in forward], [float(np.float32(c)) for c in up]
    fl = math.sqrt(dot(fw, fw))
    f = [c / fl for c in fw]
    r = cross(f, up)
    rl = math.sqrt(dot(r, r))
    r = [c / rl for c in r]
    u = cross(r, f)
    th = math.tan(0.5 * float(np.float32(fov_y)))
    tha = th * (float(width) / float(height))
    F, R, U = np.float32(f), np.float32([c * tha for c in r]), np.float32([c * th for c in u])
    one, half, two = np.float32(1), np.float32(0.5), np.float32(2)
    sx = ((np.arange(width, dtype=np.float32) + half) * (two / np.float32(width)) - one)[None, :, None]
    sy = (one - (np.arange(height, dtype=np.float32) + half) * (two / np.float32(height)))[:, None, None]
    out = np.empty((height, width, 6), np.float32)
    out[..., :3] = np.float32(eye)
    out[..., 3:] = (F + sx * R) + sy * U
    return out.reshape(-1, 6)


@pytest.mark.parametrize("flags", [0, 1], ids=["skip", "no_skip"])
def test_camera_image_equals_raycast_on_the_formulas_rays(gen, flags):
    blocks, grid, occ = on_device(gen, "ragged", 15)
    cam = dict(eye=(10.3, 180.7, 20.2), forward=(0.6, -0.5, -0.2), up=(0.0, 1.0, 0.0), fov_y=1.1, width=64, height=48)
    img = gen.ray_hits(gen.render_view(blocks, grid, occ, stop_mask=15, t_max=T_MAX, flags=flags, **cam)).reshape(-1)
    r = camera_rays(**cam)
    got = gen.ray_hits(gen.raycast(blocks, grid, occ, gen.torch.from_numpy(r).to(gen.device), 15, T_MAX))
    assert HIT in set(got["status"]) and len(set(got["status"])) > 1
    assert_records_equal(img, got)
    assert_records_equal(img, dda(np.float32, pool("ragged"), GRID, 15, r))


def test_generated_terrain(gen):
    out = gen.generate_region(1488, -1110, 2, 2)
    blocks = out["blocks"]
    grid = gen.torch.arange(4, dtype=gen.torch.int32, device=gen.device).reshape(2, 2)
    rng = np.random.default_rng(0)
    r = np.empty((2048, 6), np.float32)
    r[:, 0], r[:, 1], r[:, 2] = rng.uniform(0, 32, 2048), 383.5, rng.uniform(0, 32, 2048)
    r[:1024, 3:] = (0, -1, 0)                              # half straight down, half oblique
    r[1024:, 3:] = rng.normal(size=(1024, 3)) * (1, 0.3, 1) - (0, 0.5, 0)
    got = gen.ray_hits(gen.raycast(blocks, grid, gen.ray_occupancy(blocks, 15), gen.torch.from_numpy(r).to(gen.device), 15, 4096.0))
    b = blocks.cpu().numpy()
    assert_records_equal(got, dda(np.float32, b, grid.cpu().numpy(), 15, r, 4096.0))
    x, z = np.floor(r[:1024, 0]).astype(int), np.floor(r[:1024, 2]).astype(int)
    column = b[(z >> 4) * 2 + (x >> 4)].reshape(-1, 16, 16, 384)[np.arange(1024), z & 15, x & 15]
    top = 383 - np.argmax(column[:, ::-1] != 0, 1)
    assert (column != 0).any(1).all() and np.array_equal(got["voxel"][:1024, 1], top) and (got["face"][:1024] == np.where(top == 383, 6, 4)).all()
