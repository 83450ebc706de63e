"""GPU tests of mmgen_lod_reduce (include/mmgen.h "level-of-detail chunks") against a plain numpy restatement of the contract, byte for byte."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AIR, WATER, POPPY, STONE, DIRT, GRASS, LEAVES, BEYOND = 0, 1, 16, 57, 58, 59, 87, 200      # GRASS is the block; POPPY X-shaped; BEYOND past the enum
SENTINEL, INVALID, BLOCKS = 0xA5, 1, 98304
LEVELS = (1, 2, 3)
CONTENT = np.ones(256, bool)                               # OPAQUE, SEMI or TRANSPARENT; ids beyond the enum are OPAQUE
CONTENT[:140] = np.load(os.path.join(GOLDEN, "block_data.npz"))["block_data"][:, 12] != 3
CONTENT[AIR] = False


def lod_reference(blocks, src, level):
    """blocks [slots][98304], src: the s * s slots of one LOD chunk (-1 = absent) -> its 98 304 bytes"""
    s, W, H, base = 1 << level, 16 << level, 384 >> level, (1 << level) * np.arange(384 >> level)
    vol = np.zeros((W, W, 384 + 2 * s), np.uint8)          # the footprint [z][x][y], AIR above the world
    for q, slot in enumerate(src):
        if slot >= 0:
            vol[16 * (q // s):16 * (q // s) + 16, 16 * (q % s):16 * (q % s) + 16, :384] = blocks[slot].reshape(16, 16, 384)
    cont = CONTENT[vol]
    slabs = cont[:, :, :384].reshape(W, W, H, s)
    N = slabs.reshape(16, s, 16, s, H, s).sum(axis=(1, 3, 5))                  # [Z][X][Y]
    has = slabs.any(axis=3)                                                    # the column has a sample in this slab
    y2 = base + s - 1 - np.argmax(slabs[..., ::-1], axis=3)                    # y1: the highest content voxel of the slab
    for _ in range(2 * s):                                                     # look ahead while the voxel above is content, up to s Y + 2 s - 1
        y2 = y2 + (np.take_along_axis(cont, y2 + 1, axis=2) & (y2 + 1 <= base + 2 * s - 1))
    sample = np.take_along_axis(vol, y2, axis=2).reshape(16, s, 16, s, H).transpose(0, 2, 4, 1, 3).reshape(16, 16, H, s * s)
    has = has.reshape(16, s, 16, s, H).transpose(0, 2, 4, 1, 3).reshape(16, 16, H, s * s)
    solid = 2 * N >= s ** 3
    cell = np.broadcast_to(np.arange(solid.sum())[:, None], (solid.sum(), s * s))
    votes = np.bincount((256 * cell + sample[solid])[has[solid]], minlength=256 * solid.sum()).reshape(-1, 256)
    out = np.zeros((16, 16, 384), np.uint8)
    out[:, :, :H][solid] = votes.argmax(axis=1)                                # the first maximum: ties go to the lowest id
    return out.reshape(-1)


def run(gen, blocks, src, level, **kw):
    t = gen.torch
    return gen.lod_reduce(t.from_numpy(blocks).to(gen.device), t.from_numpy(np.asarray(src, np.int32)).to(gen.device), level, **kw).cpu().numpy()


@pytest.mark.parametrize("level", LEVELS)                  # N straddles the threshold, ties are common; shared and absent sources, scattered destinations
def test_random_pool(gen, level):
    t, rng, n = gen.torch, np.random.default_rng(level), 1 << 2 * level
    blocks = np.where(rng.random((70, BLOCKS)) < 0.5, rng.choice([WATER, GRASS, DIRT, STONE, LEAVES, BEYOND], (70, BLOCKS)),
                      rng.choice([AIR, POPPY], (70, BLOCKS))).astype(np.uint8)
    src = np.stack([rng.permutation(70)[:n], rng.permutation(70)[:n]]).astype(np.int32)
    src[1, 0], src[1, 1] = src[0, 2], -1
    out = t.full((5, BLOCKS), SENTINEL, dtype=t.uint8, device=gen.device)
    got = run(gen, blocks, src, level, out=out, dst_idx=t.tensor([3, 1], dtype=t.int32, device=gen.device))
    assert np.all(got[[0, 2, 4]] == SENTINEL)
    for i, slot in enumerate((3, 1)):
        ref = lod_reference(blocks, src[i], level)
        assert ref.any() and not ref.reshape(256, 384)[:, 384 >> level:].any() and np.array_equal(got[slot], ref)


@pytest.mark.parametrize("where", ("word", "waterline", "top"))
@pytest.mark.parametrize("level", LEVELS)
def test_column_terrain(gen, level, where):
    """the surface and its look-ahead across a 16-byte word border, across the section border at the waterline, against the top of the world"""
    s, W, y, rng = 1 << level, 16 << level, np.arange(384), np.random.default_rng(7)
    h = ({"word": 15 - s, "waterline": 62, "top": 383 - 2 * s}[where] + rng.integers(0, 2 * s + 1, (W, W)))[:, :, None]
    vol = np.select([y <= h - 4, y < h, y == h, (y == h + 1) & (rng.random((W, W, 1)) < 0.3), y <= 62], [STONE, DIRT, GRASS, POPPY, WATER], AIR).astype(np.uint8)
    blocks = vol.reshape(s, 16, s, 16, 384).transpose(0, 2, 1, 3, 4).reshape(s * s, BLOCKS)      # slot qx + s qz
    ref = lod_reference(blocks, np.arange(s * s), level)
    assert len(np.unique(ref)) > 2 and np.array_equal(run(gen, blocks, [np.arange(s * s)], level)[0], ref)


# region [s z][s x][3 s y] of a cell's cube and the two above it, as f(region, s); the id expected, and the one where the world ends above the cube
CELLS = (
    (lambda r, s: r.__setitem__((slice(None), slice(None), slice(0, s // 2)), STONE), STONE, STONE),                  # N = s^3 / 2: solid
    (lambda r, s: (r.__setitem__((slice(None), slice(None), slice(0, s // 2)), STONE), r.__setitem__((0, 0, 0), AIR)), AIR, AIR),      # one less
    (lambda r, s: r.__setitem__((slice(None), slice(None), slice(0, s)), POPPY), AIR, AIR),
    (lambda r, s: (r.__setitem__((slice(None), slice(None), slice(0, s)), DIRT), r.__setitem__((slice(0, s // 2), slice(None), slice(0, s)), STONE)), STONE, STONE),
    (lambda r, s: r.__setitem__((slice(None), slice(None), slice(0, s)), BEYOND), BEYOND, BEYOND),
    (lambda r, s: (r.__setitem__((slice(None), slice(None), slice(0, s)), DIRT), r.__setitem__((slice(None), slice(None), s), GRASS)), GRASS, DIRT),
    (lambda r, s: (r.__setitem__((slice(None), slice(None), slice(0, 2 * s + 1)), DIRT), r.__setitem__((slice(None), slice(None), 2 * s + 1), GRASS)), DIRT, DIRT),
    (lambda r, s: (r.__setitem__((slice(None), slice(None), slice(0, s)), DIRT), r.__setitem__((slice(None), slice(None), s + 1), GRASS)), DIRT, DIRT),
)


@pytest.mark.parametrize("level", LEVELS)
def test_hand_worked_cells(gen, level):
    """every cube at cell (0, 0, 0), at the last cell under the top of the world, and at the first cell of source chunk (s - 1, s - 1)"""
    s, H, g = 1 << level, 384 >> level, 16 >> level
    blocks = np.zeros((2 * len(CELLS), 16, 16, 384), np.uint8)                 # per cube the source chunks (0, 0) and (s - 1, s - 1), [z][x][y]
    src = np.full((len(CELLS), s * s), -1, np.int32)
    for i, (fill, _, _) in enumerate(CELLS):
        region = np.zeros((s, s, 3 * s), np.uint8)
        fill(region, s)
        blocks[2 * i, :s, :s, :3 * s] = region
        blocks[2 * i + 1, 16 - s:, 16 - s:, 384 - s:] = region[:, :, :s]
        blocks[2 * i + 1, :s, :s, 5 * s:8 * s] = region
        src[i, 0], src[i, s * s - 1] = 2 * i, 2 * i + 1
    got = run(gen, blocks.reshape(-1, BLOCKS), src, level).reshape(-1, 16, 16, 384)
    for i, (_, want, want_top) in enumerate(CELLS):
        assert (got[i, 0, 0, 0], got[i, 15, 15, H - 1], got[i, 16 - g, 16 - g, 5]) == (want, want_top, want), i


@pytest.fixture(scope="module")
def region(gen):
    return gen.generate_region(1488, -1110, 8, 8)["blocks"].cpu().numpy()      # slot cx + 8 cz


@pytest.mark.parametrize("level", LEVELS)
def test_generated_terrain(gen, region, level):
    s, k = 1 << level, 8 >> level
    src = np.array([[(s * lz + q // s) * 8 + s * lx + q % s for q in range(s * s)] for lz in range(k) for lx in range(k)], np.int32)
    got = run(gen, region, src, level)
    assert len(np.unique(got)) > 4 and all(np.array_equal(got[i], lod_reference(region, src[i], level)) for i in range(k * k))


def test_arguments(gen):
    t, P = gen.torch, gen._p
    b, out = t.zeros((4, BLOCKS), dtype=t.uint8, device=gen.device), t.full((1, BLOCKS), SENTINEL, dtype=t.uint8, device=gen.device)
    src = t.arange(4, dtype=t.int32, device=gen.device)
    gen.lib.mmgen_lod_reduce.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3
    assert gen.lib.mmgen_lod_reduce(P(b), P(src), 0, 1, P(out), None, None) == 0 and bool((out == SENTINEL).all())
    for args in ((P(b), P(src), 1, 0, P(out)), (P(b), P(src), 1, 4, P(out)), (P(b), P(src), -1, 1, P(out)), (None, P(src), 1, 1, P(out)),
                 (P(b), None, 1, 1, P(out)), (P(b), P(src), 1, 1, None)):
        assert gen.lib.mmgen_lod_reduce(*args, None, None) == INVALID, args
    assert bool((out == SENTINEL).all())
