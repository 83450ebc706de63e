"""GPU tests of the voxel lighting (include/mmgen.h "voxel lighting"): mmgen_light_masks + mmgen_light against a plain numpy restatement of
the contract - both fields set to their sources, then fifteen max-of-neighbours-minus-one steps - byte for byte."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GRID = np.array([[3, 0, -1], [1, 4, 2]], np.int32)         # 3 x 2 cells, one absent, slots permuted; slot 5 is named by no cell
SLOTS, SENTINEL = 6, 0xA5
AIR, WATER, POPPY, STONE, LEAVES, GLOW = 0, 1, 16, 57, 87, 121      # GLOW: GLOWSTONE, opaque, 15 in the default table
AIR_C, OPAQUE_C, XSHAPED_C = 0, 1, 4


def block_classes():
    """AIR 0, then 1 + transparency of the reference's block table (golden): OPAQUE 1, SEMI 2, TRANSPARENT 3, X_SHAPED 4; ids beyond the enum OPAQUE"""
    cls = np.full(256, OPAQUE_C, np.int8)
    cls[:140] = 1 + np.load(os.path.join(GOLDEN, "block_data.npz"))["block_data"][:, 12]
    cls[AIR] = AIR_C
    return cls


def reference(world, present, e):
    """world [16 gh][16 gw][384] block ids (z, x, y), present: the same shape, False in absent cells.  Returns (sky << 4) | block."""
    cls = block_classes()[world]
    T = (cls != OPAQUE_C) & present
    airx = ((cls == AIR_C) | (cls == XSHAPED_C)) & present
    is_open = np.logical_and.accumulate(airx[:, :, ::-1], 2)[:, :, ::-1]
    fields = []
    for f in (np.where(is_open, 15, 0).astype(np.int8), np.where(present, e[world], 0).astype(np.int8)):
        for _ in range(15):
            p = np.pad(f, 1)
            nb = np.maximum.reduce([p[2:, 1:-1, 1:-1], p[:-2, 1:-1, 1:-1], p[1:-1, 2:, 1:-1], p[1:-1, :-2, 1:-1], p[1:-1, 1:-1, 2:], p[1:-1, 1:-1, :-2]])
            f = np.maximum(f, T * np.maximum(nb - 1, 0))
        fields.append(f.astype(np.uint8))
    return (fields[0] << 4) | fields[1]


def to_slots(volume, grid, fill):
    """[16 gh][16 gw][384] -> [slots][98304] by the grid; slots no cell names hold `fill`"""
    out = np.full((SLOTS, 98304), fill, np.uint8)
    for (cz, cx), s in np.ndenumerate(grid):
        if s >= 0:
            out[s] = volume[16 * cz:16 * cz + 16, 16 * cx:16 * cx + 16].reshape(-1)
    return out


def level_table():
    """the default table, and ids 201..215 (beyond the enum: OPAQUE) emitting 1..15"""
    e = np.zeros(256, np.uint8)
    e[[2, 121, 122, 139]], e[[4, 6]], e[[92, 93, 94]], e[[33, 34, 35, 38, 39, 40]] = 15, 14, 10, 6
    e[201:216] = np.arange(1, 16)
    return e


def emitters():
    w = np.zeros((32, 48, 384), np.uint8)                  # [z][x][y]: a cavern of air under a roof, open air above it
    w[:, :, 200:300] = STONE
    w[16, 16, 100] = GLOW                                  # corner column of cell (1, 1): the diamond crosses into three neighbours
    w[20, 29, 50] = GLOW                                   # 14 from the border column x = 15 of cell (0, 1): contributes 1 there
    w[26, 30, 150] = GLOW                                  # 15 from it: contributes nothing
    for i, y in enumerate((0, 63, 64, 127, 128, 383)):     # word and slab boundaries
        w[4, 3 + 7 * i, y] = GLOW
    w[28, 4, 20] = 201                                     # level 1: lights only itself
    w[8, 20, 30], w[8, 23, 30] = 215, 209                  # overlapping, different levels
    w[16, 40, 60] = GLOW                                   # on the border to the absent cell (2, 0)
    w[10, 8, 190:200] = LEAVES                             # something that transmits but is not air, under the roof
    return w, level_table()


def corridor():
    w = np.full((32, 48, 384), STONE, np.uint8)
    w[20, 14, 100] = GLOW                                  # in cell (0, 1); the corridor leaves it at x = 16 and comes back along z = 23
    w[20, 15:19, 100] = AIR
    w[20:24, 18, 100] = AIR
    w[23, 12:19, 100] = AIR
    w[24, 40, 50] = GLOW                                   # buried, one open face
    w[24, 41:44, 50] = AIR
    return w, level_table()


def sky():
    w = np.zeros((32, 48, 384), np.uint8)
    w[:, :, :100] = STONE
    w[:, :40, 150] = STONE                                 # a flat roof over x < 40 ...
    w[24, 24, 150] = AIR                                   # ... with a hole: 15 below it, 14, 13, .. sideways under the roof
    w[18:23, 42:46, 100:105] = WATER                       # above ground, under the open sky: not open, but transmits
    w[26:31, 41:47, 110] = LEAVES
    w[24, 43, 120] = POPPY                                 # X-shaped: does not close its column
    w[:16, :16] = AIR                                      # cell (0, 0) all air, cell (1, 0) all stone (next to the absent cell)
    w[:16, 16:32] = STONE
    return w, level_table()


def noise(density):
    rng = np.random.default_rng(int(density * 100))
    w = np.where(rng.random((32, 48, 384)) < density, rng.integers(1, 256, (32, 48, 384)), 0).astype(np.uint8)
    e = rng.integers(0, 16, 256).astype(np.uint8) * (rng.random(256) < 0.3)
    e[1:16] = np.arange(1, 16)                             # every level occurs
    return w, e.astype(np.uint8)


WORLDS = {"emitters": emitters, "corridor": corridor, "sky": sky, "noise0.3": lambda: noise(0.3), "noise0.02": lambda: noise(0.02)}


@functools.lru_cache(None)
def case(name):
    """(blocks [slots][98304], emission, expected light [slots][98304] with the sentinel where nothing may be written)"""
    world, e = WORLDS[name]()
    present = np.repeat(np.repeat(GRID >= 0, 16, 0), 16, 1)[:, :, None] & np.ones(384, bool)
    ref = reference(world, present, e)
    if name == "emitters":                                 # the reference itself, where a case has a value one can name by hand
        blk = ref & 15
        assert blk[20, 15, 50] == 1 and blk[26, 15, 150] == 0 and blk[28, 4, 20] == 1 and blk[28, 5, 20] == 0 and blk[8, 21, 30] == 14 and blk[8, 22, 30] == 13
    if name == "corridor":
        assert ref[23, 12, 100] & 15 == 2 and ref[24, 43, 50] & 15 == 12
    if name == "sky":
        assert ref[24, 24, 120] >> 4 == 15 and ref[24, 20, 120] >> 4 == 11 and ref[20, 43, 104] >> 4 == 14 and ref[24, 43, 110] >> 4 == 15
        assert (ref[:16, :16] == 0xF0).all() and (ref[:16, 16:32] == 0).all()
    return to_slots(world, GRID, 77), e, to_slots(ref, GRID, SENTINEL)


def lit(gen, blocks, e, grid, cells=None, chunk_idx=None, masks=None, light=None):
    t, dev = gen.torch, gen.device
    masks = gen.light_masks(t.from_numpy(blocks).to(dev), None if chunk_idx is None else t.tensor(chunk_idx, dtype=t.int32, device=dev),
                            None if e is None else t.from_numpy(e).to(dev), out=masks)
    if light is None:
        light = t.full((blocks.shape[0], 98304), SENTINEL, dtype=t.uint8, device=dev)
    gen.light(masks, t.from_numpy(grid).to(dev), None if cells is None else t.tensor(cells, dtype=t.int32, device=dev), out=light)
    return masks, light


def assert_light_equal(got, ref):
    bad = np.argwhere(got != ref)
    if len(bad):
        s, i = bad[0]
        raise AssertionError(f"{len(bad)} bytes differ, first in slot {s} at y {i % 384}, x {i // 384 % 16}, z {i // 6144}: {got[s, i]:#04x} vs {ref[s, i]:#04x}")


@pytest.mark.parametrize("name", list(WORLDS))
def test_light_equals_the_contract(gen, name):
    blocks, e, ref = case(name)
    _, light = lit(gen, blocks, e, GRID)
    assert_light_equal(light.cpu().numpy(), ref)


def test_subsets_add_up_to_the_whole(gen):
    blocks, e, ref = case("noise0.02")
    masks, _ = lit(gen, blocks, e, GRID, cells=[], chunk_idx=[3, 0, 4])      # the masks in two parts, nothing lit yet
    masks, light = lit(gen, blocks, e, GRID, cells=[4, 0], chunk_idx=[1, 2], masks=masks)      # grid cells (1, 1) and (0, 0): slots 4 and 3
    got = light.cpu().numpy()
    assert np.array_equal(got[[4, 3]], ref[[4, 3]]) and (got[[0, 1, 2, 5]] == SENTINEL).all()
    lit(gen, blocks, e, GRID, cells=[1, 3, 5, 2], chunk_idx=[], masks=masks, light=light)      # the rest, the absent cell among them
    assert_light_equal(light.cpu().numpy(), ref)


def test_generated_world(gen):
    e = gen.light_default_emission()
    assert np.array_equal(e, level_table() * (np.arange(256) < 140))
    blocks = gen.generate_region(1488, -1110, 3, 3)["blocks"]
    grid = np.arange(9, dtype=np.int32).reshape(3, 3)
    light = gen.light(gen.light_masks(blocks), gen.torch.from_numpy(grid).to(gen.device)).cpu().numpy()
    world = blocks.cpu().numpy().reshape(3, 3, 16, 16, 384).transpose(0, 2, 1, 3, 4).reshape(48, 48, 384)
    ref = reference(world, np.ones(world.shape, bool), e)
    assert (ref & 15).max() > 0 and (ref >> 4).min() == 0 and (ref >> 4).max() == 15
    assert_light_equal(light, ref.reshape(3, 16, 3, 16, 384).transpose(0, 2, 1, 3, 4).reshape(9, 98304))


def test_invalid_arguments_and_empty_calls(gen):
    t = gen.torch
    blocks, e, ref = case("sky")
    masks, light = lit(gen, blocks, e, GRID)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    gen.lib.mmgen_light_masks.argtypes = [vp, vp, i32, vp, vp, vp]
    gen.lib.mmgen_light.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
    grid, b = t.from_numpy(GRID).to(gen.device), t.from_numpy(blocks).to(gen.device)
    P, INVALID = gen._p, 1                                 # hipErrorInvalidValue
    assert gen.lib.mmgen_light_masks(P(b), None, 0, None, P(masks), None) == 0
    assert gen.lib.mmgen_light(P(masks), P(grid), 3, 2, None, 0, P(light), None) == 0
    assert gen.lib.mmgen_light_default_emission(None) == INVALID
    for args in ((None, None, 1, None, P(masks)), (P(b), None, 1, None, None), (P(b), None, -1, None, P(masks))):
        assert gen.lib.mmgen_light_masks(*args, None) == INVALID
    for args in ((None, P(grid), 3, 2, None, 6, P(light)), (P(masks), None, 3, 2, None, 6, P(light)), (P(masks), P(grid), 3, 2, None, 6, None),
                 (P(masks), P(grid), 0, 2, None, 1, P(light)), (P(masks), P(grid), 3, 16385, None, 1, P(light)), (P(masks), P(grid), 3, 2, None, 7, P(light)),
                 (P(masks), P(grid), 3, 2, None, -1, P(light))):
        assert gen.lib.mmgen_light(*args, None) == INVALID
    cells = t.tensor([6, -1, 1 << 30], dtype=t.int32, device=gen.device)      # cells outside the grid: nothing is written for them
    gen.light(masks, grid, cells, out=light)
    assert_light_equal(light.cpu().numpy(), ref)
