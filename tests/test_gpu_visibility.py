"""GPU tests of the section visibility (include/mmgen.h "section visibility"): mmgen_section_connectivity against a numpy flood by
6-neighbour dilation inside each 16^3 box, mmgen_visible_sections against the contract's entry sets built level by level in plain Python."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AIR, WATER, POPPY, STONE, LEAVES, BEYOND = 0, 1, 16, 57, 87, 200      # POPPY is X-shaped, BEYOND an id past the enum: OPAQUE
SENTINEL, INVALID = 0xA5, 1                                # INVALID: hipErrorInvalidValue
DIRS = ((0, 0, 1), (1, 0, 0), (0, 0, -1), (-1, 0, 0), (0, 1, 0), (0, -1, 0))   # (x, y, z) of +z, +x, -z, -x, +y, -y
GRID = np.array([[3, 0, 7, 12, 5], [1, 4, 2, 9, 18], [10, 6, 13, -1, 8], [11, 14, 15, 16, 17]], np.int32)      # [cz][cx], cell (3, 2) absent, 19 slots
EYE = (2, 11, 2)                                           # the scenarios are built around this eye: the absent cell is its +x neighbour
EYES = ((0, 0, 0), (4, 23, 3), (2, -1, 2), (1, 24, 1), EYE)                   # grid corners, the middle; the eye_sy -1, 0, 23 and 24


def pair_bit(a, b):
    a, b = min(a, b), max(a, b)
    return a * (11 - a) // 2 + b - a - 1


def see_through(ids):
    opaque = np.ones(256, bool)
    opaque[:140] = np.load(os.path.join(GOLDEN, "block_data.npz"))["block_data"][:, 12] == 0
    opaque[AIR] = False
    return ~opaque[ids]


def conn_reference(chunks):
    """block ids [n][98304] -> u16 [n][24]: per section, flood from a face layer by dilation inside the box, then look at the other layers"""
    sections = see_through(chunks.reshape(-1, 16, 16, 24, 16)).transpose(0, 3, 1, 2, 4).reshape(-1, 16, 16, 16)      # [n 24][z][x][y]
    result = np.where(sections.all(axis=(1, 2, 3)), 0x7fff, 0).astype(np.uint16)
    mixed = sections.any(axis=(1, 2, 3)) & ~sections.all(axis=(1, 2, 3))       # only these need the flood
    T = sections[mixed]
    def layer(d):
        m = np.zeros(T.shape, bool)
        m[tuple((15, 15, 0, 0, 15, 0)[d] if i == (1, 2, 1, 2, 3, 3)[d] else slice(None) for i in range(4))] = True
        return m
    out = np.zeros(T.shape[0], np.uint16)
    for a in range(5):
        reach, grown = None, T & layer(a)
        while not np.array_equal(grown, reach):
            reach = grown
            p = np.pad(reach, ((0, 0), (1, 1), (1, 1), (1, 1)))
            grown = T & (reach | p[:, 2:, 1:-1, 1:-1] | p[:, :-2, 1:-1, 1:-1] | p[:, 1:-1, 2:, 1:-1] | p[:, 1:-1, :-2, 1:-1] | p[:, 1:-1, 1:-1, 2:] | p[:, 1:-1, 1:-1, :-2])
        for b in range(a + 1, 6):
            out |= (reach & layer(b)).any(axis=(1, 2, 3)).astype(np.uint16) << pair_bit(a, b)
    result[mixed] = out
    return result.reshape(-1, 24)


def stone(*holes, dig=AIR):
    p = np.full((16, 16, 16), STONE, np.uint8)             # [z][x][y]
    for h in holes:
        p[h] = dig
    return p


A, S = slice(None), slice
# rows along x at even z joined at alternating ends, only the first voxel at x = 0 and only the last at x = 15: more than 100 rounds; then
# vertical legs at even x, one-voxel links at odd x alternating between y = 14 and y = 1
SERPENTINE_XZ = [(2 * i, S(0 if i == 0 else 1, 16 if i == 7 else 15), 7) for i in range(8)] + [(2 * i + 1, 14 if i % 2 == 0 else 1, 7) for i in range(7)]
SERPENTINE_XY = [(7, x, S(1, 15)) if x % 2 == 0 else (7, x, 14 if (x // 2) % 2 == 0 else 1) for x in range(16)]
PATTERNS = {                                               # name: (16^3 block ids, the pairs worked out by hand)
    "air": (np.zeros((16, 16, 16), np.uint8), [(a, b) for a in range(6) for b in range(a + 1, 6)]), "stone": (stone(), []),
    "corner": (stone((0, 0, 0)), [(2, 3), (2, 5), (3, 5)]), "edge": (stone((0, 0, 7)), [(2, 3)]),
    "face_centre": (stone((0, 7, 7)), []), "interior": (stone((7, 7, 7)), []),
    "tunnel_x": (stone((7, A, 7)), [(1, 3)]), "tunnel_z": (stone((A, 7, 7)), [(0, 2)]), "tunnel_y": (stone((7, 7, A)), [(4, 5)]),
    # two shafts from the +y (-y) face, each bent to a side face of its own: joined only through the AIR section above (below)
    "shafts_up": (stone((3, 3, S(5, 16)), (3, S(0, 4), 5), (12, 12, S(8, 16)), (12, S(12, 16), 8)), [(3, 4), (1, 4)]),
    "shafts_down": (stone((3, 3, S(0, 11)), (3, S(0, 4), 10), (12, 12, S(0, 8)), (12, S(12, 16), 7)), [(3, 5), (1, 5)]),
    # two bent tunnels whose corner voxels (7, 7, 7) and (8, 8, 7) share an edge only
    "diagonal": (stone((7, S(0, 8), 7), (S(0, 8), 7, 7), (8, S(8, 16), 7), (S(8, 16), 8, 7)), [(2, 3), (0, 1)]),
    "serpentine_xz": (stone(*SERPENTINE_XZ), [(1, 2), (1, 3), (2, 3)]), "serpentine_xy": (stone(*SERPENTINE_XY), [(1, 3)]),
    "water": (stone((7, A, 7), dig=WATER), [(1, 3)]), "leaves": (stone((7, A, 7), dig=LEAVES), [(1, 3)]),
    "poppy": (stone((7, A, 7), dig=POPPY), [(1, 3)]), "beyond": (stone((7, A, 7), dig=BEYOND), []),
}
PLACES = (0, 11, 23)                                       # the bottom, an sy with sy % 4 == 3 (the top of a 64-voxel word), the top
DENSITIES = (0.25, 0.35, 0.6)                              # either side of where 3-D site percolation sets in (0.31)


@pytest.fixture(scope="module")
def conn_case(gen):
    """every pattern at every place in a chunk of AIR, then the random chunks: block ids [slots][98304], reference and result u16 [slots][24]"""
    chunks = np.zeros((len(PATTERNS) * len(PLACES) + len(DENSITIES), 16, 16, 384), np.uint8)
    for i, (p, _) in enumerate(PATTERNS.values()):
        for j, sy in enumerate(PLACES):
            chunks[len(PLACES) * i + j, :, :, 16 * sy:16 * sy + 16] = p
    for k, density in enumerate(DENSITIES):
        rng = np.random.default_rng(int(100 * density))
        chunks[len(PATTERNS) * len(PLACES) + k] = np.where(rng.random((16, 16, 384)) < density, rng.choice([AIR, WATER, LEAVES, POPPY], (16, 16, 384)),
                                                           rng.choice([STONE, BEYOND], (16, 16, 384)))
    chunks = chunks.reshape(len(chunks), 98304)
    return chunks, conn_reference(chunks), gen.section_connectivity(gen.torch.from_numpy(chunks).to(gen.device)).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("place", range(len(PLACES)))
@pytest.mark.parametrize("name", list(PATTERNS) + ["random"])
def test_connectivity(conn_case, name, place):
    slot = len(PLACES) * (list(PATTERNS) + ["random"]).index(name) + place      # the random chunks follow the patterns, one per "place"
    ref, got = conn_case[1][slot], conn_case[2][slot]
    if name != "random":                                   # the reference itself, against the pairs worked out by hand
        assert ref[PLACES[place]] == sum(1 << pair_bit(a, b) for a, b in PATTERNS[name][1]) and np.all(np.delete(ref, PLACES[place]) == 0x7fff)
    assert got.tolist() == ref.tolist()


def test_chunk_idx_and_invalid_arguments(gen, conn_case):
    t, P, (chunks, ref, _) = gen.torch, gen._p, conn_case
    pick = [5 * i % 9 for i in range(9) if 5 * i % 9 != 4]                     # slots 0..8 permuted, slot 4 left out
    b = t.from_numpy(chunks[:9]).to(gen.device)
    out = t.full((9, 48), SENTINEL, dtype=t.uint8, device=gen.device)
    got = gen.section_connectivity(b, chunk_idx=t.tensor(pick, dtype=t.int32, device=gen.device), out=out).cpu().numpy()
    assert np.all(got[4] == SENTINEL) and np.array_equal(np.delete(got, 4, 0).view(np.uint16), np.delete(ref[:9], 4, 0))
    assert gen.lib.mmgen_section_connectivity(P(b), None, 0, P(out), None) == 0
    for args in ((None, None, 1, P(out)), (P(b), None, 1, None), (P(b), None, -1, P(out))):
        assert gen.lib.mmgen_section_connectivity(*args, None) == INVALID
    c, g, v = P(out), P(t.from_numpy(GRID).to(gen.device)), P(t.zeros((65, 65), dtype=t.int32, device=gen.device))      # (9 slots of records: never read)
    gen.lib.mmgen_visible_sections.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2
    for args in ((None, g, 5, 4, 2, 11, 2, 1, v), (c, None, 5, 4, 2, 11, 2, 1, v), (c, g, 5, 4, 2, 11, 2, 1, None), (c, g, 0, 4, 0, 11, 2, 1, v),
                 (c, g, 5, 16385, 2, 11, 2, 1, v), (c, g, 5, 4, 5, 11, 2, 1, v), (c, g, 5, 4, 2, 11, -1, 1, v), (c, g, 5, 4, 2, -2, 2, 1, v),
                 (c, g, 5, 4, 2, 25, 2, 1, v), (c, g, 5, 4, 2, 11, 2, -1, v), (c, g, 5, 4, 2, 11, 2, 33, v)):
        assert gen.lib.mmgen_visible_sections(*args, None) == INVALID, args


def visible_reference(rec, grid, eye, radius):
    exists = lambda s: max(abs(s[0] - eye[0]), abs(s[2] - eye[2])) <= radius and 0 <= s[0] < grid.shape[1] and 0 <= s[2] < grid.shape[0] and -1 <= s[1] <= 24
    record = lambda s: 0x7fff if grid[s[2], s[0]] < 0 or s[1] in (-1, 24) else int(rec[grid[s[2], s[0]], s[1]])
    E, level = {eye: set()}, {eye: set()}
    while level:
        nxt = {}
        for s in level:
            for d, v in enumerate(DIRS):
                n, axis = (s[0] + v[0], s[1] + v[1], s[2] + v[2]), [i for i in range(3) if v[i]][0]
                if exists(n) and (n[axis] - eye[axis]) * v[axis] > 0 and (s == eye or any((record(s) >> pair_bit(f, d)) & 1 for f in E[s] if f != d)):
                    nxt.setdefault(n, set()).add(d ^ 2 if d < 4 else 9 - d)
        E.update(nxt)                                      # every step adds one to the distance: the levels are disjoint
        level = nxt
    out = np.zeros((2 * radius + 1, 2 * radius + 1), np.uint32)
    for s, e in E.items():
        if 0 <= s[1] <= 23 and grid[s[2], s[0]] >= 0 and (e or s == eye):
            out[s[2] - eye[2] + radius, s[0] - eye[0] + radius] |= np.uint32(1 << s[1])
    return out


# name: (fill, records put on top of it as ((cx, sy, cz), pairs), what it is about at EYE and radius 4 as (cx, sy, cz) -> reported).  wall: the cells at
# cx = 1 are rock but for one section that connects -x and +x; two_entries: (1, 12, 2) is entered through +x and -y, only -y leads on to -x;
# back_step: out to cx = 0, up, and back through +x, towards the eye
SCENARIOS = {
    "open": (0x7fff, [], {}), "closed": (0, [], {(0, 11, 2): False, (1, 11, 2): True, (2, 11, 2): True}),
    "wall": (0x7fff, [((1, sy, cz), [(1, 3)] if (sy, cz) == (11, 2) else []) for sy in range(24) for cz in range(4)], {(0, 11, 2): True, (1, 12, 2): True}),
    "two_entries": (0, [((2, 12, 2), [(3, 5)]), ((1, 11, 2), [(1, 4)]), ((1, 12, 2), [(3, 5)])], {(0, 12, 2): True, (0, 11, 2): False}),
    "back_step": (0, [((1, 11, 2), [(1, 3)]), ((0, 11, 2), [(1, 4)]), ((0, 12, 2), [(1, 5)])], {(0, 12, 2): True, (1, 12, 2): False}),
    "absent": (0, [], {(4, 11, 2): True, (4, 11, 1): False}),      # seen through the absent cell (3, 2)
    "random1": (0, [], {}), "random2": (0, [], {}), "random3": (0, [], {}), "random4": (0, [], {})}


@pytest.mark.parametrize("radius", (0, 1, 4, 32))                        # 4 and 32 reach beyond the grid; 32 has several columns per lane
@pytest.mark.parametrize("eye", EYES)
@pytest.mark.parametrize("name", SCENARIOS)
def test_visible_sections(gen, name, eye, radius):
    t = gen.torch
    rec = np.full((19, 24), SCENARIOS[name][0], np.uint16)
    if name.startswith("random"):                          # every other set is sparse
        rng = np.random.default_rng(int(name[6]))
        rec = (rng.integers(0, 0x8000, rec.shape) & rng.integers(0 if name[6] in "13" else 0x7fff, 0x8000, rec.shape)).astype(np.uint16)
    for (cx, sy, cz), pairs in SCENARIOS[name][1]:         # u16 [slots][24], stored through GRID
        rec[GRID[cz, cx], sy] = sum(1 << pair_bit(a, b) for a, b in pairs)
    ref = visible_reference(rec, GRID, eye, radius)
    if eye == EYE and radius == 4:
        for (cx, sy, cz), want in SCENARIOS[name][2].items():
            assert bool((ref[cz - eye[2] + 4, cx - eye[0] + 4] >> sy) & 1) == want, (cx, sy, cz)
        assert ref[4, 5] == 0                              # the absent cell is never reported
    got = gen.visible_sections(t.from_numpy(rec.view(np.uint8)).to(gen.device), t.from_numpy(GRID).to(gen.device), eye, radius).cpu().numpy()
    assert np.array_equal(got, ref), f"\n{got}\n{ref}"


def test_generated_region(gen):
    t = gen.torch
    blocks = gen.generate_region(1488, -1110, 3, 3)["blocks"]
    grid = np.arange(9, dtype=np.int32).reshape(3, 3)
    conn = gen.section_connectivity(blocks)
    ref = conn_reference(blocks.cpu().numpy())
    assert len(set(ref.reshape(-1).tolist())) > 3 and np.array_equal(conn.cpu().numpy().view(np.uint16), ref)
    # an eye two voxels above the ground of the middle column, looking down and across
    column = see_through(blocks[4].cpu().numpy().reshape(16, 16, 384)[8, 8])
    y = 2 + int(np.max(np.nonzero(~column)[0]))
    assert y < 384 and column[y]
    g = t.from_numpy(grid).to(gen.device)
    vis = gen.visible_sections(conn, g, (1, y >> 4, 1), 2).cpu().numpy()
    assert np.array_equal(vis, visible_reference(ref, grid, (1, y >> 4, 1), 2))
    hits = gen.ray_hits(gen.render_view(blocks, g, gen.ray_occupancy(blocks, stop_mask=1), (24.5, y + 0.5, 24.5), (0.8, -0.35, 0.6), width=64, height=36, stop_mask=1))
    v = hits["voxel"][hits["status"] == gen.RAY_HIT]
    seen = (vis[(v[:, 2] >> 4) - 1 + 2, (v[:, 0] >> 4) - 1 + 2] >> (v[:, 1] >> 4)) & 1
    assert len(v) > 1000 and seen.all(), v[seen == 0][:5]
