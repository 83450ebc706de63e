"""GPU tests of the section quad mesh with ambient occlusion (include/mmgen.h "section quad mesh with ambient occlusion"):
mmgen_mesh_ao_section_quads_count / _fill against the per-section contract of tests/test_gpu_lit_section_quads.py with the greedy key
id | FL << 8 | AO << 16, AO computed in numpy from an opaque array padded to 18 x 18 x 386: section counts, records, light bytes and AO bytes,
one for one, in order.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from test_gpu_quads import CLS, DIRS, OPAQUE, case, face_set, greedy
from test_gpu_section_quads import pack
from test_gpu_lit_section_quads import light_field

pytestmark = pytest.mark.gpu

ROCK = 57
# where a neighbour's columns show in the padded [z + 1][x + 1] array and which of its own [z][x] they are: N E S W, then (+x,+z) (+x,-z) (-x,-z) (-x,+z)
HALO = [(np.s_[17, 1:17], np.s_[0]), (np.s_[1:17, 17], np.s_[:, 0]), (np.s_[0, 1:17], np.s_[15]), (np.s_[1:17, 0], np.s_[:, 15]),
        (np.s_[17, 17], np.s_[0, 0]), (np.s_[0, 17], np.s_[15, 0]), (np.s_[0, 0], np.s_[15, 15]), (np.s_[17, 0], np.s_[0, 15])]


def face_ao(pool, c, nb8):
    """AO int32 [6][z][x][y] of every face position of chunk c"""
    O = np.zeros((18, 18, 386), np.int32)
    O[1:17, 1:17, 1:385] = CLS[pool[c]] == OPAQUE
    for n, (dst, src) in zip(nb8, HALO):
        if n >= 0:
            O[dst + (np.s_[1:385],)] = CLS[pool[n][src]] == OPAQUE
    at = lambda o: O[1 + o[0]:17 + o[0], 1 + o[1]:17 + o[1], 1 + o[2]:385 + o[2]]
    ao = np.zeros((6, 16, 16, 384), np.int32)
    for d, n in enumerate(np.array(DIRS)):
        er, eq = np.array((0, 1, 0) if d in (0, 2) else (1, 0, 0)), np.array((0, 0, 1) if d < 4 else (0, 1, 0))      # steps in [z][x][y]
        for k, (sr, sq) in enumerate(((-1, -1), (-1, 1), (1, -1), (1, 1))):
            s1, s2, cc = at(n + sr * er), at(n + sq * eq), at(n + sr * er + sq * eq)
            ao[d] |= np.where(s1 & s2, 0, 3 - (s1 + s2 + cc)) << (2 * k)
    return ao


def contract(pool, lp, c, nb8, mask=0xff):
    """rows (sy, record, light byte, AO byte) of chunk c, in stream order"""
    nb = list(nb8[:4])
    F, X = face_set(pool, c, nb)
    pad = np.zeros((18, 18, 386), np.uint8)                 # y = -1 stays 0x00
    pad[1:17, 1:17, 1:385], pad[1:17, 1:17, 385] = lp[c], 0xF0
    for d in range(4):
        if nb[d] >= 0:
            pad[HALO[d][0] + (np.s_[1:385],)] = lp[nb[d]][HALO[d][1]]
    ids, ao = pool[c].astype(np.int32), face_ao(pool, c, nb8)
    key = [ids | (pad[1 + dz:17 + dz, 1 + dx:17 + dx, 1 + dy:385 + dy] & mask).astype(np.int32) << 8 | ao[d] << 16 for d, (dz, dx, dy) in enumerate(DIRS)]
    own, rec = ids | (lp[c] & mask).astype(np.int32) << 8 | 0xFF << 16, []
    for sy in range(24):
        ys = slice(16 * sy, 16 * sy + 16)
        for d in range(6):
            for p in range(16):
                sel = np.s_[p, :, ys] if d in (0, 2) else np.s_[:, p, ys] if d in (1, 3) else np.s_[:, :, 16 * sy + p]
                for r, q, W, L, k in greedy(F[d][sel], key[d][sel]) if F[d][sel].any() else ():
                    xyz = (r, q, p) if d in (0, 2) else (p, q, r) if d in (1, 3) else (q, p, r)
                    rec.append((sy, pack(*xyz, d, W, L, k & 255), k >> 8 & 255, k >> 16))
        rec += [(sy, pack(x, y, z, 6, 1, 1, own[z, x, 16 * sy + y] & 255), own[z, x, 16 * sy + y] >> 8 & 255, 0xFF) for z, x, y in np.argwhere(X[:, :, ys])]
    return np.array(rec, np.int64).reshape(-1, 4)


ABSENT = [[-1] * 8]
BATCH_NB8 = [[0, -1, 1, -1, 4, 2, -1, 0], [4, 3, -1, -1, 1, 1, 3, -1], [-1, -1, -1, 0, -1, 3, 1, 2], [2, 2, 2, 2, 0, 3, 4, 1]]


@functools.lru_cache(None)
def ao_case(name):
    """(pool, light or None = the lit file's pattern "rand", chunk_idx, neighbor_idx8, records expected of chunk 0 or None, {(d, z, x, y): AO expected})"""
    rng = np.random.default_rng(5)
    b = np.zeros((3, 16, 16, 384), np.uint8)
    lp, idx, nb8, want, ao = np.full(b.shape, 0xF0, np.uint8), [0], ABSENT, None, {}
    if name == "pillar":                                   # +y of the floor: 7 x 16, 9 x 7, 9 x 6, 6 x 3 open quads and the eight cells around the voxel; floor -y; the voxel's top and four sides
        b[0, :, :, 64], b[0, 8, 8, 65], want = ROCK, ROCK, 4 + 8 + 1 + 1 + 4
        ao = {(1, 8, 8, 65): 0xDD, (4, 8, 7, 64): 0xBB, (4, 7, 7, 64): 0xBF}      # the floor under both lower corners; the voxel on the +x side; at the (+z, +x) corner
    elif name == "two_sides":                              # s1 and s2 without the corner -> 0; s1 and the corner -> 1: not 3 - popcount
        b[0, :, :, 64], b[0, 8, 9, 65], b[0, 9, 8, 65], b[0, 4, 3, 65], b[0, 4, 4, 65] = ROCK, ROCK, ROCK, ROCK, ROCK
        ao = {(4, 8, 8, 64): 0x2B, (4, 3, 3, 64): 0x6F}              # corner 3 is 0 / 1; the lone sides cost the corners beside it one each
    elif name.startswith("diag"):                          # an occluder only in the diagonal chunk (+x,+z): present, present and empty, absent
        b[0, 15, 15, 64], b[1, 0, 0, 65] = ROCK, ROCK
        nb8 = [[-1, -1, -1, -1, {"diag": 1, "diag_empty": 2, "diag_absent": -1}[name], -1, -1, -1]]
        ao = {(4, 15, 15, 64): 0xBF if name == "diag" else 0xFF}
    elif name == "side_nb":                                # the +x face's front voxel lies in E: row neighbours in E at z = 1 and, for z = -1, in the diagonal (+x,-z)
        b[0, 0, 15, 100], b[1, 1, 0, 100], b[2, 15, 0, 101] = ROCK, ROCK, ROCK
        nb8, ao = [[-1, 1, -1, -1, -1, 2, -1, -1]], {(1, 0, 15, 100): 0xAB}
    elif name == "carry":                                  # the occluder one voxel across a section border, and nothing beyond the world
        b[0, 5, 5, 15], b[0, 5, 6, 16], b[0, 9, 5, 16], b[0, 9, 6, 15], b[0, 12, 12, 0], b[0, 12, 12, 383] = (ROCK,) * 6
        b[0, 12, 13, 1], b[0, 12, 13, 382] = ROCK, ROCK
        ao = {(1, 5, 5, 15): 0xBB, (1, 9, 5, 16): 0xEE, (5, 12, 12, 0): 0xFF, (4, 12, 12, 383): 0xFF, (1, 12, 12, 0): 0xBB, (1, 12, 12, 383): 0xEE}
    elif name == "patch":                                  # 4 x 4 x 4 patches of rock / air and of three light values: merges and splits
        b = np.zeros((5, 16, 16, 384), np.uint8)
        b[..., 32:96] = (np.where(rng.random((5, 4, 4, 16)) < 0.35, ROCK, 0)).astype(np.uint8).repeat(4, 1).repeat(4, 2).repeat(4, 3)
        b[2] = 0
        lp, idx, nb8 = light_field("patch", b)[0], [3, 0, 4, 1], BATCH_NB8
    elif name == "open":                                   # nothing occludes anywhere: the lit stream
        b, idx, _, _ = case("slab_empty")
        lp, nb8 = light_field("patch", b)[0], [[1] * 8]
    else:                                                  # per-voxel random blocks and light: nearly nothing merges
        b, idx, nb, _ = case(name)
        lp, nb8 = None, BATCH_NB8 if name == "batch" else [[1] * 8] if nb else ABSENT
    return b, light_field("rand", b)[0] if lp is None else lp, idx, nb8, want, ao


def run(gen, b, lp, idx, nb8, mask=0xff, **kw):
    t = gen.torch
    dev = lambda a: t.tensor(a, dtype=t.int32, device=gen.device)
    up = lambda a: t.from_numpy(a.reshape(len(a), -1)).to(gen.device)
    out = gen.mesh_ao_section_quads(up(b), up(lp) if mask else None, neighbor_idx8=dev(nb8), chunk_idx=dev(idx), light_mask=mask, **kw)
    got = np.stack([out["quads"].cpu().numpy().astype(np.int64) & 0xffffffff, out["quad_light"].cpu().numpy(), out["quad_ao"].cpu().numpy()], 1)
    return out, got, out["section_quads"].cpu().numpy(), out["quad_offset"].cpu().numpy()


CASES = [(n, 0xff) for n in ("pillar", "two_sides", "diag", "diag_empty", "diag_absent", "side_nb", "carry", "column", "xshaped", "batch", "random", "open")] + \
        [("patch", m) for m in (0xff, 0xF0, 0)]


@pytest.mark.parametrize("name,mask", CASES)
def test_records_light_and_ao_equal_the_contract(gen, name, mask):
    b, lp, idx, nb8, want, ao = ao_case(name)
    out, got, secq, off = run(gen, b, lp, idx, nb8, mask)
    assert out["total"] == len(got) == secq.sum() and off.tolist() == (np.cumsum(secq.sum(1)) - secq.sum(1)).tolist()
    ref_ao = face_ao(b, idx[0], nb8[0])
    for (d, z, x, y), v in ao.items():                     # the hand-derived corner values pin the reference
        assert ref_ao[d, z, x, y] == v, f"face {(d, z, x, y)}: reference AO {ref_ao[d, z, x, y]:#x}, derived {v:#x}"
    for i, c in enumerate(idx):
        ref = contract(b, lp, c, nb8[i], mask)
        assert want is None or i > 0 or len(ref) == want, (len(ref), want)
        assert secq[i].tolist() == np.bincount(ref[:, 0], minlength=24).tolist(), f"chunk {i}: section counts"
        mine = got[off[i]:off[i] + len(ref)]
        bad = np.flatnonzero((mine != ref[:, 1:]).any(1))
        assert bad.size == 0, f"chunk {i}: {bad.size} records differ, first {bad[0]}: {gen.section_quad_fields(mine[bad[:1], 0])} light, AO {mine[bad[0], 1:]} vs " \
                              f"{gen.section_quad_fields(ref[bad[:1], 1])} light, AO {ref[bad[0], 2:]}"
    f = gen.section_quad_fields(got[:, 0])
    for (d, z, x, y), v in ao.items():                     # single-cell faces: the record at that voxel carries the derived byte
        hit = (f["kind"] == d) & (f["x"] == x) & (f["z"] == z) & (f["y"] == (y & 15)) & (np.repeat(np.arange(24), secq[0])[:len(got)] == y >> 4)
        assert got[hit, 2].tolist() == [v], (d, z, x, y)
    if name == "xshaped":                                  # kind-6: no occlusion, the voxel's own light
        assert got[f["kind"] == 6, 2].tolist() == [0xFF] * 3 and got[f["kind"] == 6, 1].tolist() == [lp[0, 4, x, 51] for x in (4, 5, 7)]
    if mask == 0:
        assert not got[:, 1].any()
    if name == "open":                                     # every face unoccluded: records and light are the lit stream's
        t = gen.torch
        lit = gen.mesh_lit_section_quads(t.from_numpy(b.reshape(len(b), -1)).to(gen.device), t.from_numpy(lp.reshape(len(b), -1)).to(gen.device),
                                         neighbor_idx=t.tensor([[1] * 4], dtype=t.int32, device=gen.device), chunk_idx=t.tensor(idx, dtype=t.int32, device=gen.device))
        assert (ref_ao[face_set(b, 0, [1] * 4)[0]] == 0xFF).all() and (got[:, 2] == 0xFF).all()
        assert t.equal(out["quads"], lit["quads"]) and t.equal(out["quad_light"], lit["quad_light"]) and t.equal(out["section_quads"], lit["section_quads"])


def test_capped_fill_writes_none_of_the_arrays_behind_the_cap(gen):
    b, lp, idx, nb8, _, _ = ao_case("patch")
    _, full, secq, off = run(gen, b, lp, idx, nb8)
    counts = secq.sum(1)
    assert (counts > 1).all()
    cap = int(off[2] + counts[2] - 1)                      # chunks 0 and 1 fit, chunk 2 lacks one record, chunk 3 would start inside the buffer
    out, got, secq2, off2 = run(gen, b, lp, idx, nb8, capacity_quads=cap)
    assert out["total"] == len(full) and np.array_equal(secq2, secq) and np.array_equal(off2, off) and len(got) == cap
    assert np.array_equal(got[:off[2]], full[:off[2]]) and (got[off[2]:] == [-7 & 0xffffffff, 0xf9, 0xf9]).all()


def test_generated_region_lit_by_the_light_kernels(gen):
    t = gen.torch
    blocks = gen.generate_region(1488, -1110, 3, 3)["blocks"]
    grid = t.arange(9, dtype=t.int32, device=gen.device).reshape(3, 3)
    light = gen.light(gen.light_masks(blocks), grid)
    mesh, lit = gen.mesh_ao_section_quads(blocks, light, 3, 3), gen.mesh_lit_section_quads(blocks, light, 3, 3)["chunk_quads"].cpu().numpy()
    pool, lp = blocks.cpu().numpy().reshape(-1, 16, 16, 384), light.cpu().numpy().reshape(-1, 16, 16, 384)
    quads, secq, off = mesh["quads"].cpu().numpy(), mesh["section_quads"].cpu().numpy(), mesh["quad_offset"].cpu().numpy()
    for c in range(9):
        x, z = c % 3, c // 3
        at = lambda dx, dz: c + dx + 3 * dz if 0 <= x + dx < 3 and 0 <= z + dz < 3 else -1
        nb8 = [at(0, 1), at(1, 0), at(0, -1), at(-1, 0), at(1, 1), at(1, -1), at(-1, -1), at(-1, 1)]
        f = gen.section_quad_fields(quads[off[c]:off[c] + secq[c].sum()])
        assert ((f["w"] + 1) * (f["l"] + 1))[f["kind"] < 6].sum() == face_set(pool, c, nb8[:4])[0].sum() and secq[c].sum() >= lit[c]
        if c == 4:
            ref = contract(pool, lp, c, nb8)
            got = slice(off[c], off[c] + len(ref))
            assert secq[c].tolist() == np.bincount(ref[:, 0], minlength=24).tolist()
            assert np.array_equal(quads[got].astype(np.int64) & 0xffffffff, ref[:, 1])
            assert np.array_equal(mesh["quad_light"].cpu().numpy()[got], ref[:, 2]) and np.array_equal(mesh["quad_ao"].cpu().numpy()[got], ref[:, 3])
    ground = int(np.max(np.nonzero(pool[4][8, 8])[0]))
    vis = gen.visible_sections(gen.section_connectivity(blocks), grid, (1, min(ground + 2, 383) >> 4, 1), 1)
    d, v = gen.section_draws(vis, grid, (1, 1), 1, mesh)["draws"], vis.cpu().numpy().reshape(-1)
    want = [quads[off[c] + secq[c, :sy].sum():off[c] + secq[c, :sy + 1].sum()] for c in range(9) for sy in range(24) if int(v[c]) >> sy & 1]
    assert len(d) > 0 and np.array_equal(np.concatenate([quads[f:f + n] for f, n in zip(d["first"].tolist(), d["count"].tolist())]), np.concatenate(want))
