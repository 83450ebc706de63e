"""GPU tests of the lit section quad mesh (include/mmgen.h "lit section quad mesh"): mmgen_mesh_lit_section_quads_count / _fill against the
per-section contract of tests/test_gpu_section_quads.py with the greedy key id | FL << 8, FL = the light of the voxel in front of the face
(padded with the out-of-world constants and the neighbour slots): records and light bytes, one for one, in order.  Every comparison is exact."""
import numpy as np
import pytest

from test_gpu_quads import DIRS, case, face_set, greedy
from test_gpu_section_quads import pack

pytestmark = pytest.mark.gpu


def contract(pool, lp, c, nb, mask=0xff):
    """rows (sy, record, light byte) of chunk c, in stream order"""
    F, X = face_set(pool, c, nb)
    pad = np.zeros((18, 18, 386), np.uint8)                 # y = -1 stays 0x00
    pad[1:17, 1:17, 1:385], pad[1:17, 1:17, 385] = lp[c], 0xF0
    for d, dst, src in ((0, np.s_[17, 1:17], np.s_[0]), (1, np.s_[1:17, 17], np.s_[:, 0]), (2, np.s_[0, 1:17], np.s_[15]), (3, np.s_[1:17, 0], np.s_[:, 15])):
        if nb[d] >= 0:
            pad[dst + (np.s_[1:385],)] = lp[nb[d]][src]
    ids = pool[c].astype(np.int32)
    key = [ids | (pad[1 + dz:17 + dz, 1 + dx:17 + dx, 1 + dy:385 + dy] & mask).astype(np.int32) << 8 for dz, dx, dy in DIRS]
    own, rec = ids | (lp[c] & mask).astype(np.int32) << 8, []
    for sy in range(24):
        ys = slice(16 * sy, 16 * sy + 16)
        for d in range(6):
            for p in range(16):
                sel = np.s_[p, :, ys] if d in (0, 2) else np.s_[:, p, ys] if d in (1, 3) else np.s_[:, :, 16 * sy + p]
                for r, q, W, L, k in greedy(F[d][sel], key[d][sel]) if F[d][sel].any() else ():
                    xyz = (r, q, p) if d in (0, 2) else (p, q, r) if d in (1, 3) else (q, p, r)
                    rec.append((sy, pack(*xyz, d, W, L, k & 255), k >> 8))
        rec += [(sy, pack(x, y, z, 6, 1, 1, own[z, x, 16 * sy + y] & 255), own[z, x, 16 * sy + y] >> 8) for z, x, y in np.argwhere(X[:, :, ys])]
    return np.array(rec, np.int64).reshape(-1, 3)


def run(gen, b, lp, idx=None, nb=None, **kw):
    t = gen.torch
    dev = lambda a: None if a is None else t.tensor(a, dtype=t.int32, device=gen.device)
    up = lambda a: t.from_numpy(a.reshape(len(a), -1)).to(gen.device)
    out = gen.mesh_lit_section_quads(up(b), up(lp), neighbor_idx=dev(nb), chunk_idx=dev(idx), **kw)
    return out, out["quads"].cpu().numpy().astype(np.int64) & 0xffffffff, out["quad_light"].cpu().numpy(), out["section_quads"].cpu().numpy(), out["quad_offset"].cpu().numpy()


def light_field(pattern, b):
    """the light of pool b [slots][z][x][y] for a pattern, and the records expected of chunk 0 (None = whatever the contract gives)"""
    rng = np.random.default_rng(11)
    lp, want = np.full(b.shape, 0xF0, np.uint8), None
    if pattern == "uniform":
        want = 10
    elif pattern in ("y65_x", "y65_z"):                    # the +y face splits along q / along r
        lp[(0, slice(None), slice(8, 16), 65) if pattern == "y65_x" else (0, slice(8, 16), slice(None), 65)], want = 0xE1, 11
    elif pattern == "y62_xz":                              # the -y face splits in four
        lp[0, :, 8:, 62], lp[0, 8:, :, 62], lp[0, 8:, 8:, 62], want = 0x0D, 0xE1, 0x33, 13
    elif pattern == "voxel65":                             # one deviating voxel: both the L and the W stop
        lp[0, 8, 8, 65] = 0xE1
    elif pattern == "voxel100":                            # in front of no face
        lp[0, 8, 8, 100], want = 0xE1, 10
    elif pattern == "nbslot64":                            # only the neighbour slot deviates: the border faces at y = 64 carry its light
        lp[1, :, :, 64], want = 0x0D, 10
    elif pattern == "steps":                               # the four columns around (5, 5): the sides split at y = 200 and at the section borders
        lp[:] = 0x5A
        for z, x in ((4, 5), (6, 5), (5, 4), (5, 6)):
            lp[0, z, x] = np.array([0x11, 0x22, 0x33, 0x44], np.uint8)[np.searchsorted([16, 64, 200], np.arange(384), "right")]
        want = 24 * 4 + 4 + 2
    elif pattern == "patch":                               # 4 x 4 x 4 patches over three values: merges and splits
        lp = np.array([0xF0, 0xE1, 0x0D], np.uint8)[rng.integers(0, 3, (len(b), 4, 4, 96))].repeat(4, 1).repeat(4, 2).repeat(4, 3)
    else:
        assert pattern == "rand"                           # nearly nothing merges
        lp = rng.integers(0, 256, b.shape, dtype=np.uint8)
    return lp, want


CASES = [("slab_empty", p, 0xff) for p in ("uniform", "y65_x", "y65_z", "y62_xz", "voxel65", "voxel100", "nbslot64")] + \
        [("column", "steps", 0xff), ("edge_empty", "rand", 0xff), ("xshaped", "rand", 0xff)] + \
        [(c, p, 0xff) for c in ("batch", "random") for p in ("patch", "rand")] + [("batch", "patch", 0xF0), ("batch", "patch", 0)]


@pytest.mark.parametrize("name,pattern,mask", CASES)
def test_records_and_light_equal_the_contract(gen, name, pattern, mask):
    b, idx, nb, _ = case(name)
    lp, want = light_field(pattern, b)
    out, quads, ql, secq, off = run(gen, b, lp, idx, nb, light_mask=mask)
    assert out["total"] == len(quads) == len(ql) == secq.sum() and off.tolist() == (np.cumsum(secq.sum(1)) - secq.sum(1)).tolist()
    for i, c in enumerate(idx):
        ref = contract(b, lp, c, nb[i] if nb else [-1] * 4, mask)
        assert want is None or i > 0 or len(ref) == want, (len(ref), want)
        assert secq[i].tolist() == np.bincount(ref[:, 0], minlength=24).tolist(), f"chunk {i}: section counts"
        got = slice(off[i], off[i] + len(ref))
        bad = np.flatnonzero((quads[got] != ref[:, 1]) | (ql[got] != ref[:, 2]))
        assert bad.size == 0, f"chunk {i}: {bad.size} records differ, first {bad[0]}: {gen.section_quad_fields(quads[got][bad[:1]])} light {ql[got][bad[:1]]} vs " \
                              f"{gen.section_quad_fields(ref[bad[:1], 1])} light {ref[bad[:1], 2]}"
    kind = gen.section_quad_fields(quads)["kind"]
    if name == "column":                                   # beyond the world the light is a constant, whatever d_light holds
        assert ql[kind == 4].tolist() == [0xF0] and ql[kind == 5].tolist() == [0]
    if name == "edge_empty":                               # the +x face's light is the neighbour slot's voxel
        assert ql[kind == 1].tolist() == [lp[1, 8, 0, 100]]
    if name == "xshaped":                                  # kind-6 light is the voxel's own
        assert ql[kind == 6].tolist() == [lp[0, 4, x, 51] for x in (4, 5, 7)]
    if mask == 0:                                          # the unlit stream, and no light
        t = gen.torch
        unlit = gen.mesh_section_quads(t.from_numpy(b.reshape(len(b), -1)).to(gen.device), neighbor_idx=t.tensor(nb, dtype=t.int32, device=gen.device),
                                       chunk_idx=t.tensor(idx, dtype=t.int32, device=gen.device))
        assert t.equal(out["quads"], unlit["quads"]) and t.equal(out["section_quads"], unlit["section_quads"]) and not ql.any()


def test_capped_fill_writes_neither_array_behind_the_cap(gen):
    b, idx, nb, _ = case("batch")
    lp, _ = light_field("patch", b)
    _, full, fl, secq, off = run(gen, b, lp, idx, nb)
    counts = secq.sum(1)
    assert (counts > 1).all()
    cap = int(off[2] + counts[2] - 1)                      # chunks 0 and 1 fit, chunk 2 lacks one record, chunk 3 would start inside the buffer
    out, quads, ql, secq2, off2 = run(gen, b, lp, idx, nb, capacity_quads=cap)
    assert out["total"] == len(full) and np.array_equal(secq2, secq) and np.array_equal(off2, off) and len(quads) == len(ql) == cap
    assert np.array_equal(quads[:off[2]], full[:off[2]]) and np.array_equal(ql[:off[2]], fl[:off[2]])
    assert (quads[off[2]:] == (-7 & 0xffffffff)).all() and (ql[off[2]:] == 0xf9).all()


def test_generated_region_lit_by_the_light_kernels(gen):
    t = gen.torch
    blocks = gen.generate_region(1488, -1110, 3, 3)["blocks"]
    grid = t.arange(9, dtype=t.int32, device=gen.device).reshape(3, 3)
    light = gen.light(gen.light_masks(blocks), grid)
    mesh, unlit = gen.mesh_lit_section_quads(blocks, light, 3, 3), gen.mesh_section_quads(blocks, 3, 3)["chunk_quads"].cpu().numpy()
    pool, lp = blocks.cpu().numpy().reshape(-1, 16, 16, 384), light.cpu().numpy().reshape(-1, 16, 16, 384)
    quads, ql, secq, off = mesh["quads"].cpu().numpy(), mesh["quad_light"].cpu().numpy(), mesh["section_quads"].cpu().numpy(), mesh["quad_offset"].cpu().numpy()
    for c in range(9):
        x, z = c % 3, c // 3
        nb = [c + 3 if z < 2 else -1, c + 1 if x < 2 else -1, c - 3 if z > 0 else -1, c - 1 if x > 0 else -1]
        f = gen.section_quad_fields(quads[off[c]:off[c] + secq[c].sum()])
        assert ((f["w"] + 1) * (f["l"] + 1))[f["kind"] < 6].sum() == face_set(pool, c, nb)[0].sum() and secq[c].sum() >= unlit[c]
        if c == 4:
            ref = contract(pool, lp, c, nb)
            got = slice(off[c], off[c] + len(ref))
            assert secq[c].tolist() == np.bincount(ref[:, 0], minlength=24).tolist()
            assert np.array_equal(quads[got].astype(np.int64) & 0xffffffff, ref[:, 1]) and np.array_equal(ql[got], ref[:, 2])
    ground = int(np.max(np.nonzero(pool[4][8, 8])[0]))
    vis = gen.visible_sections(gen.section_connectivity(blocks), grid, (1, min(ground + 2, 383) >> 4, 1), 1)
    d, v = gen.section_draws(vis, grid, (1, 1), 1, mesh)["draws"], vis.cpu().numpy().reshape(-1)
    want = [quads[off[c] + secq[c, :sy].sum():off[c] + secq[c, :sy + 1].sum()] for c in range(9) for sy in range(24) if int(v[c]) >> sy & 1]
    assert len(d) > 0 and np.array_equal(np.concatenate([quads[f:f + n] for f, n in zip(d["first"].tolist(), d["count"].tolist())]), np.concatenate(want))
