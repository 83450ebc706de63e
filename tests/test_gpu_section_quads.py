"""GPU tests of the section-bucketed quad mesh and its draw list (include/mmgen.h "section-bucketed quad mesh"): mmgen_mesh_section_quads_count /
_fill against the greedy rule of tests/test_gpu_quads.py restated per 16 x 16 section plane, record for record, in order; mmgen_section_draws
against numpy."""
import numpy as np
import pytest

from test_gpu_quads import CASES, case, face_set, greedy

pytestmark = pytest.mark.gpu


def pack(x, y, z, kind, W, L, b):
    return int(x) | int(y) << 4 | int(z) << 8 | kind << 12 | (W - 1) << 15 | (L - 1) << 19 | int(b) << 23


def contract(pool, c, nb):
    """the records of the 24 sections of chunk c"""
    F, X = face_set(pool, c, nb)
    b, out = pool[c], []
    for sy in range(24):
        ys, rec = slice(16 * sy, 16 * sy + 16), []
        for d in range(6):
            for p in range(16):
                Fp, ids = (F[d][p, :, ys], b[p, :, ys]) if d in (0, 2) else (F[d][:, p, ys], b[:, p, ys]) if d in (1, 3) else (F[d][:, :, 16 * sy + p], b[:, :, 16 * sy + p])
                for r, q, W, L, blk in greedy(Fp, ids) if Fp.any() else ():
                    rec.append(pack(r, q, p, d, W, L, blk) if d in (0, 2) else pack(p, q, r, d, W, L, blk) if d in (1, 3) else pack(q, p, r, d, W, L, blk))
        rec += [pack(x, y, z, 6, 1, 1, b[z, x, 16 * sy + y]) for z, x, y in np.argwhere(X[:, :, ys])]
        out.append(np.array(rec, np.int64))
    return out


def run(gen, b, idx=None, nb=None, **kw):
    t = gen.torch
    dev = lambda a: None if a is None else t.tensor(a, dtype=t.int32, device=gen.device)
    out = gen.mesh_section_quads(t.from_numpy(b.reshape(len(b), -1)).to(gen.device), neighbor_idx=dev(nb), chunk_idx=dev(idx), **kw)
    return out, out["quads"].cpu().numpy().astype(np.int64) & 0xffffffff, out["section_quads"].cpu().numpy(), out["chunk_quads"].cpu().numpy(), out["quad_offset"].cpu().numpy()


def assert_chunk(gen, got, ref, what):
    assert len(got) == len(ref), f"{what}: {len(got)} records for {len(ref)}"
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"{what}: {bad.size} records differ, first {bad[0]}: {gen.section_quad_fields(got[bad[:1]])} vs {gen.section_quad_fields(ref[bad[:1]])}"


@pytest.mark.parametrize("name", CASES)
def test_records_equal_the_contract(gen, name):
    b, idx, nb, _ = case(name)
    out, quads, secq, counts, off = run(gen, b, idx, nb)
    ref = [contract(b, c, nb[i] if nb else [-1] * 4) for i, c in enumerate(idx)]
    want = {"column": 24 * 4 + 2, "slab_empty": 10, "slab_absent": 2, "air": 0}.get(name)
    assert want is None or sum(map(len, ref[0])) == want
    assert secq.tolist() == [[len(s) for s in r] for r in ref] and counts.tolist() == secq.sum(1).tolist()
    assert off.tolist() == (np.cumsum(counts) - counts).tolist() and out["total"] == len(quads) == counts.sum()
    for i, r in enumerate(ref):
        assert_chunk(gen, quads[off[i]:off[i] + counts[i]], np.concatenate(r), f"chunk {i}")


def test_no_chunks_and_capped_fill(gen):
    out = gen.mesh_section_quads(gen.torch.zeros((0, 98304), dtype=gen.torch.uint8, device=gen.device))
    assert out["total"] == 0 and out["quads"].numel() == 0 and out["chunk_quads"].numel() == 0 and out["section_quads"].numel() == 0
    b, idx, nb, _ = case("batch")
    _, full, secq, counts, off = run(gen, b, idx, nb)
    assert (counts > 1).all()
    cap = int(off[2] + counts[2] - 1)                      # chunks 0 and 1 fit, chunk 2 lacks one record, chunk 3 would start inside the buffer
    out, quads, secq2, counts2, off2 = run(gen, b, idx, nb, capacity_quads=cap)
    assert out["total"] == len(full) and np.array_equal(secq2, secq) and np.array_equal(counts2, counts) and np.array_equal(off2, off) and len(quads) == cap
    assert np.array_equal(quads[:off[2]], full[:off[2]]) and (quads[off[2]:] == (-7 & 0xffffffff)).all()


@pytest.fixture(scope="module")
def region(gen):
    """the generated 3 x 3 region, its section mesh and its blocks on the host"""
    blocks = gen.generate_region(1488, -1110, 3, 3)["blocks"]
    return blocks, gen.mesh_section_quads(blocks, 3, 3), blocks.cpu().numpy().reshape(-1, 16, 16, 384)


def test_generated_region_is_covered_exactly_once(gen, region):
    blocks, out, pool = region
    verts = gen.create_vbos(blocks, gen.torch.zeros((9, 2), dtype=gen.torch.int32, device=gen.device), 3, 3)["chunk_verts"].cpu().numpy()
    quads, secq, off = out["quads"].cpu().numpy(), out["section_quads"].cpu().numpy(), out["quad_offset"].cpu().numpy()
    for c in range(9):
        x, z = c % 3, c // 3
        nb = [c + 3 if z < 2 else -1, c + 1 if x < 2 else -1, c - 3 if z > 0 else -1, c - 1 if x > 0 else -1]
        F, X = face_set(pool, c, nb)
        q = quads[off[c]:off[c] + secq[c].sum()]
        f = gen.section_quad_fields(q)
        y, face = 16 * np.repeat(np.arange(24), secq[c]) + f["y"], f["kind"] < 6
        ex = [np.where(f["kind"] >= 4, f["l"], np.where(f["kind"] % 2 == 0, f["w"], 0)), np.where(f["kind"] < 4, f["l"], 0),
              np.where((f["kind"] >= 4) | (f["kind"] % 2 == 1), f["w"], 0)]      # dx, dy, dz
        assert 4 * ((f["w"] + 1) * (f["l"] + 1))[face].sum() + 8 * (~face).sum() == verts[c]
        cum = np.zeros((6, 17, 385, 17), np.int32)         # [d][z][y][x]: +-1 at the corners of every box, summed along each axis = times painted
        for sz in (0, 1):
            for sy in (0, 1):
                for sx in (0, 1):
                    np.add.at(cum, (f["kind"][face], (f["z"] + sz * (ex[2] + 1))[face], (y + sy * (ex[1] + 1))[face], (f["x"] + sx * (ex[0] + 1))[face]), (-1) ** (sx + sy + sz))
        assert np.array_equal(cum.cumsum(1).cumsum(2).cumsum(3)[:, :16, :384, :16], F.transpose(0, 1, 3, 2).astype(np.int32)), f"chunk {c}: faces not covered exactly once"
        assert np.array_equal(pool[c][f["z"], f["x"], y], f["block"]) and (~face).sum() == X.sum()
        if c == 4:
            assert_chunk(gen, q.astype(np.int64) & 0xffffffff, np.concatenate(contract(pool, c, nb)), "centre chunk")


def draws_ref(vis, grid, eye, radius, mesh_pos, secq, off):
    out = []
    for wz in range(2 * radius + 1):
        for wx in range(2 * radius + 1):
            cx, cz = eye[0] + wx - radius, eye[1] + wz - radius
            s = grid[cz, cx] if 0 <= cx < grid.shape[1] and 0 <= cz < grid.shape[0] else -1
            m = -1 if s < 0 else s if mesh_pos is None else mesh_pos[s]
            out += [(off[m] + secq[m, :sy].sum(), secq[m, sy], wx | wz << 7 | sy << 14) for sy in range(24) if 0 <= m < len(secq) and int(vis[wz, wx]) >> sy & 1 and secq[m, sy] > 0]
    return out


@pytest.mark.parametrize("short", [0, 1])
def test_draw_list_of_a_synthetic_window(gen, short):
    t, rng = gen.torch, np.random.default_rng(5)
    grid = np.array([0, 1, 2, 3, 4, 5, -1, 6, 7, 8, 9, 10], np.int32).reshape(3, 4)      # slots 0 .. 10, one cell absent
    pos = rng.permutation(11).astype(np.int32)
    pos[grid[0, 1]] = -1                                    # a present chunk that was not meshed
    secq = rng.integers(0, 5, (11, 24)).astype(np.int32)    # a fifth of the sections have no record
    off = (np.cumsum(secq.sum(1)) - secq.sum(1)).astype(np.int64)
    vis = rng.integers(0, 2 ** 32, (5, 5), dtype=np.uint64).astype(np.uint32)
    ref = draws_ref(vis, grid, (0, 0), 2, pos, secq, off)  # the eye at a corner: 16 of the 25 window cells lie outside the grid
    seen = [(pos[grid[cz, cx]], int(vis[2 + cz, 2 + cx])) for cz in range(3) for cx in range(3) if grid[cz, cx] >= 0 and pos[grid[cz, cx]] >= 0]
    assert any(v >> sy & 1 and secq[m, sy] == 0 for m, v in seen for sy in range(24))      # a set bit over a section without records
    dev = lambda a: t.from_numpy(a).to(gen.device)
    mesh = dict(section_quads=dev(secq), quad_offset=dev(off))
    got = gen.section_draws(dev(vis.view(np.int32)), dev(grid), (0, 0), 2, mesh, mesh_pos=dev(pos), capacity=len(ref) - short)
    assert got["totals"] == (len(ref), sum(int(r[1]) for r in ref)) and len(ref) > 40
    assert [tuple(int(v) for v in d) for d in got["draws"]] == [tuple(int(v) for v in r) for r in ref[:len(ref) - short]]
    assert (got["buffer"].cpu().numpy()[len(ref) - short:] == 0xff).all()      # the record behind the capacity


def test_draws_gather_the_visible_sections_of_a_region(gen, region):
    blocks, mesh, pool = region
    t = gen.torch
    grid = t.arange(9, dtype=t.int32, device=gen.device).reshape(3, 3)
    ground = int(np.max(np.nonzero(pool[4][8, 8])[0]))
    vis = gen.visible_sections(gen.section_connectivity(blocks), grid, (1, min(ground + 2, 383) >> 4, 1), 1)
    got = gen.section_draws(vis, grid, (1, 1), 1, mesh)
    quads, secq, off, v = mesh["quads"].cpu().numpy(), mesh["section_quads"].cpu().numpy(), mesh["quad_offset"].cpu().numpy(), vis.cpu().numpy().reshape(-1)
    want = [quads[off[c] + secq[c, :sy].sum():off[c] + secq[c, :sy + 1].sum()] for c in range(9) for sy in range(24) if int(v[c]) >> sy & 1]
    d = got["draws"]
    assert len(d) > 0 and got["totals"] == (len(d), int(d["count"].sum()))
    assert np.array_equal(np.concatenate([quads[f:f + n] for f, n in zip(d["first"].tolist(), d["count"].tolist())]), np.concatenate(want))
    assert d["origin"].tolist() == [c % 3 | c // 3 << 7 | sy << 14 for c in range(9) for sy in range(24) if int(v[c]) >> sy & 1 and secq[c, sy]]


def test_a_pillar_through_a_culled_section_keeps_its_visible_half(gen):
    t = gen.torch
    b = np.zeros((1, 16, 16, 384), np.uint8)
    b[0, 8, 8, 32:64] = 57                                  # sections 2 and 3
    out, quads, secq, _, off = run(gen, b)
    vis = t.tensor([[1 << 3]], dtype=t.int32, device=gen.device)      # the lower section is culled
    d = gen.section_draws(vis, t.zeros((1, 1), dtype=t.int32, device=gen.device), (0, 0), 0, out)["draws"]
    assert d.tolist() == [(int(secq[0, :3].sum()), 5, 3 << 14)]
    f = gen.section_quad_fields(quads[int(d["first"][0]):int(d["first"][0]) + 5])
    assert f["kind"].tolist() == [0, 1, 2, 3, 4] and f["l"].tolist() == [15] * 4 + [0] and f["y"].tolist() == [0] * 4 + [15]
    # the chunk-wide greedy stream holds these four side faces in records whose origin lies in the culled section: culled by origin they vanish
    g = gen.quad_fields(gen.mesh_quads(t.from_numpy(b.reshape(1, -1)).to(gen.device))["quads"])
    side = g["kind"] < 4
    assert side.sum() == 4 and (g["y"][side] >> 4 == 2).all() and (g["y"][side] + g["dy"][side] == 63).all() and not (g["y"][side] >> 4 == 3).any()
