"""GPU tests of the greedy quad mesher (include/mmgen.h "greedy-merged compact quad mesh"): mmgen_mesh_quads_count / _fill against a plain
Python restatement of the contract (face set in numpy, greedy rule on Python integers as row masks), record for record, in order."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DIRS = [(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]      # dirVecs as steps in a [z][x][y] array
AIR, OPAQUE, SEMI, TRANS, XSH = range(5)
CLS = np.full(256, OPAQUE, np.int8)
CLS[:140] = 1 + np.load(os.path.join(GOLDEN, "block_data.npz"))["block_data"][:, 12]
CLS[0] = AIR


def face_set(pool, c, nb):
    """F bool [6][z][x][y] and the X mask of chunk c of pool [slots][z][x][y]; nb = its N E S W slots, -1 = absent (class -1 beyond)"""
    pad = np.full((18, 18, 386), -1, np.int8)
    pad[1:17, 1:17, 1:385], pad[1:17, 1:17, 0], pad[1:17, 1:17, 385] = CLS[pool[c]], AIR, AIR
    for d, dst, src in ((0, np.s_[17, 1:17], np.s_[0]), (1, np.s_[1:17, 17], np.s_[:, 0]), (2, np.s_[0, 1:17], np.s_[15]), (3, np.s_[1:17, 0], np.s_[:, 15])):
        if nb[d] >= 0:
            pad[dst + (np.s_[1:385],)] = CLS[pool[nb[d]][src]]
    me = pad[1:17, 1:17, 1:385]
    F = np.zeros((6, 16, 16, 384), bool)
    for d, (dz, dx, dy) in enumerate(DIRS):
        n = pad[1 + dz:17 + dz, 1 + dx:17 + dx, 1 + dy:385 + dy]
        F[d] = (n != -1) & ((((me == OPAQUE) | (me == SEMI)) & (n != OPAQUE)) | ((me == TRANS) & ((n == AIR) | (n == SEMI))))
    return F, me == XSH


def encode(x, y, z, kind, dx, dy, dz, b):
    return int(x) | int(y) << 4 | int(z) << 13 | kind << 17 | dx << 20 | dy << 24 | dz << 33 | int(b) << 37


def greedy(Fp, ids):
    """the greedy rule on one plane, rows as Python integers: (r0, q0, W, L, block) in emission order"""
    R, Q = Fp.shape
    rows = [int.from_bytes(np.packbits(f, bitorder="little").tobytes(), "little") for f in Fp]
    out = []
    for r in range(R):
        while rows[r]:
            q0 = (rows[r] & -rows[r]).bit_length() - 1
            b, L = ids[r, q0], 1
            while q0 + L < Q and rows[r] >> (q0 + L) & 1 and ids[r, q0 + L] == b:
                L += 1
            m, W = ((1 << L) - 1) << q0, 1
            while r + W < R and rows[r + W] & m == m and (ids[r + W, q0:q0 + L] == b).all():
                W += 1
            for k in range(r, r + W):
                rows[k] &= ~m
            out.append((r, q0, W, L, b))
    return out


def contract(pool, c, nb):
    F, X = face_set(pool, c, nb)
    b, rec = pool[c], []
    for d in range(6):
        for p in range(384 if d >= 4 else 16):
            Fp, ids = (F[d][p], b[p]) if d in (0, 2) else (F[d][:, p], b[:, p]) if d in (1, 3) else (F[d][:, :, p], b[:, :, p])
            for r, q, W, L, blk in greedy(Fp, ids) if Fp.any() else ():
                rec.append(encode(r, q, p, d, W - 1, L - 1, 0, blk) if d in (0, 2) else encode(p, q, r, d, 0, L - 1, W - 1, blk) if d in (1, 3) else
                           encode(q, p, r, d, L - 1, 0, W - 1, blk))
    rec += [encode(x, y, z, 6, 0, 0, 0, b[z, x, y]) for z, x, y in np.argwhere(X)]
    return np.array(rec, np.int64)


SHAPES = {"L": ["100", "100", "111"], "T": ["11111", "00100", "00100"], "stairs": ["001100", "111111", "011110"]}      # [row][q]
ALONE, EMPTY_AROUND = None, [[1, 1, 1, 1]]


@functools.lru_cache(None)
def case(name):
    """(pool [slots][z][x][y], chunk_idx or None, neighbor_idx or None, records expected of chunk 0 or None)"""
    rng = np.random.default_rng(3)
    b = np.zeros((2, 16, 16, 384), np.uint8)
    idx, nb, want = [0], ALONE, None
    if name == "interior":
        b[0, 8, 8, 100], want = 57, 6
    elif name.startswith("edge"):                          # a block on the +x edge: neighbour absent / present and empty / present and opaque
        b[0, 8, 15, 100], b[1, 8, 0, 100] = 57, 57 if name == "edge_opaque" else 0
        nb, want = (ALONE, 5) if name == "edge_absent" else ([[-1, 1, -1, -1]], 6 if name == "edge_empty" else 5)
    elif name.startswith("slab"):                          # 16 x 2 x 16 straddling a u64 word
        b[0, :, :, 63:65] = 57
        nb, want = (ALONE, 2) if name == "slab_absent" else (EMPTY_AROUND, 6)
    elif name == "column":
        b[0, 5, 5, :], want = 57, 6
    elif name == "column_runs":                            # runs of 50 cross every multiple of 64 and most multiples of 16
        b[0, 5, 5, :], want = np.array([57, 68])[(np.arange(384) // 50) % 2], 4 * 8 + 2
    elif name.split("_")[0] in SHAPES:
        s = np.array([[int(ch) for ch in row] for row in SHAPES[name.split("_")[0]]], bool)
        r, q = np.nonzero(s)
        if name.endswith("_side"):
            b[0, 3, 5 + r, 60 + q] = 57                    # plane z = 3: rows x, q = y across the word boundary at 64
        else:
            b[0, 5 + r, 7 + q, 70] = 57                    # plane y = 70: rows z, q = x
    elif name == "two_ids":
        b[0, 4, 4:8, 100], b[0, 4, 8:12, 100], b[0, 5, 4:12, 100] = 57, 68, 57
    elif name == "classes":                                # every pairing of opaque, semi, transparent, side by side and on top of each other
        for k, (a, c) in enumerate((a, c) for a in (57, 87, 1) for c in (68, 91, 103)):
            b[0, 4, 4:6, 10 + 4 * k], b[0, 9, 9, 10 + 4 * k:12 + 4 * k] = (a, c), (a, c)
    elif name == "xshaped":
        b[0, 4, 4:8, 50], b[0, 4, 4:8, 51], want = 57, (7, 16, 87, 7), 6 + 5 + 3      # the ground merges to 6 quads (plants hide nothing), the leaf shows 5 faces, 3 plants last
    elif name == "batch":                                  # five slots, a permuting work list, explicit neighbours (slot 2 is air)
        b = np.where(rng.random((5, 16, 16, 384)) < 0.01, rng.choice(np.array([57, 68, 87, 1, 7], np.uint8), (5, 16, 16, 384)), 0).astype(np.uint8)
        b[..., :30], b[..., 60:], b[2] = 0, 0, 0
        idx, nb = [3, 0, 4, 1], [[0, -1, 1, -1], [4, 3, -1, -1], [-1, -1, -1, 0], [2, 2, 2, 2]]
    elif name == "random":                                 # 16 x 48 x 16 around y = 40 .. 88, about 3 % filled with four ids
        b[:, :, :, 40:88] = np.where(rng.random((2, 16, 16, 48)) < 0.03, rng.choice(np.array([57, 68, 87, 1], np.uint8), (2, 16, 16, 48)), 0)
        nb = EMPTY_AROUND
    else:
        assert name == "air"
        want = 0
    return b, idx, nb, want


CASES = ["interior", "edge_absent", "edge_empty", "edge_opaque", "slab_absent", "slab_empty", "column", "column_runs", "two_ids", "classes", "xshaped",
         "batch", "random", "air"] + [s + o for s in SHAPES for o in ("_side", "_y")]


def run(gen, b, idx, nb, **kw):
    t = gen.torch
    dev = lambda a: None if a is None else t.tensor(a, dtype=t.int32, device=gen.device)
    out = gen.mesh_quads(t.from_numpy(b.reshape(len(b), -1)).to(gen.device), neighbor_idx=dev(nb), chunk_idx=dev(idx), **kw)
    return out, out["quads"].cpu().numpy(), out["chunk_quads"].cpu().numpy(), out["quad_offset"].cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_records_equal_the_contract(gen, name):
    b, idx, nb, want = case(name)
    out, quads, counts, off = run(gen, b, idx, nb)
    ref = [contract(b, c, nb[i] if nb else [-1] * 4) for i, c in enumerate(idx)]
    assert want is None or len(ref[0]) == want, (len(ref[0]), want)
    assert counts.tolist() == [len(r) for r in ref] and off.tolist() == np.cumsum([0] + [len(r) for r in ref])[:-1].tolist() and out["total"] == len(quads)
    for i, r in enumerate(ref):
        got = quads[off[i]:off[i] + counts[i]]
        bad = np.flatnonzero(got != r)
        assert bad.size == 0, f"chunk {i}: {bad.size} records differ, first {bad[0]}: {gen.quad_fields(got[bad[:1]])} vs {gen.quad_fields(r[bad[:1]])}"
    if name == "slab_absent":
        f = gen.quad_fields(quads)
        assert f["kind"].tolist() == [4, 5] and f["dx"].tolist() == [15, 15] and f["dz"].tolist() == [15, 15]
    if name == "column":
        assert gen.quad_fields(quads)["dy"].tolist() == [383] * 4 + [0, 0]


def test_no_chunks(gen):
    out = gen.mesh_quads(gen.torch.zeros((0, 98304), dtype=gen.torch.uint8, device=gen.device))
    assert out["total"] == 0 and out["quads"].numel() == 0 and out["chunk_quads"].numel() == 0


def test_capped_fill_leaves_what_does_not_fit_untouched(gen):
    b, idx, nb, _ = case("batch")
    _, full, counts, off = run(gen, b, idx, nb)
    assert (counts > 1).all()
    cap = int(off[2] + counts[2] - 1)                      # chunks 0 and 1 fit, chunk 2 lacks one record, chunk 3 would start inside the buffer
    out, quads, counts2, off2 = run(gen, b, idx, nb, capacity_quads=cap)
    assert out["total"] == len(full) and np.array_equal(counts2, counts) and np.array_equal(off2, off) and len(quads) == cap
    assert np.array_equal(quads[:off[2]], full[:off[2]]) and (quads[off[2]:] == -7).all()


def test_generated_region_is_covered_exactly_once(gen):
    nx = nz = 3
    blocks = gen.generate_region(1488, -1110, nx, nz)["blocks"]
    out = gen.mesh_quads(blocks, nx, nz)
    pos = gen.torch.zeros((nx * nz, 2), dtype=gen.torch.int32, device=gen.device)
    verts = gen.create_vbos(blocks, pos, nx, nz)["chunk_verts"].cpu().numpy()
    pool = blocks.cpu().numpy().reshape(-1, 16, 16, 384)
    quads, counts, off = out["quads"].cpu().numpy(), out["chunk_quads"].cpu().numpy(), out["quad_offset"].cpu().numpy()
    for c in range(nx * nz):
        x, z = c % nx, c // nx
        nb = [c + nx if z < nz - 1 else -1, c + 1 if x < nx - 1 else -1, c - nx if z > 0 else -1, c - 1 if x > 0 else -1]
        F, X = face_set(pool, c, nb)
        q = quads[off[c]:off[c] + counts[c]]
        f = gen.quad_fields(q)
        face, area = f["kind"] < 6, (f["dx"] + 1) * (f["dy"] + 1) * (f["dz"] + 1)
        assert 4 * area[face].sum() + 8 * (~face).sum() == verts[c]
        cum = np.zeros((6, 17, 385, 17), np.int32)         # [d][z][y][x]: +-1 at the corners of every box, summed along each axis = times painted
        for sz in (0, 1):
            for sy in (0, 1):
                for sx in (0, 1):
                    np.add.at(cum, (f["kind"][face], (f["z"] + sz * (f["dz"] + 1))[face], (f["y"] + sy * (f["dy"] + 1))[face], (f["x"] + sx * (f["dx"] + 1))[face]),
                              (-1) ** (sx + sy + sz))
        paint = cum.cumsum(1).cumsum(2).cumsum(3)[:, :16, :384, :16]
        assert np.array_equal(paint, F.transpose(0, 1, 3, 2).astype(np.int32)), f"chunk {c}: faces not covered exactly once"
        assert np.array_equal(pool[c][f["z"], f["x"], f["y"]], f["block"]) and (~face).sum() == X.sum()
        if c == 4:
            assert np.array_equal(q, contract(pool, c, nb))
