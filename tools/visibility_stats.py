#!/usr/bin/env python3
"""Section visibility on the 32 x 32-chunk region that tools/light_stats.py uses: the time of k_section_conn and
k_visible_sections beside the light masks and the vertex mesher's count + fill re-measured in the same process (they read the same bytes), the
flood rounds per chunk, and what an eye on the surface, in a cave and above the world gets culled: sections reported visible of the present
ones, and quads of mesh_quads that lie in visible sections (a quad counts for the section of its origin) of all quads.  Times are the library's
own per-kernel profile over the whole region, after a warm-up, median / min / max over the repeats.  MMGEN_LIB selects an A/B build.

usage: tools/visibility_stats.py [--cx 1488 --cz -1110 --nx 32 --nz 32 --warmup 5 --reps 30]"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from quad_mesh_stats import kernel_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cx", type=int, default=1488); ap.add_argument("--cz", type=int, default=-1110)
    ap.add_argument("--nx", type=int, default=32); ap.add_argument("--nz", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    pkg = importlib.import_module("mega-minecraft_amd")
    gen = pkg.MMGen(0)
    t = gen.torch
    blocks = gen.generate_region(a.cx, a.cz, a.nx, a.nz)["blocks"]
    n = a.nx * a.nz
    grid = t.arange(n, dtype=t.int32, device=gen.device).reshape(a.nz, a.nx)
    pos = t.zeros((n, 2), dtype=t.int32, device=gen.device)
    rounds = t.zeros(n, dtype=t.int32, device=gen.device)
    conn = gen.section_connectivity(blocks, rounds=rounds)
    r = rounds.cpu().numpy()
    rec = conn.cpu().numpy().view(np.uint16)
    print(f"library {pkg.LIB_PATH}")
    print(f"region {a.nx}x{a.nz} chunks at ({a.cx}, {a.cz}): {24 * n} sections, {np.count_nonzero(rec == 0x7fff)} fully connected, {np.count_nonzero(rec == 0)} "
          f"without a connection, digest {int(rec.astype(np.uint64).sum())}")
    print(f"flood rounds per chunk: min {r.min()}, median {int(np.median(r))}, max {r.max()}")

    # the eyes: the middle column of the middle chunk, two voxels above its ground; its lowest see-through voxel below the ground; above the world
    ecx, ecz = a.nx // 2, a.nz // 2
    radius = max(ecx, a.nx - 1 - ecx, ecz, a.nz - 1 - ecz)                  # the window covers the grid
    if radius > gen.VISIBLE_MAX_RADIUS:
        sys.exit(f"radius {radius} beyond {gen.VISIBLE_MAX_RADIUS}: choose a smaller region")
    ids = blocks[ecz * a.nx + ecx].cpu().numpy().reshape(16, 16, 384)[8, 8]
    masks = gen.light_masks(blocks)
    T = masks[ecz * a.nx + ecx].cpu().numpy()[:12288].view(np.uint64).reshape(256, 6)[8 + 16 * 8]      # the column's see-through bits
    through = np.array([(int(T[y >> 6]) >> (y & 63)) & 1 for y in range(384)], bool)
    ground = int(np.max(np.nonzero(~through)[0]))
    below = np.nonzero(through[:ground])[0]
    eyes = [("surface", min(ground + 2, 383) >> 4), ("above the world", 24)]
    if len(below):
        eyes.insert(1, (f"cave (y = {int(below[0])}, block {int(ids[below[0]])})", int(below[0]) >> 4))

    mesh = gen.mesh_quads(blocks, a.nx, a.nz)
    q = gen.quad_fields(mesh["quads"][:mesh["total"]])
    chunk_of = np.repeat(np.arange(n), mesh["chunk_quads"].cpu().numpy())
    for name, sy in eyes:
        vis = gen.visible_sections(conn, grid, (ecx, sy, ecz), radius).cpu().numpy()
        cells = vis[radius - ecz:radius - ecz + a.nz, radius - ecx:radius - ecx + a.nx].reshape(-1)      # the grid's cells in slot order
        seen = sum(int(v).bit_count() for v in cells)
        drawn = int(np.count_nonzero((cells[chunk_of] >> (q["y"] >> 4).astype(np.uint32)) & 1))
        print(f"eye {name}, section ({ecx}, {sy}, {ecz}), radius {radius}: {seen} of {24 * n} sections visible ({100.0 * seen / (24 * n):.1f} %), "
              f"{drawn} of {mesh['total']} quads in visible sections ({100.0 * drawn / max(mesh['total'], 1):.1f} %)")

    sy = eyes[0][1]
    for name, fn, kernels in (("section conn", lambda: gen.section_connectivity(blocks, out=conn), ("k_section_conn",)),
                              ("visible set", lambda: gen.visible_sections(conn, grid, (ecx, sy, ecz), radius), ("k_visible_sections",)),
                              ("light masks", lambda: gen.light_masks(blocks, out=masks), ("k_light_masks",)),
                              ("vertex mesher", lambda: gen.create_vbos(blocks, pos, a.nx, a.nz), ("k_mesh_count", "k_mesh_fill"))):
        med, lo, hi = kernel_ms(gen, fn, kernels, a.warmup, a.reps)
        print(f"{name:14s} median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) over {a.reps} runs = {1e3 * med / n:.2f} us per chunk")


if __name__ == "__main__":
    main()
