#!/usr/bin/env python3
"""Time and effect of the level-of-detail reduction on the 32 x 32-chunk region that tools/section_mesh_stats.py uses,
for levels 1, 2 and 3 in one process: the time of mmgen_lod_reduce over the whole region (the library's own per-kernel profile, after a
warm-up, median / min / max over the repeats), the bytes it must move (s^2 source slots read, one slot written per LOD chunk) and the rate
that gives, and the records of the section quad mesher on the level-k grid beside the level-0 records of the same area.  MMGEN_LIB selects
an A/B build.

usage: tools/lod_stats.py [--cx 1488 --cz -1110 --nx 32 --nz 32 --warmup 5 --reps 30]"""
import argparse
import hashlib
import importlib
import os
import sys

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
    if a.nx % 8 or a.nz % 8:
        sys.exit("the region must be a multiple of 8 chunks on both sides")
    pkg = importlib.import_module("mega-minecraft_amd")
    gen = pkg.MMGen(0)
    t = gen.torch
    blocks = gen.generate_region(a.cx, a.cz, a.nx, a.nz)["blocks"]
    print(f"library {os.path.relpath(pkg.LIB_PATH, ROOT)} sha16 {hashlib.sha256(open(pkg.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    base = gen.mesh_section_quads(blocks, a.nx, a.nz)["total"]
    print(f"region {a.nx}x{a.nz} chunks at ({a.cx}, {a.cz}): level 0 has {base} section quad records = {4 * base} bytes")
    for level in (1, 2, 3):
        s = 1 << level
        kx, kz = a.nx // s, a.nz // s
        src = t.tensor([[(s * lz + q // s) * a.nx + s * lx + q % s for q in range(s * s)] for lz in range(kz) for lx in range(kx)],
                       dtype=t.int32, device=gen.device)
        lod = gen.lod_reduce(blocks, src, level)
        med, lo, hi = kernel_ms(gen, lambda: gen.lod_reduce(blocks, src, level, out=lod), ("k_lod_reduce",), a.warmup, a.reps)
        moved = kx * kz * (s * s + 1) * 98304
        records = gen.mesh_section_quads(lod, kx, kz)["total"]
        print(f"level {level} (s = {s}): {kx * kz} LOD chunks, {kx * kz * s * s} workgroups; median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}) over {a.reps} runs; "
              f"{moved} bytes = {moved / (1e6 * med):.0f} GB/s; {records} section quad records = x {records / max(base, 1):.4f} of level 0 "
              f"(x {s * s * records / max(base, 1):.3f} per LOD chunk against a level-0 chunk)")


if __name__ == "__main__":
    main()
