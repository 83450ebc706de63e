#!/usr/bin/env python3
"""Time of the voxel lighting on the 32 x 32-chunk region that tools/render_view.py --measure and tools/quad_mesh_stats.py
use, beside the vertex mesher's count + fill re-measured in the same process.  Times are the library's own per-kernel profile (events on the launch
stream) over the whole region, after a warm-up, median / min / max over the repeats.  MMGEN_LIB selects an A/B build of the library.

usage: tools/light_stats.py [--cx 1488 --cz -1110 --nx 32 --nz 32 --warmup 5 --reps 30]"""
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
    masks = gen.light_masks(blocks)
    light = gen.light(masks, grid)
    L = light.cpu().numpy()
    print(f"library {pkg.LIB_PATH}")
    print(f"region {a.nx}x{a.nz} chunks at ({a.cx}, {a.cz}): voxels with block light {np.count_nonzero(L & 15)}, with sky light below 15 but above 0 "
          f"{np.count_nonzero(((L >> 4) > 0) & ((L >> 4) < 15))}, digest {int(L.astype(np.uint64).sum())}")
    for name, fn, kernels in (("light masks", lambda: gen.light_masks(blocks, out=masks), ("k_light_masks",)),
                              ("light", lambda: gen.light(masks, grid, out=light), ("k_light",)),
                              ("vertex mesher", lambda: gen.create_vbos(blocks, pos, a.nx, a.nz), ("k_mesh_count", "k_mesh_fill"))):
        med, lo, hi = kernel_ms(gen, fn, kernels, a.warmup, a.reps)
        print(f"{name:14s} median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) over {a.reps} runs = {1e3 * med / n:.2f} us per chunk")


if __name__ == "__main__":
    main()
