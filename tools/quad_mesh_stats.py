#!/usr/bin/env python3
"""Size and time of the greedy quad mesh against the reference-exact vertex mesh on the seed-0 32 x 32-chunk region that
tools/render_view.py --measure uses.  Sizes are exact counts; times are the library's own per-kernel profile (events on the launch stream),
count + fill of either mesher over the whole region, after a warm-up, median / min / max over the repeats.

usage: tools/quad_mesh_stats.py [--cx 1488 --cz -1110 --nx 32 --nz 32 --warmup 5 --reps 30]"""
import argparse
import ctypes
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_ms(gen, fn, names, warmup, reps):
    """milliseconds per call of fn spent in the kernels `names`, from the library's profile hooks: one sample per repeat"""
    lib = gen.lib
    lib.mmgen_profile_kernel_name.restype = ctypes.c_char_p
    n = lib.mmgen_profile_num_kernels()
    ids = [i for i in range(n) if lib.mmgen_profile_kernel_name(i).decode() in names]
    assert len(ids) == len(names), names
    ms, cnt = (ctypes.c_double * n)(), (ctypes.c_longlong * n)()
    for _ in range(warmup):
        fn()
    lib.mmgen_profile_enable(1)
    lib.mmgen_profile_collect(ms, cnt)
    out = []
    for _ in range(reps):
        fn()
        assert lib.mmgen_profile_collect(ms, cnt) == 0
        out.append(sum(ms[i] for i in ids))
    lib.mmgen_profile_enable(0)
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cx", type=int, default=1488); ap.add_argument("--cz", type=int, default=-1110)
    ap.add_argument("--nx", type=int, default=32); ap.add_argument("--nz", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    gen = importlib.import_module("mega-minecraft_amd").MMGen(0)
    t = gen.torch
    blocks = gen.generate_region(a.cx, a.cz, a.nx, a.nz)["blocks"]
    n = a.nx * a.nz
    pos = t.zeros((n, 2), dtype=t.int32, device=gen.device)
    q = gen.mesh_quads(blocks, a.nx, a.nz)
    v = gen.create_vbos(blocks, pos, a.nx, a.nz)
    per = q["chunk_quads"].cpu().numpy()
    verts = v["chunk_verts"].cpu().numpy().astype(np.int64)
    f = gen.quad_fields(q["quads"])
    area = ((f["dx"] + 1) * (f["dy"] + 1) * (f["dz"] + 1))[f["kind"] < 6]
    qb, vb = 8.0 * per.mean(), (40.0 + 6.0) * verts.mean()      # 40-byte vertices, 3/2 four-byte indices per vertex
    print(f"region {a.nx}x{a.nz} chunks at ({a.cx}, {a.cz}): records per chunk mean {per.mean():.1f} max {per.max()}, unit faces per quad {area.mean():.2f}")
    print(f"bytes per chunk: quad stream {qb:.0f}, vertices + indices {vb:.0f} ({vb / qb:.1f}x)")
    for name, fn, kernels in (("quad mesher", lambda: gen.mesh_quads(blocks, a.nx, a.nz), ("k_quads_count", "k_quads_fill")),
                              ("vertex mesher", lambda: gen.create_vbos(blocks, pos, a.nx, a.nz), ("k_mesh_count", "k_mesh_fill"))):
        med, lo, hi = kernel_ms(gen, fn, kernels, a.warmup, a.reps)
        print(f"{name:14s} count + fill: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) over {a.reps} runs = {1e3 * med / n:.2f} us per chunk")


if __name__ == "__main__":
    main()
