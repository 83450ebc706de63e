#!/usr/bin/env python3
"""Size and time of the section-bucketed quad mesh beside the chunk-wide greedy stream (section 6.6) on the 32 x 32-chunk
region that tools/quad_mesh_stats.py and tools/visibility_stats.py use, all in one process: records and bytes per chunk of both streams, count +
fill of both meshers, k_section_draws beside k_visible_sections, and for the three eyes of tools/visibility_stats.py the quads that the draw list
really draws beside the quads of the 64-bit stream whose ORIGIN lies in a visible section (not conservative: section 6.8); and the lit section
stream (section 6.10) on the region lit by mmgen_light: records at four light masks against the unlit stream, bytes per chunk with the light
bytes against mesh + resident light volume, count + fill twice in alternation with the unlit section mesher; and the AO section stream
(section 6.11): records at three light masks against the lit and the unlit stream, count + fill twice in alternation with the lit mesher, and
both on a flat world where nothing occludes and the two emit the same records.  Times are the
library's own per-kernel profile over the whole region, after a warm-up, median / min / max over the repeats.  MMGEN_LIB selects an A/B build.

usage: tools/section_mesh_stats.py [--cx 1488 --cz -1110 --nx 32 --nz 32 --warmup 5 --reps 30]"""
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
    print(f"library {pkg.LIB_PATH}")

    greedy = gen.mesh_quads(blocks, a.nx, a.nz)
    sec = gen.mesh_section_quads(blocks, a.nx, a.nz)
    gq, sq = greedy["chunk_quads"].cpu().numpy(), sec["chunk_quads"].cpu().numpy()
    secq = sec["section_quads"].cpu().numpy()
    f = gen.section_quad_fields(sec["quads"])
    area = ((f["w"] + 1) * (f["l"] + 1))[f["kind"] < 6]
    print(f"region {a.nx}x{a.nz} chunks at ({a.cx}, {a.cz}): greedy stream {gq.mean():.1f} records per chunk (max {gq.max()}) = {8.0 * gq.mean():.0f} bytes; "
          f"section stream {sq.mean():.1f} records per chunk (max {sq.max()}) = {4.0 * sq.mean():.0f} bytes; records x {sq.sum() / gq.sum():.3f}, bytes x "
          f"{4.0 * sq.sum() / (8.0 * gq.sum()):.3f}; {area.mean():.2f} unit faces per section quad; {np.count_nonzero(secq)} of {24 * n} sections have records, "
          f"largest section {secq.max()}")

    # the lit section stream: how much light-aware merging splits this terrain
    light = gen.light(gen.light_masks(blocks), grid)
    for mask in (0xFF, 0xF0, 0xCC, 0x00):
        lit = gen.mesh_lit_section_quads(blocks, light, a.nx, a.nz, light_mask=mask)
        lq = lit["chunk_quads"].cpu().numpy()
        same = mask != 0 or (t.equal(lit["quads"], sec["quads"]) and not bool(lit["quad_light"].any()))
        print(f"lit section stream, light_mask 0x{mask:02X}: {lit['total']} records = x {lit['total'] / max(sec['total'], 1):.4f} of the unlit {sec['total']}; "
              f"{lq.mean():.1f} per chunk (max {lq.max()}) = {5.0 * lq.mean():.0f} bytes with the light bytes, against {4.0 * sq.mean():.0f} + 98304 = "
              f"{4.0 * sq.mean() + 98304:.0f} for mesh + light volume (x {5.0 * lq.mean() / (4.0 * sq.mean() + 98304):.4f})"
              + ("" if mask else f"; equals the unlit stream: {same}"))

    # the AO section stream: what corner occlusion splits on top of the light
    for mask in (0xFF, 0xF0, 0x00):
        ao = gen.mesh_ao_section_quads(blocks, light if mask else None, a.nx, a.nz, light_mask=mask)
        lit = gen.mesh_lit_section_quads(blocks, light, a.nx, a.nz, light_mask=mask)
        aq = ao["chunk_quads"].cpu().numpy()
        print(f"AO section stream, light_mask 0x{mask:02X}: {ao['total']} records = x {ao['total'] / max(lit['total'], 1):.4f} of the lit {lit['total']}, x "
              f"{ao['total'] / max(sec['total'], 1):.4f} of the unlit {sec['total']}; {aq.mean():.1f} per chunk (max {aq.max()}) = {6.0 * aq.mean():.0f} bytes with "
              f"light and AO bytes; {100.0 * float((ao['quad_ao'] == 0xFF).float().mean()):.1f} % of the records unoccluded")
    flat = t.zeros_like(blocks).reshape(n, 256, 384)
    flat[:, :, :64] = 57
    flat = flat.reshape(n, -1)
    fl = gen.light(gen.light_masks(flat), grid)
    fa, fb = gen.mesh_ao_section_quads(flat, fl, a.nx, a.nz), gen.mesh_lit_section_quads(flat, fl, a.nx, a.nz)
    print(f"flat world (rock below y = 64): AO stream {fa['total']} records, lit stream {fb['total']}; equal records and light: "
          f"{t.equal(fa['quads'], fb['quads']) and t.equal(fa['quad_light'], fb['quad_light'])}; all unoccluded: {bool((fa['quad_ao'] == 0xFF).all())}")

    # the eyes of tools/visibility_stats.py: the middle column of the middle chunk, two voxels above its ground; its lowest see-through voxel; above the world
    ecx, ecz = a.nx // 2, a.nz // 2
    radius = max(ecx, a.nx - 1 - ecx, ecz, a.nz - 1 - ecz)
    if radius > gen.VISIBLE_MAX_RADIUS:
        sys.exit(f"radius {radius} beyond {gen.VISIBLE_MAX_RADIUS}: choose a smaller region")
    T = gen.light_masks(blocks)[ecz * a.nx + ecx].cpu().numpy()[:12288].view(np.uint64).reshape(256, 6)[8 + 16 * 8]
    through = np.array([(int(T[y >> 6]) >> (y & 63)) & 1 for y in range(384)], bool)
    ground = int(np.max(np.nonzero(~through)[0]))
    below = np.nonzero(through[:ground])[0]
    eyes = [("surface", min(ground + 2, 383) >> 4), ("above the world", 24)]
    if len(below):
        eyes.insert(1, (f"cave (y = {int(below[0])})", int(below[0]) >> 4))
    conn = gen.section_connectivity(blocks)
    q = gen.quad_fields(greedy["quads"])
    chunk_of = np.repeat(np.arange(n), gq)
    for name, sy in eyes:
        vis = gen.visible_sections(conn, grid, (ecx, sy, ecz), radius)
        d = gen.section_draws(vis, grid, (ecx, ecz), radius, sec)
        cells = vis.cpu().numpy()[radius - ecz:radius - ecz + a.nz, radius - ecx:radius - ecx + a.nx].reshape(-1)
        by_origin = int(np.count_nonzero((cells[chunk_of] >> (q["y"] >> 4).astype(np.uint32)) & 1))
        print(f"eye {name}, section ({ecx}, {sy}, {ecz}), radius {radius}: {d['totals'][0]} draws, {d['totals'][1]} of {sec['total']} section quads drawn "
              f"({100.0 * d['totals'][1] / max(sec['total'], 1):.1f} %) = {4 * d['totals'][1]} bytes; greedy stream by origin {by_origin} of {greedy['total']} "
              f"({100.0 * by_origin / max(greedy['total'], 1):.1f} %) = {8 * by_origin} bytes")

    vis = gen.visible_sections(conn, grid, (ecx, eyes[0][1], ecz), radius)
    for name, fn, kernels in (("section mesher", lambda: gen.mesh_section_quads(blocks, a.nx, a.nz), ("k_section_quads_count", "k_section_quads_fill")),
                              ("  its count", lambda: gen.mesh_section_quads(blocks, a.nx, a.nz), ("k_section_quads_count",)),
                              ("greedy mesher", lambda: gen.mesh_quads(blocks, a.nx, a.nz), ("k_quads_count", "k_quads_fill")),
                              ("  its count", lambda: gen.mesh_quads(blocks, a.nx, a.nz), ("k_quads_count",)),
                              ("section mesher", lambda: gen.mesh_section_quads(blocks, a.nx, a.nz), ("k_section_quads_count", "k_section_quads_fill")),
                              ("greedy mesher", lambda: gen.mesh_quads(blocks, a.nx, a.nz), ("k_quads_count", "k_quads_fill")),
                              ("lit section mesher", lambda: gen.mesh_lit_section_quads(blocks, light, a.nx, a.nz), ("k_lit_section_quads_count", "k_lit_section_quads_fill")),
                              ("  its count", lambda: gen.mesh_lit_section_quads(blocks, light, a.nx, a.nz), ("k_lit_section_quads_count",)),
                              ("section mesher", lambda: gen.mesh_section_quads(blocks, a.nx, a.nz), ("k_section_quads_count", "k_section_quads_fill")),
                              ("lit section mesher", lambda: gen.mesh_lit_section_quads(blocks, light, a.nx, a.nz), ("k_lit_section_quads_count", "k_lit_section_quads_fill")),
                              ("section mesher", lambda: gen.mesh_section_quads(blocks, a.nx, a.nz), ("k_section_quads_count", "k_section_quads_fill")),
                              # A/B: at light_mask 0 the lit kernels emit the unlit records, so what is left over the unlit mesher is the six staged passes
                              ("lit, mask 0x00", lambda: gen.mesh_lit_section_quads(blocks, light, a.nx, a.nz, light_mask=0), ("k_lit_section_quads_count", "k_lit_section_quads_fill")),
                              ("  its count", lambda: gen.mesh_lit_section_quads(blocks, light, a.nx, a.nz, light_mask=0), ("k_lit_section_quads_count",)),
                              ("AO section mesher", lambda: gen.mesh_ao_section_quads(blocks, light, a.nx, a.nz), ("k_ao_section_quads_count", "k_ao_section_quads_fill")),
                              ("  its count", lambda: gen.mesh_ao_section_quads(blocks, light, a.nx, a.nz), ("k_ao_section_quads_count",)),
                              ("lit section mesher", lambda: gen.mesh_lit_section_quads(blocks, light, a.nx, a.nz), ("k_lit_section_quads_count", "k_lit_section_quads_fill")),
                              ("AO section mesher", lambda: gen.mesh_ao_section_quads(blocks, light, a.nx, a.nz), ("k_ao_section_quads_count", "k_ao_section_quads_fill")),
                              ("lit section mesher", lambda: gen.mesh_lit_section_quads(blocks, light, a.nx, a.nz), ("k_lit_section_quads_count", "k_lit_section_quads_fill")),
                              ("AO, mask 0x00", lambda: gen.mesh_ao_section_quads(blocks, None, a.nx, a.nz, light_mask=0), ("k_ao_section_quads_count", "k_ao_section_quads_fill")),
                              # A/B: on the flat world nothing occludes and both emit the same records: what is left is the structure (halo, AO equality, AO bytes)
                              ("AO, flat world", lambda: gen.mesh_ao_section_quads(flat, fl, a.nx, a.nz), ("k_ao_section_quads_count", "k_ao_section_quads_fill")),
                              ("lit, flat world", lambda: gen.mesh_lit_section_quads(flat, fl, a.nx, a.nz), ("k_lit_section_quads_count", "k_lit_section_quads_fill")),
                              ("draw list", lambda: gen.section_draws(vis, grid, (ecx, ecz), radius, sec), ("k_section_draws",)),
                              ("visible set", lambda: gen.visible_sections(conn, grid, (ecx, eyes[0][1], ecz), radius), ("k_visible_sections",))):
        med, lo, hi = kernel_ms(gen, fn, kernels, a.warmup, a.reps)
        print(f"{name:18s} median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) over {a.reps} runs = {1e3 * med / n:.2f} us per chunk")


if __name__ == "__main__":
    main()
