#!/usr/bin/env python3
"""Headless preview of a generated region through the ray caster (include/mmgen.h): generates nx x nz chunks, builds the occupancy, casts
one primary ray per pixel (mmgen_raycast_camera) and one shadow ray per hit towards a fixed sun (mmgen_raycast), shades on the host from
block id, face and shadow, and writes <out>.ppm (binary P6) and <out>.npy (the hit records).  No image library.

usage: tools/render_view.py [--cx 1488 --cz -1110 --nx 8 --nz 8] [--eye surface|cave|x,y,z] [--forward x,y,z] [--size 1280x720] [--out view]
       tools/render_view.py --light ...   # shade by the light volume (mmgen_light): max(sky, block) / 15 of the voxel in front of the hit face
       tools/render_view.py --device ...  # the whole image on the device (mmgen_render_camera): light, AO, water, sun shadow, fog
       tools/render_view.py --measure     # both eyes, skip / no-skip, occupancy build, visits per ray; section 6.13: the
                                          # host-shaded path against mmgen_raycast_camera alone and mmgen_render_camera (--warmup, --reps)
Eye and forward are in grid-local block coordinates (x, z from the region's corner, y = world y)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SUN = np.array([0.45, 0.8, 0.3], np.float32)
NORMAL = np.array([[0, 0, 1], [1, 0, 0], [0, 0, -1], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0]], np.float32)      # dirVecs, then "none"
FACE_LIGHT = np.array([0.8, 0.7, 0.6, 0.7, 1.0, 0.45, 1.0], np.float32)
SKY = np.array([150, 190, 235], np.float32)


def palette():
    """a colour per block id: a few named ones, the rest a grey-brown spread by id (enough to tell materials apart in a preview)"""
    ids = np.arange(256)
    pal = np.stack([110 + (ids * 37) % 60, 100 + (ids * 53) % 50, 90 + (ids * 29) % 40], 1).astype(np.float32)
    named = {1: (40, 90, 200), 2: (230, 90, 20), 57: (125, 125, 125), 58: (120, 85, 60), 59: (90, 160, 70), 60: (220, 205, 150), 61: (140, 135, 130),
             63: (240, 245, 250), 64: (225, 235, 240), 78: (200, 110, 60), 81: (70, 150, 50), 87: (40, 120, 40), 88: (60, 130, 40), 103: (170, 210, 245),
             106: (170, 165, 80), 108: (100, 160, 80), 115: (40, 90, 60), 121: (250, 220, 120)}
    for k, c in named.items():
        pal[k] = c
    pal[3:56, 1] += 60                                     # plants and decorators lean green
    return np.clip(pal, 0, 255)


def eye_for(kind, blocks_host, nx, nz):
    """'surface': 30 blocks above the topmost block of the region's centre column; 'cave': the tallest run of air below a roof in the
    four centre chunks (the eye sits in its lower third)"""
    cx, cz = nx // 2, nz // 2
    if kind == "surface":
        col = blocks_host[cx + nx * cz].reshape(16, 16, 384)[0, 0]
        return (16.0 * cx + 0.5, float(383 - np.argmax(col[::-1] != 0)) + 30.5, 16.0 * cz + 0.5)
    best = (0, None)
    for dz in (0, -1):
        for dx in (0, -1):
            c = blocks_host[(cx + dx) + nx * (cz + dz)].reshape(16, 16, 384)
            air = c[:, :, 12:110] == 0
            roof = np.cumsum((c[:, :, ::-1] != 0), 2)[:, :, ::-1][:, :, 12:110] > 8      # at least 8 solid blocks somewhere above
            run = np.zeros(air.shape[:2], int)
            for y in range(air.shape[2]):
                run = np.where(air[:, :, y] & roof[:, :, y], run + 1, 0)
                if run.max() > best[0]:
                    z, x = np.unravel_index(np.argmax(run), run.shape)
                    best = (int(run.max()), (16.0 * (cx + dx) + int(x) + 0.5, 12.0 + y - 2 * int(run.max()) // 3 + 0.5, 16.0 * (cz + dz) + int(z) + 0.5))
    if best[1] is None:
        raise SystemExit("no cave below the centre chunks of this region")
    return best[1]


def shade_by_light(gen, hits, light, grid):
    """--light: a hit is shaded by the light volume (mmgen_light) at the voxel in front of the face that was entered, max(sky, block) / 15"""
    H = gen.ray_hits(hits)
    hit = H["status"] == gen.RAY_HIT
    v = H["voxel"][hit] + NORMAL[H["face"][hit]].astype(np.int32)
    gh, gw = grid.shape
    inside = (v[:, 0] >= 0) & (v[:, 0] < 16 * gw) & (v[:, 2] >= 0) & (v[:, 2] < 16 * gh) & (v[:, 1] >= 0) & (v[:, 1] < 384)
    vi = np.where(inside[:, None], v, 0)
    b = light[grid[vi[:, 2] >> 4, vi[:, 0] >> 4], vi[:, 1] + 384 * ((vi[:, 0] & 15) + 16 * (vi[:, 2] & 15))]
    level = np.where(inside, np.maximum(b >> 4, b & 15), np.where(v[:, 1] > 383, 15, 0)).astype(np.float32)
    img = np.broadcast_to(SKY, H.shape + (3,)).copy()
    img[hit] = palette()[H["block"][hit]] * (level / 15.0)[:, None]
    return np.clip(img, 0, 255).astype(np.uint8), H


def shade(gen, blocks, grid, occ, hits, eye, rays_d, t_max):
    H = gen.ray_hits(hits)
    h, w = H.shape
    hit = H["status"] == gen.RAY_HIT
    n = NORMAL[H["face"]]
    p = np.float32(eye) + H["t"][..., None] * rays_d + 0.01 * n      # just outside the face that was entered
    shadow_rays = np.concatenate([p, np.broadcast_to(SUN, p.shape)], 2).astype(np.float32)[hit]
    lit = np.ones(int(hit.sum()), bool)
    if len(shadow_rays):
        S = gen.ray_hits(gen.raycast(blocks, grid, occ, gen.torch.from_numpy(shadow_rays).to(gen.device), 15, t_max))
        lit = S["status"] != gen.RAY_HIT
    img = np.broadcast_to(SKY, (h, w, 3)).copy()
    base = palette()[H["block"][hit]] * FACE_LIGHT[H["face"][hit]][:, None]
    img[hit] = base * np.where(lit, 1.0, 0.55)[:, None]
    return np.clip(img, 0, 255).astype(np.uint8), H


def pixel_dirs(forward, up, fov_y, width, height):
    """directions of the camera's rays for the host-side hit points (float64 is fine here: only the shading uses them)"""
    f = np.array(forward, float) / np.linalg.norm(forward)
    r = np.cross(f, up); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    th = np.tan(0.5 * fov_y)
    sx = ((np.arange(width) + 0.5) * 2 / width - 1)[None, :, None] * th * width / height
    sy = (1 - (np.arange(height) + 0.5) * 2 / height)[:, None, None] * th
    return (f + sx * r + sy * u).astype(np.float32)


def timed(gen, fn, warmup=10, reps=200):
    """milliseconds per call from device events around each call (on the stream the library launches on): median, min, max"""
    t = gen.torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def wall_ms(gen, fn, warmup, reps):
    """milliseconds per call on the host clock, the device idle before and after each call (a path that ends in numpy has no device event
    at its end): median, min, max"""
    sync = gen.torch.cuda.synchronize
    ms = []
    for k in range(warmup + reps):
        sync(); t0 = time.perf_counter(); fn(); sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms = ms[warmup:]
    return float(np.median(ms)), min(ms), max(ms)


def device_kwargs(gen, blocks, grid, flags):
    """what mmgen_render_camera needs beside the first occupancy: the occupancy of OPAQUE | SEMI and the light volume"""
    return dict(occ_second=gen.ray_occupancy(blocks, 3), light=gen.light(gen.light_masks(blocks), grid), flags=flags, sun_dir=tuple(float(c) for c in SUN),
                fog_start=200.0, fog_end=1500.0, sky_rgb=tuple(int(c) for c in SKY))


def measure_render(gen, args, blocks, grid, occ, eye, forward, w, h):
    """the host-shaded path of this tool (camera kernel, read-back, numpy shading, shadow-ray call) against the camera
    kernel alone and the shaded render with no flag and with all four, one process, the same warm-up and repeats for each"""
    cam = dict(eye=eye, forward=forward, fov_y=1.0, width=w, height=h, t_max=4096.0)
    dirs = pixel_dirs(forward, (0.0, 1.0, 0.0), 1.0, w, h)
    dev = device_kwargs(gen, blocks, grid, 15)
    paths = (("host path: camera + read-back + numpy shading + shadow rays", lambda: shade(gen, blocks, grid, occ, gen.render_view(blocks, grid, occ, **cam), eye, dirs, 4096.0)),
             ("mmgen_raycast_camera alone", lambda: gen.render_view(blocks, grid, occ, **cam)),
             ("mmgen_render_camera flags 0", lambda: gen.render_camera(blocks, grid, occ, **dict(cam, **dict(dev, flags=0)))),
             ("mmgen_render_camera all flags", lambda: gen.render_camera(blocks, grid, occ, **dict(cam, **dev))))
    res = {}
    for name, fn in paths:
        res[name] = wall_ms(gen, fn, args.warmup, args.reps)
        print(f"render {w}x{h}, eye ({eye[0]:.1f}, {eye[1]:.1f}, {eye[2]:.1f}): {name:62s} median {res[name][0]:9.3f} ms (min {res[name][1]:.3f}, max {res[name][2]:.3f}) "
              f"over {args.reps} runs after {args.warmup}")
    m = [res[name][0] for name, _ in paths]
    print(f"render flags 0 / camera alone = {m[2] / m[1]:.3f}; host path / render all flags = {m[0] / m[3]:.1f}")


def measure(gen, args):
    nx = nz = 32
    w, h = 1280, 720
    out = gen.generate_region(args.cx, args.cz, nx, nz)
    blocks = out["blocks"]
    grid = gen.torch.arange(nx * nz, dtype=gen.torch.int32, device=gen.device).reshape(nz, nx)
    occ = gen.ray_occupancy(blocks, 15)
    med, lo, hi = timed(gen, lambda: gen.ray_occupancy(blocks, 15, out=occ))
    print(f"occupancy {nx}x{nz} chunks: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {1e6 * med / (nx * nz):.0f} ns per chunk")
    host = blocks.cpu().numpy()
    for kind, forward in (("surface", (1.0, -0.35, 0.6)), ("cave", (1.0, 0.05, 0.3))):
        eye = eye_for(kind, host, nx, nz)
        cam = dict(eye=eye, forward=forward, fov_y=1.0, width=w, height=h, t_max=4096.0)
        res = {}
        for name, flags in (("skip", 0), ("no_skip", gen.RAY_NO_SKIP)):
            med, lo, hi = timed(gen, lambda: gen.render_view(blocks, grid, occ, flags=flags, **cam))
            C = gen.ray_hits(gen.render_view(blocks, grid, occ, flags=flags | gen.RAY_COUNT_VISITS, **cam))
            res[name] = (med, gen.ray_hits(gen.render_view(blocks, grid, occ, flags=flags, **cam)))
            print(f"{kind:8s} eye ({eye[0]:.1f}, {eye[1]:.1f}, {eye[2]:.1f}) {name:8s} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}) {w * h / med / 1e3:9.1f} Mrays/s   per ray: "
                  f"{C['voxel'][..., 0].mean():.2f} blocks read, {C['voxel'][..., 1].mean():.2f} boxes, {C['voxel'][..., 2].mean():.2f} brick masks; "
                  f"status counts {np.bincount(C['status'].ravel(), minlength=5).tolist()}")
        same = all(np.array_equal(res["skip"][1][f], res["no_skip"][1][f]) for f in ("voxel", "block", "face", "status")) and \
            np.array_equal(res["skip"][1]["t"].view(np.uint32), res["no_skip"][1]["t"].view(np.uint32))
        print(f"{kind:8s} no_skip / skip = {res['no_skip'][0] / res['skip'][0]:.2f}x, images identical: {same}")
        measure_render(gen, args, blocks, grid, occ, eye, forward, w, h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cx", type=int, default=1488); ap.add_argument("--cz", type=int, default=-1110)
    ap.add_argument("--nx", type=int, default=8); ap.add_argument("--nz", type=int, default=8)
    ap.add_argument("--eye", default="surface"); ap.add_argument("--forward", default="1,-0.35,0.6")
    ap.add_argument("--fov", type=float, default=1.0); ap.add_argument("--size", default="1280x720")
    ap.add_argument("--out", default="view"); ap.add_argument("--measure", action="store_true")
    ap.add_argument("--device", action="store_true", help="shade on the device: the PPM is the output of mmgen_render_camera with all four flags")
    ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--light", action="store_true", help="shade by the light volume (sky and block light) instead of face factor and shadow ray")
    args = ap.parse_args()
    gen = importlib.import_module("mega-minecraft_amd").MMGen(0)
    if args.measure:
        return measure(gen, args)
    w, h = (int(v) for v in args.size.split("x"))
    blocks = gen.generate_region(args.cx, args.cz, args.nx, args.nz)["blocks"]
    grid = gen.torch.arange(args.nx * args.nz, dtype=gen.torch.int32, device=gen.device).reshape(args.nz, args.nx)
    occ = gen.ray_occupancy(blocks, 15)
    eye = eye_for(args.eye, blocks.cpu().numpy(), args.nx, args.nz) if args.eye in ("surface", "cave") else tuple(float(v) for v in args.eye.split(","))
    forward = tuple(float(v) for v in args.forward.split(","))
    if args.device:
        rgba, hits = gen.render_camera(blocks, grid, occ, eye, forward, fov_y=args.fov, width=w, height=h, t_max=4096.0, return_hits=True,
                                       **device_kwargs(gen, blocks, grid, 15))
        img, H = np.ascontiguousarray(rgba.cpu().numpy()[..., :3]), gen.ray_hits(hits)
    elif args.light:
        hits = gen.render_view(blocks, grid, occ, eye, forward, fov_y=args.fov, width=w, height=h, t_max=4096.0)
        img, H = shade_by_light(gen, hits, gen.light(gen.light_masks(blocks), grid).cpu().numpy(), grid.cpu().numpy())
    else:
        hits = gen.render_view(blocks, grid, occ, eye, forward, fov_y=args.fov, width=w, height=h, t_max=4096.0)
        img, H = shade(gen, blocks, grid, occ, hits, eye, pixel_dirs(forward, (0.0, 1.0, 0.0), args.fov, w, h), 4096.0)
    with open(args.out + ".ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h)); f.write(img.tobytes())
    np.save(args.out + ".npy", H)
    print(f"{args.out}.ppm {w}x{h}: eye {eye}, {int((H['status'] == gen.RAY_HIT).sum())} of {w * h} pixels hit a block; records in {args.out}.npy")


if __name__ == "__main__":
    main()
