"""GPU tests of mmgen_render_camera (include/mmgen.h "shaded camera render") against a numpy restatement of "Shading" and "The pixel".  The
restatement takes the A, B and S hit records from MMGen.raycast, which tests/test_gpu_raycast.py holds to a numpy walk of the traversal
contract; everything else is integer numpy plus the two f32 expressions.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from test_gpu_raycast import HIT, assert_records_equal, block_classes, camera_rays

pytestmark = pytest.mark.gpu

AO, TRANSLUCENT, SUN_SHADOW, FOG = 1, 2, 4, 8
T_MAX = 200.0
GRID = np.array([[0, 1, 2], [3, 4, 5], [6, 7, -1]], np.int32)      # the corner cell (2, 2) is absent
DIRV = np.array([[0, 0, 1], [1, 0, 0], [0, 0, -1], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0]])
ER = np.array([[1, 0, 0], [0, 0, 1], [1, 0, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0]])      # row axis r of a face's plane
EQ = np.array([[0, 1, 0]] * 4 + [[1, 0, 0]] * 2 + [[0, 0, 0]])                                     # fast axis q
RAMP = np.array([9, 11, 14, 18, 22, 27, 34, 43, 53, 67, 84, 104, 131, 163, 204, 255])
FACE = np.array([204, 179, 153, 179, 255, 115, 255])
AOW = np.array([115, 153, 204, 255])
PAR = dict(sun_dir=(0.45, 0.8, 0.3), fog_start=10.0, fog_end=60.0, sky_rgb=(150, 190, 235), sun_level=13, shadow_dim=140)
CAMS = {
    "oblique": dict(eye=(2.3, 76.7, 12.2), forward=(0.62, -0.55, 0.5), up=(0.0, 1.0, 0.0), fov_y=1.0),
    "in_water": dict(eye=(8.5, 60.5, 25.5), forward=(1.0, 0.2, 0.3), up=(0.0, 1.0, 0.0), fov_y=1.0),      # A is a HIT at t = 0, face 6
    "room": dict(eye=(21.5, 56.5, 5.5), forward=(1.0, -0.1, 0.6), up=(0.0, 1.0, 0.0), fov_y=1.2),         # block light, no sky
    "sky": dict(eye=(40.5, 70.5, 8.5), forward=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0), fov_y=1.0),
    "absent": dict(eye=(30.5, 66.5, 30.5), forward=(1.0, -0.15, 1.0), up=(0.0, 1.0, 0.0), fov_y=1.0),     # towards the absent cell
}
CAMS = {k: dict(v, width=40, height=24) for k, v in CAMS.items()}                                         # partial tiles on both axes


@functools.lru_cache(None)
def scene():
    """[slot][98304]: a stone slab, a water pool with a stone floor, an overhang, a closed room with a glowstone, a curb, leaves and a poppy"""
    w = np.zeros((48, 48, 384), np.uint8)                  # [z][x][y]
    w[:, :, 50:64] = 57                                    # the slab, top at y = 63
    w[20:32, 4:16, 58:64] = 1                              # the pool: six deep, stone below
    w[4:12, 20:28, 54:60] = 0                              # the room under the slab
    w[7, 23, 54] = 121                                     # ... and its glowstone
    w[20:22, 30:32, 64:72] = 57                            # a pillar
    w[14:28, 18:34, 72] = 57                               # ... that carries a roof: the sun shadow on the slab and the pool
    w[18:20, 4:20, 64] = 57                                # a curb along the pool, steps behind it: corner occlusion
    w[33, 6:14, 64:66] = 57
    w[30, 18, 64], w[30, 20, 64] = 87, 16                  # JUNGLE_LEAVES (SEMI) and a POPPY (X-shaped) on the slab
    return np.ascontiguousarray(w.reshape(3, 16, 3, 16, 384).transpose(0, 2, 1, 3, 4).reshape(9, 98304)[:8])


def fetch(vol, p, outside):
    """vol[slot][98304] at the voxels p [n][3]; `outside` where p lies outside the grid, in the absent cell or outside 0 <= y <= 383"""
    x, y, z = p.T
    ok = (x >= 0) & (x < 48) & (z >= 0) & (z < 48) & (y >= 0) & (y < 384)
    g = np.where(ok, GRID[np.clip(z, 0, 47) >> 4, np.clip(x, 0, 47) >> 4], -1)
    return np.where(g >= 0, vol[np.maximum(g, 0), np.clip(y, 0, 383) + 384 * ((x & 15) + 16 * (z & 15))], outside)


def mul8(a, b):
    return (a * b + 127) // 255


def shade(H, light, pal, sun_level):
    f = H["voxel"].astype(np.int64) + DIRV[H["face"]]
    L = np.full(len(H), 0xF0) if light is None else np.where(f[:, 1] > 383, 0xF0, np.where(f[:, 1] < 0, 0, fetch(light, f, 0))).astype(np.int64)
    lv = np.maximum((L >> 4) * sun_level // 15, L & 15)
    c = (pal[H["block"]].astype(np.int64)[:, None] >> np.array([0, 8, 16])) & 255
    return mul8(mul8(c, RAMP[lv][:, None]), FACE[H["face"]][:, None])


def ao_factor(blocks, H, rays):
    cls, face, v = block_classes(), H["face"], H["voxel"].astype(np.int64)
    f, er, eq = v + DIRV[face], ER[face], EQ[face]
    h = rays[:, :3] + H["t"][:, None] * rays[:, 3:]        # float32: one multiply, one add
    u = np.clip(np.floor((h - v.astype(np.float32)) * np.float32(16)).astype(np.int64), 0, 15)
    ur, uq, total = (u * er).sum(1), (u * eq).sum(1), 0
    occ = lambda p: (cls[fetch(blocks, p, 0)] == 1).astype(np.int64)
    for k in range(4):
        sr, sq = (1 if k & 2 else -1), (1 if k & 1 else -1)
        s1, s2, c = occ(f + sr * er), occ(f + sq * eq), occ(f + sr * er + sq * eq)
        ao = np.where((s1 & s2) == 1, 0, 3 - (s1 + s2 + c))
        total = total + (2 * ur + 1 if sr > 0 else 31 - 2 * ur) * (2 * uq + 1 if sq > 0 else 31 - 2 * uq) * AOW[ao]
    return (total + 512) >> 10


def reference(cast, blocks, light, pal, cam, flags, first_mask=15):
    """cast(rays [n][6], stop_mask) -> hit records.  Returns the RGBA words [n], walk A's records and what the image exercised."""
    cls, sky, f32 = block_classes(), np.array(PAR["sky_rgb"], np.int64), np.float32
    rays = camera_rays(**cam)
    A = cast(rays, first_mask)
    hit = np.flatnonzero(A["status"] == HIT)
    Ah, rh = A[hit], rays[hit]
    C = shade(Ah, light, pal, PAR["sun_level"])
    seen = dict(b_hit=0, shadowed=0, ao_dark=0, fog_mid=0)
    if flags & AO:
        m = (Ah["face"] != 6) & ((cls[Ah["block"]] & 3) != 0)
        a = ao_factor(blocks, Ah[m], rh[m])
        C[m], seen["ao_dark"] = mul8(C[m], a[:, None]), int((a < 255).sum())
    if flags & SUN_SHADOW:
        m = np.flatnonzero(Ah["face"] != 6)
        o = (Ah["voxel"][m] + DIRV[Ah["face"][m]]).astype(f32) + f32(0.5)
        S = cast(np.concatenate([o, np.broadcast_to(f32(PAR["sun_dir"]), o.shape)], 1), 3)
        m = m[S["status"] == HIT]
        C[m], seen["shadowed"] = mul8(C[m], PAR["shadow_dim"]), len(m)
    if flags & TRANSLUCENT:
        m = np.flatnonzero(cls[Ah["block"]] == 4)
        B = cast(rh[m], 3)
        back, bh = np.broadcast_to(sky, (len(m), 3)).copy(), B["status"] == HIT
        back[bh], seen["b_hit"] = shade(B[bh], light, pal, PAR["sun_level"]), int(bh.sum())
        al = (pal[Ah["block"][m]].astype(np.int64) >> 24)[:, None]
        C[m] = (C[m] * al + back * (255 - al) + 127) // 255
    if flags & FOG:
        x = (Ah["t"] - f32(PAR["fog_start"])) * (f32(1) / (f32(PAR["fog_end"]) - f32(PAR["fog_start"])))
        g = (np.fmin(np.fmax(x, f32(0)), f32(1)) * f32(255) + f32(0.5)).astype(np.int64)[:, None]
        C, seen["fog_mid"] = (C * (255 - g) + sky * g + 127) // 255, int(((g > 0) & (g < 255)).sum())
    rgb = np.broadcast_to(sky, (len(rays), 3)).copy()
    rgb[hit] = C
    alpha = np.where(A["status"] == HIT, 255, 0)
    return (rgb[:, 0] | rgb[:, 1] << 8 | rgb[:, 2] << 16 | alpha << 24).astype(np.uint32), A, seen


@functools.lru_cache(None)
def on_device(gen):
    t = gen.torch
    blocks, grid = t.from_numpy(scene()).to(gen.device), t.from_numpy(GRID).to(gen.device)
    light = gen.light(gen.light_masks(blocks), grid)
    return dict(blocks=blocks, grid=grid, light=light, light_host=light.cpu().numpy(), occ={m: gen.ray_occupancy(blocks, m) for m in (15, 3, 1)})


def check(gen, cam, flags, lit, first_mask=15, palette=None):
    dev, t = on_device(gen), gen.torch
    pal = gen.render_default_palette() if palette is None else palette
    cast = lambda rays, mask: gen.ray_hits(gen.raycast(dev["blocks"], dev["grid"], dev["occ"][mask], t.from_numpy(np.ascontiguousarray(rays)).to(gen.device),
                                                       mask, T_MAX))
    ref, A, seen = reference(cast, scene(), dev["light_host"] if lit else None, pal, CAMS[cam], flags, first_mask)
    rgba, hits = gen.render_camera(dev["blocks"], dev["grid"], dev["occ"][first_mask], occ_second=dev["occ"][3], light=dev["light"] if lit else None,
                                   palette=None if palette is None else t.from_numpy(palette.view(np.int32)).to(gen.device), flags=flags,
                                   first_mask=first_mask, t_max=T_MAX, return_hits=True, **CAMS[cam], **PAR)
    assert_records_equal(gen.ray_hits(hits).reshape(-1), A)
    got = rgba.cpu().numpy().view(np.uint32).reshape(-1)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"{bad.size} pixels differ, first {bad[0]}: {got[bad[0]]:08x} vs {ref[bad[0]]:08x}, record {A[bad[0]]}"
    return A, seen


@pytest.mark.parametrize("lit", [False, True], ids=["full_bright", "light_volume"])
@pytest.mark.parametrize("flags", [0, AO, TRANSLUCENT, SUN_SHADOW, FOG, 15])
@pytest.mark.parametrize("cam", list(CAMS))
def test_image_equals_the_restatement(gen, cam, flags, lit):
    A, seen = check(gen, cam, flags, lit)
    if cam == "oblique" and flags == 15:                   # the image must exercise what it claims to test
        assert seen["b_hit"] >= 20 and seen["shadowed"] >= 20 and seen["ao_dark"] >= 20 and seen["fog_mid"] >= 5, seen
    if cam == "in_water":
        assert (A["status"] == HIT).all() and (A["t"] == 0).all() and (A["face"] == 6).all()
    if cam in ("sky", "absent"):
        assert (A["status"] != HIT).any()
    if cam == "room" and lit and flags == 0:               # the room is seen by its glowstone alone: neither black nor full bright
        levels = np.unique(on_device(gen)["light_host"][1].reshape(16, 16, 384)[4:12, 4:12, 54:60])
        assert levels.max() <= 15 and len(levels) > 4


def test_first_mask_opaque_sees_through_water_and_leaves(gen):
    A, seen = check(gen, "oblique", 15, True, first_mask=1)
    assert seen["b_hit"] == 0 and 1 not in A["block"] and seen["shadowed"] >= 20


def test_custom_palette(gen):
    rng = np.random.default_rng(0)
    check(gen, "oblique", 15, True, palette=rng.integers(0, 1 << 32, 256, dtype=np.uint64).astype(np.uint32))


def test_error_returns(gen):
    dev, kw = on_device(gen), dict(CAMS["oblique"], **PAR)
    args = (dev["blocks"], dev["grid"], dev["occ"][15])
    for bad in (dict(first_mask=2), dict(first_mask=17), dict(sun_level=16), dict(flags=16), dict(flags=TRANSLUCENT), dict(flags=SUN_SHADOW),
                dict(flags=FOG, fog_end=10.0), dict(flags=FOG, fog_start=float("nan")), dict(flags=FOG, fog_end=float("inf")),
                dict(flags=SUN_SHADOW, occ_second=dev["occ"][3], sun_dir=(0.0, 0.0, 0.0)),
                dict(flags=SUN_SHADOW, occ_second=dev["occ"][3], sun_dir=(0.0, float("inf"), 0.0)), dict(t_max=-1.0), dict(fov_y=0.0), dict(width=0)):
        with pytest.raises(RuntimeError, match="mmgen_render_camera"):
            gen.render_camera(*args, **dict(kw, **bad))
    with pytest.raises(RuntimeError, match="mmgen_render_camera"):
        gen.render_camera(dev["blocks"], dev["grid"], None, **kw)
    gen.render_camera(*args, **kw)                         # the same arguments with nothing wrong
