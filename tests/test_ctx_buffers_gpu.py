"""The context owns its device and pinned buffers (DESIGN.md "Host state").

vpx_debug_live_buffers counts the allocations the library holds, over every context of the
process.  A context gives everything back in vpx_destroy, a call repeated at one size allocates
nothing more, a replaced table frees the one before it, and a device set returns its members'
buffers.  The last test pins the results of the host batch entries, whose scratch is divided by
one shared carve: a batch equals its rays one at a time, bit for bit.

Every test starts with gc.collect(): a Context an earlier test left unclosed would otherwise be
finalised in the middle of this one and move the count.  The tests work in deltas.
"""
import ctypes as C
import gc
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

X86 = os.uname().machine in ("x86_64", "i686")  # hosts that have VPX_ARITH_X86_HOST
CAM = ((0.5, 0.35, -0.6), (0.5, 0.2, 0.3))
# three sizes of everything: k = 0 small, 1 middle, 2 large
FRAMES = ((9, 5), (17, 9), (33, 17))  # 1 tile, 2 x 1 tiles, 3 x 2 tiles ragged on both edges
GRIDS = (8, 16, 32)
RAYS = (1, 30, 300)


def live(pkg):
    return int(pkg.load_library().vpx_debug_live_buffers())


def cells_of(n):
    """A floor, a block and a pillar in an n^3 grid (z, y, x order)."""
    c = np.zeros((n, n, n), np.uint8)
    c[:, :2, :] = 1
    c[n // 4:n // 2, 2:n // 2, n // 4:n // 2] = 3
    c[n // 2:n // 2 + 2, 2:n - 2, n // 2:n // 2 + 2] = 5
    return c.reshape(-1)


def scene_of(pkg, k, depth=0):
    sc = pkg.scene
    w, h = FRAMES[k]
    grid = sc.GridSpec(n=GRIDS[k], dense=cells_of(GRIDS[k]))
    return sc._scene("buffers", [grid], [sc.volume()], sc.default_materials(), [sc.point_light((0.5, 0.9, 0.3))], [], [],
                     sc.dir_light(), CAM[0], CAM[1], w, h, max_bounces=depth)


def rays_of(pkg, n, seed=7):
    rng = np.random.default_rng(seed)
    o = np.tile(np.float32([0.5, 0.5, -0.4]), (n, 1)) + rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
    d = np.tile(np.float32([0.0, -0.2, 1.0]), (n, 1)) + rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    return pkg.context.make_rays(o, d)


def tris_of(pkg, n):
    rng = np.random.default_rng(n)
    a = rng.uniform(-1, 1, (n, 3))
    v = np.concatenate([a, a + rng.uniform(0, 1, (n, 3)), a + rng.uniform(0, 1, (n, 3))], 1).astype(np.float32)
    tris = (pkg.abi.BvhTri * n)()
    np.frombuffer(tris, np.float32).reshape(-1, 9)[:] = v
    return tris


def dev(n, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype, device="cuda")


# ------------------------------------------------------------------ the calls that allocate
# name -> (call(pkg, ctx, k), the buffers the call itself may add when it has to grow).  The
# number is read off the code: a buffer that grows replaces the one before it, so a call that
# ran before adds nothing at a larger size; the bound is what a first call of its kind brings.
def c_grid(pkg, ctx, k):
    pkg.scene.GridSpec(n=GRIDS[k], dense=cells_of(GRIDS[k])).upload(ctx.lib, ctx.h, 0)


def c_volumes(pkg, ctx, k):
    sc = pkg.scene
    sc.GridSpec(n=GRIDS[k], dense=cells_of(GRIDS[k])).upload(ctx.lib, ctx.h, 1)
    count = (2, 3, 5)[k]  # two grids, a TLAS over the volumes after the first
    vols = [sc.volume()] + [sc.volume(position=(0.1 * i, 1.0, 0.0), scale=(0.3, 0.3, 0.3), grid_id=1) for i in range(1, count)]
    ctx._chk(ctx.lib.vpx_set_volumes(ctx.h, (pkg.abi.Volume * count)(*vols), count), "vpx_set_volumes")


def one_volume(pkg, ctx):
    ctx._chk(ctx.lib.vpx_set_volumes(ctx.h, (pkg.abi.Volume * 1)(pkg.scene.volume()), 1), "vpx_set_volumes")


def c_materials(pkg, ctx, k):
    ctx.set_materials(pkg.scene.default_materials())


def set_lights(pkg, ctx, n):
    sc, abi = pkg.scene, pkg.abi
    pts = (abi.PointLight * max(1, n))(*[sc.point_light((0.5, 0.9, 0.1 * i)) for i in range(n)])
    sps = (abi.SpotLight * max(1, n))(*[sc.spot_light() for _ in range(n)])
    ars = (abi.AreaLight * max(1, n))(*[sc.area_light() for _ in range(n)])
    dl = sc.dir_light()
    ctx._chk(ctx.lib.vpx_set_lights(ctx.h, pts, n, sps, n, ars, n, C.byref(dl)), "vpx_set_lights")


def c_lights(pkg, ctx, k):
    set_lights(pkg, ctx, (1, 2, 4)[k])


def c_shapes(pkg, ctx, k):
    abi, n = pkg.abi, (1, 2, 4)[k]
    v = abi.vec3
    sph = (abi.Sphere * n)(*[abi.Sphere(v((0.5, 1.5, 0.5)), 0.1, 1, (C.c_uint32 * 3)()) for _ in range(n)])
    tri = (abi.Triangle * n)(*[abi.Triangle(v((0.0, 1.5, 0.0)), v((0, 0, 0)), v((0.1, 0, 0)), v((0, 0.1, 0)), 1, (C.c_uint32 * 3)())
                               for _ in range(n)])
    ctx._chk(ctx.lib.vpx_set_shapes(ctx.h, sph, n, tri, n), "vpx_set_shapes")


def no_lights_or_shapes(pkg, ctx):
    sc, abi = pkg.scene, pkg.abi
    pt = (abi.PointLight * 1)(sc.point_light((0.5, 0.9, 0.3)))
    dl = sc.dir_light()
    ctx._chk(ctx.lib.vpx_set_lights(ctx.h, pt, 1, None, 0, None, 0, C.byref(dl)), "vpx_set_lights")
    ctx._chk(ctx.lib.vpx_set_shapes(ctx.h, None, 0, None, 0), "vpx_set_shapes")


def c_sky(pkg, ctx, k):
    w, h = ((8, 4), (16, 8), (32, 16))[k]
    ctx.set_sky(pkg.scene.synthetic_sky(w, h))
    ctx.set_sky(None)


def c_arith(pkg, ctx, k):
    if X86:
        ctx.set_arithmetic(pkg.abi.VPX_ARITH_X86_HOST)
    ctx.set_arithmetic(pkg.abi.VPX_ARITH_EXACT)


def c_bvh(pkg, ctx, k):
    ctx.bvh_set(tris_of(pkg, (2, 16, 64)[k]))


def c_model(pkg, ctx, k):
    s = (2, 4, 8)[k]
    ctx.model_upload(2, (s, s, s), np.full(s * s * s, 3, np.uint8))
    ctx.grid_load_model(3, GRIDS[k], 2)


def c_noise(pkg, ctx, k):
    ctx.grid_generate_noise(4, GRIDS[k])


def c_brush(pkg, ctx, k):
    n = GRIDS[k]
    ctx.grid_brush(0, [pkg.scene.sphere_brush((n // 2, n // 2, n // 2), (n // 4) ** 2, 2)])


def c_write_box(pkg, ctx, k):
    s = (2, 4, 8)[k]
    ctx.grid_write_box(0, np.full((s, s, s), 4, np.uint8), (0, 2, 0))


def c_tiled(pkg, ctx, k):
    m = (1, 2, 3)[k]
    spec = pkg.scene.GridSpec(n=GRIDS[k], model=np.full(m * m * m, 2, np.uint8), model_dims=(m, m, m), period=(2 * m, 2 * m, 2 * m))
    spec.upload(ctx.lib, ctx.h, 5)


def frame(pkg, k, depth=0, index=0):
    p = scene_of(pkg, k, depth).frame_params(index)
    return p, p.width * p.height


def c_render0(pkg, ctx, k):
    p, pix = frame(pkg, k)
    acc, rgb = dev(4 * pix), dev(pix, torch.int32)
    ctx.render(p, acc.data_ptr(), rgb.data_ptr())
    ctx.synchronize()


def c_render2(pkg, ctx, k):
    p, pix = frame(pkg, k, depth=2)
    acc, rgb = dev(4 * pix), dev(pix, torch.int32)
    ctx.render(p, acc.data_ptr(), rgb.data_ptr())
    ctx.synchronize()


def c_reproject_path(pkg, ctx, k):
    p, pix = frame(pkg, k)
    hist, rgb = dev(4 * pix), dev(pix, torch.int32)
    prev = pkg.scene.prev_camera(CAM[0], CAM[1], p.width, p.height)
    ctx.render_reproject(p, prev, hist.data_ptr(), rgb.data_ptr())
    ctx.synchronize()


def c_window(pkg, ctx, k):
    p, pix = frame(pkg, k)
    acc, rgb = dev(4 * pix), dev(pix, torch.int32)
    ctx.render_window(p, 3, acc.data_ptr(), rgb.data_ptr())
    ctx.synchronize()


def c_pipeline(pkg, ctx, k):
    p, pix = frame(pkg, k)
    acc, rgb = dev(4 * pix), dev(pix, torch.int32)
    ctx.set_pipeline(2)
    for f in range(2):
        p.frame_index = f
        ctx.render(p, acc.data_ptr(), rgb.data_ptr())
    ctx.synchronize()
    ctx.set_pipeline(0)


def c_tiles(pkg, ctx, k):
    p, pix = frame(pkg, k)
    packed = dev(4 * ctx.packed_len(p.width, p.height, 1))
    acc, rgb = dev(4 * pix), dev(pix, torch.int32)
    ctx.render_tiles(p, 0, 1, packed.data_ptr())
    ctx.composite_tiles(p, 1, packed.data_ptr(), acc.data_ptr(), rgb.data_ptr())
    ctx.synchronize()


def c_batches(pkg, ctx, k):
    """All nine host batch entries."""
    n = RAYS[k]
    rays, seeds = rays_of(pkg, n), np.arange(n, dtype=np.uint32) + 11
    w, h = FRAMES[k]
    ctx.find_nearest(rays)
    ctx.is_occluded(rays)
    ctx.find_nearest_filtered(rays)
    ctx.is_occluded_filtered(rays)
    ctx.find_nearest_cells(rays)
    ctx.pick_pixel(w, h, w // 2, h // 2)
    ctx.bvh_intersect(rays)
    ctx.trace(rays, seeds, 1)
    ctx.trace_probe(rays, seeds, 1)
    ctx.trace_probe(rays, seeds, 1, radiance=False)
    ctx.focus_distance(w, h)


def c_cast(pkg, ctx, k):
    rt = pkg.abi.rays_tensor(rays_of(pkg, RAYS[k]), "cuda:0")
    ctx.cast_nearest(rt, form=pkg.abi.CAST_POOL)
    ctx.synchronize()
    assert ctx.last_cast_kernel() == 2


def c_ids_denoise(pkg, ctx, k):
    p, pix = frame(pkg, k)
    ids, img = ctx.render_ids(p), dev(4 * pix) + 0.5
    ctx.denoise(p, ids, img, passes=1)
    ctx.denoise(p, ids, img, passes=3)
    ctx.synchronize()


def c_reproject_ids(pkg, ctx, k):
    sc = pkg.scene
    p, pix = frame(pkg, k)
    ids, img = ctx.render_ids(p), dev(4 * pix) + 0.5
    cam, prev = sc.look_at(CAM[0], CAM[1], p.width, p.height), sc.prev_camera(CAM[0], CAM[1], p.width, p.height)
    vols = [sc.volume(position=(0.01 * i, 0.0, 0.0)) for i in range((1, 3, 40)[k])]
    ctx.reproject(p, ids, ids, img, img.clone(), cam, prev)
    ctx.reproject(p, ids, ids, img, img.clone(), cam, prev, cur_volumes=vols, prev_volumes=vols)
    ctx.synchronize()


def c_profile(pkg, ctx, k):
    ctx.profile_enable((4, 16, 64)[k])
    ctx.profile_enable(0)


CALLS = {
    "grid upload": (c_grid, 5),                # the grid's cells, two levels and planes, the grid table
    "volumes and TLAS": (c_volumes, 8),        # a second grid and the table; volumes, bounds, the TLAS
    "materials": (c_materials, 1),
    "lights": (c_lights, 3),
    "shapes": (c_shapes, 2),
    "sky": (c_sky, 1),
    "arithmetic": (c_arith, 1),
    "bvh": (c_bvh, 1),
    "model": (c_model, 9),                     # jump tables, pinned plan, vox, mat; a grid and the table
    "noise": (c_noise, 8),                     # jump tables, pinned plan, the scratch; a grid and the table
    "brush": (c_brush, 2),                     # the refresh record and its pinned copies
    "write box": (c_write_box, 2),             # the same record (its temporary is gone when it returns)
    "tiled grid": (c_tiled, 5),
    "render depth 0": (c_render0, 1),          # the path state
    "render depth 2": (c_render2, 1),
    "static-camera path": (c_reproject_path, 2),   # the path state and the four images
    "window": (c_window, 2),                   # the path state and the chain's samples
    "pipeline": (c_pipeline, 0),               # the lanes' buffers go with vpx_set_pipeline(0)
    "tiles": (c_tiles, 1),
    "host batches": (c_batches, 1),            # the scratch
    "cast pool": (c_cast, 1),                  # the grab block
    "ids and denoise": (c_ids_denoise, 1),
    "reproject ids": (c_reproject_ids, 2),     # the scratch and the table's pinned staging copy
    "profile": (c_profile, 0),                 # events only
}


def ready_context(pkg, k=0):
    ctx = pkg.context.Context(0)
    ctx.load_scene(scene_of(pkg, k))
    ctx.bvh_set(tris_of(pkg, 2))
    return ctx


def settle(pkg, ctx):
    """Back to one volume of grid 0 without shapes or extra lights, so that every call runs on the same scene."""
    one_volume(pkg, ctx)
    no_lights_or_shapes(pkg, ctx)


# --------------------------------------------------------------------------- 1. everything back
def test_context_returns_everything(pkg):
    gc.collect()
    before = live(pkg)
    ctx = ready_context(pkg)
    try:
        assert live(pkg) > before
        for k in (0, 2, 0):
            for name, (call, _) in CALLS.items():
                call(pkg, ctx, k)
                settle(pkg, ctx)
                assert live(pkg) > before, name
    finally:
        ctx.close()
    assert live(pkg) == before


# --------------------------------------------------------------------------- 2. no accumulation
@pytest.mark.parametrize("name", list(CALLS))
def test_growth_does_not_accumulate(pkg, name):
    gc.collect()
    call, own = CALLS[name]
    ctx = ready_context(pkg, 1)
    try:
        base = live(pkg)
        call(pkg, ctx, 1)
        settle(pkg, ctx)
        first = live(pkg)
        assert first <= base + own, (name, "a first call brings at most its own buffers")
        for _ in range(9):
            call(pkg, ctx, 1)
            settle(pkg, ctx)
        assert live(pkg) == first, (name, "ten calls at one size")
        call(pkg, ctx, 0)
        settle(pkg, ctx)
        assert live(pkg) == first, (name, "a smaller size")
        call(pkg, ctx, 2)
        settle(pkg, ctx)
        assert live(pkg) <= first + own, (name, "a larger size")
    finally:
        ctx.close()


# --------------------------------------------------------------------------- 3. replacement frees
def test_replacement_frees(pkg):
    gc.collect()
    sc = pkg.scene
    ctx = ready_context(pkg)
    try:
        c_grid(pkg, ctx, 1)
        first = live(pkg)
        c_grid(pkg, ctx, 2)
        assert live(pkg) == first, "a grid id at another size"

        c_model(pkg, ctx, 0)
        first = live(pkg)
        ctx.model_upload(2, (5, 3, 2), np.full(30, 3, np.uint8))
        assert live(pkg) == first, "a model id replaced"

        set_lights(pkg, ctx, 4)
        first = live(pkg)
        set_lights(pkg, ctx, 2)
        assert live(pkg) == first, "fewer lights"
        set_lights(pkg, ctx, 0)
        assert live(pkg) == first - 3, "no lights: the three tables are gone"

        ctx.bvh_set(tris_of(pkg, 16))
        first = live(pkg)
        ctx.bvh_set(tris_of(pkg, 64))
        assert live(pkg) == first, "a BVH replaced"
        ctx.bvh_set((pkg.abi.BvhTri * 0)())
        assert live(pkg) == first - 1, "n = 0: the BVH is gone"

        base = live(pkg)
        ctx.set_sky(sc.synthetic_sky(8, 4))
        first = live(pkg)
        assert first == base + 1
        ctx.set_sky(sc.synthetic_sky(16, 8))
        assert live(pkg) == first, "a sky of another size"
        ctx.set_sky(None)
        assert live(pkg) == base, "the sky removed"
    finally:
        ctx.close()


# --------------------------------------------------------------------------- 4. a device set
def test_device_set_returns_everything(pkg):
    gc.collect()
    before = live(pkg)
    torch.cuda.set_device(0)
    desc = scene_of(pkg, 2)
    pix = desc.width * desc.height
    acc, rgb = dev(4 * pix), dev(pix, torch.int32)
    torch.cuda.synchronize()
    group = pkg.context.Context(devices=[0, 0])
    try:
        group.load_scene(desc)
        group.render(desc.frame_params(0), acc.data_ptr(), rgb.data_ptr())  # samples gathered
        group.synchronize()
        held = live(pkg)
        assert held > before
        group.render(desc.frame_params(0), 0, rgb.data_ptr())  # RGB8 gathered, sharded accumulators
        group.synchronize()
        assert live(pkg) == held, "both paths use the same per-member buffers"
    finally:
        group.close()
    assert live(pkg) == before


# --------------------------------------------------------------------------- 5. the shared carve
SIZES = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def singles(pkg):
    """The 257 rays, their seeds, and each entry's results one ray at a time."""
    gc.collect()
    n = max(SIZES)
    rays, seeds = rays_of(pkg, n, seed=3), np.arange(n, dtype=np.uint32) * 7 + 1
    ctx = ready_context(pkg, 2)
    ctx.bvh_set(tris_of(pkg, 64))
    one = {"hits": [], "cells": [], "radiance": [], "probes": [], "t": []}
    Ray = pkg.abi.Ray
    for i in range(n):
        r = (Ray * 1).from_buffer_copy(bytes(rays[i]))
        h, c = ctx.find_nearest_cells(r)
        one["hits"].append(bytes(h)), one["cells"].append(bytes(c))
        rad, pr = ctx.trace_probe(r, seeds[i:i + 1], 1)
        one["radiance"].append(rad.tobytes()), one["probes"].append(pr.tobytes())
        one["t"].append(ctx.bvh_intersect(r).tobytes())
    yield ctx, rays, seeds, {key: b"".join(v) for key, v in one.items()}
    ctx.close()


def batch(pkg, ctx, rays, seeds, n):
    r = (pkg.abi.Ray * n).from_buffer_copy(bytes(rays)[:C.sizeof(pkg.abi.Ray) * n])
    h, c = ctx.find_nearest_cells(r)
    rad, pr = ctx.trace_probe(r, seeds[:n], 1)
    return {"hits": bytes(h), "cells": bytes(c), "radiance": rad.tobytes(), "probes": pr.tobytes(),
            "t": ctx.bvh_intersect(r).tobytes()}


@pytest.mark.parametrize("n", SIZES)
def test_batch_equals_single_rays(pkg, singles, n):
    gc.collect()
    ctx, rays, seeds, one = singles
    got = batch(pkg, ctx, rays, seeds, n)
    for key, b in got.items():
        assert len(b) % n == 0
        assert b == one[key][:len(b)], (key, n)


def test_small_batch_after_a_large_one(pkg, singles):
    gc.collect()
    ctx, rays, seeds, one = singles
    batch(pkg, ctx, rays, seeds, 257)
    got = batch(pkg, ctx, rays, seeds, 1)
    for key, b in got.items():
        assert b == one[key][:len(b)], key
