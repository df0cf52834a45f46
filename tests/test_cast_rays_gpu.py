"""Device ray batches on the device (vpx_cast_nearest / vpx_cast_occluded): every record against
the host entry on the same context and rays (vpx_find_nearest_cells / vpx_is_occluded_filtered,
themselves pinned to the oracle), and for the neutral filter against the oracle directly.  Both
forms, the pool's refill edges, heavy tails and empty grabs, order independence, the reference
arithmetic, the ID buffer, stream order, side effects, refusals and the C++ mirror.  Everything is
compared bit for bit.  tests/test_cast_rays.py holds the scenes and the conditions (checked there
with the oracle alone) that keep these comparisons from being vacuous.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

from cases import SCENES, random_rays  # noqa: E402
from test_cast_rays import room_scene, wall_case  # noqa: E402
from test_hit_cells_gpu import H, W, pixel_rays  # noqa: E402
from test_ray_filter import N_RAYS, NO_RANGE, SMOKE, case_s, expected, expected_occluded, hit_rows, make_rays  # noqa: E402
from test_ray_filter_gpu import FILTERS, X86, same, x86_mode  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = {"auto": 0, "lane": 1, "pool": 2}


def words(buf, n):
    """A ctypes record array of 32-byte records as int64 rows of its eight words."""
    return np.frombuffer(buf, np.uint32, count=8 * n).reshape(n, 8).astype(np.int64)


def twords(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def check_cast(pkg, ctx, rays, flt, form, max_waves=0, what="", occlusion=True, want_kernel=None):
    """cast_nearest with and without cells, and cast_occluded, against the host entries on the
    same context, rays and filter.  Returns the hit rows (hit_rows' columns)."""
    n = len(rays)
    rt = pkg.abi.rays_tensor(rays, DEV)
    hits, cells = ctx.find_nearest_cells(rays, filter=flt)
    h, c = ctx.cast_nearest(rt, filter=flt, form=form, max_waves=max_waves)
    kernel = ctx.last_cast_kernel()
    h2, none = ctx.cast_nearest(rt, filter=flt, cells=False, form=form, max_waves=max_waves)
    assert none is None and ctx.last_cast_kernel() == kernel
    if want_kernel is not None:
        assert kernel == want_kernel, (what, kernel)
    ctx.synchronize()
    assert h.dtype == torch.int32 and tuple(h.shape) == (n, 8) and tuple(c.shape) == (n, 8)
    same(twords(h), words(hits, n), what + " hits")
    same(twords(c), words(cells, n), what + " cells")
    same(twords(h2), words(hits, n), what + " hits without cells")
    if occlusion and flt.mat_lo > flt.mat_hi:
        occ = ctx.cast_occluded(rt, filter=flt, form=form, max_waves=max_waves)
        assert form == 0 or ctx.last_cast_kernel() == kernel  # form 0: the library chooses per entry
        ctx.synchronize()
        assert occ.dtype == torch.uint8 and np.array_equal(occ.cpu().numpy(), ctx.is_occluded_filtered(rays, filter=flt)), what
    return hit_rows(hits, n)


# --------------------------------------------------------------------------- 1. scene S
@pytest.fixture(scope="module")
def s(pkg, orc):
    desc, o, d, tmax = case_s(pkg, orc)
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    yield dict(desc=desc, o=o, d=d, tmax=tmax, rays=make_rays(pkg.abi, o, d, tmax), ctx=ctx)
    ctx.close()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(FILTERS) + ["neutral"])
def test_scene_s_every_filter_and_form(pkg, orc, s, name, form):
    """Three volumes, the sphere and the triangle, 4099 rays: hits, cells and occlusion equal the
    host entries; only last_volume (first = 2 of 3) is in the pool's reach."""
    first, rng_mat, shapes = FILTERS.get(name, (0, NO_RANGE, True))
    flt = s["ctx"].ray_filter(first, rng_mat, shapes)
    kernel = 1 if name != "last_volume" else {"pool": 2, "lane": 1, "auto": None}[form]  # auto: the library's choice
    got = check_cast(pkg, s["ctx"], s["rays"], flt, FORMS[form], what=name + " " + form, want_kernel=kernel)
    if name == "neutral":
        want = expected(pkg, orc, s["desc"], s["rays"])
        same(got, want, "neutral vs oracle")
        assert int((want[:, 4] == -1).sum()) >= 50  # shape wins


# ----------------------------------------------------------- 2. one visited volume: the room
ROOM_FILTERS = {"neutral": (NO_RANGE, False), "smoke": (SMOKE, False), "raw": (NO_RANGE, True)}


@pytest.fixture(scope="module", params=[False, True], ids=["bare", "shapes"])
def room(request, pkg, orc):
    desc = room_scene(pkg, orc, request.param)
    _, o, d, tmax = case_s(pkg, orc)
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    yield dict(desc=desc, ctx=ctx, o=o, d=d, tmax=tmax, rays=make_rays(pkg.abi, o, d, tmax), shapes=request.param)
    ctx.close()


@pytest.mark.parametrize("max_waves", [0, 1, 3])
@pytest.mark.parametrize("name", list(ROOM_FILTERS))
def test_room_pool(pkg, orc, room, name, max_waves):
    """S's rays (tmax inside the smoke, just before and after the solid behind it, axis-parallel
    zero components, misses) against the room alone, with and without the shapes, in the pool."""
    rng_mat, raw = ROOM_FILTERS[name]
    ctx = room["ctx"]
    flt = ctx.ray_filter(0, rng_mat, True, raw)
    got = check_cast(pkg, ctx, room["rays"], flt, FORMS["pool"], max_waves, "room " + name, want_kernel=2)
    if name == "neutral":
        same(got, expected(pkg, orc, room["desc"], room["rays"]), "room vs oracle")
        rt = pkg.abi.rays_tensor(room["rays"], DEV)  # kept until the context's stream has run the cast
        occ = ctx.cast_occluded(rt, form=FORMS["pool"], max_waves=max_waves)
        ctx.synchronize()
        assert np.array_equal(occ.cpu().numpy(), expected_occluded(pkg, orc, room["desc"], room["rays"]))


def test_room_order_independence(pkg, orc, room):
    """5: a seeded permutation of the rays gives the same records, permuted."""
    ctx, abi = room["ctx"], pkg.abi
    perm = np.random.default_rng(41).permutation(N_RAYS)
    flt = ctx.ray_filter(0, SMOKE, True)
    shuffled = make_rays(abi, room["o"][perm], room["d"][perm], room["tmax"][perm])
    ra, rb = abi.rays_tensor(room["rays"], DEV), abi.rays_tensor(shuffled, DEV)  # both kept until the casts have run
    a = ctx.cast_nearest(ra, filter=flt, form=FORMS["pool"])
    b = ctx.cast_nearest(rb, filter=flt, form=FORMS["pool"], max_waves=3)
    ctx.synchronize()
    for x, y, what in ((a[0], b[0], "hits"), (a[1], b[1], "cells")):
        same(twords(y), twords(x)[perm], "permuted " + what)
    neutral = ctx.ray_filter()
    oa = ctx.cast_occluded(ra, filter=neutral, form=FORMS["pool"])
    ob = ctx.cast_occluded(rb, filter=neutral, form=FORMS["pool"])
    ctx.synchronize()
    assert np.array_equal(ob.cpu().numpy(), oa.cpu().numpy()[perm])


# ------------------------------------------------------------------------- 3. refill edges
@pytest.fixture(scope="module")
def teapot(pkg):
    ctx = pkg.context.Context(0)
    ctx.load_scene(SCENES["teapot128"](pkg.scene))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("max_waves", [1, 3, 0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 4099])
def test_refill_edges(pkg, teapot, n, max_waves):
    """teapot128, random_rays(n, 3): a wave's 64 lanes and a grab's 128 rays, one less and one
    more; with max_waves = 1 and n = 4099 one wave takes all 33 grabs."""
    o, d = random_rays(n, 3)
    check_cast(pkg, teapot, make_rays(pkg.abi, o, d, 1e34), teapot.ray_filter(), FORMS["pool"], max_waves,
               "teapot n=%d waves=%d" % (n, max_waves), want_kernel=2)


# ------------------------------------------------------------ 4. heavy tails, empty grabs
@pytest.fixture(scope="module")
def wall(pkg):
    desc, batches, _ = wall_case(pkg)
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    yield ctx, batches
    ctx.close()


@pytest.mark.parametrize("max_waves", [1, 0])
@pytest.mark.parametrize("batch", ["tails", "misses", "first", "mixed"])
def test_heavy_tails_and_empty_grabs(pkg, wall, batch, max_waves):
    ctx, batches = wall
    o, d = batches[batch]
    got = check_cast(pkg, ctx, make_rays(pkg.abi, o, d, 1e34), ctx.ray_filter(), FORMS["pool"], max_waves,
                     "wall " + batch, want_kernel=2)
    if batch == "first":  # origins inside solid cells: VPX_CELL_FACE clear
        rt = pkg.abi.rays_tensor(make_rays(pkg.abi, o, d, 1e34), DEV)
        _, cells = ctx.cast_nearest(rt, form=FORMS["pool"])
        ctx.synchronize()
        fl = pkg.context.unpack_cells(cells)["flags"]
        assert (got[:, 4] == 0).all() and ((fl & pkg.abi.CELL_HIT) != 0).all() and not (fl & pkg.abi.CELL_FACE).any()


# --------------------------------------------------------------------- 6. x86 arithmetic
@pytest.mark.skipif(not X86, reason="VPX_ARITH_X86_HOST needs an x86 host")
def test_x86_arithmetic(pkg, orc, room, teapot):
    """Cases 2 and 3 at n = 4099 in VPX_ARITH_X86_HOST: FastReciprocal in the nearest pool, 1 / D in
    the occlusion pool, as the host entries."""
    o, d = random_rays(4099, 3)
    jobs = [(room["ctx"], room["rays"], room["ctx"].ray_filter(0, SMOKE, True), "room smoke"),
            (room["ctx"], room["rays"], room["ctx"].ray_filter(), "room neutral"),
            (teapot, make_rays(pkg.abi, o, d, 1e34), teapot.ray_filter(), "teapot")]
    for ctx, rays, flt, what in jobs:
        exact = words(ctx.find_nearest_cells(rays, filter=flt)[0], len(rays))
        try:
            x86_mode(pkg, orc, ctx, True)
            check_cast(pkg, ctx, rays, flt, FORMS["pool"], 0, "x86 " + what, want_kernel=2)
            check_cast(pkg, ctx, rays, flt, FORMS["pool"], 1, "x86 one wave " + what, want_kernel=2)
            moved = int((words(ctx.find_nearest_cells(rays, filter=flt)[0], len(rays))[:, 0] != exact[:, 0]).sum())
        finally:
            x86_mode(pkg, orc, ctx, False)
        assert moved >= 1, what  # the mode matters for these rays


# ------------------------------------------------------------------------- 7. ID buffer
def test_id_buffer_cross_check(pkg, orc):
    """Scene S under its camera at 67 x 35: the host-built pixel rays cast on the device and packed
    as k_ids packs them equal render_ids word for word."""
    desc = case_s(pkg, orc)[0]
    with pkg.context.Context(0) as ctx:
        ctx.load_scene(desc)
        ctx.set_camera(pkg.scene.look_at(desc._cam_pos, desc._cam_target, W, H))
        _, o, d = pixel_rays(pkg, desc)
        ids = ctx.render_ids(desc.frame_params(0, width=W, height=H))
        rt = pkg.abi.rays_tensor(make_rays(pkg.abi, o, d, 1e34), DEV)
        h, c = ctx.cast_nearest(rt)
        ctx.synchronize()
        hw, cw = twords(h), twords(c)
        face = np.where(cw[:, 7] & 2, 1 + 2 * ((cw[:, 7] >> 8) & 3) + ((cw[:, 7] >> 10) & 1), 0)
        vox = hw[:, 4].astype(np.uint32).view(np.int32).astype(np.int64)
        want = np.column_stack([hw[:, 0], ((vox + 2) & 0xFFFF) | (hw[:, 5] & 255) << 16 | face << 24,
                                cw[:, 0] | cw[:, 1] << 16, cw[:, 2]])
        got = ids.cpu().numpy().view(np.uint32).reshape(-1, 4).astype(np.int64)
        same(got, want, "ids")
        assert int((vox >= 0).sum()) >= 200 and int((vox == -2).sum()) >= 20


# --------------------------------------------------- 8. stream order without synchronising
def test_stream_order(pkg, orc):
    """The rays produced by a torch op on a side stream, the cast, then a consumer op, with no
    synchronisation between them; a dig between two casts; three frames in flight, then a cast."""
    abi, sc = pkg.abi, pkg.scene
    desc = room_scene(pkg, orc, False)
    _, o, d, tmax = case_s(pkg, orc)
    rays = make_rays(abi, o, d, tmax)
    host = abi.rays_tensor(rays, "cpu")
    side = torch.cuda.Stream(device=0)
    with pkg.context.Context(0) as ctx:
        ctx.load_scene(desc)
        ctx.set_stream(side.cuda_stream)
        want = words(ctx.find_nearest_cells(rays)[0], N_RAYS)
        with torch.cuda.stream(side):
            src = host.to(DEV, non_blocking=False)
            rt = src * 1.0  # produced on the side stream, just before the cast
            h, _ = ctx.cast_nearest(rt, form=FORMS["pool"])
            out = h.clone()  # a consumer on the same stream
        side.synchronize()
        same(twords(out), want, "side stream")
        # a dig between two casts: the second sees the edit, the first does not
        hit = int(np.flatnonzero((want[:, 4] == 0))[0])
        cell = tuple(int(x) for x in words(ctx.find_nearest_cells(rays)[1], N_RAYS)[hit, :3])
        with torch.cuda.stream(side):
            a, _ = ctx.cast_nearest(rt, form=FORMS["pool"])
            ctx.grid_brush(0, [sc.box_brush(cell, cell, 255)])
            b, _ = ctx.cast_nearest(rt, form=FORMS["pool"])
        side.synchronize()
        after = words(ctx.find_nearest_cells(rays)[0], N_RAYS)
        same(twords(a), want, "before the dig")
        same(twords(b), after, "after the dig")
        assert (after[hit] != want[hit]).any()
        # frames in flight
        ctx.set_pipeline(3)
        p = desc.frame_params(0)  # the scene's own 32 x 32 camera
        acc = torch.zeros((desc.height, desc.width, 4), dtype=torch.float32, device=DEV)
        rgb = torch.zeros((desc.height, desc.width), dtype=torch.int32, device=DEV)
        side.synchronize()
        with torch.cuda.stream(side):
            for k in range(3):
                p.frame_index = k
                ctx.render(p, acc.data_ptr(), rgb.data_ptr())
            f, _ = ctx.cast_nearest(rt, form=FORMS["pool"])
        ctx.synchronize()
        same(twords(f), after, "after three frames in flight")


# ------------------------------------------------------------------------ 9. side effects
def test_no_side_effects_and_device_set(pkg, orc, room):
    ctx, abi = room["ctx"], pkg.abi
    rt = abi.rays_tensor(room["rays"], DEV)
    before, light = ctx.counters().as_dict(), ctx.player_light().as_dict()
    for form in FORMS.values():
        ctx.cast_nearest(rt, form=form)
        ctx.cast_occluded(rt, form=form)
    ctx.synchronize()
    assert ctx.counters().as_dict() == before and ctx.player_light().as_dict() == light
    single = ctx.cast_nearest(rt, form=FORMS["pool"])
    occ = ctx.cast_occluded(rt, form=FORMS["pool"])
    ctx.synchronize()
    group = pkg.context.Context(devices=[0, 0])
    try:
        group.load_scene(room["desc"])
        for form, kernel in ((FORMS["pool"], 2), (FORMS["lane"], 1)):
            g = group.cast_nearest(rt, form=form)
            assert group.last_cast_kernel() == kernel
            go = group.cast_occluded(rt, form=form)
            group.synchronize()
            same(twords(g[0]), twords(single[0]), "device set hits")
            same(twords(g[1]), twords(single[1]), "device set cells")
            assert np.array_equal(go.cpu().numpy(), occ.cpu().numpy())
    finally:
        group.close()


# --------------------------------------------------------------------------- 10. refusals
def test_refusals(pkg, room):
    abi, ctx = pkg.abi, room["ctx"]
    lib, h = ctx.lib, ctx.h
    rt = abi.rays_tensor(room["rays"], DEV)[:4].contiguous()
    hits = torch.zeros((4, 8), dtype=torch.int32, device=DEV)
    cells = torch.zeros((4, 8), dtype=torch.int32, device=DEV)
    occ = torch.zeros((4,), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    R, Hh, Cc, Oo = (C.c_void_p(t.data_ptr()) for t in (rt, hits, cells, occ))
    E = abi.VPX_E_INVALID

    def nearest(n=4, r=R, f=None, opt=None, ho=Hh, co=Cc):
        return lib.vpx_cast_nearest(h, r, n, f, opt, ho, co)

    def occluded(n=4, r=R, f=None, opt=None, oo=Oo):
        return lib.vpx_cast_occluded(h, r, n, f, opt, oo)

    assert nearest(r=None) == E and nearest(ho=None) == E and occluded(r=None) == E and occluded(oo=None) == E
    assert nearest(n=(1 << 30) + 1) == E and occluded(n=(1 << 30) + 1) == E
    for bad in ((4, 0, (0, 0)), (3, 0, (0, 0)), (0x80000000, 0, (0, 0)), (0, 0, (1, 0)), (2, 1, (0, 1))):
        opt = abi.Cast(bad[0], bad[1], (C.c_uint32 * 2)(*bad[2]))
        assert nearest(opt=C.byref(opt)) == E and occluded(opt=C.byref(opt)) == E, bad
        assert nearest(n=0, opt=C.byref(opt)) == E, bad
    for bad in ((0, 9, 256, 0), (0, 1, 0, 4), (0, 9, 14, 0x80000000)):
        assert nearest(f=C.byref(abi.RayFilter(*bad))) == E and nearest(n=0, f=C.byref(abi.RayFilter(*bad))) == E, bad
    for bad in ((0, 9, 14, 0), (0, 0, 0, 0), (0, 1, 0, 8)):  # the occlusion entry takes no material range
        assert occluded(f=C.byref(abi.RayFilter(*bad))) == E, bad
    assert lib.vpx_last_error(h)
    ctx.synchronize()
    assert not hits.cpu().numpy().any() and not occ.cpu().numpy().any(), "a refused call writes nothing"
    # what is allowed: raw directions, no cells, no filter and no options, n == 0
    raw = abi.RayFilter(0, 1, 0, abi.QUERY_RAW_DIRECTION)
    assert nearest(f=C.byref(raw)) == abi.VPX_OK and occluded(f=C.byref(raw)) == abi.VPX_OK
    assert nearest(co=None) == abi.VPX_OK and ctx.last_cast_kernel() in (1, 2)
    assert nearest(n=0, r=None, ho=None, co=None) == abi.VPX_OK and ctx.last_cast_kernel() == 0
    assert occluded(n=0, r=None, oo=None) == abi.VPX_OK and ctx.last_cast_kernel() == 0
    ctx.synchronize()
    with pytest.raises(ValueError):
        ctx.cast_nearest(abi.rays_tensor(room["rays"], "cpu"))
    with pkg.context.Context(0) as bare:  # before a scene
        assert lib.vpx_cast_nearest(bare.h, R, 4, None, None, Hh, Cc) == abi.VPX_E_STATE
        assert lib.vpx_cast_occluded(bare.h, R, 4, None, None, Oo) == abi.VPX_E_STATE
        assert bare.last_cast_kernel() == 0


# ------------------------------------------------------------------------ 11. C++ mirror
@pytest.mark.parametrize("form", [1, 2])
def test_cpp_mirror_cast(pkg, form):
    """host/vpx_demo's cast sub-command builds the pillars world in C++, casts 129 rays through
    Renderer::CastRays / CastOccluded and prints rays and records; the host entries give the same
    records for those rays from Python."""
    exe = os.path.join(os.path.dirname(pkg.__file__), "host", "vpx_demo")
    assert os.path.exists(exe), "host/vpx_demo missing: run __graft_entry__.build()"
    n = 64
    r = subprocess.run([exe, "cast", str(n), str(W), str(H), str(form), "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])["cast"]
    assert got["n"] == 129 and got["form"] == form
    rows = np.array(got["rows"], np.int64)
    assert rows.shape == (129, 25)
    rays = (pkg.abi.Ray * 129)()
    C.memmove(rays, rows[:, :8].astype(np.uint32).tobytes(), 129 * 32)
    with pkg.context.Context(0) as ctx:
        ctx.load_scene(pkg.scene.pillars_scene(n, W, H))
        hits, cells = ctx.find_nearest_cells(rays)
        same(rows[:, 8:16], words(hits, 129), "mirror hits")
        same(rows[:, 16:24], words(cells, 129), "mirror cells")
        assert np.array_equal(rows[:, 24], ctx.is_occluded_filtered(rays))
    vox = rows[:, 12].astype(np.uint32).view(np.int32)
    assert int((vox >= 0).sum()) >= 30 and int((vox < 0).sum()) >= 10
