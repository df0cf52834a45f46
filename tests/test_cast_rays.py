"""Device ray batches (vpx_cast_nearest / vpx_cast_occluded / vpx_debug_last_cast_kernel) without a
GPU: the C-ABI additions, the layout of vpx_cast, the null-context refusals, the Python surface
and both mirrors, and the scenes, rays and conditions the GPU tests (tests/test_cast_rays_gpu.py)
stand on, checked with the oracle alone so that those comparisons cannot pass vacuously.
"""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np

from cases import SCENES, random_rays
from test_hit_cells import vols_of
from test_ray_filter import N_RAYS, NO_RANGE, SMOKE, case_s, expected, make_rays

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vpx_cast_nearest", "vpx_cast_occluded", "vpx_debug_last_cast_kernel")


# ------------------------------------------------------------------- header and library
def test_header_declares_and_library_exports(pkg):
    text = open(os.path.join(REPO, "include", "vpx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in pkg.abi.SIGNATURES
        assert name in text[: text.index("#ifndef VPX_H_")], "the entry list at the top of the header"
    assert re.search(r"#define\s+VPX_CAST_PER_LANE\s+0x1u", code)
    assert re.search(r"#define\s+VPX_CAST_POOL\s+0x2u", code)
    assert re.search(r"#define\s+VPX_ABI_VERSION\s+2\b", code)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH], capture_output=True, text=True).stdout
    assert set(ENTRIES) <= set(re.findall(r" T (vpx_\w+)", out))
    assert (pkg.abi.CAST_PER_LANE, pkg.abi.CAST_POOL) == (1, 2)


def test_struct_size_and_fields(pkg):
    abi = pkg.abi
    assert C.sizeof(abi.Cast) == 16 and abi.STRUCT_SIZES[abi.Cast] == 16
    assert [(n, getattr(abi.Cast, n).offset) for n, _ in abi.Cast._fields_] == [("flags", 0), ("max_waves", 4), ("reserved", 8)]
    src = ('#include <cstddef>\n#include "vpx.h"\n'
           "static_assert(sizeof(vpx_cast) == 16, \"vpx_cast\");\n"
           "static_assert(offsetof(vpx_cast, flags) == 0, \"flags\");\n"
           "static_assert(offsetof(vpx_cast, max_waves) == 4, \"max_waves\");\n"
           "static_assert(offsetof(vpx_cast, reserved) == 8 && sizeof(((vpx_cast*)0)->reserved) == 8, \"reserved\");\n"
           "static_assert(VPX_CAST_PER_LANE == 1u && VPX_CAST_POOL == 2u && VPX_ABI_VERSION == 2, \"constants\");\n")
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(REPO, "include"), "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_context_is_refused(pkg):
    lib, abi = pkg.load_library(), pkg.abi
    f, opt = abi.RayFilter(0, 1, 0, 0), abi.Cast()
    buf = (C.c_uint8 * 64)()
    assert lib.vpx_cast_nearest(None, buf, 1, C.byref(f), C.byref(opt), buf, buf) == abi.VPX_E_INVALID
    assert lib.vpx_cast_nearest(None, None, 0, None, None, None, None) == abi.VPX_E_INVALID
    assert lib.vpx_cast_occluded(None, buf, 1, C.byref(f), C.byref(opt), buf) == abi.VPX_E_INVALID
    assert lib.vpx_cast_occluded(None, None, 0, None, None, None) == abi.VPX_E_INVALID
    assert lib.vpx_debug_last_cast_kernel(None) == 0
    assert lib.vpx_abi_version() == abi.ABI_VERSION == 2


def test_python_surface_and_mirrors(pkg):
    ctx, ren, con = pkg.context.Context, pkg.renderer.Renderer, pkg.context
    for fn in (ctx.cast_nearest, ctx.cast_occluded, ctx.last_cast_kernel, ren.CastRays, ren.CastOccluded, pkg.abi.rays_tensor,
               con.unpack_hits, con.unpack_cells, ctx.unpack_hits, ctx.unpack_cells):
        assert callable(fn)
    host = os.path.join(REPO, "raytracer-voxpopuli_amd", "host")
    for name in ("vpx_renderer.h", "vpx_renderer.cpp"):
        text = open(os.path.join(host, name)).read()
        assert "CastRays" in text and "CastOccluded" in text, name
    # the views read the records' layout: one hit and one cell record, field by field
    h = np.zeros((1, 8), np.int32)
    h[0] = [np.float32(0.5).view(np.int32), 0, np.float32(-1.0).view(np.int32), 0, 2, 7, 41, 1]
    u = con.unpack_hits(h)
    assert (u["t"][0], tuple(u["normal"][0]), u["vox_index"][0], u["material"][0], u["cells"][0], u["inside_glass"][0]) == (
        0.5, (0.0, -1.0, 0.0), 2, 7, 41, 1)
    c = np.array([[3, 4, 5, 1, 3, 3, 5, 0x107]], np.int32)
    v = con.unpack_cells(c)
    assert (tuple(v["cell"][0]), v["grid_id"][0], tuple(v["face_cell"][0]), v["flags"][0]) == ((3, 4, 5), 1, (3, 3, 5), 0x107)


# ---------------------------------------------------- the GPU tests' scenes, rays and conditions
def room_scene(pkg, orc, shapes):
    """Scene S's room (its volume 1 with grid 1) as a scene of its own, with or without S's sphere
    and triangle."""
    desc = case_s(pkg, orc)[0]
    abi = pkg.abi
    vol = abi.Volume.from_buffer_copy(bytes(desc.volumes[1]))
    vol.grid_id = 0
    return dataclasses.replace(desc, name="cast_room" + ("_shapes" if shapes else ""), grids=[desc.grids[1]],
                               volumes=(abi.Volume * 1)(vol), spheres=desc.spheres if shapes else [],
                               triangles=desc.triangles if shapes else [])


def first_cells(desc, o, d):
    """Per ray of a one-volume scene: None when Setup3DDDA fails (the ray misses the cube), else
    the byte of the walk's first cell."""
    from test_kat_paths import Ray, dsign, f32, v3
    vol = vols_of(desc)[0]
    out = []
    with np.errstate(all="ignore"):
        for j in range(len(o)):
            ray = Ray(v3(*o[j]), v3(*d[j]))
            rD = v3(*[f32(f32(1) / ray.D[k]) for k in range(3)])
            s = vol.setup(ray.O, ray.D, rD, dsign(ray.D))
            out.append(None if s is None else int(vol.cell(s["X"], s["Y"], s["Z"])))
    return out


def test_room_conditions(pkg, orc):
    """Case 2 (S's 4099 rays against the room alone), with the oracle: 2461 of the rays hit a voxel
    under the smoke filter (at least a quarter), 1881 pass through smoke before their hit (at least
    100: their unfiltered hit is smoke and the smoke filter finds something behind it), 565 are
    stopped by tmax before a hit an unbounded ray has (at least 50), and 229 miss (at least 50)."""
    abi = pkg.abi
    _, o, d, tmax = case_s(pkg, orc)
    desc = room_scene(pkg, orc, False)
    rays = make_rays(abi, o, d, tmax)
    plain = expected(pkg, orc, desc, rays, 0, NO_RANGE, False)
    filt = expected(pkg, orc, desc, rays, 0, SMOKE, False)
    unb = expected(pkg, orc, desc, make_rays(abi, o, d, 1e34), 0, SMOKE, False)
    smoke = (plain[:, 4] >= 0) & (plain[:, 5] >= 9) & (plain[:, 5] <= 14)
    counts = dict(hit=int((filt[:, 4] >= 0).sum()), through=int((smoke & (filt[:, 4] >= 0)).sum()),
                  stopped=int(((unb[:, 4] >= 0) & (filt[:, 4] < 0)).sum()), miss=int((plain[:, 4] < 0).sum()))
    print(counts)
    assert 4 * counts["hit"] >= N_RAYS and counts["through"] >= 100 and counts["stopped"] >= 50 and counts["miss"] >= 50


def test_teapot_conditions(pkg, orc):
    """Case 3 at n = 4099 (random_rays(4099, 3) on teapot128), with the oracle and the restated
    setup: 942 rays hit (at least 500), 1301 miss the cube (Setup3DDDA fails, at least 500) and 50
    start their walk in a solid cell.  The hundred such rays that were asked for cannot come from
    this scene and generator: 1.35 % of teapot128's cells are solid, and over 400 seeds (with up to
    half of the origins inside the cube) the most was 52.  Case 4 supplies the class in bulk: 4096
    first-cell hits in its 'first' batch and 1365 in 'mixed' (test_wall_conditions)."""
    desc = SCENES["teapot128"](pkg.scene)
    o, d = random_rays(4099, 3)
    got = expected(pkg, orc, desc, make_rays(pkg.abi, o, d, 1e34), 0, NO_RANGE, True)
    fc = first_cells(desc, o, d)
    counts = dict(hit=int((got[:, 4] >= 0).sum()), outside=sum(c is None for c in fc),
                  solid_start=sum(c is not None and c != 255 for c in fc))
    print(counts)
    assert counts["hit"] >= 500 and counts["outside"] >= 500 and counts["solid_start"] >= 50


WALL_N = 128
WALL_SEED = 23


def wall_case(pkg):
    """Case 4: a 128^3 grid that is empty but for one far wall (z = 120..123, metal), built like
    test_hit_cells.sparse_case, and four batches of 4096 rays: 'tails' (every 64th ray crosses the
    whole grid to the wall, the rest miss the cube), 'misses', 'first' (origins inside the wall:
    first-cell hits) and 'mixed' (the three classes by thirds, interleaved by a seeded permutation)."""
    sc = pkg.scene
    g = np.full((WALL_N,) * 3, 255, np.uint8)  # [z][y][x]
    g[120:124, :, :] = 7
    desc = sc._scene("cast_wall", [sc.GridSpec(n=WALL_N, dense=g.reshape(-1))], [sc.volume()], sc.default_materials(),
                     [sc.point_light()], [], [], sc.dir_light(), (0.5, 0.5, -1.0), (0.5, 0.5, 0.5), 32, 32)
    rng = np.random.default_rng(WALL_SEED)
    n = 4096

    def cross(k):  # from just inside the low z face across the grid, slightly oblique
        o = np.column_stack([rng.uniform(0.2, 0.8, k), rng.uniform(0.2, 0.8, k), rng.uniform(0.001, 0.01, k)])
        d = np.column_stack([rng.uniform(-0.15, 0.15, k), rng.uniform(-0.15, 0.15, k), np.ones(k)])
        return o, d

    def miss(k):  # above the cube, going up
        o = np.column_stack([rng.uniform(-0.5, 1.5, k), rng.uniform(1.2, 2.0, k), rng.uniform(-0.5, 1.5, k)])
        d = np.column_stack([rng.uniform(-0.3, 0.3, k), rng.uniform(0.5, 1.0, k), rng.uniform(-0.3, 0.3, k)])
        return o, d

    def first(k):  # inside the wall
        o = np.column_stack([rng.uniform(0.05, 0.95, k), rng.uniform(0.05, 0.95, k), rng.uniform(120.2, 123.8, k) / WALL_N])
        return o, rng.normal(size=(k, 3))

    out = {}
    o, d = miss(n)
    co, cd = cross(n // 64)
    o[::64], d[::64] = co, cd
    out["tails"] = (o, d)
    out["misses"] = miss(n)
    out["first"] = first(n)
    parts = [cross(1366), miss(1365), first(1365)]
    o, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    perm = rng.permutation(n)
    out["mixed"] = (o[perm], d[perm])
    kinds = np.concatenate([np.zeros(1366, int), np.ones(1365, int), np.full(1365, 2)])[perm]
    return desc, {k: (v[0].astype(np.float32), v[1].astype(np.float32)) for k, v in out.items()}, kinds


def test_wall_conditions(pkg, orc):
    """Case 4 with the oracle and the restated setup: in 'tails' exactly the 64 crossing rays hit,
    each after at least 100 cells, and the others fail setup; 'misses' hits nothing and enters no
    cell; every ray of 'first' hits in its walk's first cell (one cell read); in 'mixed' each class
    is a third of the rays (at least a fifth)."""
    desc, batches, kinds = wall_case(pkg)
    rows = {k: expected(pkg, orc, desc, make_rays(pkg.abi, o, d, 1e34), 0, NO_RANGE, True) for k, (o, d) in batches.items()}
    t = rows["tails"]
    assert (t[::64, 4] == 0).all() and (t[::64, 6] >= 100).all() and int((t[:, 4] >= 0).sum()) == 64
    assert all(c is None for j, c in enumerate(first_cells(desc, *batches["tails"])) if j % 64)
    assert (rows["misses"][:, 4] == -2).all() and not rows["misses"][:, 6].any()
    assert (rows["first"][:, 4] == 0).all() and (rows["first"][:, 6] == 1).all()
    m = rows["mixed"]
    assert (m[kinds == 0, 6] >= 100).all() and (m[kinds == 1, 4] == -2).all() and (m[kinds == 2, 6] == 1).all()
    assert min(np.bincount(kinds)) * 5 >= len(kinds)


def test_scene_s_shape_wins(pkg, orc):
    """Case 1: with the shapes on, at least 50 of S's rays end on the sphere or the triangle."""
    desc, o, d, tmax = case_s(pkg, orc)
    got = expected(pkg, orc, desc, make_rays(pkg.abi, o, d, tmax), 0, NO_RANGE, True)
    assert int((got[:, 4] == -1).sum()) >= 50
