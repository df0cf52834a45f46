"""Spheres, triangles and BasicBVH: the oracle against an independent restatement (CPU).

tests/shapes_ref.py restates Sphere::Hit / IsHit, Triangle::Hit / IsHit (src/BVH/Shapes.h:12-139),
the shape stages of Renderer::FindNearest (renderer.cpp:995-1016) and Renderer::IsOccluded
(:231-240) and BasicBVH::IntersectTri / IntersectAABB / IntersectBVH (src/BVH/BasicBVH.cpp:18-61)
in numpy float32 from the reference text.  Here oracle_find_nearest, oracle_is_occluded,
oracle_trace and oracle_bvh_intersect are compared with it bit for bit (t, normal, material,
voxel index, inside flag, occlusion bytes, cell counts; NaN lanes as masks): hand-derived
known answers, a table of edges, 4099 random rays over a room where volumes and shapes
compete, whole paths at depth 1 and 2, and BVH rays with zero direction components, NaN
slabs and the deepest tree vpx_bvh_set accepts.  Every condition that keeps the comparisons
from being vacuous (arm coverage, shares, sensitivity to the readings that differ) is
computed from the restatement alone.  test_kat_shapes_gpu.py runs the same cases on the device.

The restatement walks every ray in Python: the random set (computed once, shared with the GPU
file) takes about 15 s on a CPU core and the BVH sets about 10 s; the device needs milliseconds.
"""
import functools

import numpy as np
import pytest

import shapes_ref as sr
from shapes_ref import EPS, ShapeScene, make_ray, sphere, triangle
from test_bvh import lib_build, tri_array
from test_kat_paths import BIG, N, NONE, SEEDS, Rng, Vol, api_rays, f32, fbits, kat_scene, normalize, to_oracle, v3

pytestmark = [pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning"),   # 1/0 = inf, as the reference
              pytest.mark.filterwarnings("ignore:invalid value:RuntimeWarning")]    # 0/0, 0*inf = NaN, as the reference

SKY = (0.392, 0.584, 0.829)
N_RAYS = 4099  # sixteen workgroups of 256 plus three lanes
ULP = f32(2.0 ** -23)


def below(x):  # one ulp towards zero
    return np.nextafter(f32(x), f32(0))


# --------------------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def world(key):
    """'E': an empty 16^3 grid (the shapes alone); 'R<m>': the KAT room with a wall of material m."""
    if key == "E":
        return np.full(N * N * N, NONE, np.uint8)
    return kat_scene(int(key[1:]))[0]


def lights():
    _, mats, points, d = kat_scene(0)
    return mats, points, d


def scene_of(key, spheres, tris, **kw):
    mats, points, d = lights()
    return ShapeScene([Vol(world(key), N)], mats, points, spheres=spheres, triangles=tris, dir_light=d, **kw)


def desc_of(pkg, key, spheres, tris):
    """The same scene as a SceneDesc (the oracle's and the device's)."""
    abi = pkg.abi
    mats, points, d = lights()
    desc = to_oracle(pkg, None, world(key), mats, points, d, [Vol(world(key), N)])
    fl = lambda a: tuple(float(x) for x in a)
    desc.spheres = [abi.Sphere(abi.vec3(fl(c)), float(r), m) for c, r, m in spheres]
    desc.triangles = [abi.Triangle(abi.vec3(fl(p)), abi.vec3(fl(a)), abi.vec3(fl(b)), abi.vec3(fl(c)), m)
                      for p, a, b, c, m in tris]
    return desc


# ----------------------------------------------------------------------- expectations
REC = np.dtype([("t", "<u4"), ("normal", "<u4", 3), ("vox", "<i4"), ("material", "<u4"), ("cells", "<u4"),
                ("inside", "<u4")])


def expect(key, spheres, tris, rays, raw=False, **variant):
    """The restatement's records for rays = [(o, d, tmax, inside)]: a dict with
    near (REC rows, the vpx_hit fields), vol (the same before the shape stage: what the entries
    give without the shapes), occ / occ_cells (IsOccluded), occ_vol / occ_vol_cells (without
    the shapes), arms (the shape functions' arms), second (rays whose D the second
    normalisation changed), behind (volume wins with a shape hit behind them)."""
    n = len(rays)
    near, vol = np.zeros(n, REC), np.zeros(n, REC)
    occ, occ_cells = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    occ_vol, occ_vol_cells = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    arms, second, behind = set(), 0, 0

    for i, (o, d, tmax, inside) in enumerate(rays):
        s = scene_of(key, spheres, tris, **variant)
        r = make_ray(v3(*o), v3(*d), tmax, inside, raw)
        vox = s.find_nearest(r)
        near[i] = (fbits(r.t), fbits(r.N), vox, r.mat, s.cells, int(r.inside))
        vt, vn, vm, vvox, vin = s.volume_stage  # the shapes read no cell: the count is the volume loop's
        vol[i] = (fbits(vt), fbits(vn), vvox, vm, s.cells, int(vin))
        second += int(np.any(fbits(normalize(r.D)) != fbits(r.D)))
        behind += int(vox >= 0 and s.shape_t < BIG)  # a volume won and the fresh ray met a shape, not nearer
        s2 = scene_of(key, spheres, tris, **variant)
        r = make_ray(v3(*o), v3(*d), tmax, inside, raw)
        occ[i], occ_cells[i] = s2.is_occluded(r), s2.cells
        occ_vol[i], occ_vol_cells[i] = s2.volume_occluded, s2.cells
        arms |= s.shape_arms | s2.shape_arms
    return dict(near=near, vol=vol, occ=occ, occ_cells=occ_cells, occ_vol=occ_vol, occ_vol_cells=occ_vol_cells,
                arms=arms, second=second, behind=behind)


def hit_records(hits, n):
    """A ctypes array of abi.Hit (or its bytes as uint32 [n, 8]) as REC rows."""
    raw = np.frombuffer(hits, np.uint32, count=8 * n) if not isinstance(hits, np.ndarray) else hits
    return np.ascontiguousarray(raw).reshape(-1).view(REC)[:n]


def same_records(got, want, what):
    """Bit for bit; a NaN's sign and payload apart (t and the normal's lanes as NaN masks)."""
    for name in ("vox", "material", "cells", "inside"):
        bad = np.flatnonzero(got[name] != want[name])
        assert not len(bad), (what, name, bad[:8], got[bad[:4]], want[bad[:4]])
    for name in ("t", "normal"):
        g, w = got[name].view(np.float32), want[name].view(np.float32)
        gn, wn = np.isnan(g), np.isnan(w)
        assert np.array_equal(gn, wn), (what, name, "NaN mask")
        bad = np.argwhere((got[name] != want[name]) & ~gn)
        assert not len(bad), (what, name, bad[:8], g[tuple(bad[0])], w[tuple(bad[0])])


# ------------------------------------------------------------- 1. hand-derived known answers
UNIT = sphere((0, 0, 0), 1, 0)
TRI_X3 = triangle((1, 0, 0), (2, -1, -1), (2, 1, -1), (2, 0, 1), 6)  # in the plane x = 3, normal +x
KNOWN = [
    # (what, spheres, triangles, (o, d, tmax, inside), t, normal, material, vox, inside after, occluded)
    ("head on", [UNIT], [], ((0, 0, -3), (0, 0, 1), 1e34, 0), 2.0, (0.0, 0.0, -1.0), 0, -1, 0, 1),
    ("tangent", [UNIT], [], ((0, 1, -3), (0, 0, 1), 1e34, 0), 3.0, (-0.0, -1.0, -0.0), 0, -1, 1, 1),
    ("on the surface, heading in", [UNIT], [], ((0, 0, -1), (0, 0, 1), 1e34, 0), 0.0, (0.0, 0.0, -1.0), 0, -1, 0, 1),
    ("on the surface, heading out", [UNIT], [], ((0, 0, 1), (0, 0, 1), 1e34, 0), 1e34, (0.0, 0.0, 0.0), NONE, -2, 0, 0),
    ("triangle, back face", [], [TRI_X3], ((0, 0, 0), (1, 0, 0), 1e34, 0), 3.0, (-1.0, -0.0, -0.0), 6, -1, 0, 1),
    ("triangle, front face", [], [TRI_X3], ((6, 0, 0), (-1, 0, 0), 1e34, 0), 3.0, (1.0, 0.0, 0.0), 6, -1, 0, 1),
]


@pytest.mark.parametrize("case", KNOWN, ids=[k[0] for k in KNOWN])
def test_known_answers(pkg, orc, case):
    """Exactly representable inputs: the expected record is a literal worked out by hand from
    Shapes.h, and both the oracle and the restatement give it."""
    what, spheres, tris, ray, t, nrm, mat, vox, inside, occluded = case
    want = np.zeros(1, REC)
    want[0] = (fbits(f32(t)), fbits(v3(*nrm)), vox, mat, 0, inside)
    e = expect("E", spheres, tris, [ray])
    want["cells"] = e["near"]["cells"]  # the empty grid's walk where the ray crosses its cube: not this test's subject
    same_records(e["near"], want, what + " (restatement)")
    assert int(e["occ"][0]) == occluded
    o = orc.Oracle(pkg.abi, desc_of(pkg, "E", spheres, tris))
    rays = api_rays(pkg.abi, [ray])
    same_records(hit_records(o.find_nearest(rays), 1), want, what + " (oracle)")
    assert int(o.is_occluded(rays)[0][0]) == occluded


# -------------------------------------------------------------------------- 2. the edge table
AX = (0.53, 0.47)  # the x, y of the axis-parallel room rays: off every cell plane, so no 0 * inf in the DDA
T_Y = triangle((0, 0, 0), (3, 0, 0), (3, 1, 0), (3, 0, 1), 0)      # +x rays: u = O.y, v = O.z, t = 3 - O.x exactly
T_0 = triangle((0, 0, 0), (0, 0, 0), (0, 1, 0), (0, 0, 1), 0)      # the same in the plane x = 0: t = -O.x exactly
T_A = triangle((0, 0, 0), (3, -1, -1), (3, 1, -1), (3, 0, 1), 0)   # TRI_X3's plane and outline, position zero
T_FAR = triangle((0, 0, 0), (5, -1, -1), (5, 1, -1), (5, 0, 1), 15)
# the position outweighs the vertices: pos + v rounds away low bits of v, so (pos + v1) - (pos + v0) != v1 - v0
T_MANY = triangle((3.1234567, 1.7654321, -2.3333333), (0.1, -1.05, -1.02), (-0.1, 1.01, -0.97), (0.05, 0.03, 1.04), 6)
S_B = sphere((0, 0, 1), 2, 6)      # (0, 0, -3) + z reaches it at t = 2 as it reaches UNIT
S_FAR = sphere((0, 0, 5), 1, 15)   # the same ray reaches it at t = 7


def eps_tri(a):  # a = dot(edge1, cross(D, edge2)) = edge1.z for D = +x and edge2 = +y
    return triangle((0, 0, 0), (3, 0, 0), (3, 0, a), (3, 1, 0), 0)


def eps_ray(a):  # u = v = 1/4
    return ((0, 0.25, f32(a) * f32(0.25)), (1, 0, 0), 1e34, 0)


def _tie_sphere():
    """A sphere that the room ray along +z from (AX, -1) reaches at exactly the wall's t = 1.75."""
    return sphere((AX[0], AX[1], 1), 0.25, 6)


ROOM_RAY = ((AX[0], AX[1], -1), (0, 0, 1))
HEAD = ((0, 0, -3), (0, 0, 1))
PX = ((0, 0, 0), (1, 0, 0))
EDGES = [
    # (group, world, spheres, triangles, [(what, o, d, tmax, inside)])
    ("unit sphere", "E", [UNIT], [], [
        ("head on", *HEAD, 1e34, 0), ("head on, unnormalised D", (0, 0, -3), (0, 0, 2.5), 1e34, 0),
        ("tangent: disc = 0, inside flag", (0, 1, -3), (0, 0, 1), 1e34, 0),
        ("disc just below 0", (0, f32(1) + ULP, -1), (0, 0, 1), 1e34, 0),
        ("disc below 0, far origin", (0, f32(1) + f32(2.0 ** -20), -3), (0, 0, 1), 1e34, 0),
        ("on the surface, heading in", (0, 0, -1), (0, 0, 1), 1e34, 0),
        ("on the surface, heading out", (0, 0, 1), (0, 0, 1), 1e34, 0),
        ("origin inside", (0.25, 0, 0), (0, 0, 1), 1e34, 0), ("origin at the centre", (0, 0, 0), (0, 1, 0), 1e34, 0),
        ("behind the origin", (0, 0, 3), (0, 0, 1), 1e34, 0),
        ("beyond tmax", *HEAD, 1.5, 0), ("exactly at tmax", *HEAD, 2.0, 0), ("just inside tmax", *HEAD, 2.25, 0),
        ("inside_glass, sphere win from outside", *HEAD, 1e34, 1), ("inside_glass, miss", (5, 5, -3), (0, 0, 1), 1e34, 1),
        ("oblique", (0.3, -0.2, -3), (0.05, 0.1, 1), 1e34, 0),
    ]),
    ("zero radius, aimed dead on", "E", [sphere((0, 0, 2), 0, 6)], [], [("dead on", (0, 0, 0), (0, 0, 1), 1e34, 0),
                                                                       ("beside", (0.5, 0, 0), (0, 0, 1), 1e34, 0)]),
    ("negative radius", "E", [sphere((0, 0, 0), -1, 6)], [], [("head on", *HEAD, 1e34, 0)]),
    ("two spheres at equal t, a b", "E", [UNIT, S_B], [], [("tie", *HEAD, 1e34, 0), ("tie, tmax = t", *HEAD, 2.0, 0)]),
    ("two spheres at equal t, b a", "E", [S_B, UNIT], [], [("tie", *HEAD, 1e34, 0)]),
    ("near then far sphere", "E", [UNIT, S_FAR], [], [("through both", *HEAD, 1e34, 0), ("between", *HEAD, 5.0, 0)]),
    ("far then near sphere", "E", [S_FAR, UNIT], [], [("through both", *HEAD, 1e34, 0)]),
    ("two triangles at equal t, a b", "E", [], [T_A, TRI_X3], [("tie", *PX, 1e34, 0), ("tie, tmax = t", *PX, 3.0, 0),
                                                               ("tmax below t", *PX, 2.0, 0)]),
    ("two triangles at equal t, b a", "E", [], [TRI_X3, T_A], [("tie", *PX, 1e34, 0)]),
    ("near then far triangle", "E", [], [T_A, T_FAR], [("through both", *PX, 1e34, 0), ("from behind", (9, 0, 0), (-1, 0, 0), 1e34, 0)]),
    ("far then near triangle", "E", [], [T_FAR, T_A], [("through both", *PX, 1e34, 0)]),
    ("sphere and triangle", "E", [sphere((3, 0, 0), 0.5, 8)], [T_A], [("sphere first", *PX, 1e34, 1),
                                                                      ("origin inside the sphere, triangle wins", (2.75, 0, 0.1), (1, 0, 0), 1e34, 1)]),
    ("a = +0.0001f exactly", "E", [], [eps_tri(EPS)], [("proceeds", *eps_ray(EPS))]),
    ("a = -0.0001f exactly", "E", [], [eps_tri(-EPS)], [("proceeds", *eps_ray(-EPS))]),
    ("a one ulp inside +", "E", [], [eps_tri(below(EPS))], [("rejected", *eps_ray(EPS))]),
    ("a one ulp inside -", "E", [], [eps_tri(below(-EPS))], [("rejected", *eps_ray(-EPS))]),
    ("degenerate triangle", "E", [], [triangle((0, 0, 0), (3, 0, 0), (3, 0, 0), (3, 0, 0), 0),
                                      triangle((0, 0, 0), (3, 0, 0), (3, 1, 1), (3, 2, 2), 0)], [("through it", *PX, 1e34, 0)]),
    ("barycentric edges", "E", [], [T_Y], [
        ("u = 0", (0, 0, 0.5), (1, 0, 0), 1e34, 0), ("u = 1 and v = 0", (0, 1, 0), (1, 0, 0), 1e34, 0),
        ("v = 0", (0, 0.5, 0), (1, 0, 0), 1e34, 0), ("u + v = 1", (0, 0.5, 0.5), (1, 0, 0), 1e34, 0),
        ("u = v = 0", (0, 0, 0), (1, 0, 0), 1e34, 0), ("u < 0", (0, -0.125, 0.5), (1, 0, 0), 1e34, 0),
        ("u > 1", (0, 1.5, 0.25), (1, 0, 0), 1e34, 0), ("v < 0", (0, 0.5, -0.125), (1, 0, 0), 1e34, 0),
        ("u + v > 1", (0, 0.75, 0.75), (1, 0, 0), 1e34, 0), ("u + v one ulp above 1", (0, 0.5, f32(0.5) + ULP), (1, 0, 0), 1e34, 0),
        ("from behind", (6, 0.25, 0.25), (-1, 0, 0), 1e34, 0), ("parallel", (0, 0.25, 0.25), (0, 1, 0), 1e34, 0),
    ]),
    ("t = 0.0001f exactly", "E", [], [T_0], [
        ("t = eps: Hit rejects, IsHit accepts", (-EPS, 0.25, 0.25), (1, 0, 0), 1e34, 0),
        ("t one ulp above eps", (-np.nextafter(EPS, f32(1)), 0.25, 0.25), (1, 0, 0), 1e34, 0),
        ("t below eps", (-EPS * f32(0.5), 0.25, 0.25), (1, 0, 0), 1e34, 0),
        ("t = eps = tmax", (-EPS, 0.25, 0.25), (1, 0, 0), EPS, 0),
        ("behind", (1, 0.25, 0.25), (1, 0, 0), 1e34, 0),
    ]),
    ("position with many mantissa bits", "E", [], [T_MANY], [
        (f"ray {k}", (0.01 * k, 1.69 + 0.013 * k, -2.4 + 0.021 * k), (1, 0.003 * k, -0.002 * k), 1e34, 0) for k in range(12)
    ] + [("from behind", (7, 1.8, -2.3), (-1, 0.01, 0.02), 1e34, 0)]),
    ("room: sphere and wall at equal t", "R0", [_tie_sphere()], [], [("the volume keeps it", *ROOM_RAY, 1e34, 0),
                                                                    ("inside_glass, volume win", *ROOM_RAY, 1e34, 1)]),
    ("room: sphere nearer than the wall", "R0", [sphere((AX[0], AX[1], 0.3), 0.125, 6)], [], [
        ("shape win", *ROOM_RAY, 1e34, 0), ("inside_glass, sphere win", *ROOM_RAY, 1e34, 1),
        ("shape beyond tmax", *ROOM_RAY, 1.0, 0), ("past the sphere, wall beyond tmax", *ROOM_RAY, 1.5, 1)]),
    ("room: sphere behind the wall", "R0", [sphere((AX[0], AX[1], 1.5), 0.25, 6)], [], [
        ("volume win", *ROOM_RAY, 1e34, 0), ("inside_glass, volume win", *ROOM_RAY, 1e34, 1)]),
    ("room: triangle in front of the wall", "R0", [], [triangle((0.5, 0.5, 0.5), (-0.25, -0.25, 0), (0.25, -0.25, 0), (0, 0.25, 0), 15)], [
        ("inside_glass, triangle win", *ROOM_RAY, 1e34, 1), ("triangle win", *ROOM_RAY, 1e34, 0),
        ("beside the triangle, wall", (0.2, 0.7, -1), (0, 0, 1), 1e34, 1), ("inside_glass, miss", (0.53, 0.95, -1), (0, 0, 1), 1e34, 1)]),
]
EDGE_IDS = [g[0] for g in EDGES]


@functools.lru_cache(maxsize=None)
def edge_expect(i, raw=False):
    g = EDGES[i]
    rays = [r[1:] for r in g[4]]
    if raw:  # the direction handed over normalised: the restatement skips only the first normalisation
        rays = [(o, normalize(v3(*d)), t, ins) for o, d, t, ins in rays]
    return expect(g[1], g[2], g[3], rays, raw=raw)


def edge_rays(i, raw=False):
    rays = [r[1:] for r in EDGES[i][4]]
    return [(o, normalize(v3(*d)), t, ins) for o, d, t, ins in rays] if raw else rays


@pytest.mark.parametrize("i", range(len(EDGES)), ids=EDGE_IDS)
def test_edge_table(pkg, orc, i):
    group, key, spheres, tris, rows = EDGES[i]
    e = edge_expect(i)
    o = orc.Oracle(pkg.abi, desc_of(pkg, key, spheres, tris))
    rays = api_rays(pkg.abi, edge_rays(i))
    same_records(hit_records(o.find_nearest(rays), len(rows)), e["near"], group)
    occ, cells = o.is_occluded(rays)
    assert np.array_equal(occ, e["occ"]), (group, occ, e["occ"])
    assert np.array_equal(cells, e["occ_cells"]), group


def _row(i, what):
    k = [r[0] for r in EDGES[i][4]].index(what)
    e = edge_expect(i)
    return e["near"][k], int(e["occ"][k])


def test_edge_rows_do_what_they_are_named_for():
    """The rows' outcomes, from the restatement alone (so a row cannot silently stop being an edge)."""
    gi = EDGE_IDS.index
    f = lambda x: int(fbits(f32(x)))
    u = gi("unit sphere")
    for what, vox, occ in (("head on", -1, 1), ("tangent: disc = 0, inside flag", -1, 1), ("disc just below 0", -2, 0),
                           ("disc below 0, far origin", -2, 0), ("on the surface, heading in", -1, 1),
                           ("on the surface, heading out", -2, 0), ("origin inside", -2, 0), ("behind the origin", -2, 0),
                           ("beyond tmax", -2, 0), ("exactly at tmax", -2, 1), ("just inside tmax", -1, 1)):
        r, o = _row(u, what)
        assert (int(r["vox"]), o) == (vox, occ), what
    assert _row(u, "tangent: disc = 0, inside flag")[0]["inside"] == 1
    assert _row(u, "inside_glass, sphere win from outside")[0]["inside"] == 0
    assert _row(u, "inside_glass, miss")[0]["inside"] == 1
    z, _ = _row(gi("zero radius, aimed dead on"), "dead on")
    assert z["t"] == f(2) and z["inside"] == 1 and np.isnan(z["normal"].view(np.float32)).all()
    assert _row(gi("negative radius"), "head on")[0]["inside"] == 1
    # ties: a later sphere overwrites, a later triangle does not
    assert _row(gi("two spheres at equal t, a b"), "tie")[0]["material"] == 6
    assert _row(gi("two spheres at equal t, b a"), "tie")[0]["material"] == 0
    assert _row(gi("two triangles at equal t, a b"), "tie")[0]["material"] == 0
    assert _row(gi("two triangles at equal t, b a"), "tie")[0]["material"] == 6
    r, o = _row(gi("two triangles at equal t, a b"), "tie, tmax = t")
    assert (int(r["vox"]), o) == (-2, 1)  # not nearer for FindNearest, occluded for IsOccluded
    for sign in "+-":
        assert _row(gi(f"a = {sign}0.0001f exactly"), "proceeds")[0]["vox"] == -1
        assert _row(gi(f"a one ulp inside {sign}"), "rejected")[0]["vox"] == -2
    assert _row(gi("degenerate triangle"), "through it")[0]["vox"] == -2
    b = gi("barycentric edges")
    for what in ("u = 0", "u = 1 and v = 0", "v = 0", "u + v = 1", "u = v = 0", "from behind"):
        assert _row(b, what)[0]["vox"] == -1 and _row(b, what)[0]["t"] in (f(3), f(2.75)), what
    for what in ("u < 0", "u > 1", "v < 0", "u + v > 1", "u + v one ulp above 1", "parallel"):
        assert _row(b, what)[0]["vox"] == -2, what
    t0 = gi("t = 0.0001f exactly")
    assert (int(_row(t0, "t = eps: Hit rejects, IsHit accepts")[0]["vox"]), _row(t0, "t = eps: Hit rejects, IsHit accepts")[1]) == (-2, 1)
    assert (int(_row(t0, "t one ulp above eps")[0]["vox"]), _row(t0, "t one ulp above eps")[1]) == (-1, 1)
    assert (int(_row(t0, "t below eps")[0]["vox"]), _row(t0, "t below eps")[1]) == (-2, 0)
    assert _row(t0, "t = eps = tmax")[1] == 1
    # the room: who wins, and what happens to a flag the caller passed in
    tie = gi("room: sphere and wall at equal t")
    r, _ = _row(tie, "the volume keeps it")
    assert r["vox"] == 0 and r["t"] == f(1.75)
    alone = expect("E", [_tie_sphere()], [], [(*ROOM_RAY, 1e34, 0)])["near"][0]
    assert alone["vox"] == -1 and alone["t"] == f(1.75)  # the sphere alone is hit at the wall's t
    assert _row(tie, "inside_glass, volume win")[0]["inside"] == 1
    near = gi("room: sphere nearer than the wall")
    assert _row(near, "shape win")[0]["vox"] == -1 and _row(near, "inside_glass, sphere win")[0]["inside"] == 0
    r, o = _row(near, "shape beyond tmax")
    assert (int(r["vox"]), o) == (-2, 0)
    r, o = _row(near, "past the sphere, wall beyond tmax")
    assert (int(r["vox"]), int(r["inside"]), o) == (-1, 0, 1)
    st = gi("sphere and triangle")
    assert _row(st, "sphere first")[0]["material"] == 8 and _row(st, "origin inside the sphere, triangle wins")[0]["material"] == 0
    assert _row(st, "origin inside the sphere, triangle wins")[0]["inside"] == 0
    far = gi("room: sphere behind the wall")
    assert _row(far, "volume win")[0]["vox"] == 0 and _row(far, "inside_glass, volume win")[0]["inside"] == 1
    tr = gi("room: triangle in front of the wall")
    assert _row(tr, "inside_glass, triangle win")[0]["vox"] == -1 and _row(tr, "inside_glass, triangle win")[0]["inside"] == 0
    assert _row(tr, "beside the triangle, wall")[0]["vox"] == 0 and _row(tr, "beside the triangle, wall")[0]["inside"] == 1
    assert _row(tr, "inside_glass, miss")[0]["vox"] == -2 and _row(tr, "inside_glass, miss")[0]["inside"] == 1


def test_edges_are_sensitive_to_the_vertex_offset():
    """Forming the edges from the raw vertices, v1 - v0 for (pos + v1) - (pos + v0), changes t
    for at least one row of the many-bit triangle."""
    i = EDGE_IDS.index("position with many mantissa bits")
    g = EDGES[i]
    wrong = expect(g[1], g[2], g[3], edge_rays(i), raw_edges=True)
    changed = int((wrong["near"]["t"] != edge_expect(i)["near"]["t"]).sum())
    print(f"vertex offset: raw edges change t in {changed} of {len(g[4])} rows")
    assert changed >= 1 and int((edge_expect(i)["near"]["vox"] == -1).sum()) >= 8


# ------------------------------------------------------------------------ 3. the random set
R_SPHERES = [sphere((0.3, 0.5, 0.4), 0.12, 0), sphere((0.72, 0.6, 0.45), 0.1, 8), sphere((0.5, 0.5, 1.3), 0.25, 6)]
R_TRIS = [triangle((0.5, 0.45, 0.62), (-0.2, -0.2, 0.0), (0.2, -0.2, 0.05), (0.0, 0.25, 0.0), 15),
          triangle((-0.35, 0.5, 0.5), (0.0, -0.3, -0.3), (0.0, 0.3, -0.3), (0.05, 0.0, 0.35), 11)]


@functools.lru_cache(maxsize=None)
def random_rays():
    """4099 rays in and around the KAT room, aimed at the three spheres and two triangles and at
    the room itself, a third of them bounded near their target: [(o, d, tmax, inside)]."""
    rng = np.random.default_rng(20)
    targets = [np.array(s[0], np.float64) for s in R_SPHERES] + [np.array(t[0], np.float64) + 0.02 for t in R_TRIS]
    rays = []
    for k in range(N_RAYS):
        o = rng.uniform(-0.9, 1.9, 3)
        if k % 5 == 4:
            tgt = rng.uniform(0.05, 0.95, 3)
        else:
            tgt = targets[k % 5 if k % 5 < 4 else 0] + rng.normal(0, 0.08, 3)
            if k % 10 == 3:
                tgt = targets[4] + rng.normal(0, 0.08, 3)
        if k % 7 == 0:  # through the wall towards the sphere behind it
            o = np.array([rng.uniform(0.25, 0.75), rng.uniform(0.25, 0.75), rng.uniform(-0.9, 0.3)])
            tgt = targets[2] + rng.normal(0, 0.05, 3)
        d = (tgt - o) * rng.uniform(0.5, 2.0)
        dist = float(np.linalg.norm(tgt - o))
        tmax = 1e34 if k % 3 else dist * rng.uniform(0.6, 1.4)
        rays.append((tuple(np.float32(o)), tuple(np.float32(d)), float(np.float32(tmax)), int(k % 4 == 1)))
    return rays


@functools.lru_cache(maxsize=None)
def random_expect():
    return expect("R0", R_SPHERES, R_TRIS, random_rays())


def random_raw_rays():
    """The same rays with the direction handed over normalised (for VPX_QUERY_RAW_DIRECTION: the
    records are random_expect()'s, since only the first normalisation is skipped)."""
    return [(o, normalize(v3(*d)), t, ins) for o, d, t, ins in random_rays()]


def test_random_set(pkg, orc):
    e = random_expect()
    near = e["near"]
    shape_wins = int((near["vox"] == -1).sum())
    print(f"random set: {shape_wins} shape wins, {int((near['vox'] >= 0).sum())} volume wins, "
          f"{int((near['vox'] == -2).sum())} misses of {N_RAYS}; second normalisation changes D for {e['second']}; "
          f"{e['behind']} volume wins with a shape behind; occluded {int(e['occ'].sum())}, by the volume alone "
          f"{int(e['occ_vol'].sum())}; flags cleared {int(((near['inside'] == 0) & np.array([r[3] for r in random_rays()], bool)).sum())}")
    assert shape_wins * 4 >= N_RAYS
    assert e["second"] * 10 >= N_RAYS
    assert e["behind"] >= 50
    assert int((e["occ"] != e["occ_vol"]).sum()) >= 100  # rays that only a shape occludes
    o = orc.Oracle(pkg.abi, desc_of(pkg, "R0", R_SPHERES, R_TRIS))
    rays = api_rays(pkg.abi, random_rays())
    same_records(hit_records(o.find_nearest(rays), N_RAYS), near, "random set")
    occ, cells = o.is_occluded(rays)
    assert np.array_equal(occ, e["occ"]) and np.array_equal(cells, e["occ_cells"])


def test_random_set_is_sensitive_to_the_second_normalisation():
    """Without the second normalisation of renderer.cpp:997 the first 400 rays' records change."""
    sub = random_rays()[:400]
    right = random_expect()["near"][:400]
    wrong = expect("R0", R_SPHERES, R_TRIS, sub, second_normalize=False)["near"]
    changed = int(((wrong["t"] != right["t"]) | (wrong["normal"] != right["normal"]).any(axis=1)).sum())
    print(f"double normalisation: skipping it changes {changed} of 400 records")
    assert changed >= 10


def test_shape_arms_are_covered():
    """The union over the table and the random set holds every early-out and both outcomes of
    every branch of the four functions; the sphere's inside arm comes from the constructed rows."""
    arms = set(random_expect()["arms"])
    table = set()
    for i in range(len(EDGES)):
        table |= edge_expect(i)["arms"]
    print("arms, random set:", sorted(arms))
    print("arms, table only:", sorted(table - arms))
    assert sr.ALL_ARMS <= arms | table, sorted(sr.ALL_ARMS - (arms | table))
    assert arms | table <= sr.ALL_ARMS, sorted((arms | table) - sr.ALL_ARMS)
    assert ("sphere_hit", "inside") in table


# --------------------------------------------------------------------------- 4. whole paths
GLASS_IN = sphere((0.3, 0.3, 0.25), 0.125, 8)
# reaches the floor at about (0.35, 0.125, 0.35); the point light (0.5, 0.9, 0.2) and the directional light
# (arriving along (-0.3, -1, 0.4)) are both behind a shape placed at about (0.467, 0.6, 0.21)
FLOOR_RAY = ((-0.5, 0.6, 0.35), (0.85, -0.475, 0.003), False)
PATHS = [
    # (what, wall material, spheres, triangles, (o, d, inside), material the ray must reach first, -1 = a shape)
    *[(f"sphere {m}", 0, [sphere((AX[0], AX[1], 0.4), 0.125, m)], [], ((AX[0], AX[1], -0.8), (0.02, 0.03, 1.0), False), m)
      for m in (0, 6, 8, 11, 15, 20)],
    *[(f"triangle {m}", 0, [], [triangle((0.5, 0.5, 0.45), (-0.25, -0.25, 0.02), (0.25, -0.25, 0), (0, 0.25, -0.02), m)],
       ((AX[0], AX[1], -0.8), (0.02, 0.03, 1.0), False), m) for m in (0, 6, 8, 11, 15, 20)],
    ("floor shadowed by a sphere", 0, [sphere((0.467, 0.6, 0.21), 0.15, 15)], [], FLOOR_RAY, 20),
    ("floor shadowed by a triangle", 0, [], [triangle((0.467, 0.6, 0.21), (-0.2, 0, -0.2), (0.2, 0, -0.2), (0, 0.02, 0.25), 15)],
     FLOOR_RAY, 20),
    # the guard needs a SPHERE win that sets the flag: a hit from outside clears it, and a triangle win copies the
    # fresh ray's cleared flag, so only a sphere's inside arm (tangent, zero or negative radius) reaches it
    ("glass sphere, inside flag set", 0, [sphere((AX[0], AX[1], 0.4), -0.125, 8)], [], ((AX[0], AX[1], -0.8), (0.02, 0.03, 1.0), False), 8),
    ("smoke sphere, inside flag set", 0, [sphere((AX[0], AX[1], 0.4), -0.125, 11)], [], ((AX[0], AX[1], -0.8), (0.02, 0.03, 1.0), True), 11),
    ("glass triangle, inside flag set", 0, [], [triangle((0.5, 0.5, 0.45), (-0.25, -0.25, 0.02), (0.25, -0.25, 0), (0, 0.25, -0.02), 8)],
     ((AX[0], AX[1], -0.8), (0.02, 0.03, 1.0), True), 8),
    # refracted into the glass sphere (the flag is set, the path never leaves: origin inside never hits),
    # then the glass block behind it (x, y in [3/16, 6/16], z in [6/16, 9/16]) from the inside branch
    ("carried flag into the glass block", 0, [GLASS_IN], [], ((0.3, 0.3, -0.5), (0.01, 0.02, 1.0), False), 8),
]
PATH_IDS = [p[0] for p in PATHS]
DEPTHS = (1, 2)


def path_scene(i):
    what, wall, spheres, tris, ray, first = PATHS[i]
    mats, points, d = lights()
    return lambda: ShapeScene([Vol(world(f"R{wall}"), N)], mats, points, spheres=spheres, triangles=tris, dir_light=d)


@functools.lru_cache(maxsize=None)
def path_expect(i, depth):
    """The restatement's radiance per seed, the shadow-ray and cell totals, the arms and the guards."""
    what, wall, spheres, tris, (o, d, inside), first = PATHS[i]
    make = path_scene(i)
    rad, shadows, cells, arms, guards, shape_shadow = [], 0, 0, set(), 0, 0
    for seed in SEEDS:
        s = make()
        rad.append(s.trace(make_ray(v3(*o), v3(*d), BIG, inside), depth, Rng(seed)))
        shadows, cells, guards = shadows + s.shadows, cells + s.cells, guards + s.guards
        arms |= s.arms | s.shape_arms
    return dict(rad=np.array(rad, np.float32), shadows=shadows, cells=cells, arms=arms, guards=guards)


def path_rays(pkg, i):
    o, d, inside = PATHS[i][4]
    return api_rays(pkg.abi, [(o, d, 1e34, inside)] * len(SEEDS))


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("i", range(len(PATHS)), ids=PATH_IDS)
def test_paths_with_shapes(pkg, orc, i, depth):
    """Trace(ray, depth) over 24 seeds with a shape in front of the wall: radiance, shadow-ray and
    cell counts equal the restatement's."""
    what, wall, spheres, tris, (o, d, inside), first = PATHS[i]
    e = path_expect(i, depth)
    orac = orc.Oracle(pkg.abi, desc_of(pkg, f"R{wall}", spheres, tris))
    h = orac.find_nearest(api_rays(pkg.abi, [(o, d, 1e34, inside)]))[0]
    assert h.material == first and (h.vox_index == -1) == (first != 20 or "floor" not in what), (what, h.material, h.vox_index)
    got, st = orac.trace(path_rays(pkg, i), np.array(SEEDS, np.uint32), depth, SKY, 3)
    bad = [hex(s) for k, s in enumerate(SEEDS) if not np.array_equal(fbits(got[k]), fbits(e["rad"][k]))]
    assert not bad, (what, depth, bad)
    assert (st.shadow_rays, st.dda_cells) == (e["shadows"], e["cells"]), what


def test_path_arms_are_covered():
    """What the path cases exist for, from the restatement alone: the guard in the glass and the
    smoke branch, shadow rays that only a shape blocks, and the carried flag."""
    gi = PATH_IDS.index
    assert ("guard", "glass") in path_expect(gi("glass sphere, inside flag set"), 1)["arms"]
    assert ("guard", "smoke") in path_expect(gi("smoke sphere, inside flag set"), 1)["arms"]
    # a triangle win clears the flag: the glass branch runs from outside, no guard
    tri = path_expect(gi("glass triangle, inside flag set"), 1)
    assert tri["guards"] == 0 and any(a[:2] == ("glass", "outside") for a in tri["arms"])
    for what, fn in (("floor shadowed by a sphere", "sphere_is_hit"), ("floor shadowed by a triangle", "tri_is_hit")):
        i = gi(what)
        _, wall, spheres, tris, (o, d, inside), _ = PATHS[i]
        e = path_expect(i, 1)
        assert (fn, "len <= t", "nearer") in e["arms"] or (fn, "t <= ray.t", "nearer") in e["arms"], what
        # the same point without the shape is lit: only the shape blocks the shadow rays
        mats, points, dl = lights()
        lit = blocked = 0
        for seed in SEEDS:
            a = ShapeScene([Vol(world(f"R{wall}"), N)], mats, points, dir_light=dl)
            ra = a.trace(make_ray(v3(*o), v3(*d), BIG, inside), 0, Rng(seed))
            b = path_scene(i)()
            rb = b.trace(make_ray(v3(*o), v3(*d), BIG, inside), 0, Rng(seed))
            lit += int(a.shadows == 1 and np.any(ra != 0))
            blocked += int(b.shadows == 1 and not np.any(rb != 0))
        print(f"{what}: {lit} of {len(SEEDS)} seeds lit without the shape, {blocked} dark with it")
        assert lit == len(SEEDS) and blocked == len(SEEDS), what
    # the carried flag: refracted into the glass sphere at level 0, the glass block's inside branch at level 1
    c = path_expect(gi("carried flag into the glass block"), 2)
    carried = {a for a in c["arms"] if a[:2] == ("glass", "inside")}
    print("carried flag arms:", sorted(carried), "guards:", c["guards"])
    assert carried and c["guards"] == 0


# -------------------------------------------------------- 4b. a shape between an area light and the floor
# From FLOOR_RAY's hit point, about (0.35, 0.125, 0.35), the sphere covers most of the mixed set's first
# area light (samples in (0.3, 0.8, -0.6) + 0.3 * [0, 1]^3) and leaves the rest of it in view.
LIGHT_SPHERE = sphere((0.42, 0.5, 0.05), 0.08, 15)
LIGHT_SAMPLES = 15


def _mixed_lights():
    from test_kat_lights import LIGHT_SETS, lights_of

    kw = lights_of(LIGHT_SETS["mixed"])
    return kw.pop("points"), kw


def light_path_scene(spheres):
    mats, _, d = lights()
    points, kw = _mixed_lights()
    s = ShapeScene([Vol(world("R0"), N)], mats, points, spheres=spheres, dir_light=d, **kw)
    s.area_samples = LIGHT_SAMPLES
    return s


def light_path_desc(pkg):
    mats, _, d = lights()
    points, kw = _mixed_lights()
    desc = to_oracle(pkg, None, world("R0"), mats, points, d, [Vol(world("R0"), N)], **kw)
    c, r, m = LIGHT_SPHERE
    desc.spheres = [pkg.abi.Sphere(pkg.abi.vec3(tuple(float(x) for x in c)), float(r), m)]
    return desc


@functools.lru_cache(maxsize=None)
def light_path_expect(depth):
    """FLOOR_RAY over SEEDS with the mixed light set, 15 area samples and LIGHT_SPHERE: radiance,
    counts, and per seed the floor's pick with and without the sphere."""
    o, d, inside = FLOOR_RAY
    rad, shadows, cells, picks, arms = [], 0, 0, [], set()
    for seed in SEEDS:
        s, bare = light_path_scene([LIGHT_SPHERE]), light_path_scene([])
        rad.append(s.trace(make_ray(v3(*o), v3(*d), BIG, inside), depth, Rng(seed)))
        bare.trace(make_ray(v3(*o), v3(*d), BIG, inside), depth, Rng(seed))
        shadows, cells, arms = shadows + s.shadows, cells + s.cells, arms | s.shape_arms
        picks.append((s.picks[0], bare.picks[0]))
    return dict(rad=np.array(rad, np.float32), shadows=shadows, cells=cells, picks=picks, arms=arms)


@pytest.mark.parametrize("depth", DEPTHS)
def test_sphere_between_an_area_light_and_the_floor(pkg, orc, depth):
    """The shape stage of IsOccluded under AreaLightEvaluation: of one pick's 15 samples the sphere
    blocks some and not others (the same samples are all lit without it), and oracle_trace equals
    the restatement: radiance, shadow rays (a rejected sample sends none), cells."""
    e = light_path_expect(depth)
    area = [(p, q) for p, q in e["picks"] if p[0] == "area" and p[1] == 0]
    assert len(area) >= 2
    assert all(p[:3] == q[:3] for p, q in e["picks"])  # the sphere changes no draw before the pick
    assert any({"occluded", "lit"} <= set(p[3]) and set(q[3]) == {"lit"} for p, q in area), area
    assert ("sphere_is_hit", "len <= t", "nearer") in e["arms"]
    o, d, inside = FLOOR_RAY
    orac = orc.Oracle(pkg.abi, light_path_desc(pkg))
    got, st = orac.trace(api_rays(pkg.abi, [(o, d, 1e34, inside)] * len(SEEDS)), np.array(SEEDS, np.uint32), depth, SKY,
                         LIGHT_SAMPLES)
    bad = [hex(s) for k, s in enumerate(SEEDS) if not np.array_equal(fbits(got[k]), fbits(e["rad"][k]))]
    assert not bad, (depth, bad)
    assert (st.shadow_rays, st.dda_cells) == (e["shadows"], e["cells"])


# ---------------------------------------------------------------------------------- 5. BVH
def chain(abi, sign):
    """test_gpu_parity.chain_tris(abi, 64) (sign = 1: centroids at x = 2^i, a chain 63 deep) or
    its mirror (x = -2^i)."""
    v = np.zeros((64, 9), np.float32)
    x = f32(sign) * f32(2.0) ** np.arange(64, dtype=np.float32)
    v[:, 0], v[:, 3], v[:, 6] = x, x, x
    v[:, 4], v[:, 8] = 1.0, 1.0
    return tri_array(abi, v)


def bvh_sets(abi, orc):
    ref, _ = orc.BasicBVH.random_tris(abi)
    rng = np.random.default_rng(5)
    sets = {"reference-ctor": ref}
    for n in (1, 2, 3, 5, 64, 200):  # test_bvh.tri_sets' random sets
        a = rng.uniform(-5, 4, (n, 3))
        sets[f"random{n}"] = tri_array(abi, np.concatenate([a, a + rng.uniform(0, 1, (n, 3)), a + rng.uniform(0, 1, (n, 3))], 1))
    return sets


def bvh_rays(arrays, seed, count=24):
    """[(o, d, tmax)] chosen by reading the built tree: axis directions, one and two zero
    components in both signs, origins on a root or child slab plane with that component zero
    (a NaN slab), origins inside the root box, tmax at a node's entry distance, and bounds that
    an earlier leaf shortens (tmax = 1e34 through several triangles)."""
    bmin, bmax, left_first, tri_count, tri_idx, verts = arrays
    rng = np.random.default_rng(seed)
    cen = verts.mean(1)
    lo, hi = bmin[0].astype(np.float64), bmax[0].astype(np.float64)
    mid = (lo + hi) / 2
    rays = []
    for a in range(3):  # each axis direction +-, through a centroid, from outside and from inside the root box
        for sgn in (1.0, -1.0):
            c = cen[rng.integers(len(cen))].astype(np.float64)
            d = np.zeros(3)
            d[a] = sgn
            o = c.copy()
            o[a] = (lo[a] - 2) if sgn > 0 else (hi[a] + 2)
            rays.append((o, d.copy(), 1e34))
            rays.append((o, np.where(d == 0, -0.0, d), 1e34))  # the zero components negative: -inf slabs
            rays.append((c - d * 0.01, d.copy(), 1e34))
    boxes = [0] + ([int(left_first[0]), int(left_first[0]) + 1] if tri_count[0] == 0 else [])
    for b in boxes:  # origins exactly on a slab plane of the box, that direction component +-0: 0 / 0 = NaN
        for a in range(3):
            for plane in (bmin[b][a], bmax[b][a]):
                for z in (0.0, -0.0):
                    c = cen[rng.integers(len(cen))].astype(np.float64)
                    k = (a + 1) % 3
                    o = c.copy()
                    o[a], o[k] = float(plane), lo[k] - 1.5
                    d = (c - o)
                    d[a] = z
                    rays.append((o, d, 1e34))
    for _ in range(count):  # one zero component, either sign, aimed at a centroid; some from inside the root box
        c = cen[rng.integers(len(cen))].astype(np.float64) + rng.normal(0, 0.05, 3)
        o = rng.uniform(lo - 3, hi + 3) if rng.random() < 0.6 else rng.uniform(lo, hi)
        a = int(rng.integers(3))
        o[a] = c[a]
        d = c - o
        d[a] = 0.0 if rng.random() < 0.5 else -0.0
        rays.append((o, d, 1e34))
    for _ in range(count):  # general position, unbounded and bounded
        c = cen[rng.integers(len(cen))].astype(np.float64) + rng.normal(0, 0.05, 3)
        o = rng.uniform(lo - 3, hi + 3)
        rays.append((o, c - o, 1e34 if rng.random() < 0.5 else float(np.linalg.norm(c - o)) * rng.uniform(0.7, 1.3)))
    for a in range(3):  # tmax equal to the root's entry distance (tmin < ray.t fails), and one ulp more
        o = mid.copy()
        o[a] = float(f32(lo[a])) - 2.0
        d = np.zeros(3)
        d[a] = 1.0
        entry = f32(f32(bmin[0][a]) - f32(o[a]))
        rays.append((o, d, float(entry)))
        rays.append((o, d, float(np.nextafter(entry, f32(np.inf)))))
    return [(tuple(np.float32(o)), tuple(np.float32(d)), float(np.float32(t))) for o, d, t in rays]


def chain_rays(sign):
    """Rays along +-x through every triangle of a chain (from between each pair of neighbours,
    both ways, and from either end), and rays that miss."""
    rays = []
    for i in range(64):
        x = sign * 1.5 * 2.0 ** i
        for d in (1.0, -1.0):
            rays.append(((x, 0.25, 0.25), (d, 0.0, 0.0), 1e34))
    for o, d in (((sign * -1.0, 0.25, 0.25), (sign * 1.0, 0, 0)), ((sign * 2.0 ** 64, 0.25, 0.25), (sign * -1.0, 0, 0)),
                 ((sign * -1.0, 0.3, 0.1), (sign * 1.0, 0.0, -0.0)), ((sign * -1.0, 2.0, 0.25), (sign * 1.0, 0, 0)),
                 ((sign * 3.0, 0.25, 5.0), (0, 0, -1.0)), ((sign * -1.0, 0.75, 0.75), (sign * 1.0, 0, 0)),
                 ((sign * -1.0, 0.25, 0.25), (sign * -1.0, 0, 0)), ((sign * -1.0, 0.0, 0.25), (sign * 1.0, 0, 0)),
                 ((sign * -1.0, 0.25, 0.0), (sign * 1.0, 0, -0.0)), ((sign * -1.0, 0.0, 0.25), (sign * 1.0, -0.0, 0)), ((sign * 2.0 ** 40, 0.1, 0.1), (sign * 1.0, 1e-14, 0))):
        rays.append((o, d, 1e34))
    return [(tuple(np.float32(o)), tuple(np.float32(d)), float(np.float32(t))) for o, d, t in rays]


def slab_tris(abi):
    """Six triangles in the planes z = 0..5 that share the edges x = 0 and y = 0 with their boxes:
    a ray inside such a plane still hits the edge (u = 0 or v = 0 is accepted), so whether a NaN
    slab culls the node shows in t."""
    return tri_array(abi, np.array([[0, 0, k, 0, 1, k, 1, 0, k] for k in range(6)], np.float32))


SLAB_RAYS = [((0, 0.25, 9), (0, 0, -1), 1e34), ((0.25, 0, 9), (0, 0, -1), 1e34), ((0, 0.25, 9), (-0.0, 0, -1), 1e34),
             ((0.25, 0, 9), (0, -0.0, -1), 1e34), ((0, 0.25, -4), (0, 0, 1), 1e34), ((0.25, 0, -4), (0, -0.0, 1), 1e34),
             ((0, 0, 9), (0, 0, -1), 1e34), ((0.25, 0.25, 9), (0, 0, -1), 1e34), ((0.25, 0.25, 9), (-0.0, -0.0, -1), 3.5),
             ((1, 0, 9), (0, 0, -1), 1e34), ((0, 1, 9), (-0.0, 0, -1), 1e34), ((0.5, 0.5, 2.5), (0, 0, 1), 1e34)]


@functools.lru_cache(maxsize=None)
def bvh_cases(pkg, orc):
    """{set: tris, the host-built tree, rays, the restatement's t per ray, the stack model's
    high-water mark, the tree's depth}, computed once."""
    abi = pkg.abi
    out = {}
    sets = dict(bvh_sets(abi, orc))
    sets["slabs"] = slab_tris(abi)
    sets["chain+"], sets["chain-"] = chain(abi, 1), chain(abi, -1)
    for k, (name, tris) in enumerate(sets.items()):
        nodes, idx, used = lib_build(pkg, tris)
        arrays = sr.bvh_arrays(nodes, idx, tris, used)
        rays = chain_rays(1 if name == "chain+" else -1) if name.startswith("chain") else bvh_rays(arrays, 100 + k)
        if name == "slabs":
            rays = [(tuple(np.float32(o)), tuple(np.float32(d)), t) for o, d, t in SLAB_RAYS] + rays
        t, high = [], 0
        for o, d, tmax in rays:
            tt, h = sr.bvh_intersect(arrays, make_ray(v3(*o), v3(*d), tmax))
            t.append(tt)
            high = max(high, h)
        depth = pkg.load_library().vpx_bvh_depth(nodes, used)
        out[name] = dict(tris=tris, nodes=nodes, idx=idx, used=used, rays=rays, t=np.array(t, np.float32),
                         arrays=arrays, high=high, depth=depth)
    return out


def bvh_symmetric(c):
    """The same rays with IntersectAABB's min / max evaluated symmetrically (NOT the reference)."""
    return np.array([sr.bvh_intersect(c["arrays"], make_ray(v3(*o), v3(*d), tmax), symmetric=True)[0]
                     for o, d, tmax in c["rays"]], np.float32)


BVH_SETS = ["reference-ctor", "random1", "random2", "random3", "random5", "random64", "random200", "slabs", "chain+", "chain-"]


@pytest.mark.parametrize("name", BVH_SETS)
def test_bvh_oracle_equals_restatement(pkg, orc, name):
    c = bvh_cases(pkg, orc)[name]
    o = orc.BasicBVH(pkg.abi, c["tris"])
    assert o.used == c["used"] and bytes(o.nodes)[: 32 * o.used] == bytes(c["nodes"])[: 32 * o.used]
    got = o.intersect(api_rays(pkg.abi, [(o_, d, t, 0) for o_, d, t in c["rays"]]))
    hits = int((c["t"] < np.array([r[2] for r in c["rays"]], np.float32)).sum())
    print(f"bvh {name}: {len(c['rays'])} rays, {hits} shorten t, depth {c['depth']}, stack high-water mark {c['high']}")
    assert np.array_equal(fbits(got), fbits(c["t"])), np.flatnonzero(fbits(got) != fbits(c["t"]))[:8]
    assert hits >= (1 if name.startswith("random") and len(c["tris"]) < 4 else 10)


def test_bvh_rays_are_sensitive_to_the_min_max_operand_order(pkg, orc):
    """IntersectAABB with symmetric, NaN-dropping min / max changes the answer for some ray: the
    NaN slabs rest on std::min / std::max's operand order."""
    changed = {n: int((fbits(c["t"]) != fbits(bvh_symmetric(c))).sum()) for n, c in bvh_cases(pkg, orc).items()
               if n in ("reference-ctor", "slabs", "chain+", "chain-")}
    print("min/max operand order: rays whose t a symmetric min / max changes:", changed)
    assert changed["slabs"] >= 2 and changed["chain+"] + changed["chain-"] >= 2


def test_bvh_deepest_accepted_tree(pkg, orc):
    """chain_tris(abi, 64) and its mirror are as deep as vpx_bvh_set accepts, and the explicit
    stack of the traversal (64 entries) peaks one below its capacity for one of them."""
    cs = bvh_cases(pkg, orc)
    for name in ("chain+", "chain-"):
        assert cs[name]["depth"] == pkg.abi.BVH_MAX_DEPTH, name
        through = cs[name]["t"][:128] < 1e33
        assert int(through.sum()) == 127, name  # from between two neighbours both ways: all but the outward one at the far end
        assert len(np.unique(cs[name]["t"][:128])) >= 64  # and the nearest differs from ray to ray
    high = {n: cs[n]["high"] for n in ("chain+", "chain-")}
    print("bvh stack high-water mark (of 64 entries):", high)
    assert max(high.values()) >= pkg.abi.BVH_MAX_DEPTH - 1
    assert max(high.values()) <= 64  # the device's stack holds it
