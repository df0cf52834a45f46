"""Hit cells (vpx_find_nearest_cells / vpx_pick_pixel / vpx_render_ids) without a GPU: the C-ABI
additions, the Python surface, unpack_ids, and the plain-DDA restatement the GPU tests
(tests/test_hit_cells_gpu.py) compare the cell records with, together with the conditions on
their ray sets.

The cell record describes the winning volume's walk as the reference's plain loop runs it
(Scene::FindNearest / FindNearestExcept, template/scene.cpp:751-873): the (X, Y, Z) at which the
loop returned, and the axis and step of the last tmax advance before it.  plain_walk() below is
that loop with test_kat_paths' Setup3DDDA and stepping in numpy float32; the axis of each advance
is chosen here by the strict compares of scene.cpp:773-802, not read off the coordinates.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from test_kat_paths import NONE, Ray, Vol, dsign, f32, v3, xform_pos_sse, xform_vec_sse
from test_ray_filter import N_RAYS, NO_RANGE, SMOKE, case_s

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vpx_find_nearest_cells", "vpx_pick_pixel", "vpx_render_ids")
CELL_DT = np.dtype([("cell", "<i4", 3), ("grid_id", "<u4"), ("face_cell", "<i4", 3), ("flags", "<u4")])


# ------------------------------------------------------------------- header and library
def test_header_declares_and_library_exports(pkg):
    text = open(os.path.join(REPO, "include", "vpx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in pkg.abi.SIGNATURES
        assert name in text[: text.index("#ifndef VPX_H_")], "the entry list at the top of the header"
    assert re.search(r"#define\s+VPX_CELL_HIT\s+0x1u", code)
    assert re.search(r"#define\s+VPX_CELL_FACE\s+0x2u", code)
    assert re.search(r"#define\s+VPX_CELL_FACE_IN\s+0x4u", code)
    assert re.search(r"#define\s+VPX_ABI_VERSION\s+2\b", code)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH], capture_output=True, text=True).stdout
    assert set(ENTRIES) <= set(re.findall(r" T (vpx_\w+)", out))
    assert (pkg.abi.CELL_HIT, pkg.abi.CELL_FACE, pkg.abi.CELL_FACE_IN) == (1, 2, 4)


def test_struct_size_and_fields(pkg):
    abi = pkg.abi
    assert C.sizeof(abi.HitCell) == 32 and abi.STRUCT_SIZES[abi.HitCell] == 32 and CELL_DT.itemsize == 32
    assert [(n, getattr(abi.HitCell, n).offset) for n, _ in abi.HitCell._fields_] == [
        ("cell", 0), ("grid_id", 12), ("face_cell", 16), ("flags", 28)]
    src = ('#include <cstddef>\n#include "vpx.h"\n'
           "static_assert(sizeof(vpx_hit_cell) == 32, \"vpx_hit_cell\");\n"
           "static_assert(offsetof(vpx_hit_cell, cell) == 0, \"cell\");\n"
           "static_assert(offsetof(vpx_hit_cell, grid_id) == 12, \"grid_id\");\n"
           "static_assert(offsetof(vpx_hit_cell, face_cell) == 16, \"face_cell\");\n"
           "static_assert(offsetof(vpx_hit_cell, flags) == 28, \"flags\");\n"
           "static_assert(VPX_CELL_HIT == 1u && VPX_CELL_FACE == 2u && VPX_CELL_FACE_IN == 4u && VPX_ABI_VERSION == 2, \"constants\");\n")
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(REPO, "include"), "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_context_is_refused(pkg):
    lib, abi = pkg.load_library(), pkg.abi
    f = abi.RayFilter(0, 1, 0, 0)
    ray, hit, cell = (abi.Ray * 1)(), (abi.Hit * 1)(), (abi.HitCell * 1)()
    p = abi.FrameParams()
    p.width, p.height = 8, 8
    assert lib.vpx_find_nearest_cells(None, ray, 1, C.byref(f), hit, cell) == abi.VPX_E_INVALID
    assert lib.vpx_find_nearest_cells(None, None, 0, None, None, None) == abi.VPX_E_INVALID
    assert lib.vpx_pick_pixel(None, 8, 8, 0, 0, C.byref(f), hit, cell) == abi.VPX_E_INVALID
    assert lib.vpx_pick_pixel(None, 8, 8, 0, 0, None, None, None) == abi.VPX_E_INVALID
    assert lib.vpx_render_ids(None, C.byref(p), None, None) == abi.VPX_E_INVALID
    assert lib.vpx_abi_version() == abi.ABI_VERSION == 2


def test_python_surface(pkg):
    ctx, ren = pkg.context.Context, pkg.renderer.Renderer
    for name in ("find_nearest_cells", "pick_pixel", "render_ids", "unpack_ids"):
        assert callable(getattr(ctx, name)), name
    assert callable(pkg.context.unpack_ids) and callable(pkg.context.cells_to_numpy)
    assert callable(ren.PickPixel) and callable(ren.pick_pixel) and callable(ren.FindNearestCells)
    text = open(os.path.join(REPO, "raytracer-voxpopuli_amd", "host", "vpx_renderer.h")).read()
    for name in ("PickPixel", "FindNearestCells", "vpx_hit_cell"):
        assert name in text, name
    assert "pick" in open(os.path.join(REPO, "raytracer-voxpopuli_amd", "host", "vpx_demo.cpp")).read()


def pack_ids(t, vox, mat, face, cell):
    """The ID word layout of include/vpx.h, packed by hand."""
    t, vox, mat, face, cell = (np.asarray(a) for a in (t, vox, mat, face, cell))
    out = np.zeros(t.shape + (4,), np.uint32)
    out[..., 0] = t.astype(np.float32).view(np.uint32)
    out[..., 1] = ((vox + 2) & 0xFFFF) | (mat.astype(np.uint32) << 16) | (face.astype(np.uint32) << 24)
    out[..., 2] = cell[..., 0].astype(np.uint32) | (cell[..., 1].astype(np.uint32) << 16)
    out[..., 3] = cell[..., 2].astype(np.uint32)
    return out


def test_unpack_ids_inverts_a_hand_packed_array(pkg):
    rng = np.random.default_rng(3)
    h, w = 5, 7
    t = rng.uniform(0.1, 3.0, (h, w)).astype(np.float32)
    vox = rng.integers(-2, 65534, (h, w))
    vox[0, :4] = (-2, -1, 0, 65533)
    mat = rng.integers(0, 256, (h, w))
    face = rng.integers(0, 7, (h, w))
    face[1, :7] = np.arange(7)
    cell = rng.integers(0, 4096, (h, w, 3))
    cell[2, 0] = (4095, 0, 4095)
    ids = pack_ids(t, vox, mat, face, cell)
    for arr in (ids, ids.view(np.int32)):  # the tensor render_ids returns is int32
        u = pkg.context.unpack_ids(arr)
        assert np.array_equal(u["t"].view(np.uint32), t.view(np.uint32))
        assert np.array_equal(u["vox_index"], vox) and np.array_equal(u["material"], mat)
        assert np.array_equal(u["face"], face) and np.array_equal(u["cell"], cell)
        assert np.array_equal(u["axis"], np.where(face > 0, (face - 1) // 2, 0))
        assert np.array_equal(u["step"], np.where(face > 0, np.where((face - 1) % 2 == 1, -1, 1), 0))
    assert pkg.context.Context.unpack_ids(ids)["t"].shape == (h, w)


# ------------------------------------------------------------------ the plain DDA, restated
def vols_of(desc):
    return [Vol(np.asarray(desc.grids[v.grid_id].dense, np.uint8), desc.grids[v.grid_id].n, list(v.matrix),
                list(v.inv_matrix), tuple(v.b0), tuple(v.b1)) for v in desc.volumes]


def choose_axis(tm):
    """The axis of the next advance, scene.cpp:773-802: x<y ? (x<z ? x : z) : (y<z ? y : z), strict."""
    if tm[0] < tm[1]:
        return 0 if tm[0] < tm[2] else 2
    return 1 if tm[1] < tm[2] else 2


def plain_walk(vols, o, d, tmax, first=0, rng_mat=NO_RANGE):
    """Renderer::FindNearest's loop over the volumes first.. (renderer.cpp:946-1018, no shapes), each
    walked as Scene::FindNearestExcept with exact 1 / D, to the first cell that is neither NONE nor
    excepted.  Returns (t, record): record None on a miss, else vox, cell, axis (-1: the hit cell is
    the walk's first), step, passed (excepted cells the winning walk passed through) and visited
    (the cells the whole query read, vpx_hit.cells)."""
    lo, hi = rng_mat
    ray = Ray(v3(*o), v3(*d), t=f32(tmax))
    rec, visited = None, 0
    with np.errstate(all="ignore"):
        for i in range(first, len(vols)):
            v = vols[i]
            O = xform_pos_sse(ray.O, v.inv)
            D = xform_vec_sse(ray.D, v.inv)
            rD = v3(*[f32(f32(1) / D[k]) for k in range(3)])
            s = v.setup(O, D, rD, dsign(D))
            if s is None:
                continue
            axis, passed = -1, 0
            while s["t"] < ray.t:
                c = v.cell(s["X"], s["Y"], s["Z"])
                visited += 1
                if c != NONE and (c < lo or c > hi):
                    ray.t = s["t"]
                    rec = dict(vox=i, cell=(s["X"], s["Y"], s["Z"]), axis=axis, step=s["step"][axis] if axis >= 0 else 0,
                               passed=passed, material=c)
                    break
                passed += c != NONE
                k = choose_axis(s["tmax"])
                if not Vol.advance(s, v.n):
                    break
                axis = k
    if rec is not None:
        rec["visited"] = visited
    return ray.t, rec, visited


def face_of(rec):
    """The ID buffer's face number: 0 none, else 1 + 2 * axis + (step < 0)."""
    return 0 if rec is None or rec["axis"] < 0 else 1 + 2 * rec["axis"] + (rec["step"] < 0)


# --------------------------------------------------------------- test 2's subset of scene S
EXTRA_SEED = 11
SUBSET = {"plain": (0, NO_RANGE), "smoke": (0, SMOKE)}  # name: (first_volume, material range), shapes off


def extra_rays():
    """Rays scene S's set is thin on: walks that enter a solid cell through its low y face (a step
    of +1 on y).  From the gap under the glass and emissive plates of the room (cells x = 9 and
    x = 22, y 4..9, z 12..17; the gap is y 2..3) and from under the small rotated volume, upwards."""
    rng = np.random.default_rng(EXTRA_SEED)
    o, d = [], []
    for j in range(48):
        x = (9.0 if j % 2 == 0 else 22.0) + rng.uniform(0.2, 0.8)
        z = rng.uniform(12.2, 17.8)
        o.append((x / 32.0, rng.uniform(2.1, 3.2) / 32.0, z / 32.0))
        d.append((rng.uniform(-0.01, 0.01), 1.0, rng.uniform(-0.05, 0.05)))
    return np.array(o, np.float32), np.array(d, np.float32), np.full(len(o), 1e34, np.float32)


_SUB = {}


def subset_s(pkg, orc):
    """{name: (origins, directions, tmax, [plain_walk results])} — computed once, left unchanged.
    'plain': no material excepted (rays that start inside the smoke hit their first cell); 'smoke':
    the smoke range passed through."""
    if _SUB:
        return _SUB
    desc, o, d, tmax = case_s(pkg, orc)
    vols = vols_of(desc)
    eo, ed, et = extra_rays()
    pick = {"plain": np.concatenate([np.arange(0, 230), np.arange(N_RAYS - 128, N_RAYS - 64)]),
            "smoke": np.concatenate([np.arange(230, 560), np.arange(N_RAYS - 128 - 60, N_RAYS - 128)])}
    for name, (first, rng_mat) in SUBSET.items():
        i = pick[name]
        so, sd, st = o[i], d[i], tmax[i]
        if name == "plain":
            so, sd, st = np.concatenate([so, eo]), np.concatenate([sd, ed]), np.concatenate([st, et])
        _SUB[name] = (so, sd, st, [plain_walk(vols, so[j], sd[j], st[j], first, rng_mat) for j in range(len(so))])
    return _SUB


def test_scene_s_subset_conditions(pkg, orc):
    """With the restatement alone: the subset holds at least 500 hitting rays, at least 10 hits in
    the walk's first cell, at least 10 on each of the six faces, and at least 10 walks that passed
    an excepted cell before their hit."""
    sub = subset_s(pkg, orc)
    recs = [r for name in sub for _, r, _ in sub[name][3] if r is not None]
    faces = np.bincount([face_of(r) for r in recs], minlength=7)
    passed = sum(1 for _, r, _ in sub["smoke"][3] if r is not None and r["passed"] > 0)
    print("hits", len(recs), "faces (none, +x, -x, +y, -y, +z, -z)", faces.tolist(), "passed", passed,
          "volumes", np.bincount([r["vox"] for r in recs]).tolist())
    assert len(recs) >= 500
    assert (faces >= 10).all(), faces
    assert passed >= 10


# ------------------------------------------------------------------- test 4's sparse grid
SPARSE_N = 128
SPARSE_SEED = 17


def sparse_grid():
    """128^3, empty except a far wall (x = 120, 121; material 7) and 48 isolated cells (material
    16 + k % 4) in front of it, each alone in its brick's neighbourhood."""
    n = SPARSE_N
    g = np.full((n, n, n), NONE, np.uint8)  # [z][y][x]
    g[:, :, 120:122] = 7
    rng = np.random.default_rng(SPARSE_SEED)
    iso = []
    for k in range(48):
        c = (int(rng.integers(24, 112)), int(rng.integers(8, 120)), int(rng.integers(8, 120)))
        iso.append(c)
        g[c[2], c[1], c[0]] = 16 + k % 4
    # cells on the diagonals the corner rays run along
    for c in ((40, 52, 64), (72, 72, 72), (56, 64, 56 + 12)):
        iso.append(c)
        g[c[2], c[1], c[0]] = 5
    return g, iso


def sparse_rays(iso):
    """620 rays towards +x: 240 aimed at isolated cells, 240 at the wall, 60 that start inside the
    grid, 40 axis-parallel (exact zeros, so two tdelta are infinite; half through cell centres, where
    two tmax tie at infinity all the way, half along cell edges, where they are NaN and the reference's loop ends at once), 40 along face and space diagonals from origins on the cell lattice, so
    that they pass through cell corners (ties of two and of three tmax)."""
    rng = np.random.default_rng(SPARSE_SEED + 1)
    n = float(SPARSE_N)
    o, d = [], []
    for j in range(240):
        c = iso[j % len(iso)]
        tgt = (np.array(c) + rng.uniform(0.15, 0.85, 3)) / n
        org = np.array([rng.uniform(-0.5, -0.05), rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8)])
        o.append(org), d.append(tgt - org)
    for j in range(240):
        tgt = np.array([120.0 / n, rng.uniform(0.03, 0.97), rng.uniform(0.03, 0.97)])
        org = np.array([rng.uniform(-0.5, -0.05), rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9)])
        o.append(org), d.append(tgt - org)
    for j in range(60):
        org = np.array([rng.uniform(0.02, 0.15), rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9)])
        tgt = np.array([120.0 / n, rng.uniform(0.03, 0.97), rng.uniform(0.03, 0.97)])
        o.append(org), d.append(tgt - org)
    for j in range(40):
        y, z = int(rng.integers(4, 124)), int(rng.integers(4, 124))
        off = 0.5 if j % 2 == 0 else 0.0  # cell centres / cell edges (exact in float32)
        o.append(np.array([-0.25, (y + off) / n, (z + off) / n])), d.append(np.array([1.0 + j % 3, 0.0, 0.0]))
    for j in range(40):
        kind = j % 4
        dd = [(1.0, 1.0, 0.0), (1.0, 0.0, 1.0), (1.0, 1.0, 1.0), (1.0, -1.0, 0.0)][kind]
        # a moving axis starts within 7 cells of the face it runs away from, so the ray reaches the wall
        y = int(rng.integers(40, 90)) if dd[1] == 0 else (int(rng.integers(1, 8)) if dd[1] > 0 else int(rng.integers(121, 128)))
        z = int(rng.integers(40, 90)) if dd[2] == 0 else int(rng.integers(1, 8))
        # the axis the ray does not move along sits at a cell centre (on the lattice its tmax is NaN)
        org = np.array([-0.25, (y + (0.5 if dd[1] == 0 else 0.0)) / n - 0.25 * dd[1],
                        (z + (0.5 if dd[2] == 0 else 0.0)) / n - 0.25 * dd[2]])
        o.append(org), d.append(np.array(dd))
    # three that run into the cells put on their diagonals (through their low corners)
    for c, dd in (((40, 52, 64), (1.0, 1.0, 0.0)), ((72, 72, 72), (1.0, 1.0, 1.0)), ((56, 64, 68), (1.0, 0.0, 1.0))):
        dd = np.array(dd)
        o.append((np.array(c) + 0.5 * (dd == 0)) / n - 0.25 * dd), d.append(dd)
    return np.array(o, np.float32), np.array(d, np.float32), np.full(len(o), 1e34, np.float32)


_SPARSE = {}


def sparse_case(pkg):
    """(desc, origins, directions, tmax, [plain_walk results], open run per ray); computed once."""
    if _SPARSE:
        return _SPARSE["v"]
    sc = pkg.scene
    g, iso = sparse_grid()
    desc = sc._scene("hit_cells_sparse", [sc.GridSpec(n=SPARSE_N, dense=g.reshape(-1))], [sc.volume()],
                     sc.default_materials(), [sc.point_light()], [], [], sc.dir_light(), (0.5, 0.5, -1.0), (0.5, 0.5, 0.5),
                     32, 32)
    o, d, tmax = sparse_rays(iso)
    vols = vols_of(desc)
    res = [plain_walk(vols, o[j], d[j], tmax[j]) for j in range(len(o))]
    _SPARSE["v"] = (desc, g, o, d, tmax, res)
    return _SPARSE["v"]


def open_bricks(g):
    """[bz][by][bx]: the 4^3 brick and its 26 neighbours (those inside the grid) hold no solid cell,
    so its distance-field cube is at least two bricks in every octant."""
    nb = g.shape[0] // 4
    occ = (g.reshape(nb, 4, nb, 4, nb, 4) != NONE).any(axis=(1, 3, 5))
    pad = np.pad(occ, 1, constant_values=False)
    near = np.zeros_like(occ)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                near |= pad[dz:dz + nb, dy:dy + nb, dx:dx + nb]
    return ~near


def test_sparse_case_conditions(pkg):
    """At least 500 hitting rays, hits on isolated cells and on the wall, first-step ties among
    the lattice rays, and open space on the way: at least half of the hitting rays start their
    walk in a brick that open_bricks() marks (there the walkers' classification is "skip": an empty
    brick whose cube is at least the FindNearest walks' minimum of two)."""
    desc, g, o, d, tmax, res = sparse_case(pkg)
    hits = [r for _, r, _ in res if r is not None]
    assert len(hits) >= 500
    assert sum(r["material"] != 7 for r in hits) >= 100 and sum(r["material"] == 7 for r in hits) >= 200
    assert all(r is not None and r["material"] == 5 for _, r, _ in res[-3:])  # the corner hits
    vol = vols_of(desc)[0]
    opened = open_bricks(g)
    ties = started_open = 0
    with np.errstate(all="ignore"):
        for j in range(len(o)):
            ray = Ray(v3(*o[j]), v3(*d[j]))
            rD = v3(*[f32(f32(1) / ray.D[k]) for k in range(3)])
            s = vol.setup(ray.O, ray.D, rD, dsign(ray.D))
            if s is None or res[j][1] is None:
                continue
            tm = s["tmax"]
            ties += j >= 540 and (tm[0] == tm[1] or tm[1] == tm[2] or tm[0] == tm[2])
            started_open += bool(opened[s["Z"] // 4, s["Y"] // 4, s["X"] // 4])
    print("hits", len(hits), "ties", ties, "start in open space", started_open)
    assert ties >= 30
    assert 2 * started_open >= len(hits)
