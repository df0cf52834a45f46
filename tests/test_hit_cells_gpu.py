"""Hit cells on the device (vpx_find_nearest_cells / vpx_pick_pixel / vpx_render_ids): the hit
records against the oracle on the filtered grids, the cell records against the plain DDA restated
in numpy (tests/test_hit_cells.py), their properties over every ray of scene S, a sparse 128^3
grid whose walks skip, the ID buffer against the batch entry and the pixel entry, a pick / edit /
pick round trip, the refusals and the C++ mirror.  Everything is compared bit for bit.
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

from cases import bits  # noqa: E402
from test_hit_cells import SUBSET, sparse_case, subset_s  # noqa: E402
from test_kat_reproject import Camera  # noqa: E402
from test_ray_filter import N_RAYS, NO_RANGE, SMOKE, case_s, expected, hit_rows, make_rays  # noqa: E402
from test_ray_filter_gpu import FILTERS, X86, same, x86_mode  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 67, 35  # no multiple of the 16x16 tile either way: edge tiles on both sides


@pytest.fixture(scope="module")
def s(pkg, orc):
    """Scene S on the device and its rays."""
    desc, o, d, tmax = case_s(pkg, orc)
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    yield dict(desc=desc, o=o, d=d, tmax=tmax, rays=make_rays(pkg.abi, o, d, tmax), ctx=ctx)
    ctx.close()


def cell_rows(pkg, cells, n):
    return pkg.context.cells_to_numpy(cells, n)


def flags_of(c):
    f = c["flags"]
    return dict(hit=(f & 1) != 0, face=(f & 2) != 0, face_in=(f & 4) != 0, axis=((f >> 8) & 3).astype(np.int64),
                neg=((f >> 10) & 1).astype(np.int64), rest=f & ~np.uint32(0x707))


# ------------------------------------------------------------------------------ 1. records
@pytest.mark.parametrize("name", list(FILTERS))
def test_hits_equal_oracle_and_filtered_entry(pkg, orc, s, name):
    first, rng_mat, shapes = FILTERS[name]
    want = expected(pkg, orc, s["desc"], s["rays"], first, rng_mat, shapes)
    hits, _ = s["ctx"].find_nearest_cells(s["rays"], first, rng_mat, shapes)
    got = hit_rows(hits, N_RAYS)
    same(got, want, name)
    same(got, hit_rows(s["ctx"].find_nearest_filtered(s["rays"], first, rng_mat, shapes), N_RAYS), name + " vs filtered")


@pytest.mark.skipif(not X86, reason="VPX_ARITH_X86_HOST needs an x86 host")
def test_hits_x86_arithmetic(pkg, orc, s):
    exact = expected(pkg, orc, s["desc"], s["rays"], 1, SMOKE, False)
    try:
        x86_mode(pkg, orc, s["ctx"], True)
        want = expected(pkg, orc, s["desc"], s["rays"], 1, SMOKE, False)
        hits, cells = s["ctx"].find_nearest_cells(s["rays"], 1, SMOKE, shapes=False)
        filt = hit_rows(s["ctx"].find_nearest_filtered(s["rays"], 1, SMOKE, shapes=False), N_RAYS)
    finally:
        x86_mode(pkg, orc, s["ctx"], False)
    assert int((want[:, 0] != exact[:, 0]).sum()) >= 1  # the mode matters for these rays
    got = hit_rows(hits, N_RAYS)
    same(got, want, "player filter, x86 arithmetic")
    same(got, filt, "x86 vs filtered")
    c = cell_rows(pkg, cells, N_RAYS)
    assert np.array_equal((c["flags"] & 1) != 0, got[:, 4] >= 0)


# ------------------------------------------------------- 2. cells against the plain DDA
def compare_with_plain(pkg, ctx, o, d, tmax, res, first, rng_mat, what):
    """hits and cells of the device against plain_walk()'s results; t bit-equal for EVERY ray."""
    n = len(o)
    hits, cells = ctx.find_nearest_cells(make_rays(pkg.abi, o, d, tmax), first, rng_mat, shapes=False)
    h, c = hit_rows(hits, n), cell_rows(pkg, cells, n)
    fl = flags_of(c)
    bad = []
    for j, (t, rec, visited) in enumerate(res):
        assert int(h[j, 0]) == int(bits(np.float32(t)).reshape(-1)[0]), (what, j, "t")
        assert int(h[j, 6]) == visited, (what, j, "cells")
        if rec is None:
            ok = h[j, 4] == -2 and not c[j].tobytes().strip(b"\0")
        else:
            ok = (h[j, 4] == rec["vox"] and tuple(c["cell"][j]) == rec["cell"] and bool(fl["hit"][j]) and
                  h[j, 5] == rec["material"] and bool(fl["face"][j]) == (rec["axis"] >= 0))
            if ok and rec["axis"] >= 0:
                ok = fl["axis"][j] == rec["axis"] and fl["neg"][j] == (rec["step"] < 0)
        if not ok:
            bad.append(j)
    assert not bad, (what, len(bad), bad[:5], [(res[j][1], c[j], h[j]) for j in bad[:3]])
    return h, c


@pytest.mark.parametrize("name", list(SUBSET))
def test_cells_equal_plain_dda(pkg, orc, s, name):
    first, rng_mat = SUBSET[name]
    o, d, tmax, res = subset_s(pkg, orc)[name]
    compare_with_plain(pkg, s["ctx"], o, d, tmax, res, first, rng_mat, name)


# ------------------------------------------------------------------------- 3. properties
@pytest.mark.parametrize("name", list(FILTERS) + ["neutral"])
def test_cell_properties(pkg, s, name):
    first, rng_mat, shapes = FILTERS.get(name, (0, NO_RANGE, True))
    desc = s["desc"]
    hits, cells = s["ctx"].find_nearest_cells(s["rays"], first, rng_mat, shapes)
    h, c = hit_rows(hits, N_RAYS), cell_rows(pkg, cells, N_RAYS)
    fl = flags_of(c)
    won = h[:, 4] >= 0
    assert np.array_equal(fl["hit"], won) and not fl["rest"].any()
    raw = np.frombuffer(c.tobytes(), np.uint32).reshape(N_RAYS, 8)
    assert not raw[~won].any(), "misses and shape wins are all-zero"
    assert int(won.sum()) >= 200 and int((h[:, 4] == -1).sum()) >= (5 if shapes else 0)
    lo, hi = rng_mat
    for v in range(len(desc.volumes)):
        m = won & (h[:, 4] == v)
        if not m.any():
            continue
        gid = desc.volumes[v].grid_id
        n = desc.grids[gid].n
        g = np.asarray(desc.grids[gid].dense, np.uint8)
        cell, fc = c["cell"][m].astype(np.int64), c["face_cell"][m].astype(np.int64)
        assert (c["grid_id"][m] == gid).all()
        assert ((cell >= 0) & (cell < n)).all()
        assert np.array_equal(g[cell[:, 0] + cell[:, 1] * n + cell[:, 2] * n * n], h[m, 5])
        face, axis, neg = fl["face"][m], fl["axis"][m], fl["neg"][m]
        step = np.zeros_like(cell)
        step[np.arange(len(cell)), axis] = np.where(neg == 1, -1, 1)
        step[~face] = 0
        assert np.array_equal(fc[face], (cell - step)[face]), "face_cell = cell - step on axis"
        assert not fc[~face].any() and not axis[~face].any() and not neg[~face].any()
        inb = ((fc >= 0) & (fc < n)).all(axis=1)
        assert np.array_equal(fl["face_in"][m], face & inb)
        assert np.array_equal(fl["face_in"][m], face), "the cell visited before the hit is a cell of the grid"
        fb = g[fc[face][:, 0] + fc[face][:, 1] * n + fc[face][:, 2] * n * n]
        assert ((fb == 255) | ((fb >= lo) & (fb <= hi))).all(), "face_cell is empty or excepted"
    if name == "neutral":
        assert int((fl["face"] & won).sum()) >= 500 and int((~fl["face"] & won).sum()) >= 10


# ------------------------------------------------------------ 4. skips end at the hit
def test_sparse_grid_skips_end_at_the_hit(pkg):
    """The 128^3 grid of test_hit_cells.sparse_case: isolated cells and one far wall, so that the
    closed-form skips and wide boxes land on the hit cell.  Same comparison as above over its
    623 rays (603 hit), axis-parallel and corner rays included.
    vpx_hit.cells counts every visit of the reference's loop, the skipped ones included (the
    closed forms add them: it equals the oracle's count by contract, and is compared here), so
    "fewer cells read than the plain loop" cannot be observed in that field.  That the walks do
    skip is asserted on the grid instead (test_hit_cells.test_sparse_case_conditions): every
    hitting ray starts its walk in an empty brick with 26 empty neighbours, which walk_wave
    classifies as a skip."""
    desc, g, o, d, tmax, res = sparse_case(pkg)
    with pkg.context.Context(0) as ctx:
        ctx.load_scene(desc)
        h, c = compare_with_plain(pkg, ctx, o, d, tmax, res, 0, NO_RANGE, "sparse")
    hit = h[:, 4] >= 0
    assert int(hit.sum()) >= 500
    plain = np.array([v for _, _, v in res])
    assert np.array_equal(h[:, 6], plain)
    assert int((plain[hit] >= 32).sum()) * 2 >= int(hit.sum())  # long walks: the skips had room


# ---------------------------------------------------------------------------- 5. ID buffer
def pixel_rays(pkg, desc):
    """GetPrimaryRayNoDOF (camera.h:103-110) for every pixel of W x H, float32 as the restated
    Camera of test_kat_reproject: origins and unnormalised directions, row-major."""
    cam = Camera(desc._cam_pos, desc._cam_target, W, H)
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    u = (x.reshape(-1) * np.float32(np.float32(1.0) / np.float32(W))).astype(np.float32)
    v = (y.reshape(-1) * np.float32(np.float32(1.0) / np.float32(H))).astype(np.float32)
    tl = cam.top_left
    a = ((cam.top_right - tl).astype(np.float32)[None, :] * u[:, None]).astype(np.float32)
    b = ((cam.bottom_left - tl).astype(np.float32)[None, :] * v[:, None]).astype(np.float32)
    p = ((tl[None, :] + a).astype(np.float32) + b).astype(np.float32)
    d = (p - cam.pos[None, :]).astype(np.float32)
    ray = cam.primary_ray(5, 7)  # the vectorised form against the scalar one
    from test_kat_paths import normalize
    assert np.array_equal(bits(normalize(d[7 * W + 5])), bits(ray.D))
    return cam, np.broadcast_to(cam.pos, d.shape).copy(), d


@pytest.fixture(scope="module")
def s67(pkg, orc):
    """Scene S under its camera at 67 x 35."""
    desc = case_s(pkg, orc)[0]
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    cam = pkg.scene.look_at(desc._cam_pos, desc._cam_target, W, H)
    ctx.set_camera(cam)
    rcam, o, d = pixel_rays(pkg, desc)
    assert np.array_equal(bits(np.array(cam.top_left, np.float32)), bits(rcam.top_left))
    assert np.array_equal(bits(np.array(cam.bottom_left, np.float32)), bits(rcam.bottom_left))
    p = desc.frame_params(0, width=W, height=H)
    p.flags = pkg.abi.VPX_FLAG_AA | pkg.abi.VPX_FLAG_DOF  # ignored by the ID pass
    yield dict(desc=desc, ctx=ctx, rays=make_rays(pkg.abi, o, d, 1e34), params=p)
    ctx.close()


ID_FILTERS = {"neutral": None, "player": (1, SMOKE, False)}


@pytest.mark.parametrize("name", list(ID_FILTERS))
def test_id_buffer(pkg, s67, name):
    ctx, abi = s67["ctx"], pkg.abi
    flt = None if ID_FILTERS[name] is None else ctx.ray_filter(*ID_FILTERS[name])
    first, rng_mat, shapes = ID_FILTERS[name] or (0, NO_RANGE, True)
    before, light = ctx.counters().as_dict(), ctx.player_light().as_dict()
    ids = ctx.render_ids(s67["params"], flt)
    ctx.synchronize()
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (H, W, 4)
    assert ctx.counters().as_dict() == before and ctx.player_light().as_dict() == light
    u = pkg.context.unpack_ids(ids)
    n = W * H
    hits, cells = ctx.find_nearest_cells(s67["rays"], first, rng_mat, shapes)
    h, c = hit_rows(hits, n), cell_rows(pkg, cells, n)
    fl = flags_of(c)
    assert np.array_equal(u["t"].view(np.uint32).reshape(-1), h[:, 0])
    assert np.array_equal(u["vox_index"].reshape(-1), h[:, 4])
    assert np.array_equal(u["material"].reshape(-1), h[:, 5])
    assert np.array_equal(u["cell"].reshape(-1, 3), c["cell"])
    face = np.where(fl["face"], 1 + 2 * fl["axis"] + fl["neg"], 0)
    assert np.array_equal(u["face"].reshape(-1), face)
    # the scene fills about a fifth of this view: enough voxel hits, misses and faces for the comparison to mean something
    assert int((h[:, 4] >= 0).sum()) >= 200 and int((h[:, 4] == -2).sum()) >= 20
    assert len(np.unique(face[face > 0])) >= 2  # one camera sees at most three of the six face directions
    if shapes:
        assert int((h[:, 4] == -1).sum()) >= 5
    rng = np.random.default_rng(67)
    px = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)] + [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(50)]
    for x, y in px:
        hit, cell = ctx.pick_pixel(W, H, x, y, filter=flt)
        j = y * W + x
        assert bytes(hit) == bytes(hits[j]), (x, y, "hit")
        assert bytes(cell) == bytes(cells[j]), (x, y, "cell")


# ------------------------------------------------------------------ 6. pick, edit, pick
def test_pick_dig_build(pkg):
    sc = pkg.scene
    desc = sc.pillars_scene(64, W, H)
    with pkg.context.Context(0) as ctx:
        ctx.load_scene(desc)
        found = None
        for x, y in ((W // 2, H // 2), (W // 3, 2 * H // 3), (2 * W // 3, H // 2), (W // 2, H - 3)):
            hit, cell = ctx.pick_pixel(W, H, x, y)
            if hit.vox_index == 0 and cell.flags & pkg.abi.CELL_FACE:
                found = (x, y)
                break
        assert found, "no pixel of the pillars scene hits a cell through a face"
        x, y = found
        c0, f0 = tuple(cell.cell), tuple(cell.face_cell)
        assert cell.flags & pkg.abi.CELL_FACE_IN
        assert int(ctx.grid_read_box(0, c0, (1, 1, 1))[0, 0, 0]) == hit.material != 255
        assert int(ctx.grid_read_box(0, f0, (1, 1, 1))[0, 0, 0]) == 255
        ctx.grid_brush(0, [sc.box_brush(c0, c0, 255)])  # dig
        hit1, cell1 = ctx.pick_pixel(W, H, x, y)
        assert int(ctx.grid_read_box(0, c0, (1, 1, 1))[0, 0, 0]) == 255
        assert bytes(cell1) != bytes(cell) and tuple(cell1.cell) != c0
        assert hit1.t >= hit.t  # the walk went on from the dug cell
        ctx.grid_brush(0, [sc.box_brush(f0, f0, 17, match=(255, 255))])  # build on the face
        hit2, cell2 = ctx.pick_pixel(W, H, x, y)
        assert tuple(cell2.cell) == f0 and hit2.material == 17 and hit2.vox_index == 0
        assert hit2.t <= hit.t  # the face cell is visited before the cell


# ------------------------------------------------------------------------- 7. refusals
def test_refusals(pkg, s67):
    abi, ctx = pkg.abi, s67["ctx"]
    lib, h = ctx.lib, ctx.h
    rays = s67["rays"]
    hits, cells = (abi.Hit * 4)(), (abi.HitCell * 4)()
    ok = abi.RayFilter(0, 1, 0, 0)
    ids = torch.zeros((H, W, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    p = s67["params"]
    # null outputs with n > 0; n == 0 is fine
    assert lib.vpx_find_nearest_cells(h, rays, 4, C.byref(ok), None, cells) == abi.VPX_E_INVALID
    assert lib.vpx_find_nearest_cells(h, rays, 4, C.byref(ok), hits, None) == abi.VPX_E_INVALID
    assert lib.vpx_find_nearest_cells(h, None, 4, C.byref(ok), hits, cells) == abi.VPX_E_INVALID
    assert lib.vpx_find_nearest_cells(h, None, 0, C.byref(ok), None, None) == abi.VPX_OK
    assert lib.vpx_find_nearest_cells(h, rays, 4, None, hits, cells) == abi.VPX_E_INVALID
    assert lib.vpx_pick_pixel(h, W, H, 0, 0, None, None, cells) == abi.VPX_E_INVALID
    assert lib.vpx_pick_pixel(h, W, H, 0, 0, None, hits, None) == abi.VPX_E_INVALID
    assert lib.vpx_render_ids(h, C.byref(p), None, None) == abi.VPX_E_INVALID
    assert lib.vpx_render_ids(h, None, None, C.c_void_p(ids.data_ptr())) == abi.VPX_E_INVALID
    # unknown flag bits, bad ranges: as the filtered entry
    for bad in ((0, 9, 256, 0), (0, 1, 0, 4), (0, 9, 14, 0x80000000)):
        f = abi.RayFilter(*bad)
        assert lib.vpx_find_nearest_cells(h, rays, 4, C.byref(f), hits, cells) == abi.VPX_E_INVALID, bad
        assert lib.vpx_find_nearest_cells(h, None, 0, C.byref(f), None, None) == abi.VPX_E_INVALID, bad
        assert lib.vpx_pick_pixel(h, W, H, 0, 0, C.byref(f), hits, cells) == abi.VPX_E_INVALID, bad
        assert lib.vpx_render_ids(h, C.byref(p), C.byref(f), C.c_void_p(ids.data_ptr())) == abi.VPX_E_INVALID, bad
    # the library builds the pixel rays: no raw directions there; the batch entry takes them
    raw = abi.RayFilter(0, 1, 0, abi.QUERY_RAW_DIRECTION)
    assert lib.vpx_pick_pixel(h, W, H, 0, 0, C.byref(raw), hits, cells) == abi.VPX_E_INVALID
    assert lib.vpx_render_ids(h, C.byref(p), C.byref(raw), C.c_void_p(ids.data_ptr())) == abi.VPX_E_INVALID
    assert lib.vpx_find_nearest_cells(h, rays, 4, C.byref(raw), hits, cells) == abi.VPX_OK
    # the pixel and the frame
    for bad in ((W, 0), (0, H), (0xFFFFFFFF, 0)):
        assert lib.vpx_pick_pixel(h, W, H, bad[0], bad[1], None, hits, cells) == abi.VPX_E_INVALID, bad
    assert lib.vpx_pick_pixel(h, 0, H, 0, 0, None, hits, cells) == abi.VPX_E_INVALID
    assert lib.vpx_pick_pixel(h, W, H, W - 1, H - 1, None, hits, cells) == abi.VPX_OK
    ctx.synchronize()
    assert not ids.cpu().numpy().any(), "a refused call writes nothing"
    # no camera
    with pkg.context.Context(0) as bare:
        desc = s67["desc"]
        for gid, g in enumerate(desc.grids):
            g.upload(bare.lib, bare.h, gid)
        bare._chk(bare.lib.vpx_set_volumes(bare.h, desc.volumes, len(desc.volumes)), "vpx_set_volumes")
        bare._chk(bare.lib.vpx_set_materials(bare.h, desc.materials, 256), "vpx_set_materials")
        assert bare.lib.vpx_pick_pixel(bare.h, W, H, 0, 0, None, hits, cells) == abi.VPX_E_STATE
        assert bare.lib.vpx_render_ids(bare.h, C.byref(p), None, C.c_void_p(ids.data_ptr())) == abi.VPX_E_STATE
        assert bare.lib.vpx_find_nearest_cells(bare.h, rays, 4, C.byref(ok), hits, cells) == abi.VPX_OK  # needs no camera


# ----------------------------------------------------------------------- 8. C++ mirror
def test_cpp_mirror_pick(pkg):
    """host/vpx_demo's pick sub-command builds the pillars world and its camera in C++ and prints
    Renderer::PickPixel's record; the Python path gives the same one."""
    exe = os.path.join(os.path.dirname(pkg.__file__), "host", "vpx_demo")
    assert os.path.exists(exe), "host/vpx_demo missing: run __graft_entry__.build()"
    n = 64
    desc = pkg.scene.pillars_scene(n, W, H)
    faces = 0
    with pkg.context.Context(0) as ctx:
        ctx.load_scene(desc)
        for x, y in ((W // 2, H // 2), (3, H - 2), (W - 1, 0), (W // 3, 2 * H // 3)):
            r = subprocess.run([exe, "pick", str(n), str(W), str(H), str(x), str(y)], capture_output=True, text=True,
                               timeout=120)
            assert r.returncode == 0, r.stderr
            got = json.loads(r.stdout.strip().splitlines()[-1])["pick"]
            hit, cell = ctx.pick_pixel(W, H, x, y)
            want = dict(x=x, y=y, t_bits=int(bits(np.float32(hit.t)).reshape(-1)[0]), vox=hit.vox_index,
                        material=hit.material, cells=hit.cells, cell=list(cell.cell), grid_id=cell.grid_id,
                        face_cell=list(cell.face_cell), flags=cell.flags)
            assert got == want, (x, y)
            faces += bool(cell.flags & pkg.abi.CELL_FACE)
    assert faces >= 1
