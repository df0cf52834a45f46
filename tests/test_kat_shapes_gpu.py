"""Spheres, triangles and BasicBVH on the device against the independent restatement
(tests/shapes_ref.py), no oracle in between, bit for bit (NaN lanes as masks).

The cases are test_kat_shapes.py's, where the oracle is pinned to the same restatement and
where the conditions that keep them from being vacuous are asserted: the known answers, the
edge table and the 4099 random rays go through every ray entry (vpx_find_nearest,
vpx_is_occluded, the filtered pair with the shapes on, off and with VPX_QUERY_RAW_DIRECTION,
vpx_find_nearest_cells, vpx_cast_nearest / vpx_cast_occluded in the per-lane and the pool
form), the depth-1 and depth-2 paths through vpx_trace, the BVH ray sets with both 63-deep
chains through vpx_bvh_set + vpx_bvh_intersect, and vpx_render_ids over the shape room against
vpx_pick_pixel and the restatement.

Whole frames over the shape room (two spheres, one of glass, and two triangles; 40x24,
VPX_FLAG_AA) are compared with the oracle: accumulator bits, RGB8 and the shadow / bounce / cell
counts.  They carry the shape stage through each kernel family that contains it (launch_render
in csrc/vpx_kernels.hip; shapes keep every frame off the one-launch k_frame0, so
vpx_debug_last_frame_kernel is 0 and the stages launch separately, which vpx_profile_read shows):
  depth 0, point light                 k_primary<false, ...> + k_shadow_finish<false>
  depth 2, point light                 k_nearest_tile, k_shadow_tile<false>, k_shadow_list<false>
  depth 2, one area light, 3 samples   k_shadow_pool<true> + k_shadow_slots
  depth 8                              k_tail
  depth 2 with 2 lanes                 the same kernels on a lane's stream
  one vpx_render_reproject frame       the static-camera path
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import test_kat_shapes as K  # noqa: E402
from test_kat_paths import SEEDS, api_rays, f32, fbits, v3  # noqa: E402
from test_kat_reproject import Camera  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:invalid value:RuntimeWarning")]
DEV = "cuda:0"
W, H = 40, 24
PER_LANE, POOL = 1, 2


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.context.Context(0)
    yield c
    c.close()


def tensor_records(t, n):
    return K.hit_records(t.cpu().numpy().view(np.uint32).reshape(-1), n)


def check_ray_entries(pkg, ctx, rays, raw_rays, e, what):
    """Every ray entry on the loaded scene against the restatement's records e (test_kat_shapes.expect)."""
    abi, n = pkg.abi, len(rays)
    api, raw = api_rays(abi, rays), api_rays(abi, raw_rays)
    given = np.array([r[3] for r in rays], np.uint32)
    K.same_records(K.hit_records(ctx.find_nearest(api), n), e["near"], what + ": vpx_find_nearest")
    assert np.array_equal(ctx.is_occluded(api), e["occ"]), what + ": vpx_is_occluded"
    K.same_records(K.hit_records(ctx.find_nearest_filtered(api), n), e["near"], what + ": filtered, shapes on")
    off = K.hit_records(ctx.find_nearest_filtered(api, shapes=False), n)
    K.same_records(off, e["vol"], what + ": filtered, VPX_QUERY_NO_SHAPES")
    assert np.array_equal(off["inside"], given) and not (off["vox"] == -1).any(), what + ": shapes off keep the flag"
    K.same_records(K.hit_records(ctx.find_nearest_filtered(raw, raw_direction=True), n), e["near"],
                   what + ": filtered, VPX_QUERY_RAW_DIRECTION")
    assert np.array_equal(ctx.is_occluded_filtered(api), e["occ"]), what + ": vpx_is_occluded_filtered"
    assert np.array_equal(ctx.is_occluded_filtered(api, shapes=False), e["occ_vol"]), what + ": occluded, shapes off"
    assert np.array_equal(ctx.is_occluded_filtered(raw, raw_direction=True), e["occ"]), what + ": occluded, raw direction"
    hits, cells = ctx.find_nearest_cells(api)
    K.same_records(K.hit_records(hits, n), e["near"], what + ": vpx_find_nearest_cells")
    cw = np.frombuffer(cells, np.uint32, count=8 * n).reshape(n, 8)
    lost = e["near"]["vox"] < 0
    assert not cw[lost].any(), what + ": a shape win or a miss gives an all-zero cell record"
    assert (cw[~lost, 7] & 1).all(), what + ": VPX_CELL_HIT on volume wins"
    rt = abi.rays_tensor(api, DEV)  # kept until the casts have run
    for form in (PER_LANE, POOL):  # one volume: first_volume == count - 1, the pool serves the batch
        h, c = ctx.cast_nearest(rt, form=form)
        assert ctx.last_cast_kernel() == form, (what, form)
        occ = ctx.cast_occluded(rt, form=form)
        assert ctx.last_cast_kernel() == form, (what, form)
        ctx.synchronize()
        K.same_records(tensor_records(h, n), e["near"], f"{what}: vpx_cast_nearest form {form}")
        assert np.array_equal(c.cpu().numpy().view(np.uint32).reshape(n, 8), cw), f"{what}: cast cells form {form}"
        assert np.array_equal(occ.cpu().numpy(), e["occ"]), f"{what}: vpx_cast_occluded form {form}"


# ---------------------------------------------------------------- 1. known answers and edges
@pytest.mark.parametrize("case", K.KNOWN, ids=[k[0] for k in K.KNOWN])
def test_known_answers_on_device(pkg, ctx, case):
    what, spheres, tris, ray, t, nrm, mat, vox, inside, occluded = case
    e = K.expect("E", spheres, tris, [ray])
    want = np.zeros(1, K.REC)
    want[0] = (fbits(f32(t)), fbits(v3(*nrm)), vox, mat, e["near"]["cells"][0], inside)
    ctx.load_scene(K.desc_of(pkg, "E", spheres, tris))
    api = api_rays(pkg.abi, [ray])
    K.same_records(K.hit_records(ctx.find_nearest(api), 1), want, what)
    assert int(ctx.is_occluded(api)[0]) == occluded, what


@pytest.mark.parametrize("i", range(len(K.EDGES)), ids=K.EDGE_IDS)
def test_edge_table_on_device(pkg, ctx, i):
    group, key, spheres, tris, rows = K.EDGES[i]
    ctx.load_scene(K.desc_of(pkg, key, spheres, tris))
    check_ray_entries(pkg, ctx, K.edge_rays(i), K.edge_rays(i, raw=True), K.edge_expect(i), group)


# ------------------------------------------------------------------------ 2. the random set
def test_random_set_on_device(pkg, ctx):
    """4099 rays (sixteen workgroups plus three lanes) over the room with three spheres and two
    triangles, through every entry."""
    ctx.load_scene(K.desc_of(pkg, "R0", K.R_SPHERES, K.R_TRIS))
    check_ray_entries(pkg, ctx, K.random_rays(), K.random_raw_rays(), K.random_expect(), "random set")


# ------------------------------------------------------------------------------- 3. paths
@pytest.mark.parametrize("depth", K.DEPTHS)
def test_paths_with_shapes_on_device(pkg, ctx, depth):
    """test_kat_shapes.PATHS through vpx_trace, 24 seeds each."""
    for i, (what, wall, spheres, tris, ray, first) in enumerate(K.PATHS):
        ctx.load_scene(K.desc_of(pkg, f"R{wall}", spheres, tris))
        got = ctx.trace(K.path_rays(pkg, i), np.array(SEEDS, np.uint32), depth, K.SKY, 3)
        want = K.path_expect(i, depth)["rad"]
        bad = [hex(s) for k, s in enumerate(SEEDS) if not np.array_equal(fbits(np.asarray(got[k], np.float32)), fbits(want[k]))]
        assert not bad, (what, depth, bad)


# --------------------------------------------------------------------------------- 4. BVH
@pytest.mark.parametrize("name", K.BVH_SETS)
def test_bvh_on_device(pkg, orc, ctx, name):
    """vpx_bvh_set + vpx_bvh_intersect: zero direction components in both signs, NaN slabs,
    origins inside the root box, tmax at a node's entry, and both chains at VPX_BVH_MAX_DEPTH."""
    c = K.bvh_cases(pkg, orc)[name]
    if name.startswith("chain"):
        assert c["depth"] == pkg.abi.BVH_MAX_DEPTH and c["high"] <= 64
    ctx.bvh_set(c["tris"])
    got = ctx.bvh_intersect(api_rays(pkg.abi, [(o, d, t, 0) for o, d, t in c["rays"]]))
    bad = np.flatnonzero(fbits(got) != fbits(c["t"]))
    assert not len(bad), (name, bad[:8], got[bad[:4]], c["t"][bad[:4]])


# ------------------------------------------------------------------------- 5. the ID buffer
FRAME_SPHERES = K.R_SPHERES[:2]  # non-metal and glass
FRAME_TRIS = K.R_TRIS            # emissive, and smoke beside the room


def frame_desc(pkg, depth=0, area=False):
    desc = K.desc_of(pkg, "R0", FRAME_SPHERES, FRAME_TRIS).with_size(W, H)
    desc.max_bounces, desc.flags, desc.area_samples = depth, pkg.abi.VPX_FLAG_AA, 3
    if area:
        desc.points, desc.areas = [], [pkg.scene.area_light((0.5, 0.9, 0.2), (1.0, 0.95, 0.9), 1.2, 0.1)]
    return desc


@functools.lru_cache(maxsize=None)
def pixel_expect():
    """The restatement on GetPrimaryRayNoDOF's rays (camera.h:103-110, test_kat_reproject.Camera),
    row-major: REC rows."""
    cam = Camera((0.5, 0.5, -1.0), (0.5, 0.5, 0.5), W, H)
    rays = []
    for y in range(H):
        for x in range(W):
            r = cam.primary_ray(x, y)
            rays.append((tuple(r.O), tuple(r.D), 1e34, 0))
    # D is normalised already: hand it over raw, so that the records are those of Ray(O, P - O)
    return K.expect("R0", FRAME_SPHERES, FRAME_TRIS, rays, raw=True)["near"]


def test_id_buffer_over_the_shape_room(pkg, ctx):
    """vpx_render_ids at 40x24: every pixel equals vpx_pick_pixel's record and the restatement's;
    a shape pixel is .y = 1 | material << 16, face 0, cell 0."""
    desc = frame_desc(pkg)
    ctx.load_scene(desc)
    ids = ctx.render_ids(desc.frame_params(0))
    ctx.synchronize()
    u = pkg.context.unpack_ids(ids)
    raw = ids.cpu().numpy().view(np.uint32).reshape(-1, 4)
    want = pixel_expect()
    t, vox, mat = u["t"].reshape(-1), u["vox_index"].reshape(-1), u["material"].reshape(-1)
    assert np.array_equal(t.view(np.uint32), want["t"]), np.flatnonzero(t.view(np.uint32) != want["t"])[:8]
    assert np.array_equal(vox, want["vox"])
    assert np.array_equal(mat[vox != -2], want["material"][vox != -2])
    shape = vox == -1
    print(f"id buffer: {int(shape.sum())} shape pixels, {int((vox >= 0).sum())} voxel pixels, {int((vox == -2).sum())} misses")
    assert int(shape.sum()) >= 40 and int((vox >= 0).sum()) >= 200 and len(set(mat[shape])) >= 3
    assert np.array_equal(raw[shape, 1], 1 | (want["material"][shape] << 16)) and not raw[shape, 2:].any()
    for k in range(W * H):
        hit, cell = ctx.pick_pixel(W, H, k % W, k // W)
        face = 0 if not cell.flags & 2 else 1 + 2 * ((cell.flags >> 8) & 3) + ((cell.flags >> 10) & 1)
        rec = (int(fbits(f32(hit.t))), ((hit.vox_index + 2) & 0xFFFF) | (hit.material & 0xFF) << 16 | face << 24,
               (cell.cell[0] & 0xFFFF) | (cell.cell[1] << 16), cell.cell[2])
        assert tuple(int(v) for v in raw[k]) == rec, (k, raw[k], rec)


# ------------------------------------------------------------------------------ 6. frames
FRAMES = {
    # name: (depth, area light, lanes, stages that must launch, stages that must not)
    "depth 0": (0, False, 0, ("primary", "shadow"), ("frame",)),
    "depth 2": (2, False, 0, ("primary", "shadow", "bounce"), ("frame",)),
    "depth 2, area light": (2, True, 0, ("primary", "shadow", "bounce"), ("frame",)),
    "depth 8": (8, False, 0, ("primary", "shadow", "bounce"), ("frame",)),
    "depth 2, 2 lanes": (2, False, 2, (), ()),
}


@pytest.mark.parametrize("name", list(FRAMES))
def test_frames_over_the_shape_room(pkg, orc, name):
    """vpx_render against the oracle: accumulator bits, RGB8, shadow / bounce / cell counts."""
    depth, area, lanes, ran, idle = FRAMES[name]
    desc = frame_desc(pkg, depth, area)
    acc_o, rgb_o, st_o = orc.Oracle(pkg.abi, desc).render(desc.frame_params(0))
    c = pkg.context.Context(0)
    try:
        c.load_scene(desc)
        c.set_pipeline(lanes)
        acc = torch.zeros(W * H * 4, dtype=torch.float32, device=DEV)
        rgb = torch.zeros(W * H, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        c.counters(reset=True)
        if not lanes:
            c.profile_enable(4096)
            c.profile_read(reset=True)
        c.render(desc.frame_params(0), acc.data_ptr(), rgb.data_ptr())  # no stats: a frame with stats leaves the lanes
        c.synchronize()
        st = c.counters()
        if not lanes:
            launches = {k: v[1] for k, v in c.profile_read(reset=True).items()}
            print(name, "stage launches", launches, "frame kernel", c.last_frame_kernel())
            assert c.last_frame_kernel() == 0, name
            assert all(launches[s] > 0 for s in ran) and all(launches[s] == 0 for s in idle), (name, launches)
        got_acc = acc.cpu().numpy().view(np.uint32).reshape(-1, 4)
        got_rgb = rgb.cpu().numpy().view(np.uint32)
    finally:
        c.close()
    want = np.ascontiguousarray(acc_o, np.float32).view(np.uint32).reshape(-1, 4)
    assert not np.isnan(acc_o).any()
    bad = np.flatnonzero((got_acc != want).any(axis=1))
    assert not len(bad), (name, len(bad), bad[:8], got_acc[bad[:2]], want[bad[:2]])
    assert np.array_equal(got_rgb, rgb_o), name
    assert (st.shadow_rays, st.bounce_rays, st.dda_cells) == (st_o.shadow_rays, st_o.bounce_rays, st_o.dda_cells), name
    assert st.shadow_rays > 0 and (depth == 0 or st.bounce_rays > 0)


def test_reproject_frame_over_the_shape_room(pkg, orc):
    """One vpx_render_reproject frame (depth 2, the previous camera equal to the live one) against
    the oracle: history bits, RGB8 and the counts."""
    desc = frame_desc(pkg, 2)
    prev = pkg.scene.prev_camera(desc._cam_pos, desc._cam_target, W, H)
    hist_o = np.zeros((W * H, 4), np.float32)
    rgb_o, st_o = orc.Oracle(pkg.abi, desc).render_reproject(desc.frame_params(0), prev, hist_o)
    c = pkg.context.Context(0)
    try:
        c.load_scene(desc)
        hist = torch.zeros(W * H * 4, dtype=torch.float32, device=DEV)
        rgb = torch.zeros(W * H, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        st = c.render_reproject(desc.frame_params(0), prev, hist.data_ptr(), rgb.data_ptr(), stats=True)
        c.synchronize()
        got = hist.cpu().numpy().view(np.uint32).reshape(-1, 4)
        got_rgb = rgb.cpu().numpy().view(np.uint32)
    finally:
        c.close()
    assert not np.isnan(hist_o).any()
    bad = np.flatnonzero((got[:, :3] != hist_o.view(np.uint32)[:, :3]).any(axis=1))
    assert not len(bad), (len(bad), bad[:8])
    assert np.array_equal(got_rgb, rgb_o)
    assert (st.shadow_rays, st.bounce_rays, st.dda_cells) == (st_o.shadow_rays, st_o.bounce_rays, st_o.dda_cells)
