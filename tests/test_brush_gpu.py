"""Brush edits on the GPU (vpx_grid_brush) and the region-local level refresh behind them.

Bytes: after a call with 8 mixed brushes the whole grid equals the host restatement, with the
counts.  Levels: the 24 plane words, their low halves and the two mask levels equal those of a
fresh context that uploaded the final bytes (the full rebuild), and for the canyon the host
builder's words: a block placed high above the street (far influence on a width byte), a sphere
dug out of the ground so that bricks empty (values rise), a repaint (no brick flips), a 1 % random
37^3 grid with 8 brushes, a brush outside the grid, a whole-grid erase and a whole-grid fill.
Frames: the canyon at depth 0 and 2, serial and with 2 frames in flight with the edit between
them, a brush on the shared 32^3 grid of four instances, and a [0, 0] device set: every frame
equals the oracle on the edited grid bit for bit (accumulator floats, RGB8, ray / cell counts).
"""
import numpy as np
import pytest

from cases import bits
from test_axis_boxes import _torch, check, oracle_frames
from test_brush import mixed_brushes, numpy_brushes, world
from test_wide_boxes import build_wide_exe
from test_wide_boxes_gpu import BLOCK_ORIGIN, N, canyon_grid, canyon_scene, edited_grid, host_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wide_exe(tmp_path_factory):
    return build_wide_exe(tmp_path_factory.mktemp("wide_brush") / "wide_box_test")


def levels(ctx, n, grid_id=0):
    return {"wide": ctx.grid_wide_planes(grid_id, n), "axis": ctx.grid_axis_planes(grid_id, n),
            "l1": ctx.grid_level_words(grid_id, n, 1), "l2": ctx.grid_level_words(grid_id, n, 2)}


def rebuilt_levels(pkg, cells, n):
    """The levels of a fresh context that uploaded `cells`: the full rebuild."""
    ctx = pkg.context.Context(0)
    pkg.scene.GridSpec(n=n, dense=np.ascontiguousarray(cells).reshape(-1)).upload(ctx.lib, ctx.h, 0)
    out = levels(ctx, n)
    ctx.close()
    return out


def same_levels(got, want, what):
    for k in ("l2", "l1", "axis", "wide"):
        bad = np.flatnonzero(got[k].reshape(-1) != want[k].reshape(-1))
        assert len(bad) == 0, (what, k, len(bad), bad[:5], got[k].reshape(-1)[bad[:5]], want[k].reshape(-1)[bad[:5]])


def brushed(pkg, cells, n, brushes):
    """Upload, brush: (cells read back, result, levels after)."""
    ctx = pkg.context.Context(0)
    pkg.scene.GridSpec(n=n, dense=np.ascontiguousarray(cells).reshape(-1)).upload(ctx.lib, ctx.h, 0)
    res = ctx.grid_brush(0, brushes)
    got = ctx.grid_read_box(0, (0, 0, 0), (n, n, n)).reshape(-1)
    lv = levels(ctx, n)
    ctx.close()
    return got, res, lv


def check_edit(pkg, cells, n, brushes, what):
    want, changed, flipped = numpy_brushes(np.ascontiguousarray(cells).reshape(-1), n, brushes)
    got, res, lv = brushed(pkg, cells, n, brushes)
    assert np.array_equal(got, want), what
    assert (res.changed, res.flipped) == (changed, flipped), (what, res.changed, res.flipped, changed, flipped)
    same_levels(lv, rebuilt_levels(pkg, want, n), what)
    return want, res, lv


@pytest.mark.parametrize("n", [64, 37])
def test_bytes_and_counts(pkg, n):
    _torch()
    cells = world(n)
    brushes = mixed_brushes(pkg.scene, n)
    want, res, _ = check_edit(pkg, cells, n, brushes, f"8 mixed brushes, n={n}")
    host = cells.copy()
    hres = pkg.scene.apply_brushes(host, n, brushes)
    assert np.array_equal(host, want) and (hres.changed, hres.flipped) == (res.changed, res.flipped)
    assert res.changed > 0 and res.flipped > 0


def test_canyon_block_by_box_brush(pkg, wide_exe, tmp_path):
    """The block high above the street: the width of brick (7, 1, 4)'s box shrinks, far from the edit."""
    _torch()
    sc = pkg.scene
    x, y, z = BLOCK_ORIGIN
    want, res, lv = check_edit(pkg, canyon_grid(), N, [sc.box_brush((x, y, z), (x + 3, y + 3, z + 3), 1)], "canyon block")
    assert np.array_equal(want, edited_grid().reshape(-1)) and (res.changed, res.flipped) == (64, 1)
    assert np.array_equal(lv["wide"], host_words(wide_exe, tmp_path, edited_grid(), N))


def test_canyon_dig_raises_values(pkg, wide_exe, tmp_path):
    """A sphere dug out of the ground slab: bricks empty, cubes, lengths and widths grow."""
    _torch()
    sc = pkg.scene
    cells = canyon_grid()
    cells[:, 0:4, :] = 1  # a ground one brick thick
    before = rebuilt_levels(pkg, cells, N)
    want, res, lv = check_edit(pkg, cells, N, [sc.sphere_brush((30, 1, 20), 64, 255)], "canyon dig")
    assert res.flipped > 0 and res.changed > 0
    assert np.array_equal(lv["wide"], host_words(wide_exe, tmp_path, want.reshape(N, N, N), N))
    k0, k1 = before["wide"] & 255, lv["wide"] & 255
    assert (k1 > k0).any() and not (k1 < k0).any()


def test_repaint_flips_nothing(pkg):
    _torch()
    sc = pkg.scene
    cells = canyon_grid()
    before = rebuilt_levels(pkg, cells, N)
    _, res, lv = check_edit(pkg, cells, N, [sc.box_brush((0, 0, 0), (N - 1, 20, N - 1), 6, (0, 254))], "repaint")
    assert res.flipped == 0 and res.changed > 0
    same_levels(lv, before, "repaint leaves the levels")
    # digging inside bricks that stay occupied flips nothing either, but changes their cell masks
    _, res, lv = check_edit(pkg, cells, N, [sc.box_brush((2, 0, 2), (2, 0, 2), 255)], "one-cell dig in the ground")
    assert (res.changed, res.flipped) == (1, 0)
    assert np.array_equal(lv["wide"], before["wide"]) and not np.array_equal(lv["l1"], before["l1"])


def test_random_grid_eight_brushes(pkg):
    _torch()
    n = 37
    rng = np.random.default_rng(n)
    cells = np.where(rng.random(n ** 3) < 0.01, 3, 255).astype(np.uint8)
    sc = pkg.scene
    brushes = [sc.sphere_brush(rng.integers(-3, n + 3, 3), int(rng.integers(0, 60)), 255 if k % 2 else 4) for k in range(4)]
    for k in range(4):
        lo = rng.integers(-2, n, 3)
        brushes.append(sc.box_brush(lo, lo + rng.integers(0, 9, 3), 255 if k % 2 else 2, [(0, 255), (255, 255), (0, 254), (0, 255)][k]))
    _, res, _ = check_edit(pkg, cells, n, brushes, "random 37^3")
    assert res.flipped > 0


def test_brush_outside_and_whole_grid(pkg):
    _torch()
    sc, abi = pkg.scene, pkg.abi
    n = 37
    cells = world(n, 3)
    before = rebuilt_levels(pkg, cells, n)
    _, res, lv = check_edit(pkg, cells, n, [sc.sphere_brush((-20, 5, 5), 100, 3), sc.box_brush((n, 0, 0), (n + 5, 5, 5), 3)], "outside")
    assert (res.changed, res.flipped) == (0, 0)
    same_levels(lv, before, "a brush outside the grid")
    whole = ((0, 0, 0), (n - 1, n - 1, n - 1))
    # erase everything: equal to grid_fill(255); then fill everything from empty
    ctx = pkg.context.Context(0)
    sc.GridSpec(n=n, dense=cells).upload(ctx.lib, ctx.h, 0)
    res = ctx.grid_brush(0, [sc.box_brush(*whole, 255)])
    erased = levels(ctx, n)
    assert res.changed == int((cells != 255).sum()) and res.flipped > 0
    res = ctx.grid_brush(0, [sc.box_brush(*whole, 5)])
    filled = levels(ctx, n)
    assert res.changed == n ** 3 and res.flipped == ((n + 3) // 4) ** 3
    assert (ctx.grid_read_box(0, (0, 0, 0), (n, n, n)) == 5).all()
    ctx.grid_fill(0, 255)
    same_levels(erased, levels(ctx, n), "whole-grid erase against grid_fill(255)")
    ctx.grid_fill(0, 5)
    same_levels(filled, levels(ctx, n), "whole-grid fill against grid_fill(5)")
    # validation
    lib, good = ctx.lib, sc.box_brush((0, 0, 0), (1, 1, 1), 2)
    one = (abi.Brush * 1)(good)
    assert lib.vpx_grid_brush(ctx.h, 0, None, 1, None) == abi.VPX_E_INVALID
    assert lib.vpx_grid_brush(ctx.h, 0, one, 0, None) == abi.VPX_E_INVALID
    assert lib.vpx_grid_brush(ctx.h, 0, (abi.Brush * 257)(*[good] * 257), 257, None) == abi.VPX_E_INVALID
    assert lib.vpx_grid_brush(ctx.h, 7, one, 1, None) == abi.VPX_E_INVALID
    for field, value in (("shape", 2), ("reserved", 1), ("match_lo", 9)):
        bad = sc.box_brush((0, 0, 0), (1, 1, 1), 2, (0, 8))
        setattr(bad, field, value)
        assert lib.vpx_grid_brush(ctx.h, 0, (abi.Brush * 1)(bad), 1, None) == abi.VPX_E_INVALID, field
    assert lib.vpx_grid_level_words(ctx.h, 0, 3, filled["l1"].ctypes.data, 1) == abi.VPX_E_INVALID
    assert lib.vpx_grid_level_words(ctx.h, 0, 2, filled["l1"].ctypes.data, filled["l2"].size + 1) == abi.VPX_E_INVALID
    assert lib.vpx_grid_brush(ctx.h, 0, one, 1, None) == abi.VPX_OK  # out may be NULL
    ctx.close()


def render(pkg, desc, frames, lanes, brushes, grid_id=0, devices=None):
    """`frames` frames accumulated, the brushes applied after the first (test_axis_boxes.render with a brush)."""
    torch = _torch()
    ctx = pkg.context.Context(0) if devices is None else pkg.context.Context(devices=devices)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    ctx.load_scene(desc)
    ctx.set_pipeline(lanes)
    W, H = desc.width, desc.height
    acc = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.counters(reset=True)
    with torch.cuda.stream(s):
        for f in range(frames):
            if f == 1:
                ctx.grid_brush(grid_id, brushes)
            ctx.render(desc.frame_params(f), acc.data_ptr(), rgb.data_ptr())
    ctx.synchronize()
    st = ctx.counters()
    out = (bits(acc.cpu().numpy().reshape(-1, 4)), rgb.cpu().numpy().view(np.uint32),
           tuple(int(getattr(st, k)) for k in ("primary_rays", "shadow_rays", "bounce_rays", "dda_cells")))
    ctx.close()
    return out


@pytest.mark.parametrize("depth", [0, 2])
def test_canyon_frames_after_a_brush(pkg, orc, depth):
    _torch()
    sc = pkg.scene
    desc = canyon_scene(pkg, depth)
    x, y, z = BLOCK_ORIGIN
    brushes = [sc.box_brush((x, y, z), (x + 3, y + 3, z + 3), 1), sc.sphere_brush((31, 0, 40), 30, 255)]
    edited, _, _ = numpy_brushes(canyon_grid().reshape(-1), N, brushes)
    after = canyon_scene(pkg, depth, edited.reshape(N, N, N))
    want = oracle_frames(orc, pkg, [desc, after, after])
    unedited = oracle_frames(orc, pkg, [desc] * 3)
    assert not np.array_equal(want[1], unedited[1])  # the edit is in view
    for lanes in (0, 2):
        check(render(pkg, desc, 3, lanes, brushes), want, f"depth {depth}, {lanes} lanes")


def test_brush_on_a_shared_grid(pkg, orc):
    _torch()
    sc, abi = pkg.scene, pkg.abi

    def scene(small):
        desc = sc.model_scene("monu3", 64, 64, 64, 0, city_lights=True)
        desc.grids.append(sc.GridSpec(n=32, dense=small.reshape(-1).copy()))
        rng = np.random.default_rng(23)
        vols = [sc.volume()]
        for k in range(4):
            pos = (0.45 * (k % 2) - 0.1, 0.55, 0.45 * (k // 2) - 0.1)
            vols.append(sc.volume(pos, tuple(rng.uniform(0.2, 0.3, 3)), tuple(rng.uniform(-2, 2, 3)), grid_id=1))
        desc.volumes = (abi.Volume * len(vols))(*vols)
        desc.flags = abi.VPX_FLAG_AA
        return desc

    small = canyon_grid(32)
    brushes = [sc.sphere_brush((16, 20, 16), 40, 5), sc.box_brush((0, 0, 0), (31, 0, 12), 255)]
    edited, _, flipped = numpy_brushes(small.reshape(-1), 32, brushes)
    assert flipped > 0
    desc = scene(small)
    want = oracle_frames(orc, pkg, [desc, scene(edited.reshape(32, 32, 32))])
    assert not np.array_equal(want[1], oracle_frames(orc, pkg, [desc, desc])[1])
    check(render(pkg, desc, 2, 0, brushes, grid_id=1), want, "four instances of one brushed 32^3 canyon")


def test_brush_on_a_device_set(pkg):
    _torch()
    sc = pkg.scene
    desc = canyon_scene(pkg, 0)
    x, y, z = BLOCK_ORIGIN
    brushes = [sc.box_brush((x, y, z), (x + 3, y + 3, z + 3), 1), sc.sphere_brush((31, 0, 40), 30, 255)]
    single = render(pkg, desc, 2, 0, brushes)
    check(render(pkg, desc, 2, 0, brushes, devices=[0, 0]), single, "device set [0, 0]")
