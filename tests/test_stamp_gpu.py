"""Model stamps on the GPU (vpx_grid_stamp, vpx_model_capture, vpx_model_read).

Bytes, counts and levels: one call of 48 stamps, every orientation, in a 64^3 world (16-byte
spans), a 37^3 and a 40^3 one (one thread per cell) against tests/stamp_ref.py, the levels against
a fresh context's full rebuild of the final bytes.  Span edges: a 33x2x2 model at x = -1, 0, 15,
16, 17, 31 and 40 of 64^3 and 48^3, plain and mirrored, a 1x1x1 model, model z along grid x.
Stamps that change nothing or flip nothing leave the levels alone.  A box of the canyon is
captured, dug out and put down 5 cells further with a quarter turn without leaving the device.
Frames: the canyon at depth 0 and 2, serial and with 2 frames in flight, stamped between two
frames, equals the oracle on the edited grid bit for bit; a [0, 0] device set equals the single
device.  A context that captured and stamped gives every buffer back.
"""
import ctypes as C
import gc

import numpy as np
import pytest

from cases import bits
from stamp_ref import CONSTANT, GRID_BYTES, ORIENTATIONS, numpy_stamps
from test_axis_boxes import _torch, check, oracle_frames
from test_brush import world
from test_brush_gpu import levels, rebuilt_levels, same_levels
from test_wide_boxes_gpu import BLOCK_ORIGIN, N, canyon_grid, canyon_scene

pytestmark = pytest.mark.gpu


def stamped(pkg, cells, n, models, stamps):
    """Upload the grid and the models, stamp: (cells read back, result, levels after)."""
    ctx = pkg.context.Context(0)
    pkg.scene.GridSpec(n=n, dense=np.ascontiguousarray(cells).reshape(-1)).upload(ctx.lib, ctx.h, 0)
    for k, (size, vox) in enumerate(models):
        ctx.model_upload(k, size, vox)
    res = ctx.grid_stamp(0, stamps)
    got = ctx.grid_read_box(0, (0, 0, 0), (n, n, n)).reshape(-1)
    lv = levels(ctx, n)
    ctx.close()
    return got, res, lv


def check_edit(pkg, cells, n, models, stamps, what):
    want, changed, flipped = numpy_stamps(cells, n, models, stamps)
    got, res, lv = stamped(pkg, cells, n, models, stamps)
    assert np.array_equal(got, want), what
    assert (res.changed, res.flipped) == (changed, flipped), (what, res.changed, res.flipped, changed, flipped)
    same_levels(lv, rebuilt_levels(pkg, want, n), what)
    host = np.ascontiguousarray(cells, np.uint8).reshape(-1).copy()
    hres = pkg.scene.apply_stamps(host, n, models, stamps)
    assert np.array_equal(host, want) and (hres.changed, hres.flipped) == (changed, flipped), what
    return want, res, lv


@pytest.mark.parametrize("n", [64, 37, 40])
def test_every_orientation(pkg, n):
    """48 stamps that do not overlap, on a lattice wider than the model's longest side."""
    _torch()
    sc = pkg.scene
    rng = np.random.default_rng(n)
    vox = rng.integers(1, 255, 105).astype(np.uint8)
    vox[rng.random(105) < 0.2] = 0
    models = [((3, 5, 7), vox)]
    pitch = 9 if n == 37 else 8
    per = n // pitch
    assert per ** 3 >= 48
    stamps = []
    for k, (axes, flips) in enumerate(ORIENTATIONS):
        slot = (k % per, (k // per) % per, k // (per * per))
        stamps.append(sc.stamp(0, [s * pitch + k % (pitch - 6) for s in slot], sc.orient(axes, flips)))
    _, res, _ = check_edit(pkg, world(n), n, models, stamps, f"48 orientations, n={n}")
    assert res.changed > 48 * 60 and res.flipped > 0


@pytest.mark.parametrize("n", [64, 48])
def test_span_edges(pkg, n):
    _torch()
    sc = pkg.scene
    rng = np.random.default_rng(n + 1)
    models = [((33, 2, 2), rng.integers(1, 256, 132).astype(np.uint8)), ((1, 1, 1), np.array([9], np.uint8)),
              ((2, 3, 33), rng.integers(0, 5, 198).astype(np.uint8))]
    stamps = []
    for k, x in enumerate((-1, 0, 15, 16, 17, 31, 40)):
        stamps.append(sc.stamp(0, (x, 3 + 3 * k, 5)))
        stamps.append(sc.stamp(0, (x, 3 + 3 * k, 9), sc.orient((0, 1, 2), (True, False, False))))
        stamps.append(sc.stamp(1, (max(x, 0), 30, 2 + k)))
        stamps.append(sc.stamp(2, (x, 32, 3 * k + 2), sc.orient((2, 1, 0), (bool(k & 1), False, False))))  # model z on grid x
    stamps += [sc.stamp(1, (n - 1, n - 1, n - 1)), sc.stamp(1, (n, 0, 0)), sc.stamp(0, (n - 1, 0, 0)), sc.stamp(0, (-32, 2, 0))]
    _, res, _ = check_edit(pkg, world(n), n, models, stamps, f"span edges, n={n}")
    assert res.changed > 0


def test_no_flip(pkg):
    _torch()
    sc = pkg.scene
    cells = canyon_grid()
    before = rebuilt_levels(pkg, cells, N)
    models = [((20, 6, 20), np.full(2400, 6, np.uint8))]
    # the filter excludes every cell: nothing is placed
    _, res, lv = check_edit(pkg, cells, N, models, [sc.stamp(0, (20, 0, 20), match=(7, 7))], "nothing placed")
    assert (res.changed, res.flipped) == (0, 0)
    same_levels(lv, before, "a stamp that places nothing")
    # a repaint of what is solid
    _, res, lv = check_edit(pkg, cells, N, models, [sc.stamp(0, (20, 0, 20), flags=CONSTANT, value=6, match=(0, 254))], "repaint")
    assert res.changed > 0 and res.flipped == 0
    same_levels(lv, before, "a repaint leaves the levels")


def test_capture_round_trip(pkg):
    """Copy, dig and paste with a quarter turn: the move never leaves the device."""
    _torch()
    sc = pkg.scene
    cells = canyon_grid()
    origin, shape = (25, 0, 22), (7, 6, 14)  # x 25..38 across both walls and the ground, straddling bricks
    ctx = pkg.context.Context(0)
    sc.GridSpec(n=N, dense=cells.reshape(-1).copy()).upload(ctx.lib, ctx.h, 0)
    ctx.model_capture(3, 0, origin, shape)
    box = ctx.grid_read_box(0, origin, shape)
    assert np.array_equal(ctx.model_read(3), box) and (box != 255).any() and (box == 255).any()
    ctx.model_capture(1, 0, (16, 0, 20), (4, 5, 32))  # 16-byte rows
    assert np.array_equal(ctx.model_read(1), ctx.grid_read_box(0, (16, 0, 20), (4, 5, 32)))
    ctx.model_capture(1, 0, (0, 0, 0), (1, 1, 1))  # replaced
    assert ctx.model_read(1).shape == (1, 1, 1)
    turn = sc.orient((2, 1, 0), (True, False, False))
    move = [sc.stamp(3, origin, flags=GRID_BYTES | CONSTANT, value=255), sc.stamp(3, (origin[0], 0, origin[2] + 5), turn, GRID_BYTES)]
    models = [None, None, None, ((shape[2], shape[1], shape[0]), box.reshape(-1))]
    want, changed, flipped = numpy_stamps(cells, N, models, move)
    res = ctx.grid_stamp(0, move)
    assert np.array_equal(ctx.grid_read_box(0, (0, 0, 0), (N, N, N)).reshape(-1), want)
    assert (res.changed, res.flipped) == (changed, flipped) and changed > 0 and flipped > 0
    same_levels(levels(ctx, N), rebuilt_levels(pkg, want, N), "the move")
    # put back: into the emptied box, identity with GRID_BYTES restores the captured cells
    ctx.grid_brush(0, [sc.box_brush(origin, (origin[0] + shape[2] - 1, origin[1] + shape[1] - 1, origin[2] + shape[0] - 1), 255)])
    ctx.grid_stamp(0, [sc.stamp(3, origin, pkg.abi.ORIENT_IDENTITY, GRID_BYTES)])
    assert np.array_equal(ctx.grid_read_box(0, origin, shape), box)
    ctx.close()


def test_captured_material_zero_survives(pkg):
    _torch()
    sc = pkg.scene
    n = 37
    cells = world(n).reshape(n, n, n)
    cells[5:9, 3:6, 7:12] = 0  # material 0
    ctx = pkg.context.Context(0)
    sc.GridSpec(n=n, dense=cells.reshape(-1).copy()).upload(ctx.lib, ctx.h, 0)
    origin, shape = (6, 2, 4), (6, 5, 7)
    ctx.model_capture(0, 0, origin, shape)
    box = ctx.model_read(0)
    assert np.array_equal(box, cells[4:10, 2:7, 6:13]) and (box == 0).any()
    st = [sc.stamp(0, (20, 20, 20), sc.orient((1, 0, 2), (False, True, False)), GRID_BYTES)]
    want, changed, flipped = numpy_stamps(cells, n, [((7, 5, 6), box.reshape(-1))], st)
    res = ctx.grid_stamp(0, st)
    got = ctx.grid_read_box(0, (0, 0, 0), (n, n, n))
    assert np.array_equal(got.reshape(-1), want) and (res.changed, res.flipped) == (changed, flipped)
    assert (got[20:, 20:, 20:] == 0).sum() == (box == 0).sum() > 0
    same_levels(levels(ctx, n), rebuilt_levels(pkg, want, n), "material 0")
    ctx.close()


# the edit of the frame tests: a block above the street, and a ring dug out of the ground
def frame_edit(pkg):
    sc = pkg.scene
    ring = np.zeros((9, 1, 9), np.uint8)  # [z, y, x]
    zz, xx = np.mgrid[0:9, 0:9]
    ring[:, 0, :][(zz - 4) ** 2 + (xx - 4) ** 2 <= 18] = 3
    models = [((4, 4, 4), np.ones(64, np.uint8)), ((9, 1, 9), ring.reshape(-1))]
    stamps = [sc.stamp(0, BLOCK_ORIGIN, match=(255, 255)), sc.stamp(1, (27, 0, 36), flags=CONSTANT, value=255)]
    return models, stamps


def render(pkg, desc, frames, lanes, models, stamps, devices=None):
    """`frames` frames accumulated, the stamps applied after the first (test_brush_gpu.render with stamps)."""
    torch = _torch()
    ctx = pkg.context.Context(0) if devices is None else pkg.context.Context(devices=devices)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    ctx.load_scene(desc)
    for k, (size, vox) in enumerate(models):
        ctx.model_upload(k, size, vox)
    ctx.set_pipeline(lanes)
    W, H = desc.width, desc.height
    acc = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.counters(reset=True)
    with torch.cuda.stream(s):
        for f in range(frames):
            if f == 1:
                ctx.grid_stamp(0, stamps)
            ctx.render(desc.frame_params(f), acc.data_ptr(), rgb.data_ptr())
    ctx.synchronize()
    st = ctx.counters()
    out = (bits(acc.cpu().numpy().reshape(-1, 4)), rgb.cpu().numpy().view(np.uint32),
           tuple(int(getattr(st, k)) for k in ("primary_rays", "shadow_rays", "bounce_rays", "dda_cells")))
    ctx.close()
    return out


@pytest.mark.parametrize("depth", [0, 2])
def test_canyon_frames_after_a_stamp(pkg, orc, depth):
    _torch()
    desc = canyon_scene(pkg, depth)
    models, stamps = frame_edit(pkg)
    edited, changed, flipped = numpy_stamps(canyon_grid().reshape(-1), N, models, stamps)
    assert changed > 64 and flipped > 0
    after = canyon_scene(pkg, depth, edited.reshape(N, N, N))
    want = oracle_frames(orc, pkg, [desc, after, after])
    unedited = oracle_frames(orc, pkg, [desc] * 3)
    assert not np.array_equal(want[1], unedited[1])  # the edit is in view
    for lanes in (0, 2):
        check(render(pkg, desc, 3, lanes, models, stamps), want, f"depth {depth}, {lanes} lanes")


def test_stamp_on_a_device_set(pkg):
    _torch()
    desc = canyon_scene(pkg, 0)
    models, stamps = frame_edit(pkg)
    single = render(pkg, desc, 2, 0, models, stamps)
    check(render(pkg, desc, 2, 0, models, stamps, devices=[0, 0]), single, "device set [0, 0]")
    # a capture on the set: every member holds it, the first one is read
    ctx = pkg.context.Context(devices=[0, 0])
    ctx.load_scene(desc)
    ctx.model_capture(0, 0, (24, 0, 20), (3, 4, 16))
    box = canyon_grid()[20:23, 0:4, 24:40]
    assert np.array_equal(ctx.model_read(0), box)
    paste = [pkg.scene.stamp(0, (24, 42, 20), flags=GRID_BYTES)]
    want, changed, flipped = numpy_stamps(canyon_grid(), N, [((16, 4, 3), box.reshape(-1))], paste)
    res = ctx.grid_stamp(0, paste)
    assert (res.changed, res.flipped) == (changed, flipped) and changed == int((box != 255).sum())
    assert np.array_equal(ctx.grid_read_box(0, (0, 0, 0), (N, N, N)).reshape(-1), want)
    ctx.close()


def test_buffers_come_back(pkg):
    _torch()
    gc.collect()
    lib = pkg.load_library()
    before = int(lib.vpx_debug_live_buffers())
    ctx = pkg.context.Context(0)
    pkg.scene.GridSpec(n=N, dense=canyon_grid().reshape(-1)).upload(ctx.lib, ctx.h, 0)
    ctx.model_capture(0, 0, (25, 0, 22), (7, 6, 14))
    ctx.model_capture(5, 0, (16, 0, 16), (2, 2, 16))
    held = int(lib.vpx_debug_live_buffers())
    assert held > before
    res = ctx.grid_stamp(0, [pkg.scene.stamp(0, (25, 20, 22), flags=GRID_BYTES), pkg.scene.stamp(5, (3, 40, 3), flags=GRID_BYTES)])
    assert res.changed > 0
    after_first = int(lib.vpx_debug_live_buffers())
    ctx.grid_stamp(0, [pkg.scene.stamp(0, (25, 30, 22), flags=GRID_BYTES)])
    assert int(lib.vpx_debug_live_buffers()) == after_first  # a stamp call allocates nothing of its own
    ctx.model_capture(0, 0, (0, 0, 0), (3, 3, 3))  # a replaced model frees the one before it
    assert int(lib.vpx_debug_live_buffers()) == after_first
    ctx.close()
    assert int(lib.vpx_debug_live_buffers()) == before


def test_refusals(pkg):
    _torch()
    abi, sc = pkg.abi, pkg.scene
    n = 16
    ctx = pkg.context.Context(0)
    sc.GridSpec(n=n, dense=world(n)).upload(ctx.lib, ctx.h, 0)
    ctx.model_upload(0, (2, 2, 2), np.ones(8, np.uint8))
    lib, good = ctx.lib, sc.stamp(0, (0, 0, 0))
    one = (abi.Stamp * 1)(good)
    assert lib.vpx_grid_stamp(ctx.h, 0, one, 1, None) == abi.VPX_OK  # out may be NULL
    assert lib.vpx_grid_stamp(ctx.h, 0, None, 1, None) == abi.VPX_E_INVALID
    assert lib.vpx_grid_stamp(ctx.h, 0, one, 0, None) == abi.VPX_E_INVALID
    assert lib.vpx_grid_stamp(ctx.h, 0, (abi.Stamp * 257)(*[good] * 257), 257, None) == abi.VPX_E_INVALID
    assert lib.vpx_grid_stamp(ctx.h, 0, (abi.Stamp * 256)(*[good] * 256), 256, None) == abi.VPX_OK
    assert lib.vpx_grid_stamp(ctx.h, 7, one, 1, None) == abi.VPX_E_INVALID  # unknown grid
    for model_id in (1, 4097, 2 ** 32 - 1):  # unknown model
        assert lib.vpx_grid_stamp(ctx.h, 0, (abi.Stamp * 1)(sc.stamp(model_id, (0, 0, 0))), 1, None) == abi.VPX_E_INVALID
    for field, value in (("orient", 0x00), ("orient", 0x14), ("orient", 0x27), ("orient", 0x24 | 0x40), ("orient", 0x24 | 0x800),
                         ("flags", 4), ("reserved", 1), ("reserved2", 1), ("match_lo", 9)):
        bad = sc.stamp(0, (0, 0, 0), match=(0, 8))
        setattr(bad, field, value)
        assert lib.vpx_grid_stamp(ctx.h, 0, (abi.Stamp * 2)(good, bad), 2, None) == abi.VPX_E_INVALID, (field, value)
    before = ctx.grid_read_box(0, (0, 0, 0), (n, n, n))
    cap = lib.vpx_model_capture
    assert cap(ctx.h, 2, 7, 0, 0, 0, 2, 2, 2) == abi.VPX_E_INVALID  # unknown grid
    assert cap(ctx.h, 4097, 0, 0, 0, 0, 2, 2, 2) == abi.VPX_E_INVALID
    for box in ((0, 0, 0, 0, 2, 2), (0, 0, 0, 2, 2, 0), (15, 0, 0, 2, 2, 2), (0, 0, 16, 1, 1, 1), (0, 0, 0, 17, 1, 1), (2 ** 32 - 1, 0, 0, 2, 1, 1)):
        assert cap(ctx.h, 0, 0, *box) == abi.VPX_E_INVALID, box
    assert ctx.model_read(0).shape == (2, 2, 2)  # a refused capture leaves the model
    size = (C.c_uint32 * 3)()
    buf = np.zeros(8, np.uint8)
    assert lib.vpx_model_read(ctx.h, 1, None, 0, size) == abi.VPX_E_INVALID  # unknown model
    assert lib.vpx_model_read(ctx.h, 0, buf.ctypes.data, 7, size) == abi.VPX_E_INVALID  # cap too small
    assert lib.vpx_model_read(ctx.h, 0, buf.ctypes.data, 8, None) == abi.VPX_E_INVALID
    assert lib.vpx_model_read(ctx.h, 0, None, 0, size) == abi.VPX_OK and tuple(size) == (2, 2, 2)
    assert lib.vpx_model_read(ctx.h, 0, buf.ctypes.data, 8, size) == abi.VPX_OK and (buf == 1).all()
    ctx.model_upload(0, None, None)
    assert lib.vpx_grid_stamp(ctx.h, 0, one, 1, None) == abi.VPX_E_INVALID  # the model is gone
    assert np.array_equal(ctx.grid_read_box(0, (0, 0, 0), (n, n, n)), before)
    ctx.close()
