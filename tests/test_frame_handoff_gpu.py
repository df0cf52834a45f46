"""The depth-0 frame kernel's walk-state handoff and its LDS list (csrc/vpx_wavefront.hpp: WalkStash,
Frame0Lds), on the GPU.

In k_frame0 a pixel thread whose Setup3DDDA succeeds leaves the walk's start state (cell, t, tmax,
tdelta, the three step signs) in the path's own LDS records, and the walker lane that takes the
path after the tile's compaction starts from it instead of setting the walk up again; the tile's
shadow list lives in the .w words of its SL records.  Nothing may change: every case compares the
accumulator floats, RGB8 and the primary / shadow / nearest (bounce_rays) / DDA-cell counters with
the oracle bit for bit, in both arithmetic modes, serial, with three lanes and as rank 0 of 2's
packed shard.

The 128^3 monu3 city of test_frame_views_gpu.py from cameras that reach every branch of the setup:
  inside   the camera inside the grid (Setup3DDDA's Contains branch, every pixel walks), 64x48 and
           70x50 (a ragged last tile), AA on;
  partial  outside, the cube covering part of the frame (the Intersect branch; tiles with 0, a few
           and 256 walkers: checked below from the camera's own rays), AA on;
  away     looking away from the cube: no walker in any tile, no cell read;
  axis     axis-aligned without AA, 65x49 from in front of the cube's centre and 64x48 from (0, 0.5, -1),
           whose centre column and row have a direction component of exactly 0 (u = 32 / 64,
           v = 24 / 48: an infinite tdelta, the sign word).
One context renders inside, away, inside (stale stash words); a depth-2 frame and a two-volume
frame take no stash and still match.
"""
import numpy as np
import pytest

from cases import bits
from test_axis_boxes import X86, _torch, check, oracle_frames
from test_frame_views_gpu import COUNTS, open_ctx, render_frames, replace

pytestmark = pytest.mark.gpu

FRAMES = 2
ARITH = ["exact", pytest.param("x86", marks=pytest.mark.skipif(not X86, reason="x86 intrinsics"))]
# name: (camera position, target, (width, height), AA)
VIEWS = {
    "inside": ((0.5, 0.9, 0.5), (0.3, 0.1, 0.7), (64, 48), True),
    "inside ragged": ((0.5, 0.9, 0.5), (0.3, 0.1, 0.7), (70, 50), True),
    "partial": ((1.5, 1.1, -0.7), (1.1, 0.6, 0.4), (64, 48), True),
    "away": ((0.5, 0.5, -1.0), (0.5, 0.5, -3.0), (64, 48), True),
    "axis 65x49": ((0.5, 0.5, -1.0), (0.5, 0.5, 0.5), (65, 49), False),
    "axis zero": ((0.0, 0.5, -1.0), (0.0, 0.5, 0.5), (64, 48), False),
}


def view(pkg, name, depth=0):
    pos, target, size, aa = VIEWS[name]
    _torch()
    desc = pkg.scene.city_scene("monu3", 128, size[0], size[1], depth, cam=(pos, target))
    desc.flags = pkg.abi.VPX_FLAG_AA if aa else 0
    return desc


def pixel_dirs(desc):
    """P - cam_pos of every pixel without AA (primary_ray's float32 operations), [H, W, 3]."""
    f = np.float32
    cam = desc.camera
    v3 = lambda a: np.array(list(a), f)
    tl, tr, bl, cp = v3(cam.top_left), v3(cam.top_right), v3(cam.bottom_left), v3(cam.cam_pos)
    u = np.arange(desc.width, dtype=f) * (f(1.0) / f(desc.width))
    v = np.arange(desc.height, dtype=f) * (f(1.0) / f(desc.height))
    P = (tl + (tr - tl) * u[None, :, None]) + (bl - tl) * v[:, None, None]
    return (P - cp).astype(f), cp


def meets_cube(desc):
    """Whether each pixel's ray (no AA) meets the unit cube of the one volume, [H, W]."""
    d, cp = pixel_dirs(desc)
    d = d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (0.0 - cp) / d, (1.0 - cp) / d
    lo = np.nanmax(np.minimum(t0, t1), axis=2)
    hi = np.nanmin(np.maximum(t0, t1), axis=2)
    return (lo <= hi) & (hi > 0)


def test_views_reach_their_branches(pkg):
    """The cameras do what the cases are named for (from the cameras' own rays, no render)."""
    inside = view(pkg, "inside")
    cp = inside.camera.cam_pos
    assert all(0.0 < c < 1.0 for c in cp)
    m = meets_cube(view(pkg, "partial"))
    per_tile = [int(m[y:y + 16, x:x + 16].sum()) for y in range(0, 48, 16) for x in range(0, 64, 16)]
    assert 0 in per_tile and 256 in per_tile and any(0 < n < 256 for n in per_tile), per_tile
    assert not meets_cube(view(pkg, "away")).any()
    d, _ = pixel_dirs(view(pkg, "axis zero"))
    assert (d[:, 32, 0] == 0).all() and (d[24, :, 1] == 0).all()
    assert meets_cube(view(pkg, "axis zero")).any() and meets_cube(view(pkg, "axis 65x49")).any()


_WANT = {}


def want_of(pkg, orc, key, descs, x86=False):
    if key not in _WANT:
        _WANT[key] = oracle_frames(orc, pkg, descs, x86=x86)
    return _WANT[key]


def render_rank0(pkg, desc, arith):
    """render_tiles_accum for both ranks of 2; rank 0's packed shard scattered to its pixels."""
    torch = _torch()
    ctx, s = open_ctx(pkg, desc, arith)
    W, H = desc.width, desc.height
    L = ctx.packed_len(W, H, 2)
    ctx.counters(reset=True)
    forms, shard = [], None
    for rank in range(2):
        acc = torch.zeros(L * 4, dtype=torch.float32, device="cuda")
        rgb = torch.zeros(L, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for f in range(FRAMES):
                ctx.render_tiles_accum(desc.frame_params(f), rank, 2, acc.data_ptr(), rgb.data_ptr())
                forms.append(ctx.last_frame_kernel())
        ctx.synchronize()
        if rank == 0:
            shard = (bits(acc.cpu().numpy().reshape(-1, 4)), rgb.cpu().numpy().view(np.uint32))
    st = ctx.counters()
    counts = tuple(int(getattr(st, k)) for k in COUNTS)
    ctx.close()
    return shard, counts, forms


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("how", ["serial", "lanes", "rank"])
@pytest.mark.parametrize("name", list(VIEWS))
def test_view_frames(pkg, orc, name, how, arith):
    desc = view(pkg, name)
    want = want_of(pkg, orc, (name, arith), [desc] * FRAMES, x86=arith == "x86")
    primary, shadow, _, cells = want[2]
    assert primary > 0
    if name == "away":
        assert shadow == 0 and cells == 0, want[2]
    else:
        assert shadow > 0 and cells > 0, want[2]
    if how == "rank":
        shard, counts, forms = render_rank0(pkg, desc, arith)
        assert forms == [2] * (2 * FRAMES)
        ids = pkg.dist.rank_pixel_ids(desc.width, desc.height, 0, 2)
        ok = ids >= 0
        assert ok.sum() > 0
        assert np.array_equal(shard[0][ok], want[0][ids[ok]]), f"packed accumulator ({name}, {arith})"
        assert np.array_equal(shard[1][ok], want[1][ids[ok]]), f"packed RGB8 ({name}, {arith})"
        assert counts == want[2], (name, arith, counts, want[2])
        return
    got, forms = render_frames(pkg, [desc] * FRAMES, arith, 3 if how == "lanes" else 0)
    assert forms == [2] * FRAMES
    check(got, want, f"{name}, {arith}, {how}")


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("how", ["serial", "lanes"])
def test_inside_away_inside(pkg, orc, how, arith):
    """One context, the camera moving before every frame: every tile full of walkers, none, full
    again.  Each frame alone, in an accumulator of its own, equals the oracle's frame of that view
    (a walker starting from words an earlier frame left behind would not)."""
    torch = _torch()
    inside, away = view(pkg, "inside"), view(pkg, "away")
    descs = [inside, away, inside]
    ctx, s = open_ctx(pkg, inside, arith, 3 if how == "lanes" else 0)
    W, H = inside.width, inside.height
    accs = [torch.zeros(W * H * 4, dtype=torch.float32, device="cuda") for _ in descs]
    rgbs = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in descs]
    torch.cuda.synchronize()
    forms, counts = [], []
    for f, d in enumerate(descs):
        ctx.counters(reset=True)
        ctx.set_camera(d.camera)
        with torch.cuda.stream(s):
            ctx.render(d.frame_params(0), accs[f].data_ptr(), rgbs[f].data_ptr())
        forms.append(ctx.last_frame_kernel())
        st = ctx.counters()
        counts.append(tuple(int(getattr(st, k)) for k in COUNTS))
    ctx.synchronize()
    assert forms == [2, 2, 2]
    for f, d in enumerate(descs):
        kind = "inside" if d is inside else "away"
        want = want_of(pkg, orc, (kind, arith, "one frame"), [d], x86=arith == "x86")
        got = (bits(accs[f].cpu().numpy().reshape(-1, 4)), rgbs[f].cpu().numpy().view(np.uint32), counts[f])
        check(got, want, f"frame {f} ({kind}), {arith}, {how}")
    ctx.close()


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("kind", ["depth2", "two volumes"])
def test_paths_without_a_stash(pkg, orc, kind, arith):
    """The heads that take no stash (the split frame's k_primary, the multi-volume kernels), from
    the inside view."""
    sc = pkg.scene
    if kind == "depth2":
        desc = view(pkg, "inside", depth=2)
    else:
        vols = [sc.volume(), sc.volume(position=(0.2, 1.0, 0.2), scale=(0.3, 0.3, 0.3))]
        desc = replace(view(pkg, "inside"), volumes=(pkg.abi.Volume * 2)(*vols))
    want = want_of(pkg, orc, (kind, arith), [desc] * FRAMES, x86=arith == "x86")
    got, forms = render_frames(pkg, [desc] * FRAMES, arith, 0)
    assert forms == [0] * FRAMES
    check(got, want, f"{kind}, {arith}")
