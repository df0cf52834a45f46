"""The walkers' instruction forms (csrc/vpx_skip.hpp box_sel / df_box_sel, seg_params_nb, step1;
csrc/vpx_trace.hpp walk_wave's class table; the walk kinds' `packed`), on the GPU.

k_frame0's two walk kinds take their boxes through selectors packed once per walk and their
class outcomes from a table; every kernel shares the rewritten closed-form parameters and step.
Nothing may change: the 128^3 monu3 city of test_frame_views_gpu.py from the cameras of
test_frame_handoff_gpu.py (inside the grid at 64x48 and 70x50, outside with partly walking tiles,
looking away, axis-aligned without AA: direction components of exactly 0, so a sign bit of -0 and
an infinite tdelta reach the packed word), in both arithmetic modes, serial, with three lanes and as
rank 0 of 2, against the oracle bit for bit: accumulator, RGB8, and the ray and cell counts.  A
sky-texture frame runs a guaranteed-form instance; a depth-2 frame and a two-volume frame run the
kinds that keep today's boxes; the axis-aligned rays through the hit-cell query (walk_wave's REC,
whose stepped axis is read off the coordinates) against the restated plain DDA.
"""
import dataclasses

import numpy as np
import pytest

from test_axis_boxes import X86, check
from test_frame_handoff_gpu import VIEWS, pixel_dirs, render_rank0, view, want_of
from test_frame_views_gpu import render_frames, replace, variant
from test_frame_views_gpu import want_of as want_lit
from test_hit_cells import plain_walk, vols_of
from test_ray_filter import NO_RANGE

pytestmark = pytest.mark.gpu

FRAMES = 2
ARITH = ["exact", pytest.param("x86", marks=pytest.mark.skipif(not X86, reason="x86 intrinsics"))]
NAMES = ["inside", "inside ragged", "partial", "away", "axis zero"]


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("how", ["serial", "lanes", "rank"])
@pytest.mark.parametrize("name", NAMES)
def test_view_frames(pkg, orc, name, how, arith):
    desc = view(pkg, name)
    assert (desc.width, desc.height) == VIEWS[name][2]
    want = want_of(pkg, orc, (name, arith), [desc] * FRAMES, x86=arith == "x86")
    primary, shadow, _, cells = want[2]
    assert primary > 0 and (name == "away") == (cells == 0), want[2]
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
    assert forms == [2] * FRAMES  # the lean form of k_frame0
    check(got, want, f"{name}, {arith}, {how}")


def test_sky_texture_frame(pkg, orc):
    """The guaranteed-form instance of k_frame0 (the sky texture keeps the lean form out)."""
    desc = variant(pkg, (64, 48), "sky")
    want = want_lit(pkg, orc, ("sky", (64, 48), "exact"), [desc] * FRAMES)
    got, forms = render_frames(pkg, [desc] * FRAMES, "exact", 0)
    assert forms == [1] * FRAMES
    check(got, want, "sky texture")


@pytest.mark.parametrize("kind", ["depth2", "two volumes"])
def test_kinds_outside_the_frame_kernel(pkg, orc, kind):
    """The split frame's kernels (k_primary, the tile shadow walkers, the bounce walks) and the
    multi-volume kernels: the kinds without `packed`, on the shared step and closed forms."""
    sc = pkg.scene
    if kind == "depth2":
        desc = view(pkg, "inside", depth=2)
    else:
        vols = [sc.volume(), sc.volume(position=(0.2, 1.0, 0.2), scale=(0.3, 0.3, 0.3))]
        desc = replace(view(pkg, "inside"), volumes=(pkg.abi.Volume * 2)(*vols))
    want = want_of(pkg, orc, (kind, "exact"), [desc] * FRAMES)
    got, forms = render_frames(pkg, [desc] * FRAMES, "exact", 0)
    assert forms == [0] * FRAMES
    check(got, want, kind)


def test_axis_rays_through_the_hit_cell_query(pkg):
    """Rays of the axis-aligned view as one vpx_trace batch through find_nearest_cells: the right
    half of its centre row (direction y exactly 0; the left half and the centre column miss the
    cube), a grid of its right-hand pixels, and rays with one or two components of exactly +0 or -0
    from points in front of and inside the cube.  t, cell, stepped axis and its sign, and the visit
    count of every ray against the plain DDA."""
    from test_hit_cells_gpu import compare_with_plain  # (skips at import without a GPU)

    desc = view(pkg, "axis zero")
    d, cp = pixel_dirs(desc)
    H, W = d.shape[:2]
    rows = [d[24, x] for x in range(32, W)] + [d[y, x] for y in range(0, H, 4) for x in range(33, W, 4)]
    o = [np.array(cp, np.float32)] * len(rows)
    nz = np.float32(-0.0)
    for ox, oy in [(0.5, 0.5), (0.26, 0.74), (0.9, 0.1), (0.51, 0.03)]:
        for dd in [(0, 0, 1), (nz, 0, 1), (0, nz, 1), (0.3, 0, 1), (0, 0.2, 1), (nz, -0.3, 1), (-0.2, nz, 1)]:
            rows.append(np.array(dd, np.float32))
            o.append(np.array((ox, oy, -1.0), np.float32))
    for dd in [(1, 0, 0), (-1, 0, nz), (0, 1, 0), (0, -1, 0), (nz, nz, -1), (1, 0, 0.25), (0, -1, 0.5)]:  # from inside
        rows.append(np.array(dd, np.float32))
        o.append(np.array((0.5, 0.9, 0.5), np.float32))
    dirs, o = np.array(rows, np.float32), np.array(o, np.float32)
    tmax = np.full(len(dirs), 1e34, np.float32)
    # the city's grid is generated on the device; the restated DDA walks the same world as dense bytes
    world = [dataclasses.replace(g, dense=pkg.scene._tiled_numpy(g).reshape(-1)) if g.dense is None else g for g in desc.grids]
    vols = vols_of(replace(desc, grids=world))
    res = [plain_walk(vols, o[j], dirs[j], tmax[j]) for j in range(len(dirs))]
    walked = np.array([r[2] > 0 for r in res])
    assert sum(r[1] is not None for r in res) >= 20
    assert int((walked & (dirs == 0).any(axis=1)).sum()) >= 20  # infinite tdeltas that do walk
    with pkg.context.Context(0) as ctx:
        ctx.load_scene(desc)
        compare_with_plain(pkg, ctx, o, dirs, tmax, res, 0, NO_RANGE, "axis rays")
