"""The axis planes' widths (csrc/vpx_skip.hpp GridView::dfw), on the GPU.

A 64^3 street canyon (ground, two walls along z, a crossing street, a pillar) rendered 64x64 at
depth 0 and 2, serial and with frames in flight; the device's 32-bit plane words against the host
builder's (tests/native/wide_box_test.cpp); an edit that puts a block high above the street, far
to the side of the wide box of a brick near the ground, which must shrink that box's width and
nothing else of its word, with the frame after it; four instances of one canyon grid.  Every
frame equals the oracle bit for bit: accumulator floats, RGB8 and ray / cell counts.
"""
import subprocess

import numpy as np
import pytest

from test_axis_boxes import _torch, check, oracle_frames, render
from test_wide_boxes import build_wide_exe

N = 64


def canyon_grid(n=N):
    """Index x + y*n + z*n*n, as tests/native/wide_box_test.cpp's street canyon, scaled to n."""
    g = np.full((n, n, n), 255, np.uint8)  # [z, y, x]
    a, b, top = 26 * n // 64, 37 * n // 64, 41 * n // 64
    g[:, 0, :] = 1                       # ground
    for x in (a, b):                     # walls (metal: they bounce at depth 2), open at the crossing
        g[:, 1:top, x] = 5
        g[30 * n // 64:36 * n // 64, 1:top, x] = 255
    g[50 * n // 64, 1:20 * n // 64, 31 * n // 64] = 2  # pillar
    return g


# the edit: a 4^3 block (brick (8, 9, 6)) between the walls, 8 bricks above brick (7, 1, 4)
BLOCK_ORIGIN = (32, 36, 24)
BRICK = (7, 1, 4)


def edited_grid():
    g = canyon_grid()
    x, y, z = BLOCK_ORIGIN
    g[z:z + 4, y:y + 4, x:x + 4] = 1
    return g


def canyon_scene(pkg, depth, grid=None):
    sc, abi = pkg.scene, pkg.abi
    cells = canyon_grid() if grid is None else grid
    desc = sc._scene("canyon64", [sc.GridSpec(n=N, dense=cells.reshape(-1).copy())], [sc.volume()],
                     sc.default_materials(), [sc.point_light((0.5, 0.75, 0.45), (1.0, 1.0, 1.0))], [], [],
                     sc.dir_light(), (0.47, 0.1, 0.03), (0.52, 0.45, 0.6), 64, 64, max_bounces=depth)
    desc.flags = abi.VPX_FLAG_AA
    return desc


@pytest.fixture(scope="module")
def wide_exe(tmp_path_factory):
    return build_wide_exe(tmp_path_factory.mktemp("wide") / "wide_box_test")


def host_words(wide_exe, tmp_path, cells, n):
    src, dst = tmp_path / "cells.bin", tmp_path / "planes.bin"
    cells.reshape(-1).tofile(src)
    subprocess.run([wide_exe, "planes", str(src), str(n), str(dst)], check=True, timeout=60)
    return np.fromfile(dst, np.uint32).reshape(24, -1)


def blk_index(bx, by, bz, n):
    nb2 = ((n + 3) // 4 + 3) // 4
    return ((((bz >> 2) * nb2 + (by >> 2)) * nb2 + (bx >> 2)) << 6) | (bx & 3) | ((by & 3) << 2) | ((bz & 3) << 4)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, 2])
def test_canyon_frames_bit_exact(pkg, orc, depth):
    _torch()
    desc = canyon_scene(pkg, depth)
    frames = 2
    want = oracle_frames(orc, pkg, [desc] * frames)
    assert want[2][1] > 0 and want[2][3] > 0 and (depth == 0 or want[2][2] > 0)
    for lanes in (0, 2):
        check(render(pkg, desc, frames, lanes), want, f"depth {depth}, {lanes} lanes")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 37])
def test_device_words(pkg, wide_exe, tmp_path, n):
    _torch()
    if n == 64:
        cells = canyon_grid().reshape(-1)
    else:
        rng = np.random.default_rng(n)
        cells = np.where(rng.random(n ** 3) < 0.01, 3, 255).astype(np.uint8)
    host = host_words(wide_exe, tmp_path, cells, n)
    ctx = pkg.context.Context(0)
    pkg.scene.GridSpec(n=n, dense=cells).upload(ctx.lib, ctx.h, 0)
    dev = ctx.grid_wide_planes(0, n)
    low = ctx.grid_axis_planes(0, n)
    ctx.close()
    assert host.shape == dev.shape
    m = host >> 16
    assert ((m & 255) != (m >> 8)).any() and (m & 255).max() == 255 and (host == 0).any()
    bad = np.argwhere(host != dev)
    assert len(bad) == 0, (len(bad), bad[:5], host[host != dev][:5], dev[host != dev][:5])
    assert np.array_equal(low, (dev & 0xffff).astype(np.uint16))


@pytest.mark.gpu
def test_edit_beside_a_wide_box(pkg, orc, wide_exe, tmp_path):
    _torch()
    desc = canyon_scene(pkg, 0)
    block = np.full((4, 4, 4), 1, np.uint8)
    before, after = host_words(wide_exe, tmp_path, canyon_grid(), N), host_words(wide_exe, tmp_path, edited_grid(), N)
    # octant + + +, axis z: b = x, c = y.  The box of BRICK runs along the street, two bricks
    # wide (the wall), and up to the grid's top before the edit, up to the block after it.
    i = blk_index(*BRICK, N)
    w0, w1 = int(before[2, i]), int(after[2, i])
    assert w0 & 0xffffff == w1 & 0xffffff and w0 & 255 == 2 and (w0 >> 16) & 255 == 2
    assert w0 >> 24 == 255 and w1 >> 24 == 8
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    dev0 = ctx.grid_wide_planes(0, N)
    ctx.grid_write_box(0, block, BLOCK_ORIGIN)
    dev1 = ctx.grid_wide_planes(0, N)
    ctx.close()
    assert np.array_equal(dev0, before) and np.array_equal(dev1, after)
    want = oracle_frames(orc, pkg, [desc, canyon_scene(pkg, 0, edited_grid())])
    unedited = oracle_frames(orc, pkg, [desc, desc])
    assert not np.array_equal(want[1], unedited[1])  # the block is in view
    check(render(pkg, desc, 2, 0, None, (block, BLOCK_ORIGIN)), want, "after the edit")


@pytest.mark.gpu
def test_instances_of_a_canyon(pkg, orc):
    _torch()
    sc, abi = pkg.scene, pkg.abi
    desc = sc.model_scene("monu3", 64, 64, 64, 0, city_lights=True)
    desc.grids.append(sc.GridSpec(n=32, dense=canyon_grid(32).reshape(-1).copy()))
    rng = np.random.default_rng(23)
    vols = [sc.volume()]
    for k in range(4):
        pos = (0.45 * (k % 2) - 0.1, 0.55, 0.45 * (k // 2) - 0.1)
        vols.append(sc.volume(pos, tuple(rng.uniform(0.2, 0.3, 3)), tuple(rng.uniform(-2, 2, 3)), grid_id=1))
    desc.volumes = (abi.Volume * len(vols))(*vols)
    desc.flags = abi.VPX_FLAG_AA
    want = oracle_frames(orc, pkg, [desc])
    assert want[2][1] > 0 and want[2][3] > 0
    check(render(pkg, desc, 1), want, "four instances of one 32^3 canyon")
