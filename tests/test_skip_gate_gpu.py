"""The walkers' maturity gate and lean skips (csrc/vpx_trace.hpp walk_wave, the walk kinds' gate
fields in csrc/vpx_walk_kinds.hpp), on the GPU.

A 128^3 town (ground, blocks of different heights between streets, thin walls) under a point and a
directional light, seen from outside the grid in 64x64 and 128x96 pixels at depth 0, once at depth 2
(the bounce walks), and once from inside the grid, where the primary rays start at t = 0 like the
shadow and bounce rays.  Each is rendered as serial frames, with 3 lanes in flight and as one
render_window, in exact and in reference (x86) arithmetic, and equals the oracle bit for bit:
accumulator floats, RGB8, and the primary / shadow / bounce ray and DDA-cell counts.
"""
import numpy as np
import pytest

from cases import bits
from test_axis_boxes import X86, _torch, check, oracle_frames

pytestmark = pytest.mark.gpu

N = 128
FRAMES = 2
OUTSIDE = ((1.1, 1.25, -0.3), (0.45, 0.1, 0.5))
INSIDE = ((0.27, 0.6, 0.04), (0.4, 0.0, 0.6))  # above a street, below the highest roofs


def town_grid(n=N):
    """Index x + y*n + z*n*n.  Streets 6 cells wide every 32 cells, blocks of seeded heights."""
    g = np.full((n, n, n), 255, np.uint8)  # [z, y, x]
    g[:, 0, :] = 1
    rng = np.random.default_rng(5)
    for bz in range(4):
        for bx in range(4):
            h = int(rng.integers(4, 70))
            g[bz * 32 + 6:(bz + 1) * 32, 1:h, bx * 32 + 6:(bx + 1) * 32] = 5 if (bx + bz) % 3 == 0 else 2  # some metal
    g[40:70, 1:30, 3] = 7       # a thin wall along a street
    g[100, 1:50, 32:38] = 7      # one across a street
    return g


def town_scene(pkg, w, h, depth, cam):
    sc, abi = pkg.scene, pkg.abi
    desc = sc._scene("town128", [sc.GridSpec(n=N, dense=town_grid().reshape(-1).copy())], [sc.volume()],
                     sc.default_materials(), [sc.point_light((0.5, 1.5, 0.5), (1.0, 1.0, 1.0))], [], [],
                     sc.dir_light((-0.3, -1.0, -0.2), (1.0, 1.0, 1.0)), cam[0], cam[1], w, h, max_bounces=depth)
    desc.flags = abi.VPX_FLAG_AA
    return desc


def render(pkg, desc, how, mode):
    """FRAMES accumulated frames: 'serial', 'lanes' (3 in flight) or 'window' (one render_window)."""
    torch = _torch()
    ctx = pkg.context.Context(0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    ctx.load_scene(desc)
    ctx.set_arithmetic(mode)
    ctx.set_pipeline(3 if how == "lanes" else 0)
    W, H = desc.width, desc.height
    acc = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.counters(reset=True)
    with torch.cuda.stream(s):
        if how == "window":
            ctx.render_window(desc.frame_params(0), FRAMES, acc.data_ptr(), rgb.data_ptr())
        else:
            for f in range(FRAMES):
                ctx.render(desc.frame_params(f), acc.data_ptr(), rgb.data_ptr())
    ctx.synchronize()
    st = ctx.counters()
    out = (bits(acc.cpu().numpy().reshape(-1, 4)), rgb.cpu().numpy().view(np.uint32),
           tuple(int(getattr(st, k)) for k in ("primary_rays", "shadow_rays", "bounce_rays", "dda_cells")))
    ctx.close()
    return out


ARITH = ["exact", pytest.param("x86", marks=pytest.mark.skipif(not X86, reason="x86 intrinsics"))]


def run_case(pkg, orc, w, h, depth, cam, arith):
    _torch()
    abi = pkg.abi
    desc = town_scene(pkg, w, h, depth, cam)
    want = oracle_frames(orc, pkg, [desc] * FRAMES, x86=arith == "x86")
    primary, shadow, bounce, cells = want[2]
    assert primary > 0 and shadow > 0 and cells > 0 and (depth == 0 or bounce > 0), want[2]
    mode = abi.VPX_ARITH_X86_HOST if arith == "x86" else abi.VPX_ARITH_EXACT
    for how in ("serial", "lanes", "window"):
        check(render(pkg, desc, how, mode), want, f"{w}x{h} depth {depth}, {arith}, {how}")


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("size", [(64, 64), (128, 96)])
def test_town_depth0_bit_exact(pkg, orc, size, arith):
    run_case(pkg, orc, size[0], size[1], 0, OUTSIDE, arith)


@pytest.mark.parametrize("arith", ARITH)
def test_town_bounces_bit_exact(pkg, orc, arith):
    run_case(pkg, orc, 64, 64, 2, OUTSIDE, arith)


@pytest.mark.parametrize("arith", ARITH)
def test_camera_inside_the_grid(pkg, orc, arith):
    run_case(pkg, orc, 64, 64, 0, INSIDE, arith)
