"""The walkers' plain-step prefix (csrc/vpx_walk_kinds.hpp, the walk kinds' pre; csrc/vpx_skip.hpp
skip_box_lean's PRE), on the GPU, with the library as shipped.

The 128^3 town of test_skip_gate_gpu.py under a point and a directional light: 64x64 and 128x96 at
depth 0 from outside the grid (k_frame0: primary and compacted shadow walks), 64x64 from a camera
inside the grid (primary rays that start at t = 0, every axis immature), 64x64 at depth 2 (the
bounce pool, the tile / list shadow walkers) and 64x64 with one sphere area light of 3 samples (the
shadow pool).  Each is rendered as serial frames, with 3 lanes in flight and as one render_window,
in exact and in reference (x86) arithmetic, and equals the oracle bit for bit: accumulator floats,
RGB8, and the primary / shadow / bounce ray and DDA-cell counts.
"""
import pytest

from test_axis_boxes import _torch, check, oracle_frames
from test_skip_gate_gpu import ARITH, FRAMES, INSIDE, OUTSIDE, render, run_case, town_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("size", [(64, 64), (128, 96)])
def test_prefix_town_depth0_bit_exact(pkg, orc, size, arith):
    run_case(pkg, orc, size[0], size[1], 0, OUTSIDE, arith)


@pytest.mark.parametrize("arith", ARITH)
def test_prefix_camera_inside_the_grid(pkg, orc, arith):
    run_case(pkg, orc, 64, 64, 0, INSIDE, arith)


@pytest.mark.parametrize("arith", ARITH)
def test_prefix_town_bounces_bit_exact(pkg, orc, arith):
    run_case(pkg, orc, 64, 64, 2, OUTSIDE, arith)


@pytest.mark.parametrize("arith", ARITH)
def test_prefix_area_light_shadow_pool(pkg, orc, arith):
    _torch()
    abi, sc = pkg.abi, pkg.scene
    plain = town_scene(pkg, 64, 64, 0, OUTSIDE)
    desc = town_scene(pkg, 64, 64, 0, OUTSIDE)
    desc.areas = [sc.area_light((0.5, 1.6, 0.4), radius=0.3)]
    assert desc.area_samples == 3
    without = oracle_frames(orc, pkg, [plain] * FRAMES, x86=arith == "x86")[2]
    want = oracle_frames(orc, pkg, [desc] * FRAMES, x86=arith == "x86")
    primary, shadow, _, cells = want[2]
    # the area light's samples come on top of the point and the directional light's rays
    assert primary > 0 and shadow > without[1] > 0 and cells > without[3], (want[2], without)
    mode = abi.VPX_ARITH_X86_HOST if arith == "x86" else abi.VPX_ARITH_EXACT
    for how in ("serial", "lanes", "window"):
        check(render(pkg, desc, how, mode), want, f"64x64 area light, {arith}, {how}")
