"""The depth-0 frame kernel's compile-time views (csrc/vpx_wavefront.hpp: frame0_scene / frame0_args,
chosen in launch_render), on the GPU.

The kernel is built in two forms: one with the facts every launch of it guarantees folded in as
constants (one volume, no shapes, depth 0, one shadow slot per path), and a lean one that also has
no spot or area lights, a constant sky and no thin lens.  vpx_debug_last_frame_kernel says which
form the last render launched (1, 2; 0: the frame did not run as one launch).

The 128^3 monu3 city at 64x48 and at 70x50 (partial tiles), two accumulated AA frames, against the
oracle bit for bit: accumulator floats, RGB8 and the primary / shadow / bounce ray and DDA-cell
counts.  The lean-eligible scene (point + directional light, constant sky) in both arithmetic modes,
serial, with three lanes (packed samples + composite) and as rank 0 of 2's packed accumulator; a
spot light, one area light with one sample, the sky texture and the thin lens each keep the kernel
but not the lean form; one context whose lights alternate between the two from frame to frame;
a depth-2 frame and a two-volume frame launch neither.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from cases import bits
from test_axis_boxes import X86, _torch, check, oracle_frames

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (70, 50)]
FRAMES = 2
ARITH = ["exact", pytest.param("x86", marks=pytest.mark.skipif(not X86, reason="x86 intrinsics"))]
COUNTS = ("primary_rays", "shadow_rays", "bounce_rays", "dda_cells")


def city(pkg, size, depth=0):
    desc = pkg.scene.city_scene("monu3", 128, size[0], size[1], depth)
    desc.flags = pkg.abi.VPX_FLAG_AA
    return desc


def replace(desc, **kw):
    d = dataclasses.replace(desc, **kw)
    d._cam_pos, d._cam_target = desc._cam_pos, desc._cam_target
    return d


def variant(pkg, size, kind):
    """The city with one thing the lean form excludes (or 'lean': nothing)."""
    _torch()
    sc, abi = pkg.scene, pkg.abi
    desc = city(pkg, size)
    if kind == "spot":
        return replace(desc, spots=[sc.spot_light((0.5, 1.2, 0.2), (0.0, -1.0, 0.3), (2.0, 1.8, 1.5))])
    if kind == "area1":
        return replace(desc, areas=[sc.area_light((0.5, 2.0, 0.5))], area_samples=1)
    if kind == "sky":
        return sc.with_sky(desc)
    if kind == "dof":
        ctx = pkg.context.Context(0)
        ctx.load_scene(desc)
        fd = ctx.focus_distance(desc.width, desc.height)
        ctx.close()
        cam = type(desc.camera).from_buffer_copy(desc.camera)
        cam.focal_distance = fd
        return replace(desc, camera=cam, flags=desc.flags | abi.VPX_FLAG_DOF)
    assert kind == "lean"
    return desc


_WANT = {}


def want_of(pkg, orc, key, descs, x86=False):
    """The oracle's frames (one accumulated frame per description), computed once per key."""
    if key not in _WANT:
        _WANT[key] = oracle_frames(orc, pkg, descs, x86=x86)
        primary, shadow, _, cells = _WANT[key][2]
        assert primary > 0 and shadow > 0 and cells > 0, _WANT[key][2]
    return _WANT[key]


def open_ctx(pkg, desc, arith="exact", lanes=0):
    torch = _torch()
    abi = pkg.abi
    ctx = pkg.context.Context(0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    ctx.load_scene(desc)
    ctx.set_arithmetic(abi.VPX_ARITH_X86_HOST if arith == "x86" else abi.VPX_ARITH_EXACT)
    ctx.set_pipeline(lanes)
    return ctx, s


def set_lights(pkg, ctx, desc):
    """The description's lights on a context that already holds its grids (vpx_set_lights, which
    waits for the frames in flight)."""
    abi = pkg.abi
    pts = (abi.PointLight * max(1, len(desc.points)))(*desc.points)
    sps = (abi.SpotLight * max(1, len(desc.spots)))(*desc.spots)
    ars = (abi.AreaLight * max(1, len(desc.areas)))(*desc.areas)
    ctx._chk(ctx.lib.vpx_set_lights(ctx.h, pts, len(desc.points), sps, len(desc.spots), ars, len(desc.areas),
                                    C.byref(desc.dir_light)), "vpx_set_lights")


def render_frames(pkg, descs, arith, lanes):
    """One accumulated frame per description on one context (the first one's grids and camera; the
    lights follow the descriptions): the result like test_axis_boxes.render, and the form each
    frame launched."""
    torch = _torch()
    ctx, s = open_ctx(pkg, descs[0], arith, lanes)
    W, H = descs[0].width, descs[0].height
    acc = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.counters(reset=True)
    forms = []
    with torch.cuda.stream(s):
        for f, d in enumerate(descs):
            if f and d is not descs[f - 1]:
                set_lights(pkg, ctx, d)
            ctx.render(d.frame_params(f), acc.data_ptr(), rgb.data_ptr())
            forms.append(ctx.last_frame_kernel())
    ctx.synchronize()
    st = ctx.counters()
    out = (bits(acc.cpu().numpy().reshape(-1, 4)), rgb.cpu().numpy().view(np.uint32),
           tuple(int(getattr(st, k)) for k in COUNTS))
    ctx.close()
    return out, forms


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("how", ["serial", "lanes"])
@pytest.mark.parametrize("size", SIZES)
def test_lean_scene_frames(pkg, orc, size, how, arith):
    desc = variant(pkg, size, "lean")
    want = want_of(pkg, orc, ("lean", size, arith), [desc] * FRAMES, x86=arith == "x86")
    got, forms = render_frames(pkg, [desc] * FRAMES, arith, 3 if how == "lanes" else 0)
    assert forms == [2] * FRAMES
    check(got, want, f"lean {size}, {arith}, {how}")


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("size", SIZES)
def test_lean_scene_rank_share(pkg, orc, size, arith):
    """render_tiles_accum for rank 0 of 2: its packed running average and RGB8 are the oracle's at
    its tiles' pixels.  (Rank 1's follows only so that the two ranks' counts add up to the frame's.)"""
    torch = _torch()
    desc = variant(pkg, size, "lean")
    want = want_of(pkg, orc, ("lean", size, arith), [desc] * FRAMES, x86=arith == "x86")
    ctx, s = open_ctx(pkg, desc, arith)
    W, H = size
    R = 2
    L = ctx.packed_len(W, H, R)
    ctx.counters(reset=True)
    for rank in range(R):
        acc = torch.zeros(L * 4, dtype=torch.float32, device="cuda")
        rgb = torch.zeros(L, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for f in range(FRAMES):
                ctx.render_tiles_accum(desc.frame_params(f), rank, R, acc.data_ptr(), rgb.data_ptr())
                assert ctx.last_frame_kernel() == 2
        ctx.synchronize()
        if rank == 0:
            ids = pkg.dist.rank_pixel_ids(W, H, 0, R)
            ok = ids >= 0
            assert ok.sum() > 0
            assert np.array_equal(bits(acc.cpu().numpy().reshape(-1, 4))[ok], want[0][ids[ok]]), "packed accumulator"
            assert np.array_equal(rgb.cpu().numpy().view(np.uint32)[ok], want[1][ids[ok]]), "packed RGB8"
    st = ctx.counters()
    assert tuple(int(getattr(st, k)) for k in COUNTS) == want[2]
    ctx.close()


@pytest.mark.parametrize("kind", ["spot", "area1", "sky", "dof"])
@pytest.mark.parametrize("size", SIZES)
def test_guaranteed_form_scenes(pkg, orc, size, kind):
    """Scenes the kernel still takes, each with one thing the lean form has compiled out."""
    desc = variant(pkg, size, kind)
    want = want_of(pkg, orc, (kind, size, "exact"), [desc] * FRAMES)
    got, forms = render_frames(pkg, [desc] * FRAMES, "exact", 0)
    assert forms == [1] * FRAMES
    check(got, want, f"{kind} {size}")


@pytest.mark.parametrize("how", ["serial", "lanes"])
@pytest.mark.parametrize("size", SIZES)
def test_alternating_light_sets(pkg, orc, size, how):
    """One context, the lights changing before every frame: lean, spot, lean, spot.  The form
    follows the scene, and every frame alone (rendered into an accumulator of its own, so that no
    frame's error can hide in another's) equals the oracle's frame of that scene."""
    torch = _torch()
    lean, spot = variant(pkg, size, "lean"), variant(pkg, size, "spot")
    descs = [lean, spot, lean, spot]
    ctx, s = open_ctx(pkg, lean, "exact", 3 if how == "lanes" else 0)
    W, H = size
    accs = [torch.zeros(W * H * 4, dtype=torch.float32, device="cuda") for _ in descs]
    rgbs = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in descs]
    torch.cuda.synchronize()
    forms, counts = [], []
    for f, d in enumerate(descs):
        ctx.counters(reset=True)
        set_lights(pkg, ctx, d)
        with torch.cuda.stream(s):
            ctx.render(d.frame_params(0), accs[f].data_ptr(), rgbs[f].data_ptr())
        forms.append(ctx.last_frame_kernel())
        st = ctx.counters()
        counts.append(tuple(int(getattr(st, k)) for k in COUNTS))
    ctx.synchronize()
    assert forms == [2, 1, 2, 1]
    for f, d in enumerate(descs):
        kind = "lean" if d is lean else "spot"
        want = want_of(pkg, orc, (kind, size, "one frame"), [d])
        got = (bits(accs[f].cpu().numpy().reshape(-1, 4)), rgbs[f].cpu().numpy().view(np.uint32),
               counts[f])
        check(got, want, f"frame {f} ({kind}) {size}, {how}")
    ctx.close()


@pytest.mark.parametrize("kind", ["depth2", "two volumes"])
@pytest.mark.parametrize("size", SIZES)
def test_frames_the_kernel_does_not_take(pkg, orc, size, kind):
    sc = pkg.scene
    if kind == "depth2":
        desc = city(pkg, size, depth=2)
    else:
        base = city(pkg, size)
        vols = [sc.volume(), sc.volume(position=(0.2, 1.0, 0.2), scale=(0.3, 0.3, 0.3))]
        desc = replace(base, volumes=(pkg.abi.Volume * 2)(*vols))
    want = want_of(pkg, orc, (kind, size, "exact"), [desc] * FRAMES)
    got, forms = render_frames(pkg, [desc] * FRAMES, "exact", 0)
    assert forms == [0] * FRAMES
    check(got, want, f"{kind} {size}")
