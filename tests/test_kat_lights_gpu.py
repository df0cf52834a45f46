"""Spot lights, area lights and the light pick on the device against the numpy Trace — no oracle here.

The device holds Illumination twice: illumination() in csrc/vpx_trace.hpp serves the per-ray entries,
emit_illumination + resolve_path_by in csrc/vpx_wavefront.hpp the frame kernels, where the pick, the
slot mask, the sample count, the level and lightCount travel in bit fields and the shadow lists are
bucketed by the light index modulo 16.  Both are held to tests/test_kat_paths.Scene.illumination,
bit for bit (a NaN's sign and payload apart), in exact arithmetic (VPX_ARITH_EXACT):

  vpx_trace        every run of tests/test_kat_lights.py (four light sets, 0 / 1 / 3 / 15 samples, a second
                   volume, depth 1 over SEEDS and 2 / 3 / 5 over SEEDS[:8]), the spot edges, the sphere
                   between an area light and the floor, and vpx_trace_probe on the smoke probe that
                   draws an area light; the light at the hit point (dst = 0) stays on the CPU
  whole frames     test_kat_frame's "mixed lights" scene (19x13, AA + DOF, three accumulated frames) at
                   depth 0 and 2 through vpx_render serial and with 2 lanes, vpx_render_window and
                   vpx_render_tiles_accum for 2 ranks; one frame with the wide set and 15 samples at
                   depth 2 (every slot bit, indices that share a bucket)
Which kernels ran is read from vpx_debug_last_frame_kernel and vpx_profile_read on the serial context.
With an area light and more than one sample a depth-0 frame has several shadow slots per path and
launch_render splits it (k_primary, the shadow pool, k_resolve_finish); the one-launch k_frame0 takes
the mixed set with one sample, which has its own case.  The serial frames' shadow-ray and DDA-cell
counters (vpx_get_counters, which counts render calls; vpx_trace keeps no counters) equal the restatement's.
"""
import numpy as np
import pytest

import epilogue_ref as E
import test_kat_frame as K
import test_kat_lights as L
import test_kat_shapes as S
import test_player_light as P
from test_kat_frame_gpu import _torch, cached, dev, expect, host, open_ctx
from test_kat_paths import DEPTHS, SEEDS, api_rays

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning",
                                                          "ignore:invalid value:RuntimeWarning")]

AA, DOF, SKY = K.AA, K.DOF, K.SKY
W, H = K.FRAME_W, K.FRAME_H
PIX = W * H


def trace_ctx(pkg, desc):
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    ctx.set_arithmetic(pkg.abi.VPX_ARITH_EXACT)
    return ctx


# ------------------------------------------------------------------------ vpx_trace
@pytest.mark.parametrize("cfg", L.SHALLOW, ids=[L.run_id((c, 1))[:-3] for c in L.SHALLOW])
def test_trace_equals_restatement(pkg, cfg):
    """One light set, sample count and volume list: the three rays x the seeds in one vpx_trace call
    per depth (1, then 2, 3, 5)."""
    _torch()
    name, samples, second = cfg
    desc, _ = L.build(pkg, L.LIGHT_SETS[name], second)
    ctx = trace_ctx(pkg, desc)
    got = {}
    for depth in (1,) + DEPTHS:
        rays, seeds = L.batch(pkg.abi, list(L.RAYS.values()), L.seeds_of(depth))
        got[depth] = ctx.trace(rays, seeds, depth, SKY, samples).copy()
    ctx.close()
    for depth, g in got.items():
        e = cached(("lights", cfg, depth), lambda: L.expected(cfg, depth))
        L.same_radiance(g, e["rad"], L.run_id((cfg, depth)))


def test_spot_edges(pkg):
    """cos == angle (at 1 and in general position), one ulp to either side, alpha == 1 and the spot on
    the far side of the floor: test_kat_lights.edge_sets, every set through vpx_trace on one context."""
    _torch()
    ctx = None
    got = {}
    for name in L.EDGE_NAMES:
        desc, _ = L.build(pkg, L.edge_sets()[name][0])
        if ctx is None:
            ctx = trace_ctx(pkg, desc)
        else:
            ctx.load_scene(desc, upload_grids=False)
        rays, seeds = L.batch(pkg.abi, [L.RAYS["default"]], SEEDS)
        got[name] = ctx.trace(rays, seeds, 1, SKY, 3).copy()
    ctx.close()
    for name, g in got.items():
        L.same_radiance(g, L.edge_expected(name)["rad"], name)


@pytest.mark.parametrize("depth", S.DEPTHS)
def test_sphere_between_an_area_light_and_the_floor(pkg, depth):
    """test_kat_shapes' case: IsOccluded's shape stage on an area light's 15 shadow rays."""
    _torch()
    e = S.light_path_expect(depth)
    o, d, inside = S.FLOOR_RAY
    ctx = trace_ctx(pkg, S.light_path_desc(pkg))
    got = ctx.trace(api_rays(pkg.abi, [(o, d, 1e34, inside)] * len(SEEDS)), np.array(SEEDS, np.uint32), depth, SKY,
                    S.LIGHT_SAMPLES).copy()
    ctx.close()
    L.same_radiance(got, e["rad"], f"sphere and area light, depth {depth}")


def test_probe_draws_area_lights(pkg):
    """vpx_trace_probe with the mixed set: per ray the probes, the lit count and the bits of max_sqr,
    and the radiance of the path that goes on after the probe's draws, at depth 0, 1 and 3."""
    _torch()
    from test_kat_paths import N, Vol, to_oracle

    cells, mats, points, d, kw = P.probe_lights(P.MIXED)
    ctx = trace_ctx(pkg, to_oracle(pkg, None, cells, mats, points, d, [Vol(cells, N)], **kw))
    rr = P.probe_rays()
    rays = api_rays(pkg.abi, [(o, dd, 1e34, inside) for o, dd, inside, _ in rr])
    seeds = np.array([s for *_, s in rr], np.uint32)
    got = {depth: ctx.trace_probe(rays, seeds, depth, SKY, 3) for depth in P.DEPTHS}
    ctx.close()
    for depth, (rad, pr) in got.items():
        want = P.reference(P.MIXED, depth)
        rows = np.stack([pr["probes"].astype(np.uint64), pr["lit"].astype(np.uint64),
                         pr["max_sqr"].view(np.uint32).astype(np.uint64)], axis=1)
        assert np.array_equal(rows, want), (depth, np.argwhere(rows != want)[:4])
        L.same_radiance(rad, P.reference_paths(P.MIXED, depth)[0], f"probe paths, depth {depth}")


# --------------------------------------------------------------------- whole frames
# (scene, depth) -> (vpx_debug_last_frame_kernel, stages that must launch, stages that must not)
FORMS = {
    ("mixed lights, 1 sample", 0): (1, ("frame",), ("primary", "shadow", "finish")),    # k_frame0, the guaranteed view
    ("mixed lights", 0): (0, ("primary", "shadow", "finish"), ("frame",)),             # 3 slots: the pool, k_resolve_finish
    ("mixed lights", 2): (0, ("primary", "shadow", "bounce"), ("frame",)),
    ("wide lights", 2): (0, ("primary", "shadow", "bounce"), ("frame",)),
}


def frames_of(pkg, abi, which, depth):
    n = 1 if which == "wide lights" else 3
    desc, cam, frames, refused = K.expected_frames(pkg, abi, which, depth, frames=n)
    assert len(refused) == 0 and len(frames) == n, refused
    params = [K.frame_params(abi, W, H, f, 0, AA | DOF, 1.0, depth, K.frame_samples(which)) for f in range(n)]
    return desc, cam, frames, params


@pytest.mark.parametrize("which,depth", list(FORMS), ids=[f"{w}-d{d}" for w, d in FORMS])
def test_serial_frames(pkg, abi, which, depth):
    """vpx_render on the serial context: accumulator and RGB8 after every frame, the kernels that ran,
    and the frame's shadow-ray and DDA-cell counters."""
    torch = _torch()
    desc, cam, frames, params = frames_of(pkg, abi, which, depth)
    form, ran, idle = FORMS[(which, depth)]
    ctx = open_ctx(pkg, desc, cam)
    ctx.profile_enable(4096)
    d_acc, d_rgb = dev(np.zeros(PIX * 4, np.uint32)), dev(np.zeros(PIX, np.uint32))
    torch.cuda.synchronize()
    got = []
    for p in params:
        ctx.profile_read(reset=True)
        ctx.counters(reset=True)
        ctx.render(p, d_acc.data_ptr(), d_rgb.data_ptr())
        ctx.synchronize()
        st = ctx.counters()
        launches = {k: v[1] for k, v in ctx.profile_read(reset=True).items()}
        got.append((host(d_acc).reshape(-1, 4), host(d_rgb), ctx.last_frame_kernel(), launches, (st.shadow_rays, st.dda_cells)))
    ctx.close()
    for f, ((acc, rgb, kernel, launches, counts), (want_acc, want_rgb, shadows, cells, _)) in enumerate(zip(got, frames)):
        what = f"{which} depth {depth} frame {f}"
        print(what, "frame kernel", kernel, "stage launches", launches, "counts", counts, (shadows, cells))
        assert kernel == form, (what, kernel)
        assert all(launches[s] > 0 for s in ran) and all(launches[s] == 0 for s in idle), (what, launches)
        expect(acc, rgb, want_acc, want_rgb, what)
        assert counts == (shadows, cells), (what, counts, (shadows, cells))


@pytest.mark.parametrize("depth", [0, 2])
def test_frames_in_flight(pkg, abi, depth):
    """vpx_render with 2 lanes, after every frame."""
    torch = _torch()
    desc, cam, frames, params = frames_of(pkg, abi, "mixed lights", depth)
    ctx = open_ctx(pkg, desc, cam, lanes=2)
    d_acc, d_rgb = dev(np.zeros(PIX * 4, np.uint32)), dev(np.zeros(PIX, np.uint32))
    torch.cuda.synchronize()
    got = []
    for p in params:
        ctx.render(p, d_acc.data_ptr(), d_rgb.data_ptr())
        ctx.synchronize()
        got.append((host(d_acc).reshape(-1, 4), host(d_rgb)))
    ctx.close()
    for f, ((acc, rgb), (want_acc, want_rgb, *_)) in enumerate(zip(got, frames)):
        expect(acc, rgb, want_acc, want_rgb, f"2 lanes, depth {depth}, frame {f}")


@pytest.mark.parametrize("depth", [0, 2])
def test_window_of_three_frames(pkg, abi, depth):
    """vpx_render_window: the three frames in one chain, blended in frame order."""
    torch = _torch()
    desc, cam, frames, params = frames_of(pkg, abi, "mixed lights", depth)
    ctx = open_ctx(pkg, desc, cam)
    d_acc, d_rgb = dev(np.zeros(PIX * 4, np.uint32)), dev(np.zeros(PIX, np.uint32))
    torch.cuda.synchronize()
    ctx.render_window(params[0], 3, d_acc.data_ptr(), d_rgb.data_ptr())
    ctx.synchronize()
    acc, rgb = host(d_acc), host(d_rgb)
    ctx.close()
    expect(acc, rgb, frames[2][0], frames[2][1], f"window, depth {depth}")


@pytest.mark.parametrize("depth", [0, 2])
def test_tiles_accum_for_two_ranks(pkg, abi, depth):
    """vpx_render_tiles_accum, both ranks of 2, into the rank's packed accumulator; after every frame
    the slots (epilogue_ref.slot_pixels) hold the restatement's pixels and the padding 0 / 0."""
    torch = _torch()
    R = 2
    desc, cam, frames, params = frames_of(pkg, abi, "mixed lights", depth)
    length, slots = E.slot_pixels(W, H, R)
    ok = slots >= 0
    assert sorted(slots[ok].tolist()) == list(range(PIX))
    ctx = open_ctx(pkg, desc, cam)
    bufs = [(dev(np.zeros(length * 4, np.uint32)), dev(np.full(length, 0xDEADBEEF, np.uint32))) for _ in range(R)]
    torch.cuda.synchronize()
    got = []
    for p in params:
        for rank, (d_acc, d_rgb) in enumerate(bufs):
            ctx.render_tiles_accum(p, rank, R, d_acc.data_ptr(), d_rgb.data_ptr())
        ctx.synchronize()
        got.append((np.concatenate([host(a).reshape(-1, 4) for a, _ in bufs]), np.concatenate([host(r) for _, r in bufs])))
    ctx.close()
    for f, ((acc, rgb), (want_acc, want_rgb, *_)) in enumerate(zip(got, frames)):
        wa, wr = np.zeros_like(acc), np.zeros(len(slots), np.uint32)
        wa[ok], wr[ok] = want_acc[slots[ok]], want_rgb[slots[ok]]
        expect(acc, rgb, wa, wr, f"tiles_accum R=2, depth {depth}, frame {f}")
