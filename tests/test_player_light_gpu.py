"""The player light probe on the device (Renderer::inLight, renderer.h:231): the unit entry
against the numpy restatement (A), the four light evaluators against oracle pieces in a scene
where only volume 0 is the player (B), and every frame entry point against the unit entry (C).
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

from cases import bits  # noqa: E402
from test_kat_paths import N, Vol, api_rays, to_oracle  # noqa: E402
from test_player_light import (COLOURS, DEPTHS, SEEDS, player_case, player_scene, probe_rays, probe_scene,  # noqa: E402
                               reference)

pytestmark = pytest.mark.gpu
X86 = os.uname().machine in ("x86_64", "i686")  # hosts that have VPX_ARITH_X86_HOST (tests/test_x86_arith.py)
SKY = (0.392, 0.584, 0.829)


def kat_desc(pkg, c, width=16, height=16, max_bounces=0):
    cells, mats, points, d = probe_scene(c)
    desc = to_oracle(pkg, None, cells, mats, points, d, [Vol(cells, N)])
    if (width, height) != (16, 16):
        desc = desc.with_size(width, height)
    desc.max_bounces = max_bounces
    return desc


def probe_rows(pr):
    """(probes, lit, bits of max_sqr) per ray of a trace_probe record array."""
    return np.stack([pr["probes"].astype(np.uint64), pr["lit"].astype(np.uint64),
                     pr["max_sqr"].view(np.uint32).astype(np.uint64)], axis=1)


# ------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("c", COLOURS)
def test_trace_probe_equals_numpy_restatement(pkg, c):
    """vpx_trace_probe (trace_probe_k) on the two smoke rays x 24 seeds at depths 0, 1, 3: per
    ray, probes, lit and the bits of max_sqr equal the numpy restatement's, and the radiance
    equals vpx_trace's bit for bit (with and without a radiance buffer)."""
    desc = kat_desc(pkg, c)
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    rr = probe_rays()
    rays = api_rays(pkg.abi, [(o, d, 1e34, inside) for o, d, inside, _ in rr])
    seeds = np.array([s for *_, s in rr], np.uint32)
    assert len(seeds) == 2 * len(SEEDS)
    try:
        for depth in DEPTHS:
            want = reference(c, depth)
            rad, pr = ctx.trace_probe(rays, seeds, depth, SKY, 3)
            got = probe_rows(pr)
            print(f"c={c} depth={depth}: probes {int(got[:, 0].sum())} lit {int(got[:, 1].sum())} "
                  f"max {pr['max_sqr'].max():.6f}; expected {int(want[:, 0].sum())} {int(want[:, 1].sum())}")
            assert int(want[:, 0].sum()) >= len(seeds)  # every ray probes at least once
            assert np.array_equal(got, want), (c, depth, np.argwhere(got != want)[:4])
            assert not pr["reserved"].any()
            assert np.array_equal(bits(rad), bits(ctx.trace(rays, seeds, depth, SKY, 3))), (c, depth)
            _, pr2 = ctx.trace_probe(rays, seeds, depth, SKY, 3, radiance=False)
            assert np.array_equal(probe_rows(pr2), want)
        assert ctx.player_light().probes == 0  # the unit entries do not add to the context's record
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ B
def test_four_evaluators_and_only_the_player(pkg, orc):
    """About 2 000 rays at depth 0 into the two-volume scene (the player model as volume 0, a
    room with its own smoke block as volume 1; point, spot, area x 3 samples and directional
    lights) through vpx_trace_probe: per ray the record equals the oracle pieces' (the hit from
    oracle_find_nearest, the evaluator Illumination draws from oracle_kat_light); rays that end
    in volume 1's smoke report no probe.  test_player_light.test_player_scene_conditions holds
    the conditions on the expected set (every evaluator, lit and unlit, the other smoke)."""
    desc, rays, seeds, e = player_case(pkg, orc)
    probes = e[e[:, 0] == 1]
    assert all(int((probes[:, 3] == k).sum()) >= 20 for k in range(4))
    assert int(probes[:, 1].sum()) >= 20 and int((probes[:, 1] == 0).sum()) >= 20
    other = (e[:, 5] == 1) & (e[:, 4] >= 9) & (e[:, 4] <= 14)
    assert int(other.sum()) >= 100
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    try:
        arr = api_rays(pkg.abi, [(o, d, 1e34, False) for o, d in rays])
        rad, pr = ctx.trace_probe(arr, seeds, 0, SKY, desc.area_samples)
        got = probe_rows(pr)
        print(f"probes {int(got[:, 0].sum())} lit {int(got[:, 1].sum())}; expected {int(e[:, 0].sum())} "
              f"{int(e[:, 1].sum())}")
        bad = np.argwhere((got != e[:, :3].astype(np.uint64)).any(axis=1)).reshape(-1)
        assert bad.size == 0, (bad[:5], got[bad[:5]], e[bad[:5]])
        assert not got[other].any()
        assert np.array_equal(bits(rad), bits(ctx.trace(arr, seeds, 0, SKY, desc.area_samples)))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ C
W, H = 72, 40  # 5 x 3 tiles, the right column and the bottom row partial


def primary_rays(pkg, desc, frame):
    """The frame's primary rays as the library states them (camera.h:71-73, no AA, no lens):
    P = (tl + (tr - tl) * u) + (bl - tl) * v with u = float(x) * (1 / W), the ray (camPos,
    P - camPos); and the pixels' seeds from vpx_pixel_seed."""
    f32 = np.float32
    cam = desc.camera
    tl, tr, bl, cp = (np.array(v[:], f32) for v in (cam.top_left, cam.top_right, cam.bottom_left, cam.cam_pos))
    x = np.tile(np.arange(W, dtype=f32), H)
    y = np.repeat(np.arange(H, dtype=f32), W)
    u = (x * (f32(1.0) / f32(W))).astype(f32)[:, None]
    v = (y * (f32(1.0) / f32(H))).astype(f32)[:, None]
    P = ((tl + ((tr - tl) * u).astype(f32)).astype(f32) + ((bl - tl) * v).astype(f32)).astype(f32)
    d = (P - cp).astype(f32)
    rays = pkg.context.make_rays(np.broadcast_to(cp, d.shape), d)
    lib = pkg.load_library()
    seeds = np.array([lib.vpx_pixel_seed(0, frame, W, H, int(i % W), int(i // W)) for i in range(W * H)], np.uint32)
    return rays, seeds


def record(pl):
    return (int(pl.probes), int(pl.lit), int(np.float32(pl.max_sqr).view(np.uint32)), int(pl.in_light))


def summed(rows):
    lit = int(rows[:, 1].sum())
    return (int(rows[:, 0].sum()), lit, int(rows[:, 2].max()), 1 if lit else 0)


def merged(recs):
    lit = sum(r[1] for r in recs)
    return (sum(r[0] for r in recs), lit, max(r[2] for r in recs), 1 if lit else 0)


ZERO = (0, 0, 0, 0)


class Frames:
    """A context on its own torch stream with an image accumulator and screen."""

    def __init__(self, pkg, desc, lanes=0, devices=None, arith=None):
        self.ctx = pkg.context.Context(0, devices=devices)
        self.s = torch.cuda.Stream()
        self.ctx.set_stream(self.s.cuda_stream)
        self.ctx.load_scene(desc)
        if arith is not None:
            self.ctx.set_arithmetic(arith)
        self.ctx.set_pipeline(lanes)
        self.acc = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        self.rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def image(self):
        self.ctx.synchronize()
        return bits(self.acc.cpu().numpy().reshape(-1, 4)), self.rgb.cpu().numpy().view(np.uint32).copy()

    def read(self):
        """The record read with reset, and the read after it (which must be zero)."""
        got = record(self.ctx.player_light(reset=True))
        assert record(self.ctx.player_light()) == ZERO
        return got

    def close(self):
        self.ctx.close()


def frame_paths(pkg, desc, expect, tag):
    """Every frame entry point's record against `expect` (per frame 0..2: the summed record of
    vpx_trace_probe over the frame's primary rays)."""
    ctx_never = Frames(pkg, desc)  # never asks for the record: its images after frame 0 and after frames 0..2
    with torch.cuda.stream(ctx_never.s):
        ctx_never.ctx.render(desc.frame_params(0), ctx_never.acc.data_ptr(), ctx_never.rgb.data_ptr())
    img_never = ctx_never.image()
    with torch.cuda.stream(ctx_never.s):
        for f in (1, 2):
            ctx_never.ctx.render(desc.frame_params(f), ctx_never.acc.data_ptr(), ctx_never.rgb.data_ptr())
    img_never3 = ctx_never.image()
    ctx_never.close()

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    fr = Frames(pkg, desc)  # vpx_render, serial
    with torch.cuda.stream(fr.s):
        fr.ctx.render(desc.frame_params(0), fr.acc.data_ptr(), fr.rgb.data_ptr())
    got = fr.read()
    print(tag, "serial", got, "expected", expect[0])
    assert got == expect[0], (tag, "serial")
    img = fr.image()
    assert same(img, img_never), (tag, "image")
    # vpx_get_counters' reset leaves the record, and the record's reset leaves the work counters
    with torch.cuda.stream(fr.s):
        fr.ctx.render(desc.frame_params(1), fr.acc.data_ptr(), fr.rgb.data_ptr())
    work = fr.ctx.counters(reset=True)
    assert work.primary_rays == 2 * W * H
    assert record(fr.ctx.player_light()) == expect[1], (tag, "after the counters' reset")
    with torch.cuda.stream(fr.s):
        fr.ctx.render(desc.frame_params(2), fr.acc.data_ptr(), fr.rgb.data_ptr())
    assert fr.read() == merged(expect[1:3]), (tag, "accumulates over calls")
    assert fr.ctx.counters().primary_rays == W * H
    assert same(fr.image(), img_never3), (tag, "image after three frames with reads between them")
    fr.close()

    fr = Frames(pkg, desc, lanes=3)  # three frames in flight
    with torch.cuda.stream(fr.s):
        for f in range(3):
            fr.ctx.render(desc.frame_params(f), fr.acc.data_ptr(), fr.rgb.data_ptr())
    got = fr.read()
    print(tag, "lanes", got, "expected", merged(expect))
    assert got == merged(expect), (tag, "3 lanes")
    assert same(fr.image(), img_never3), (tag, "lanes image")
    fr.close()

    fr = Frames(pkg, desc)  # vpx_render_window of 3 frames
    with torch.cuda.stream(fr.s):
        fr.ctx.render_window(desc.frame_params(0), 3, fr.acc.data_ptr(), fr.rgb.data_ptr())
    got = fr.read()
    print(tag, "window", got)
    assert got == merged(expect), (tag, "window")
    assert same(fr.image(), img_never3), (tag, "window image")
    fr.close()

    fr = Frames(pkg, desc)  # vpx_render_tiles_accum, ranks 0..2 of 3
    L = fr.ctx.packed_len(W, H, 3)
    recs = []
    for r in range(3):
        acc = torch.zeros(L * 4, dtype=torch.float32, device="cuda")
        rgb = torch.zeros(L, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(fr.s):
            fr.ctx.render_tiles_accum(desc.frame_params(0), r, 3, acc.data_ptr(), rgb.data_ptr())
        recs.append(fr.read())
    print(tag, "tiles", recs)
    assert merged(recs) == expect[0], (tag, "tiles of 3 ranks")
    fr.close()

    fr = Frames(pkg, desc, devices=[0, 0])  # a device set: the members' records summed
    with torch.cuda.stream(fr.s):
        fr.ctx.render(desc.frame_params(0), fr.acc.data_ptr(), fr.rgb.data_ptr())
    got = fr.read()
    print(tag, "device set", got)
    assert got == expect[0], (tag, "device set")
    fr.close()


def expected_frames(pkg, desc, depth):
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    out = []
    for f in range(3):
        rays, seeds = primary_rays(pkg, desc, f)
        _, pr = ctx.trace_probe(rays, seeds, depth, SKY, desc.area_samples, radiance=False)
        out.append(summed(probe_rows(pr)))
    ctx.close()
    return out


@pytest.mark.skipif(not X86, reason="VPX_ARITH_X86_HOST needs an x86 host")
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("depth", [0, 2, 5])
def test_x86_arithmetic_paths_agree(pkg, two, depth):
    """VPX_ARITH_X86_HOST (the reference-arithmetic instances of the kernels): the records of three
    serial frames, three frames in flight and a window of three agree, and hold probes.  Any
    error of vpx_set_arithmetic on an x86 host fails the test."""
    desc = player_scene(pkg, W, H, depth) if two else kat_desc(pkg, 4.5, W, H, depth)
    mode = pkg.abi.VPX_ARITH_X86_HOST
    got = {}
    for name, lanes, window in (("serial", 0, False), ("lanes", 3, False), ("window", 0, True)):
        fr = Frames(pkg, desc, lanes=lanes, arith=mode)
        try:
            with torch.cuda.stream(fr.s):
                if window:
                    fr.ctx.render_window(desc.frame_params(0), 3, fr.acc.data_ptr(), fr.rgb.data_ptr())
                else:
                    for f in range(3):
                        fr.ctx.render(desc.frame_params(f), fr.acc.data_ptr(), fr.rgb.data_ptr())
            got[name] = fr.read()
        finally:
            fr.close()
    print("x86", two, depth, got)
    assert got["serial"] == got["lanes"] == got["window"] and got["serial"][0] > 0, got


@pytest.mark.parametrize("depth", [0, 2, 5])
def test_frame_paths_single_volume(pkg, depth):
    """kat_scene(0) with the point light at c = 4.5 as a 72 x 40 single-volume frame (15 tiles,
    partial ones on two edges; one shadow slot per path).  Kernels that resolve the probe here:
    depth 0 — k_frame0 (serial, lanes as packed samples, tiles as the packed accumulator, the
    device set) and, for the window chain, k_primary's fused head with k_shadow_finish<true>;
    depth 2 and 5 — k_resolve on the levels before the last and k_shadow_finish<true> on the
    last (serial, tiles, window, device set), and with lanes k_shadow_pool -> k_resolve, then
    k_resolve_finish on the last level.  Not reached at these sizes: k_tail (max_bounces >= 8,
    see test_frame_paths_deep_tail) and k_finish_window<true> (window chains of frames of at
    least 16384 tiles with area lights: test_window_fused_tail_big_frames)."""
    desc = kat_desc(pkg, 4.5, W, H, depth)
    expect = expected_frames(pkg, desc, depth)
    print("expected per frame", expect)
    assert all(e[0] > 0 for e in expect) and merged(expect)[1] > 0 and merged(expect)[1] < merged(expect)[0]
    frame_paths(pkg, desc, expect, f"one volume, depth {depth}")


@pytest.mark.parametrize("depth", [0, 2, 5])
def test_frame_paths_two_volumes(pkg, depth):
    """The scene of test B as a 72 x 40 frame: two volumes (the multi-volume instances), area
    light samples (3 shadow slots per path, so the shadow pool everywhere).  Kernels that resolve
    the probe: depth 0 — k_primary<DEFER> / k_instances_list shade, k_shadow_pool<true> +
    k_shadow_slots, then k_resolve_finish; depth 2 and 5 — k_primary + k_instances, k_shade, the
    pool and k_resolve per level, k_resolve_finish on the last; the window chain ends in
    blend_window after k_resolve_finish's packed samples.  Volume 1's smoke must add nothing."""
    desc = player_scene(pkg, W, H, depth)
    expect = expected_frames(pkg, desc, depth)
    print("expected per frame", expect)
    assert all(e[0] > 0 for e in expect) and merged(expect)[1] > 0 and merged(expect)[1] < merged(expect)[0]
    frame_paths(pkg, desc, expect, f"two volumes, depth {depth}")


@pytest.mark.parametrize("two", [False, True])
def test_reproject_reports(pkg, two):
    """vpx_render_reproject at max_bounces 0 (Renderer::Tick's static branch, whose TraceSmoke
    makes the same probe, renderer.cpp:1438-1450): k_primary, k_shadow_tile and k_resolve (the
    reprojection keeps the tile kernels' SD flags), through Renderer.Tick with trackPlayerLight."""
    desc = player_scene(pkg, W, H, 0) if two else kat_desc(pkg, 4.5, W, H, 0)
    expect = expected_frames(pkg, desc, 0)[0]
    assert expect[0] > 0
    r = pkg.renderer.Renderer(desc, 0).Init()
    r.staticCamera = True
    r.Tick(0.0)
    assert r.inLight is False and r.last_player_light is None  # not tracked: no read, no synchronisation
    got = record(r.ctx.player_light(reset=True))
    print("reproject", got, "expected", expect)
    assert got == expect
    r.ResetAccumulator()
    r.trackPlayerLight = True
    r.Tick(0.0)
    assert record(r.last_player_light) == expect and r.inLight == bool(expect[3])
    assert record(r.ctx.player_light()) == ZERO  # Tick read and cleared it (renderer.cpp:2206)
    r.staticCamera = False
    r.ResetAccumulator()
    r.Tick(0.0)  # the moving-camera branch: vpx_render
    assert record(r.last_player_light) == expect and r.inLight == bool(expect[3])
    r.ctx.close()


def test_frame_paths_deep_tail(pkg):
    """max_bounces 8 on the single-volume frame, so the deep levels run in k_tail (serial: from
    level 6; frames in flight: from level 7), whose per-lane loop resolves in divergent code."""
    desc = kat_desc(pkg, 4.5, W, H, 8)
    expect = expected_frames(pkg, desc, 8)
    deeper = expected_frames(pkg, kat_desc(pkg, 4.5, W, H, 5), 5)
    print("expected per frame", expect, "at depth 5", deeper)
    assert merged(expect)[0] > merged(deeper)[0]  # probes beyond level 5 exist
    for lanes in (0, 3):
        fr = Frames(pkg, desc, lanes=lanes)
        with torch.cuda.stream(fr.s):
            for f in range(3):
                fr.ctx.render(desc.frame_params(f), fr.acc.data_ptr(), fr.rgb.data_ptr())
        got = fr.read()
        print("deep", lanes, got)
        assert got == merged(expect), lanes
        fr.close()


def demo_player_scene(pkg, n, w, h, depth):
    """host/vpx_demo's world in its 'p' mode: the pillars, a block of player smoke (cells x in
    [3n/4, 7n/8), y in [2, 2 + n/4), z in [n/4, 3n/8)) with albedo (0.8, 0.75, 0.7), and the point
    light at colour 8."""
    sc = pkg.scene
    desc = sc.pillars_scene(n, w, h, depth)
    g = desc.grids[0].dense.reshape(n, n, n).copy()  # [z][y][x]
    g[n // 4:3 * n // 8, 2:2 + n // 4, 3 * n // 4:7 * n // 8] = 14
    desc.grids[0] = sc.GridSpec(n=n, dense=g.reshape(-1))
    m = desc.materials[14]
    m.albedo[0], m.albedo[1], m.albedo[2] = 0.8, 0.75, 0.7
    desc.points = [sc.point_light((0.5, 1.5, 0.5), (8.0, 8.0, 8.0))]
    return desc


def test_cpp_mirror_tracks_player_light(pkg):
    """host/vpx_demo in its 'p' mode drives the C++ mirror (host/vpx_renderer.cpp) with
    trackPlayerLight over 3 Ticks at depth 1: the sums of the Ticks' records, the number of
    Ticks that set inLight and the record left after the last Tick (nothing) equal what the same
    frames give through the Python context, read and reset per frame (vpx_render serial, pinned
    by the frame tests above).  The world holds player smoke under a bright light, so the record
    is not empty and some Ticks are in light.  Without the letter: one line, as before."""
    import json
    import subprocess

    n, w, h, frames, depth = 32, 48, 32, 3, 1
    desc = demo_player_scene(pkg, n, w, h, depth)
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    acc = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    recs = []
    for f in range(frames):
        ctx.render(desc.frame_params(f), acc.data_ptr())
        recs.append(record(ctx.player_light(reset=True)))
    ctx.close()
    want = merged(recs)
    print("per frame", recs)
    assert want[0] > 0 and 0 < want[1] < want[0]
    exe = os.path.join(os.path.dirname(pkg.__file__), "host", "vpx_demo")
    r = subprocess.run([exe, str(n), str(w), str(h), str(frames), str(depth), "-", "p"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.strip().splitlines()]
    assert len(lines) == 2 and lines[0]["frames"] == frames
    pl = lines[1]["player_light"]
    print("demo", pl)
    got = (pl["probes"], pl["lit"], int(np.float32(pl["max_sqr"]).view(np.uint32)), pl["ticks_in_light"],
           pl["left_after_ticks"])
    assert got == (want[0], want[1], want[2], sum(1 for x in recs if x[3]), 0)
    r = subprocess.run([exe, str(n), str(w), str(h), "2", "1", "-", "-"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == 1


def test_window_fused_tail_big_frames(pkg):
    """k_finish_window<true>: a window chain whose own tail resolves the last level and blends
    (lanes, frames of at least 16384 tiles, area light samples: 2048 x 2048, 2 lanes, 4 frames
    at depth 0, so each chain holds two frames and the tail's loop p = p0 + b * stride resolves
    both).  The record and the image equal those of the same frames rendered one by one on the
    context's stream (the shadow pool and k_resolve_finish, pinned at 72 x 40 by
    test_frame_paths_two_volumes): every path of a chain is resolved exactly once."""
    w = h = 2048
    desc = player_scene(pkg, w, h, 0)
    assert (w // 16) * (h // 16) >= 16384 and len(desc.areas) and desc.area_samples > 1

    def run(lanes, window):
        ctx = pkg.context.Context(0)
        s = torch.cuda.Stream()
        ctx.set_stream(s.cuda_stream)
        ctx.load_scene(desc)
        ctx.set_pipeline(lanes)
        acc = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
        rgb = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(s):
                if window:
                    ctx.render_window(desc.frame_params(0), 4, acc.data_ptr(), rgb.data_ptr())
                else:
                    for f in range(4):
                        ctx.render(desc.frame_params(f), acc.data_ptr(), rgb.data_ptr())
            rec = record(ctx.player_light(reset=True))
            assert record(ctx.player_light()) == ZERO
            return rec, acc.cpu().numpy().view(np.uint32), rgb.cpu().numpy()
        finally:
            ctx.close()

    want = run(0, False)
    got = run(2, True)
    print("per frame", want[0], "window chains", got[0])
    assert want[0][0] > 10000 and 0 < want[0][1] < want[0][0]
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
