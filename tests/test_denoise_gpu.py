"""The plane-keyed a-trous filter on the device (vpx_denoise_ids) against the numpy restatement
(tests/denoise_ref.py) and the host path, bit for bit: the synthetic patterns of
tests/test_denoise.py on a context that has neither a world nor a camera, the NaN / infinity
poisoning, a rendered frame of scene S end to end (and Renderer.Denoise on it), stream order,
scratch growth, the refusals, and frames in flight.

Scene S's own camera sees voxels in a fifth of a 67 x 35 frame (tests/test_hit_cells_gpu.py), too
few for the end-to-end condition (a quarter of the pixels filtered); the camera here stands
closer and looks down at the room: VIEW_POS -> VIEW_TARGET, two thirds of the pixels on voxels.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import denoise_ref  # noqa: E402
from test_denoise import (PASSES, PATTERNS, POISON, SIGMAS, SIZES, pattern, poisoned, reference, refusals, same_bits,  # noqa: E402
                          u32)
from test_ray_filter import case_s  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 67, 35
VIEW_POS, VIEW_TARGET = (0.5, 0.5, 0.0), (0.5, 0.1, 0.5)


def size_params(pkg, w, h):
    p = pkg.abi.FrameParams()
    p.width, p.height = w, h
    return p


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype).copy()).cuda()


def device_denoise(pkg, ctx, w, h, ids, img, passes, sigma_l, rgb=False):
    """vpx_denoise_ids on numpy inputs: out [H, W, 4], or (out, rgb8 [H, W])."""
    d_ids, d_img = on_device(ids), on_device(img)
    d_rgb = torch.zeros(w * h, dtype=torch.int32, device="cuda") if rgb else None
    torch.cuda.synchronize()
    out = ctx.denoise(size_params(pkg, w, h), d_ids, d_img, None, passes, sigma_l, d_rgb.data_ptr() if rgb else None)
    ctx.synchronize()
    assert np.array_equal(u32(d_img.cpu().numpy()), u32(img)), "the input is read only"
    o = out.cpu().numpy().reshape(h, w, 4)
    return (o, d_rgb.cpu().numpy().view(np.uint32).reshape(h, w)) if rgb else o


@pytest.fixture(scope="module")
def bare(pkg):
    """A context without a world and without a camera: the filter reads only its arguments."""
    ctx = pkg.context.Context(0)
    yield ctx
    ctx.close()


# -------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", PATTERNS)
def test_device_equals_restatement_and_host(pkg, bare, name, size):
    w, h = size
    ids, img, _ = pattern(name, w, h)
    for sigma_l in SIGMAS:
        outs, _ = reference(name, w, h, sigma_l)
        for passes in PASSES:
            rgb = passes == 2  # both forms of the call: rgb8 NULL and not
            got = device_denoise(pkg, bare, w, h, ids, img, passes, sigma_l, rgb)
            host = pkg.context.denoise_host(w, h, ids, img, passes, sigma_l, rgb)
            if rgb:
                (got, got_rgb), (host, host_rgb) = got, host
                assert np.array_equal(got_rgb, host_rgb), (name, size, passes, sigma_l, "rgb8")
            want = outs[passes - 1]
            assert np.array_equal(u32(got), u32(want)), (name, size, passes, sigma_l, int((u32(got) != u32(want)).sum()))
            assert np.array_equal(u32(got), u32(host)), (name, size, passes, sigma_l, "host")


# ------------------------------------------------------------------------- 2. poisoning
@pytest.mark.parametrize("name", POISON)
def test_nan_and_inf_stay_on_their_plane(pkg, bare, name):
    for w, h in ((67, 35), (16, 16)):
        ids, img, region = pattern(name, w, h)
        for sigma_l in SIGMAS:
            for passes in (1, 5):
                clean = reference(name, w, h, sigma_l)[0][passes - 1]
                for value in (np.nan, np.inf):
                    got = device_denoise(pkg, bare, w, h, ids, poisoned(img, region, value), passes, sigma_l)
                    assert np.array_equal(u32(got)[region == 0], u32(clean)[region == 0]), (name, passes, sigma_l, value)
                    assert not np.isfinite(got[..., :3][region == 1]).any()


# ------------------------------------------------------------------------ 3. end to end
def view_desc(pkg, orc):
    """Scene S at 67 x 35 under the closer camera, depth 2, no AA."""
    d = case_s(pkg, orc)[0].with_size(W, H)
    d.camera = pkg.scene.look_at(VIEW_POS, VIEW_TARGET, W, H)
    d._cam_pos, d._cam_target = VIEW_POS, VIEW_TARGET
    d.max_bounces, d.flags = 2, 0
    return d


def frames_then_denoise(pkg, desc, frames=1, lanes=0, sync_each=True, passes=5, sigma_l=0.0):
    """`frames` accumulated frames, the ids, the denoise, queued on one stream; sync_each: a
    synchronise after every call, else one at the end.  Returns numpy (acc, ids, out, rgb8)."""
    ctx = pkg.context.Context(0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    ctx.load_scene(desc)
    ctx.set_pipeline(lanes)
    acc = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before, light = ctx.counters(reset=True).as_dict(), None
    with torch.cuda.stream(s):
        for f in range(frames):
            ctx.render(desc.frame_params(f), acc.data_ptr(), None)
            if sync_each:
                ctx.synchronize()
        if sync_each:
            before, light = ctx.counters().as_dict(), ctx.player_light().as_dict()
        ids = ctx.render_ids(desc.frame_params(0))
        if sync_each:
            ctx.synchronize()
        ctx.denoise(desc.frame_params(0), ids, acc, out, passes, sigma_l, rgb.data_ptr())
    ctx.synchronize()
    if sync_each:  # nothing added to the work counters or the player-light record
        assert ctx.counters().as_dict() == before and ctx.player_light().as_dict() == light
    res = (acc.cpu().numpy().reshape(H, W, 4), ids.cpu().numpy().view(np.uint32), out.cpu().numpy().reshape(H, W, 4),
           rgb.cpu().numpy().view(np.uint32).reshape(H, W))
    ctx.close()
    return res


@pytest.fixture(scope="module")
def frame(pkg, orc):
    desc = view_desc(pkg, orc)
    return (desc,) + frames_then_denoise(pkg, desc)


def test_rendered_frame_end_to_end(pkg, frame):
    desc, acc, ids, out, rgb = frame
    assert np.isfinite(acc[..., :3]).all(), "scene S renders no NaN here (the comparison below would still hold)"
    outs, taps = denoise_ref.run(ids, acc, 5, 0.0)
    ka, kb = denoise_ref.keys(ids)
    filtered = (kb != 0) & (taps >= 2)  # the centre and one other tap
    assert int(filtered.sum()) * 4 >= W * H, int(filtered.sum())
    planes = {(int(a), int(b)) for a, b in zip(ka[kb != 0], kb[kb != 0])}
    print("filtered pixels", int(filtered.sum()), "of", W * H, "invalid", int((kb == 0).sum()), "distinct keys", len(planes))
    # misses and shapes pass through; the floor, and the block's mixed smoke: more than a few keys
    assert int((kb == 0).sum()) >= 100 and len(planes) >= 4
    same_bits(out, outs[4], "device vs restatement")
    assert not np.array_equal(u32(out)[filtered], u32(acc)[filtered])
    host, host_rgb = pkg.context.denoise_host(W, H, ids, acc, 5, 0.0, rgb=True)
    same_bits(out, host, "device vs host")
    assert np.array_equal(rgb, host_rgb)
    # the filter does what it is for: on the filtered pixels the image is smoother than it was
    rough = lambda a: float(np.abs(np.diff(a[..., :3], axis=1))[filtered[:, 1:] & filtered[:, :-1]].mean())  # noqa: E731
    assert rough(out) < rough(acc)


def test_sigma_on_a_rendered_frame(pkg, frame):
    desc, acc, ids, _, _ = frame
    with pkg.context.Context(0) as ctx:
        got = device_denoise(pkg, ctx, W, H, ids, acc, 5, 0.5)
    same_bits(got, denoise_ref.run(ids, acc, 5, 0.5)[0][4], "sigma_l 0.5")


def test_renderer_denoise(pkg, frame):
    desc, acc, ids, out, rgb = frame
    r = pkg.renderer.Renderer(desc, 0).Init()
    r.Tick(0.0)
    got = r.Denoise()
    assert got is r.denoised
    same_bits(r.accumulator_host(), acc, "the same frame")
    assert np.array_equal(r.ids.cpu().numpy().view(np.uint32), ids)
    same_bits(r.denoised_host(), out, "Renderer.Denoise")
    assert np.array_equal(r.screen_host(), rgb)
    r.Denoise(passes=2, sigma_l=0.5)  # queued on the renderer's stream: denoised_host() synchronises it
    same_bits(r.denoised_host(), denoise_ref.run(ids, acc, 2, 0.5)[0][1], "Renderer.Denoise(2, 0.5)")
    r.ctx.close()


# ------------------------------------------------------------------------ 4. stream order
def test_stream_order(pkg, frame):
    desc, acc, ids, out, rgb = frame
    acc2, ids2, out2, rgb2 = frames_then_denoise(pkg, desc, sync_each=False)
    same_bits(acc2, acc, "accumulator")
    assert np.array_equal(ids2, ids) and np.array_equal(rgb2, rgb)
    same_bits(out2, out, "render, ids, denoise back to back")


# ---------------------------------------------------------------------- 5. scratch growth
def test_scratch_growth(pkg):
    with pkg.context.Context(0) as ctx:
        for w, h, passes in ((16, 16, 1), (16, 16, 5), (67, 35, 5), (16, 16, 5), (67, 35, 1), (5, 3, 2)):
            ids, img, _ = pattern("stripes3", w, h)
            got = device_denoise(pkg, ctx, w, h, ids, img, passes, 0.5)
            want = reference("stripes3", w, h, 0.5)[0][passes - 1]
            assert np.array_equal(u32(got), u32(want)), (w, h, passes)


# --------------------------------------------------------------------------- 6. refusals
def test_refusals_then_a_normal_frame(pkg, frame):
    desc, acc, _, _, _ = frame
    abi = pkg.abi
    ids, img, _ = pattern("one_plane", W, H)
    d_ids, d_img = on_device(ids), on_device(img)
    d_out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pkg.context.Context(0) as ctx:
        ctx.load_scene(desc)
        lib, h = ctx.lib, ctx.h

        def call(w, hh, i, s, o, d):
            return lib.vpx_denoise_ids(h, C.byref(size_params(pkg, w, hh)), None if i is None else C.c_void_p(i.data_ptr()),
                                       None if s is None else C.c_void_p(s.data_ptr()),
                                       None if o is None else C.c_void_p(o.data_ptr()), None,
                                       C.byref(d) if d is not None else None)

        refusals(abi, call, d_ids, d_img, d_out)
        ok = abi.Denoise(2, 0.5, 0, 0)
        assert lib.vpx_denoise_ids(h, None, C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_img.data_ptr()),
                                   C.c_void_p(d_out.data_ptr()), None, C.byref(ok)) == abi.VPX_E_INVALID
        assert lib.vpx_denoise_ids(None, C.byref(size_params(pkg, W, H)), C.c_void_p(d_ids.data_ptr()),
                                   C.c_void_p(d_img.data_ptr()), C.c_void_p(d_out.data_ptr()), None,
                                   C.byref(ok)) == abi.VPX_E_INVALID
        ctx.synchronize()
        d_out.zero_()
        torch.cuda.synchronize()
        assert call(W, H, d_ids, d_img, d_out, abi.Denoise(6, 0.0, 0, 0)) == abi.VPX_E_INVALID
        ctx.synchronize()
        assert not d_out.cpu().numpy().any(), "a refused call writes nothing"
        a = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.render(desc.frame_params(0), a.data_ptr(), None)
        ctx.synchronize()
        same_bits(a.cpu().numpy().reshape(H, W, 4), acc, "the context renders as before")


# -------------------------------------------------------------------- 7. frames in flight
def test_after_pipelined_frames(pkg, orc):
    desc = view_desc(pkg, orc)
    acc0, ids0, out0, rgb0 = frames_then_denoise(pkg, desc, frames=3, lanes=0)
    acc3, ids3, out3, rgb3 = frames_then_denoise(pkg, desc, frames=3, lanes=3, sync_each=False)
    same_bits(acc3, acc0, "three frames, three lanes")
    assert np.array_equal(ids3, ids0) and np.array_equal(rgb3, rgb0)
    same_bits(out3, out0, "denoise after frames in flight")
    same_bits(out0, denoise_ref.run(ids0, acc0, 5, 0.0)[0][4], "three accumulated frames vs restatement")
