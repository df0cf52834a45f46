"""The variance-guided a-trous filter on the device (vpx_denoise_var) against the numpy restatement
(tests/denoise_var_ref.py) and the host path, bit for bit: tests/test_denoise.py's patterns, sizes
and passes (both LDS kernels and the gather, edge tiles, an image smaller than the step) on a
context that has neither a world nor a camera, moments NULL and given, rgb8 NULL and given; the
NaN / infinity poisoning; the refusals; scratch growth; the library's buffer count after close;
and the call queued without a synchronise behind a render on a user stream, frames in flight
included.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

from test_denoise import PASSES, PATTERNS, POISON, SIZES, pattern, poisoned, same_bits, u32  # noqa: E402
from test_denoise_gpu import on_device, size_params, view_desc  # noqa: E402
from test_denoise_var import VAR, denoise_var_refusals, inputs, reference  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 67, 35


def device_denoise_var(pkg, ctx, w, h, ids, img, mom, passes, rgb=False, **kw):
    """vpx_denoise_var on numpy inputs: out [H, W, 4], or (out, rgb8 [H, W])."""
    d_ids, d_img = on_device(ids), on_device(img)
    d_mom = None if mom is None else on_device(mom)
    d_rgb = torch.zeros(w * h, dtype=torch.int32, device="cuda") if rgb else None
    torch.cuda.synchronize()
    out = ctx.denoise_var(size_params(pkg, w, h), d_ids, d_img, d_mom, None, passes, rgb_ptr=d_rgb.data_ptr() if rgb else None,
                          **dict(VAR, **kw))
    ctx.synchronize()
    assert np.array_equal(u32(d_img.cpu().numpy()).reshape(-1), u32(img).reshape(-1)), "the input is read only"
    assert np.array_equal(u32(d_ids.cpu().numpy()).reshape(-1), u32(ids).reshape(-1)), "the ids are read only"
    if mom is not None:
        assert np.array_equal(u32(d_mom.cpu().numpy()).reshape(-1), u32(mom).reshape(-1)), "the moments are read only"
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
    for given in (False, True):
        ids, img, mom = inputs(name, w, h, given)
        outs = reference(name, w, h, given)[0]
        for passes in PASSES:
            rgb = passes == 2  # both forms of the call: rgb8 NULL and not
            got = device_denoise_var(pkg, bare, w, h, ids, img, mom, passes, rgb)
            host = pkg.context.denoise_var_host(w, h, ids, img, mom, passes=passes, rgb=rgb, **VAR)
            if rgb:
                (got, got_rgb), (host, host_rgb) = got, host
                assert np.array_equal(got_rgb, host_rgb), (name, size, passes, given, "rgb8")
            same_bits(got, outs[passes - 1], (name, size, passes, given, "restatement"))
            same_bits(got, host, (name, size, passes, given, "host"))


# ------------------------------------------------------------------------- 2. poisoning
@pytest.mark.parametrize("name", POISON)
def test_nan_and_inf_stay_on_their_plane(pkg, bare, name):
    for w, h in ((67, 35), (16, 16)):
        _, _, region = pattern(name, w, h)
        for given in (False, True):
            ids, img, mom = inputs(name, w, h, given)
            for passes in (1, 5):
                clean = reference(name, w, h, given)[0][passes - 1]
                for value in (np.nan, np.inf):
                    got = device_denoise_var(pkg, bare, w, h, ids, poisoned(img, region, value), mom, passes)
                    assert np.array_equal(u32(got)[region == 0], u32(clean)[region == 0]), (name, passes, given, value)
                    assert not np.isfinite(got[..., :3][region == 1]).any()
                    if given:
                        bad = mom.copy()
                        bad[region == 1] = value
                        got = device_denoise_var(pkg, bare, w, h, ids, img, bad, passes)
                        assert np.array_equal(u32(got)[region == 0], u32(clean)[region == 0]), (name, passes, "mom", value)
                        same_bits(got, pkg.context.denoise_var_host(w, h, ids, img, bad, passes=passes, **VAR), "poisoned moments")


# ---------------------------------------------------------------------- 3. scratch growth
def live(pkg):
    return int(pkg.load_library().vpx_debug_live_buffers())


def test_scratch_growth_and_buffer_count(pkg, bare):
    before = live(pkg)
    ctx = pkg.context.Context(0)
    for w, h, passes, given in ((16, 16, 1, False), (16, 16, 5, True), (67, 35, 5, True), (16, 16, 5, False), (67, 35, 1, True),
                                (5, 3, 2, True), (67, 35, 2, False)):
        ids, img, mom = inputs("stripes3", w, h, given)
        got = device_denoise_var(pkg, ctx, w, h, ids, img, mom, passes)
        same_bits(got, reference("stripes3", w, h, given)[0][passes - 1], (w, h, passes, given))
    assert live(pkg) > before, "the scratch is the context's"
    ctx.close()
    assert live(pkg) == before, "vpx_debug_live_buffers is balanced after close"


# --------------------------------------------------------------------------- 4. refusals
def test_refusals_then_a_normal_call(pkg, bare):
    abi = pkg.abi
    ids, img, mom = inputs("one_plane", W, H, True)
    d_ids, d_img, d_mom = on_device(ids), on_device(img), on_device(mom)
    d_out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lib, h = bare.lib, bare.h
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def call(w, hh, i, s, m, o, d):
        return lib.vpx_denoise_var(h, C.byref(size_params(pkg, w, hh)), ptr(i), ptr(s), ptr(m), ptr(o), None,
                                   C.byref(d) if d is not None else None)

    denoise_var_refusals(abi, call, d_ids, d_img, d_mom, d_out)
    ok = abi.denoise_var(2)
    args = (ptr(d_ids), ptr(d_img), ptr(d_mom), ptr(d_out), None, C.byref(ok))
    assert lib.vpx_denoise_var(h, None, *args) == abi.VPX_E_INVALID
    assert lib.vpx_denoise_var(None, C.byref(size_params(pkg, W, H)), *args) == abi.VPX_E_INVALID
    bare.synchronize()
    d_out.zero_()
    torch.cuda.synchronize()
    assert call(W, H, d_ids, d_img, d_mom, d_out, abi.denoise_var(6)) == abi.VPX_E_INVALID
    bare.synchronize()
    assert not d_out.cpu().numpy().any(), "a refused call writes nothing"
    got = device_denoise_var(pkg, bare, W, H, ids, img, mom, 5)
    same_bits(got, reference("one_plane", W, H, True)[0][4], "a normal call after the refusals")


# ------------------------------------------------------------------------ 5. stream order
def frames_then_denoise_var(pkg, desc, frames, lanes, sync_each):
    """`frames` accumulated frames, the ids, vpx_denoise_var (no moments) queued on one user stream;
    sync_each: a synchronise after every call, else one at the end.  Returns numpy (acc, ids, out, rgb8)."""
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
        ctx.denoise_var(desc.frame_params(0), ids, acc, None, out, 5, rgb_ptr=rgb.data_ptr(), **VAR)
    ctx.synchronize()
    if sync_each:  # nothing added to the work counters or the player-light record
        assert ctx.counters().as_dict() == before and ctx.player_light().as_dict() == light
    res = (acc.cpu().numpy().reshape(H, W, 4), ids.cpu().numpy().view(np.uint32).reshape(H, W, 4),
           out.cpu().numpy().reshape(H, W, 4), rgb.cpu().numpy().view(np.uint32).reshape(H, W))
    ctx.close()
    return res


def test_queued_behind_a_render_and_frames_in_flight(pkg, orc):
    desc = view_desc(pkg, orc)
    acc0, ids0, out0, rgb0 = frames_then_denoise_var(pkg, desc, 3, 0, True)
    host, host_rgb = pkg.context.denoise_var_host(W, H, ids0, acc0, None, passes=5, rgb=True, **VAR)
    same_bits(out0, host, "device vs host on a rendered frame")
    assert np.array_equal(rgb0, host_rgb)
    assert not np.array_equal(u32(out0)[..., :3], u32(acc0)[..., :3]), "the frame was filtered"
    for lanes in (0, 2):
        acc, ids, out, rgb = frames_then_denoise_var(pkg, desc, 3, lanes, False)
        same_bits(acc, acc0, (lanes, "accumulator"))
        assert np.array_equal(ids, ids0) and np.array_equal(rgb, rgb0), lanes
        same_bits(out, out0, (lanes, "render, ids, denoise back to back"))


def test_renderer_denoise_variance(pkg, orc):
    desc = view_desc(pkg, orc)
    r = pkg.renderer.Renderer(desc, 0).Init()
    r.Tick(0.0)
    got = r.Denoise(variance=dict(sigma_v=2.0, epsilon=2.0 ** -6, passes=3))
    assert got is r.denoised
    acc, ids = r.accumulator_host(), r.ids.cpu().numpy().view(np.uint32).reshape(H, W, 4)
    want, want_rgb = pkg.context.denoise_var_host(W, H, ids, acc, None, passes=3, sigma_v=2.0, epsilon=2.0 ** -6, min_history=1,
                                                  rgb=True)
    same_bits(r.denoised_host(), want, "Renderer.Denoise(variance=...)")
    assert np.array_equal(r.screen_host(), want_rgb)
    r.ctx.close()
