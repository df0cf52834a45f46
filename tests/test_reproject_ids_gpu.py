"""The plane-keyed reprojection on the device (vpx_reproject_ids) against the numpy restatement
(tests/reproject_ids_ref.py) and the host path, bit for bit: the synthetic cases of
tests/test_reproject_ids.py on a context that has neither a world nor a camera (poisoned
histories and moving volumes included, with and without rgb8), real ids of scene S from a moving
camera (one step and a chain of six ticks), Renderer's temporal mode, stream order, scratch
growth, the refusals, frames in flight, and the frame path before and after a call.

Scene S is seen as tests/test_denoise_gpu.py sees it (its camera stands closer than the scene's
own, two thirds of the pixels on voxels), the camera then moving along PATH.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import denoise_ref  # noqa: E402
import epilogue_ref  # noqa: E402
import reproject_ids_ref as ref  # noqa: E402
from test_denoise_gpu import VIEW_POS, VIEW_TARGET, on_device, size_params, view_desc  # noqa: E402
from test_reproject_ids import (cameras, case, moving_case, moving_reference, moving_volumes, poison_case, reference,  # noqa: E402
                                refusals, same_bits, u32)

pytestmark = pytest.mark.gpu
W, H = 67, 35
NOHIST = (1, 0)  # scene S's voxels are of the view-dependent materials Renderer's default range leaves out
PATH = [(VIEW_POS[0] + 0.012 * k, VIEW_POS[1] + 0.004 * k, VIEW_POS[2] + 0.009 * k) for k in range(6)]


def device_reproject(pkg, ctx, c, rgb=False, **kw):
    """vpx_reproject_ids on a case's numpy inputs: out [H, W, 4], or (out, rgb8 [H, W])."""
    w, h = c["w"], c["h"]
    cam, prev = cameras(pkg, c)
    a = dict(ids_prev=c["ids_prev"], cur=c["cur"], hist_in=c["hist_in"])
    a.update({k: kw.pop(k) for k in list(kw) if k in a})
    dev = {k: None if v is None else on_device(v) for k, v in a.items()}
    d_ids = on_device(c["ids_cur"])
    d_rgb = torch.zeros(w * h, dtype=torch.int32, device="cuda") if rgb else None
    torch.cuda.synchronize()
    out = ctx.reproject(size_params(pkg, w, h), d_ids, dev["ids_prev"], dev["cur"], dev["hist_in"], cam, prev,
                        rgb_ptr=d_rgb.data_ptr() if rgb else None, **kw)
    ctx.synchronize()
    for k, v in a.items():
        if v is not None:
            assert np.array_equal(u32(dev[k].cpu().numpy()).reshape(-1), u32(v).reshape(-1)), "the inputs are read only"
    o = out.cpu().numpy().reshape(h, w, 4)
    return (o, d_rgb.cpu().numpy().view(np.uint32).reshape(h, w)) if rgb else o


def tonemap_of(img):
    return np.array([epilogue_ref.tonemap_ref(px[:3].astype(np.float64)) for px in img.reshape(-1, 4)], np.uint32)


@pytest.fixture(scope="module")
def bare(pkg):
    """A context without a world and without a camera: the pass reads only its arguments."""
    ctx = pkg.context.Context(0)
    yield ctx
    ctx.close()


# -------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("size", ((67, 35), (33, 17)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", ("identical", "translation", "yaw", "dolly", "behind"))
def test_device_equals_restatement_and_host(pkg, bare, pair, size):
    w, h = size
    c = case(pair, w, h)
    want, arm, _ = reference(pair, w, h)
    plain = device_reproject(pkg, bare, c)
    got, rgb = device_reproject(pkg, bare, c, rgb=True)
    host, host_rgb = pkg.context.reproject_host(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], *cameras(pkg, c),
                                                rgb=True)
    same_bits(got, want, (pair, size, "restatement"))
    same_bits(got, host, (pair, size, "host"))
    same_bits(plain, got, (pair, size, "with and without rgb8"))
    assert np.array_equal(rgb, host_rgb) and np.array_equal(rgb.reshape(-1), tonemap_of(got))
    if pair != "behind":
        assert (arm == ref.HISTORY).sum() * 4 >= w * h


def test_variants_of_the_call(pkg, bare):
    """max_history 1, a nohist range, no previous frame."""
    w, h = 33, 17
    c = case("translation", w, h)
    same_bits(device_reproject(pkg, bare, c, max_history=1), reference("translation", w, h, 1)[0], "max_history 1")
    same_bits(device_reproject(pkg, bare, c, nohist=(4, 5)), reference("translation", w, h, 32, (4, 5))[0], "nohist 4..5")
    got = device_reproject(pkg, bare, c, ids_prev=None, hist_in=None)
    assert np.array_equal(u32(got)[..., :3], u32(c["cur"])[..., :3]) and (got[..., 3] == 1.0).all()


@pytest.mark.parametrize("value", (np.nan, np.inf))
def test_poison_stays_off_the_floor(pkg, bare, value):
    for w, h in ((67, 35), (33, 17)):
        c = poison_case(w, h, value)
        clean, arm, _ = reference("translation", w, h)
        got, rgb = device_reproject(pkg, bare, c, rgb=True)
        floor = (c["ids_cur"][..., 1] >> 16 & 255 == 3) & (c["ids_cur"][..., 1] >> 24 > 0)
        assert np.array_equal(u32(got)[floor], u32(clean)[floor]) and np.isfinite(got[floor]).all()
        host = pkg.context.reproject_host(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], *cameras(pkg, c))
        same_bits(got, host, ("poison", value))
        assert np.array_equal(rgb[floor], tonemap_of(got).reshape(h, w)[floor])


@pytest.mark.parametrize("size", ((67, 35), (33, 17)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_moving_volumes(pkg, bare, size):
    w, h = size
    c = moving_case(w, h)
    got = {}
    for mode in ("moved", "static", "short", "equal"):
        cv, pv = moving_volumes(c, mode)
        got[mode], rgb = device_reproject(pkg, bare, c, rgb=True, cur_volumes=cv, prev_volumes=pv)
        same_bits(got[mode], moving_reference(w, h, mode)[0], (mode, size))
        assert np.array_equal(rgb.reshape(-1), tonemap_of(got[mode]))
        same_bits(device_reproject(pkg, bare, c, cur_volumes=cv, prev_volumes=pv), got[mode], (mode, "without rgb8"))
    assert np.array_equal(u32(got["equal"]), u32(got["static"])) and not np.array_equal(u32(got["moved"]), u32(got["static"]))


# ------------------------------------------------------------------------ 2. real ids
def view_at(pkg, orc, pos):
    d = view_desc(pkg, orc)
    d.camera = pkg.scene.look_at(pos, VIEW_TARGET, W, H)
    d._cam_pos, d._cam_target = pos, VIEW_TARGET
    return d


def tick_params(desc, k):
    """Tick k's frame: frame_index 0 (the accumulator is this tick's samples alone), tick k's seeds."""
    p = desc.frame_params(0)
    p.seed_base = (p.seed_base + k * W * H) & 0xFFFFFFFF
    return p


def device_chain(pkg, orc, ticks=6, lanes=0, sync_each=True, denoise=None, max_history=32, nohist=NOHIST, warm_frames=0):
    """render -> ids -> reproject (-> denoise) per tick along PATH on one stream, every tick into
    buffers of its own; sync_each: a synchronise after every call, else one at the end.  Returns
    per tick numpy (acc, ids, hist, denoised or None, rgb8)."""
    descs = [view_at(pkg, orc, PATH[k]) for k in range(ticks)]
    ctx = pkg.context.Context(0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    ctx.load_scene(descs[0])
    ctx.set_pipeline(lanes)
    new = lambda n, t: [torch.zeros(n, dtype=t, device="cuda") for _ in range(ticks)]  # noqa: E731
    acc, hist, den = new(W * H * 4, torch.float32), new(W * H * 4, torch.float32), new(W * H * 4, torch.float32)
    ids, rgb = new(W * H * 4, torch.int32), new(W * H, torch.int32)
    torch.cuda.synchronize()
    sync = ctx.synchronize if sync_each else (lambda: None)
    with torch.cuda.stream(s):
        for f in range(warm_frames):  # accumulated frames in flight ahead of the chain
            ctx.render(descs[0].frame_params(f), acc[0].data_ptr(), None)
        for k, d in enumerate(descs):
            ctx.set_camera(d.camera)
            p = tick_params(d, k)
            ctx.render(p, acc[k].data_ptr(), None)
            sync()
            ctx._chk(ctx.lib.vpx_render_ids(ctx.h, C.byref(p), None, C.c_void_p(ids[k].data_ptr())), "vpx_render_ids")
            sync()
            before = ctx.counters().as_dict() if sync_each else None
            prev_cam = pkg.scene.prev_camera(PATH[k - 1], VIEW_TARGET, W, H) if k else pkg.scene.prev_camera(PATH[0], VIEW_TARGET, W, H)
            ctx.reproject(p, ids[k], ids[k - 1] if k else None, acc[k], hist[k - 1] if k else None, d.camera, prev_cam,
                          out=hist[k], max_history=max_history, nohist=nohist, rgb_ptr=None if denoise else rgb[k].data_ptr())
            sync()
            if sync_each:  # nothing added to the work counters
                assert ctx.counters().as_dict() == before
            if denoise:
                ctx.denoise(p, ids[k], hist[k], den[k], denoise, 0.0, rgb[k].data_ptr())
                sync()
    ctx.synchronize()
    out = [(acc[k].cpu().numpy().reshape(H, W, 4), ids[k].cpu().numpy().view(np.uint32).reshape(H, W, 4),
            hist[k].cpu().numpy().reshape(H, W, 4), den[k].cpu().numpy().reshape(H, W, 4) if denoise else None,
            rgb[k].cpu().numpy().view(np.uint32).reshape(H, W)) for k in range(ticks)]
    ctx.close()
    return out


@pytest.fixture(scope="module")
def chain(pkg, orc):
    return device_chain(pkg, orc)


def host_chain(pkg, frames, max_history=32, nohist=NOHIST):
    """The same ticks on the host, from the device's samples and ids."""
    hists = []
    for k, (acc, ids, _, _, _) in enumerate(frames):
        cam = pkg.scene.look_at(PATH[k], VIEW_TARGET, W, H)
        prev = pkg.scene.prev_camera(PATH[max(k - 1, 0)], VIEW_TARGET, W, H)
        hists.append(pkg.context.reproject_host(W, H, ids, frames[k - 1][1] if k else None, acc, hists[-1] if k else None, cam,
                                                prev, max_history=max_history, nohist=nohist))
    return hists


def test_real_ids_one_step(pkg, chain):
    """Scene S from two cameras a step apart: the first tick has no history, the second takes it on
    most voxel pixels; device, host and restatement agree."""
    from test_kat_reproject import Camera
    (acc0, ids0, hist0, _, rgb0), (acc1, ids1, hist1, _, rgb1) = chain[0], chain[1]
    assert np.array_equal(u32(hist0)[..., :3], u32(acc0)[..., :3]) and (hist0[..., 3] == 1.0).all()
    assert not np.array_equal(ids0, ids1), "the camera moved"
    want, arm, mask = ref.run(W, H, ids1, ids0, acc1, hist0, Camera(PATH[1], VIEW_TARGET, W, H), Camera(PATH[0], VIEW_TARGET, W, H),
                              32, NOHIST)
    kb = denoise_ref.keys(ids1)[1]
    print("valid keys", int((kb != 0).sum()), "took history", int((arm == ref.HISTORY).sum()), "arms", np.bincount(arm.reshape(-1), minlength=8).tolist())
    assert int((arm == ref.HISTORY).sum()) * 4 >= W * H
    same_bits(hist1, want, "device vs restatement")
    same_bits(hist1, host_chain(pkg, chain[:2])[1], "device vs host")
    assert (hist1[..., 3][arm == ref.HISTORY] == 2.0).all()
    assert np.array_equal(rgb1.reshape(-1), tonemap_of(hist1))


def test_chain_of_six_ticks(pkg, chain):
    hists = host_chain(pkg, chain)
    for k in range(6):
        same_bits(chain[k][2], hists[k], f"tick {k}")
    lengths = np.array([c[2][..., 3].max() for c in chain])
    assert lengths.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], lengths
    # the accumulated image is smoother than the tick's own samples where history was kept
    kept = chain[5][2][..., 3] >= 4.0
    assert kept.sum() >= 200
    rough = lambda a: float(np.abs(np.diff(a[..., :3], axis=1))[kept[:, 1:] & kept[:, :-1]].mean())  # noqa: E731
    assert rough(chain[5][2]) < rough(chain[5][0])


def test_renderer_temporal_mode(pkg, orc, chain):
    """Renderer(temporal=...) over four ticks equals the explicit chain; with a denoise the history is
    the same and the denoised image is the filter of it."""
    r = pkg.renderer.Renderer(view_at(pkg, orc, PATH[0]), 0, temporal=dict(nohist=NOHIST, denoise=dict(passes=2))).Init()
    for k in range(4):
        r.LookAt(PATH[k], VIEW_TARGET)
        r.Tick(0.0)
        acc, ids, hist, _, _ = chain[k]
        same_bits(r.temporal_history_host(), hist, f"tick {k}: history")
        same_bits(r.accumulator_host(), acc, f"tick {k}: samples")
        assert np.array_equal(r.ids.cpu().numpy().view(np.uint32).reshape(H, W, 4), ids)
        want = pkg.context.denoise_host(W, H, ids, hist, 2, 0.0, rgb=True)
        same_bits(r.denoised_host(), want[0], f"tick {k}: denoised")
        assert np.array_equal(r.screen_host(), want[1])
    r.DropHistory()
    r.Tick(0.0)
    assert (r.temporal_history_host()[..., 3] == 1.0).all()
    r.ctx.close()
    plain = pkg.renderer.Renderer(view_at(pkg, orc, PATH[0]), 0, temporal=True).Init()
    assert plain.temporal == dict(max_history=32, nohist=(5, 14), denoise=None)
    plain.temporal["nohist"] = NOHIST
    for k in range(2):
        plain.LookAt(PATH[k], VIEW_TARGET)
        plain.Tick(0.0)
    same_bits(plain.temporal_history_host(), chain[1][2], "temporal=True")
    assert np.array_equal(plain.screen_host(), chain[1][4])
    plain.ctx.close()
    off = pkg.renderer.Renderer(view_at(pkg, orc, PATH[0]), 0).Init()  # the default stays as it was
    off.Tick(0.0)
    assert off.history is None and off.numRenderedFrames == 1
    off.ctx.close()


# ------------------------------------------------------------------------ 3. stream order
def test_stream_order(pkg, orc, chain):
    """render -> ids -> reproject -> denoise, six ticks back to back, read once at the end."""
    synced = device_chain(pkg, orc, denoise=3)
    queued = device_chain(pkg, orc, denoise=3, sync_each=False)
    for k in range(6):
        same_bits(synced[k][2], chain[k][2], f"tick {k}: the denoise does not touch the history")
        for i, what in ((0, "samples"), (2, "history"), (3, "denoised")):
            same_bits(queued[k][i], synced[k][i], f"tick {k}: {what}")
        assert np.array_equal(queued[k][1], synced[k][1]) and np.array_equal(queued[k][4], synced[k][4]), k
        want = pkg.context.denoise_host(W, H, synced[k][1], synced[k][2], 3, 0.0, rgb=True)
        same_bits(synced[k][3], want[0], f"tick {k}: denoised")
        assert np.array_equal(synced[k][4], want[1])


# ---------------------------------------------------------------------- 4. scratch growth
def test_scratch_growth(pkg):
    """Small, large, small: sizes and volume tables (the table is the context's scratch)."""
    with pkg.context.Context(0) as ctx:
        for (w, h), extra in (((33, 17), 0), ((67, 35), 300), ((33, 17), 0), ((67, 35), 0), ((33, 17), 300)):
            c = moving_case(w, h)
            cv, pv = moving_volumes(c, "moved")
            pad = tuple(pkg.scene.volume(position=(float(i), 0.0, 0.0)) for i in range(extra))  # never referenced by an id
            got = device_reproject(pkg, ctx, c, cur_volumes=cv + pad, prev_volumes=pv + pad)
            same_bits(got, moving_reference(w, h, "moved")[0], (w, h, extra))
            got = device_reproject(pkg, ctx, c, cur_volumes=cv + pad, prev_volumes=pv + pad)  # the table is already there
            same_bits(got, moving_reference(w, h, "moved")[0], (w, h, extra, "again"))
            cs = case("translation", w, h)
            same_bits(device_reproject(pkg, ctx, cs), reference("translation", w, h)[0], (w, h, "static"))


# --------------------------------------------------------------------------- 5. refusals
def test_refusals_then_a_normal_frame(pkg, orc, chain):
    c = case("translation", W, H)
    cam, prev = cameras(pkg, c)
    d = {k: on_device(c[k]) for k in ("ids_cur", "ids_prev", "cur", "hist_in")}
    d_out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    vols = (pkg.abi.Volume * 2)(pkg.scene.volume(), pkg.scene.volume())
    torch.cuda.synchronize()
    desc = view_at(pkg, orc, PATH[0])
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    with pkg.context.Context(0) as ctx:
        ctx.load_scene(desc)
        lib, h = ctx.lib, ctx.h

        def call(w, hh, ic, ip, cu, hi, ho, r, cv, pv):
            return lib.vpx_reproject_ids(h, C.byref(size_params(pkg, w, hh)), ptr(ic), ptr(ip), ptr(cu), ptr(hi), ptr(ho), None,
                                         C.byref(r) if r is not None else None, cv, pv)

        refusals(pkg, call, d["ids_cur"], d["ids_prev"], d["cur"], d["hist_in"], d_out, cam, prev, vols)
        ctx.synchronize()
        same_bits(d_out.cpu().numpy().reshape(H, W, 4), reference("translation", W, H)[0], "the normal call after the refusals")
        ok = pkg.context.reproject_desc(cam, prev)[0]
        args = (ptr(d["ids_cur"]), ptr(d["ids_prev"]), ptr(d["cur"]), ptr(d["hist_in"]), ptr(d_out), None, C.byref(ok), None, None)
        assert lib.vpx_reproject_ids(h, None, *args) == pkg.abi.VPX_E_INVALID
        assert lib.vpx_reproject_ids(None, C.byref(size_params(pkg, W, H)), *args) == pkg.abi.VPX_E_INVALID
        d_out.zero_()
        torch.cuda.synchronize()
        bad = pkg.context.reproject_desc(cam, prev, 0.5)[0]
        assert call(W, H, d["ids_cur"], d["ids_prev"], d["cur"], d["hist_in"], d_out, bad, None, None) == pkg.abi.VPX_E_INVALID
        ctx.synchronize()
        assert not d_out.cpu().numpy().any(), "a refused call writes nothing"
        a = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.render(tick_params(desc, 0), a.data_ptr(), None)
        ctx.synchronize()
        same_bits(a.cpu().numpy().reshape(H, W, 4), chain[0][0], "the context renders as before")


# -------------------------------------------------------------------- 6. frames in flight
def test_after_pipelined_frames(pkg, orc, chain):
    """Three accumulated frames in flight on three lanes, then the chain without a synchronise."""
    piped = device_chain(pkg, orc, ticks=3, lanes=3, sync_each=False, warm_frames=3)
    for k in range(3):
        same_bits(piped[k][0], chain[k][0], f"tick {k}: samples")
        assert np.array_equal(piped[k][1], chain[k][1]) and np.array_equal(piped[k][4], chain[k][4])
        same_bits(piped[k][2], chain[k][2], f"tick {k}: history")


# ------------------------------------------------------------------ 7. the frame path
def test_frame_path_is_untouched(pkg, orc, bare):
    """vpx_debug_last_frame_kernel and a depth-0 frame's accumulator, before and after a call."""
    desc = view_at(pkg, orc, PATH[0])
    desc.max_bounces = 0
    c = case("translation", W, H)
    with pkg.context.Context(0) as ctx:
        ctx.load_scene(desc)
        frames, forms = [], []
        for i in range(2):
            a = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ctx.render(desc.frame_params(0), a.data_ptr(), None)
            ctx.synchronize()
            frames.append(a.cpu().numpy())
            forms.append(ctx.last_frame_kernel())
            if i == 0:
                same_bits(device_reproject(pkg, ctx, c), reference("translation", W, H)[0], "the call in between")
                assert ctx.last_frame_kernel() == forms[0]
        assert forms[0] == forms[1]
        same_bits(frames[1], frames[0], "depth-0 frame")


# ------------------------------------------------------------------- 8. the C++ mirror
def test_cpp_mirror_temporal_mode(pkg, tmp_path):
    """host/vpx_demo in mode 't' (Renderer::temporal, a step along a path per tick) shows the
    screen of the Python Renderer's temporal mode over the same three ticks."""
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(pkg.__file__), "host", "vpx_demo")
    if not os.path.exists(exe):
        pytest.fail("host/vpx_demo missing: run __graft_entry__.build()")
    n, w, h, ticks, depth = 64, 96, 64, 3, 1
    out = tmp_path / "frame.rgb8"
    run = subprocess.run([exe, str(n), str(w), str(h), str(ticks), str(depth), str(out), "t"], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr
    desc = pkg.scene.pillars_scene(n, w, h, depth)
    f = np.float32
    pos, tgt = [f(v) for v in desc._cam_pos], desc._cam_target
    r = pkg.renderer.Renderer(desc, 0, temporal=dict(nohist=NOHIST)).Init()
    for k in range(ticks):
        if k:  # the demo's float arithmetic: pos + step * k
            r.LookAt((float(pos[0] + f(0.01) * f(k)), float(pos[1] + f(0.004) * f(k)), float(pos[2] - f(0.008) * f(k))), tgt)
        r.Tick(0.0)
    lengths = r.temporal_history_host()[..., 3]
    valid = denoise_ref.keys(r.ids.cpu().numpy().view(np.uint32).reshape(h, w, 4))[1] != 0
    print("valid keys", int(valid.sum()), "of", w * h, "took history", int((lengths > 1.0).sum()), "longest", float(lengths.max()))
    # not a vacuous comparison: as on the synthetic cases, at least half of the keyed pixels keep their history
    assert lengths.max() == 3.0 and (lengths > 1.0).sum() * 2 >= valid.sum() >= 500
    assert np.array_equal(np.fromfile(out, np.uint32), r.screen_host().reshape(-1))
    r.ctx.close()
