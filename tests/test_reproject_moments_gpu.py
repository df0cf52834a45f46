"""vpx_reproject_moments on the device, and the variance-guided pipeline end to end: scene S from a
moving camera (tests/test_reproject_ids_gpu.py's view of it), six ticks.  Per tick hist_out is
vpx_reproject_ids' bit for bit and mom_out is the host twin's; Renderer(temporal=dict(variance=...))
equals the host pipeline (vpx_reproject_moments_host, vpx_denoise_var_host) run on the read-back
ids and samples; the synthetic cases of tests/test_reproject_ids.py (moving volumes included)
against the restatement; the refusals.

The camera dollies backwards (PATH), so that every tick brings pixels into view that have no
history: with MIN_HISTORY = 3 the last tick's filter takes the temporal arm where the history is
three frames or longer and the spatial arm on the rim and behind the parallax edges.  Both shares
are asserted, on the host pipeline's own history lengths.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import denoise_ref  # noqa: E402
import reproject_moments_ref  # noqa: E402
import test_reproject_ids as tri  # noqa: E402
from test_denoise import same_bits, u32  # noqa: E402
from test_denoise_gpu import VIEW_POS, VIEW_TARGET, on_device, size_params  # noqa: E402
from test_denoise_var import moments_for, reproject_moments_refusals  # noqa: E402
from test_reproject_ids_gpu import NOHIST, tick_params, view_at  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 67, 35
TICKS, MIN_HISTORY = 6, 3
PATH = [(VIEW_POS[0] + 0.012 * k, VIEW_POS[1] + 0.004 * k, VIEW_POS[2] - 0.015 * k) for k in range(TICKS)]
VARIANCE = dict(sigma_v=4.0, epsilon=2.0 ** -10, min_history=MIN_HISTORY, passes=5)


@pytest.fixture(scope="module")
def bare(pkg):
    ctx = pkg.context.Context(0)
    yield ctx
    ctx.close()


def view(pkg, orc, k):
    return view_at(pkg, orc, PATH[k])


def prev_cam(pkg, k):
    return pkg.scene.prev_camera(PATH[max(k - 1, 0)], VIEW_TARGET, W, H)


@pytest.fixture(scope="module")
def chain(pkg, orc):
    """Per tick: render, ids, vpx_reproject_moments and, on the same inputs, vpx_reproject_ids, queued
    on one user stream and read at the end.  Returns per tick numpy (acc, ids, hist, mom, plain hist, rgb8)."""
    descs = [view(pkg, orc, k) for k in range(TICKS)]
    ctx = pkg.context.Context(0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    ctx.load_scene(descs[0])
    new = lambda n, t: [torch.zeros(n, dtype=t, device="cuda") for _ in range(TICKS)]  # noqa: E731
    acc, hist, plain = (new(W * H * 4, torch.float32) for _ in range(3))
    mom, ids, rgb = new(W * H * 2, torch.float32), new(W * H * 4, torch.int32), new(W * H, torch.int32)
    torch.cuda.synchronize()
    before = ctx.counters(reset=True).as_dict()
    with torch.cuda.stream(s):
        for k, d in enumerate(descs):
            ctx.set_camera(d.camera)
            p = tick_params(d, k)
            ctx.render(p, acc[k].data_ptr(), None)
            ctx._chk(ctx.lib.vpx_render_ids(ctx.h, C.byref(p), None, C.c_void_p(ids[k].data_ptr())), "vpx_render_ids")
            if k == TICKS - 1:
                ctx.synchronize()
                before = ctx.counters().as_dict()
            a = (p, ids[k], ids[k - 1] if k else None, acc[k], hist[k - 1] if k else None)
            ctx.reproject_moments(*a, mom[k - 1] if k else None, d.camera, prev_cam(pkg, k), out=hist[k], mom_out=mom[k],
                                  nohist=NOHIST, rgb_ptr=rgb[k].data_ptr())
            ctx.reproject(*a, d.camera, prev_cam(pkg, k), out=plain[k], nohist=NOHIST)
    ctx.synchronize()
    assert ctx.counters().as_dict() == before, "nothing added to the work counters"
    out = [(acc[k].cpu().numpy().reshape(H, W, 4), ids[k].cpu().numpy().view(np.uint32).reshape(H, W, 4),
            hist[k].cpu().numpy().reshape(H, W, 4), mom[k].cpu().numpy().reshape(H, W, 2),
            plain[k].cpu().numpy().reshape(H, W, 4), rgb[k].cpu().numpy().view(np.uint32).reshape(H, W)) for k in range(TICKS)]
    ctx.close()
    return out


@pytest.fixture(scope="module")
def host_chain(pkg, chain):
    """The same ticks through the host twins, from the device's samples and ids: per tick (hist, mom, rgb8)."""
    res = []
    for k, (acc, ids, _, _, _, _) in enumerate(chain):
        cam = pkg.scene.look_at(PATH[k], VIEW_TARGET, W, H)
        res.append(pkg.context.reproject_moments_host(W, H, ids, chain[k - 1][1] if k else None, acc, res[-1][0] if k else None,
                                                      res[-1][1] if k else None, cam, prev_cam(pkg, k), nohist=NOHIST, rgb=True))
    return res


def arms_of_the_last_tick(chain, host_chain):
    """(valid-key mask, temporal-arm mask) of the last tick's filter, from the host pipeline's history."""
    valid = denoise_ref.keys(chain[-1][1])[1] != 0
    return valid, valid & (host_chain[-1][0][..., 3] >= MIN_HISTORY)


def test_the_path_covers_both_arms(chain, host_chain):
    valid, temporal = arms_of_the_last_tick(chain, host_chain)
    spatial = valid & ~temporal
    lengths = host_chain[-1][0][..., 3]
    print("pixels", W * H, "valid", int(valid.sum()), "temporal", int(temporal.sum()), "spatial", int(spatial.sum()),
          "lengths", np.bincount(lengths.astype(np.int64).reshape(-1)).tolist())
    assert int(temporal.sum()) * 4 >= W * H, "a quarter of the pixels take the temporal arm"
    assert int(spatial.sum()) * 100 >= W * H, "1 % take the spatial arm under a valid key"


def test_device_chain_equals_reproject_ids_and_the_host_twin(pkg, chain, host_chain):
    for k in range(TICKS):
        acc, ids, hist, mom, plain, rgb = chain[k]
        assert np.array_equal(u32(hist), u32(plain)), f"tick {k}: hist_out is vpx_reproject_ids'"
        same_bits(hist, host_chain[k][0], f"tick {k}: history vs host")
        same_bits(mom, host_chain[k][1], f"tick {k}: moments vs host")
        assert np.array_equal(rgb, host_chain[k][2]), f"tick {k}: rgb8"
    lum0 = denoise_ref.lum(chain[0][0])
    assert np.array_equal(u32(chain[0][3][..., 0]), u32(lum0)), "tick 0: the sample's own luminance"
    m1, m2 = chain[-1][3][..., 0].astype(np.float64), chain[-1][3][..., 1].astype(np.float64)
    kept = chain[-1][2][..., 3] >= 4.0
    assert kept.sum() >= 100 and ((m2 - m1 * m1)[kept] > 0).sum() * 2 >= kept.sum(), "one sample per pixel does vary"


def test_renderer_variance_mode_equals_the_host_pipeline(pkg, orc, chain, host_chain):
    r = pkg.renderer.Renderer(view(pkg, orc, 0), 0, temporal=dict(nohist=NOHIST, variance=VARIANCE)).Init()
    assert r.temporal["variance"] == VARIANCE and r.temporal["denoise"] is None
    for k in range(TICKS):
        r.LookAt(PATH[k], VIEW_TARGET)
        r.Tick(0.0)
        acc, ids = chain[k][0], chain[k][1]
        same_bits(r.accumulator_host(), acc, f"tick {k}: samples")
        assert np.array_equal(r.ids.cpu().numpy().view(np.uint32).reshape(H, W, 4), ids)
        hist, mom, _ = host_chain[k]
        same_bits(r.temporal_history_host(), hist, f"tick {k}: history")
        same_bits(r.temporal_moments_host(), mom, f"tick {k}: moments")
        want, want_rgb = pkg.context.denoise_var_host(W, H, ids, hist, mom, rgb=True, **VARIANCE)
        same_bits(r.denoised_host(), want, f"tick {k}: denoised")
        assert np.array_equal(r.screen_host(), want_rgb), f"tick {k}: screen"
    valid, temporal = arms_of_the_last_tick(chain, host_chain)
    assert int(temporal.sum()) * 4 >= W * H and int((valid & ~temporal).sum()) * 100 >= W * H
    plain = pkg.context.denoise_host(W, H, ids, hist, 5, 0.0)
    assert not np.array_equal(u32(plain), u32(want)), "not the plane-key filter's result"
    r.ResetTemporal()
    r.Tick(0.0)
    assert (r.temporal_history_host()[..., 3] == 1.0).all()
    lq = denoise_ref.lum(r.accumulator_host())
    assert np.array_equal(u32(r.temporal_moments_host()[..., 0]), u32(lq)), "the moments are dropped with the history"
    r.ctx.close()


# ------------------------------------------------------------------- the synthetic cases
def device_moments(pkg, ctx, c, mom_in, rgb=False, **kw):
    w, h = c["w"], c["h"]
    cam, prev = tri.cameras(pkg, c)
    d = {k: on_device(c[k]) for k in ("ids_cur", "ids_prev", "cur", "hist_in")}
    d_mom = on_device(mom_in)
    d_rgb = torch.zeros(w * h, dtype=torch.int32, device="cuda") if rgb else None
    torch.cuda.synchronize()
    out, mom = ctx.reproject_moments(size_params(pkg, w, h), d["ids_cur"], d["ids_prev"], d["cur"], d["hist_in"], d_mom, cam, prev,
                                     rgb_ptr=d_rgb.data_ptr() if rgb else None, **kw)
    ctx.synchronize()
    for k, v in d.items():
        assert np.array_equal(u32(v.cpu().numpy()).reshape(-1), u32(c[k]).reshape(-1)), "the inputs are read only"
    assert np.array_equal(u32(d_mom.cpu().numpy()).reshape(-1), u32(mom_in).reshape(-1))
    res = (out.cpu().numpy().reshape(h, w, 4), mom.cpu().numpy().reshape(h, w, 2))
    return res + (d_rgb.cpu().numpy().view(np.uint32).reshape(h, w),) if rgb else res


@pytest.mark.parametrize("size", ((67, 35), (33, 17), (1, 1)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", ("translation", "dolly"))
def test_synthetic_cases(pkg, bare, pair, size):
    w, h = size
    c = tri.case(pair, w, h)
    mom_in = moments_for(c, 0)
    got, mom, rgb = device_moments(pkg, bare, c, mom_in, rgb=True)
    want_hist, want_mom, _ = reproject_moments_ref.run(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], mom_in, c["cam"],
                                                       c["prev"])
    same_bits(got, want_hist, (pair, size))
    same_bits(mom, want_mom, (pair, size, "moments"))
    host = pkg.context.reproject_moments_host(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], mom_in,
                                              *tri.cameras(pkg, c), rgb=True)
    same_bits(mom, host[1], (pair, size, "host"))
    assert np.array_equal(rgb, host[2])
    plain = device_moments(pkg, bare, c, mom_in)
    same_bits(plain[1], mom, "with and without rgb8")


def test_synthetic_moving_volume(pkg, bare):
    w, h = 33, 17
    c = tri.moving_case(w, h)
    mom_in = moments_for(c, 1)
    cv, pv = tri.moving_volumes(c, "moved")
    got, mom = device_moments(pkg, bare, c, mom_in, cur_volumes=cv, prev_volumes=pv)
    want_hist, want_mom, _ = reproject_moments_ref.run(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], mom_in, c["cam"],
                                                       c["prev"], 32, (1, 0), c["cur_ref"], c["prev_ref"])
    same_bits(got, want_hist, "moving volume")
    same_bits(mom, want_mom, "moving volume, moments")


def test_refusals(pkg, bare):
    c = tri.case("translation", 67, 35)
    bufs = [on_device(c[k]) for k in ("ids_cur", "ids_prev", "cur", "hist_in")] + [on_device(moments_for(c, 0))]
    bufs += [torch.zeros(W * H * 4, dtype=torch.float32, device="cuda"), torch.zeros(W * H * 2, dtype=torch.float32, device="cuda")]
    torch.cuda.synchronize()
    lib, h = bare.lib, bare.h
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def call(w, hh, ic, ip, cu, hi, mi, ho, mo, r, cv, pv):
        return lib.vpx_reproject_moments(h, C.byref(size_params(pkg, w, hh)), ptr(ic), ptr(ip), ptr(cu), ptr(hi), ptr(mi), ptr(ho),
                                         ptr(mo), None, C.byref(r) if r is not None else None, cv, pv)

    reproject_moments_refusals(pkg, call, c, bufs)
    bare.synchronize()
    same_bits(bufs[5].cpu().numpy().reshape(H, W, 4), tri.reference("translation", 67, 35)[0], "the normal call after the refusals")


# ------------------------------------------------------------------- the C++ mirror
def test_cpp_mirror_variance_mode(pkg, tmp_path):
    """host/vpx_demo in mode 'tv' (Renderer::temporalVariance with its defaults, a step along a path
    per tick) shows the screen of the Python Renderer's variance mode over the same four ticks."""
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(pkg.__file__), "host", "vpx_demo")
    if not os.path.exists(exe):
        pytest.fail("host/vpx_demo missing: run __graft_entry__.build()")
    n, w, h, ticks, depth = 64, 96, 64, 4, 1
    out = tmp_path / "frame.rgb8"
    run = subprocess.run([exe, str(n), str(w), str(h), str(ticks), str(depth), str(out), "tv"], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr
    desc = pkg.scene.pillars_scene(n, w, h, depth)
    f = np.float32
    pos, tgt = [f(v) for v in desc._cam_pos], desc._cam_target
    r = pkg.renderer.Renderer(desc, 0, temporal=dict(nohist=NOHIST, variance=True)).Init()
    assert r.temporal["variance"] == dict(sigma_v=4.0, epsilon=2.0 ** -10, min_history=4, passes=5)
    for k in range(ticks):
        if k:  # the demo's float arithmetic: pos + step * k
            r.LookAt((float(pos[0] + f(0.01) * f(k)), float(pos[1] + f(0.004) * f(k)), float(pos[2] - f(0.008) * f(k))), tgt)
        r.Tick(0.0)
    lengths = r.temporal_history_host()[..., 3]
    valid = denoise_ref.keys(r.ids.cpu().numpy().view(np.uint32).reshape(h, w, 4))[1] != 0
    print("valid keys", int(valid.sum()), "of", w * h, "temporal arm", int((valid & (lengths >= 4.0)).sum()))
    assert (valid & (lengths >= 4.0)).sum() * 4 >= valid.sum() >= 500 and (valid & (lengths < 4.0)).any()
    assert np.array_equal(np.fromfile(out, np.uint32), r.screen_host().reshape(-1))
    r.ctx.close()
