"""The device's moving-camera frame against tests/frame_head_ref.py — no oracle on this side.

Tier A: whole frames.  head -> numpy Trace (test_kat_paths.Scene) -> blend_ref -> tonemap_ref, the
expected values tests/test_kat_frame.py also holds oracle_render to, equal vpx_render's accumulator
and RGB8: the two 19x13 scenes at depth 0 and 2 over three accumulated AA+DOF frames, the forced
edge draws on a 1x1 frame, and vpx_focus_distance on the five focus cases.
The head cases at the parameter ends (K.head_cases, inside the closed lit box) and the two parting-
pixel sets (fma against mul + add, (p * jitter) / W against p * (jitter / W)) are compared as raw
samples (VPX_FLAG_NO_TONEMAP) with head() composed with vpx_trace.

Tier B: the head in every kernel that computes it.  The expected sample of a pixel is head() composed
with the device's own vpx_trace(origin, direction, state) — the entry test_kat_paths_on_device and
test_kat_lights_gpu pin to the numpy Trace — folded with epilogue_ref.blend_ref; for the "spot" and
"area3" forms the composed samples are held to the numpy Trace as well.  Forms as tests/test_epilogue_gpu.py's FORMS, each confirmed on
the serial vpx_render with vpx_debug_last_frame_kernel and vpx_profile_read; a 37x21 frame (partial
right and bottom tiles), frames 0..2 (and 2..4 for the second window), through vpx_render with 0 and
2 lanes, vpx_render_tiles_accum for every rank of 1, 2 and 3, vpx_render_window, and vpx_render /
vpx_render_window on the device set [0, 0].  All forms run AA + DOF except "lean": k_frame0's lean
view is launched only without the thin lens (frame0_lean), so the head it computes is the AA one;
the AA + DOF head inside k_frame0 is the "spot" form's.
One large form: a 2048x2048 window of 4 frames on 2 lanes with an area light (the k_finish_window
chain), checked on a sample of pixels: corners, both sides of tile seams, the last row and column.

Comparisons are epilogue_ref.compare (accumulator lanes bit-equal, a NaN's sign and payload apart;
RGB8 equal), in exact arithmetic (VPX_ARITH_EXACT).
"""
import numpy as np
import pytest

import epilogue_ref as E
import frame_head_ref as F
import test_kat_frame as K
from test_epilogue_gpu import KINDS, check_form
from test_kat_paths import N, Vol, api_rays, fbits, kat_scene, to_oracle

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning",
                                                          "ignore:invalid value:RuntimeWarning")]

AA, DOF, SKY = K.AA, K.DOF, K.SKY
_CACHE = {}


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dev(words):
    return _torch().from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32).reshape(-1).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


def open_ctx(pkg, desc, cam, lanes=0, devices=None):
    ctx = pkg.context.Context(0, devices=devices)
    ctx.load_scene(desc)
    ctx.set_camera(cam)
    ctx.set_arithmetic(pkg.abi.VPX_ARITH_EXACT)
    ctx.set_pipeline(lanes)
    return ctx


def expect(got_acc, got_rgb, want_acc, want_rgb, what):
    ga = np.asarray(got_acc).reshape(-1, 4)
    bad, left_out = E.compare(ga, got_rgb, want_acc, want_rgb)
    assert left_out == 0, what
    if bad:
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(ga)} pixels differ; first at {i}: got "
                             f"{[hex(int(v)) for v in ga[i]]} want {[hex(int(v)) for v in np.asarray(want_acc)[i]]}"
                             + ("" if got_rgb is None else f" rgb got {int(got_rgb[i]):#x} want {int(want_rgb[i]):#x}"))


def render_frames(ctx, params, pixels):
    """vpx_render over `params` from a zero accumulator: (accumulator bits, RGB8) after each frame."""
    d_acc, d_rgb = dev(np.zeros(pixels * 4, np.uint32)), dev(np.zeros(pixels, np.uint32))
    _torch().cuda.synchronize()
    out = []
    for p in params:
        ctx.render(p, d_acc.data_ptr(), d_rgb.data_ptr())
        ctx.synchronize()
        out.append((host(d_acc).reshape(-1, 4), host(d_rgb)))
    return out


# ------------------------------------------------------------------ tier A
@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("which", list(K.FRAME_SCENES))
def test_whole_frames_equal_the_restatement(pkg, abi, which, depth):
    """vpx_render, three accumulated 19x13 AA+DOF frames: accumulator and RGB8 after every frame
    equal head -> numpy Trace -> blend_ref -> tonemap_ref."""
    _torch()
    desc, cam, frames, refused = K.expected_frames(pkg, abi, which, depth)
    assert len(refused) == 0 and len(frames) == 3, refused
    ctx = open_ctx(pkg, desc, cam)
    params = [K.frame_params(abi, K.FRAME_W, K.FRAME_H, f, 0, AA | DOF, 1.0, depth, K.frame_samples(which)) for f in range(3)]
    got = render_frames(ctx, params, K.FRAME_W * K.FRAME_H)
    ctx.close()
    for f, ((acc, rgb), (want_acc, want_rgb, *_)) in enumerate(zip(got, frames)):
        expect(acc, rgb, want_acc, want_rgb, f"{which} depth {depth} frame {f}")


@pytest.mark.parametrize("name", list(K.FORCED))
def test_forced_draws(pkg, abi, name):
    """The edge draws of the pixel stream on a 1x1 AA+DOF frame (K.FORCED through seed_base_for)."""
    _torch()
    desc, (cells, mats, points, d, vols) = K.forced_scene(pkg, name)
    cam = K.camera(pkg, 1, 1, cam=K.FORCED_CAM, **K.FORCED_LENS)
    p = K.forced_params(abi, name)
    assert F.pixel_seed(p.seed_base, 0, 1, 1, 0, 0) == K.FORCED[name]
    want_acc, want_rgb = F.frame(K.Scene(vols, mats, points, d, sky=SKY), cam, p, np.zeros((1, 4), np.uint32))
    ctx = open_ctx(pkg, desc, cam)
    (acc, rgb), = render_frames(ctx, [p], 1)
    ctx.close()
    expect(acc, rgb, want_acc, want_rgb, name)


def raw_samples(ctx, abi, cases, form):
    """The listed pixels' raw samples (VPX_FLAG_NO_TONEMAP) from vpx_render, frame by frame; every
    frame must run k_frame0 in `form`."""
    w, h = cases[0][0].width, cases[0][0].height
    d_acc = dev(np.zeros(w * h * 4, np.uint32))
    _torch().cuda.synchronize()
    got = []
    for p, ids in cases:
        if ids:
            p.flags |= abi.VPX_FLAG_NO_TONEMAP
            ctx.render(p, d_acc.data_ptr(), None)
            assert ctx.last_frame_kernel() == form
            ctx.synchronize()
            got.append(host(d_acc).reshape(-1, 4)[ids, :3])
    return np.concatenate(got)


def test_aa_jitter_is_one_rounding(pkg, abi):
    """K.jitter_cases on the device: the raw samples of the pixels where fma(rand, aa, x) and
    rand * aa + x land on different floats are the fma reading's, and the other reading's differ on
    enough of them to be told apart (k_frame0's lean form: AA only, depth 0)."""
    _torch()
    desc, cam = K.jitter_scene(pkg)
    cases = K.jitter_cases(abi)
    ctx = open_ctx(pkg, desc, cam)
    one, two = K.jitter_readings(lambda rays, seeds, d: ctx.trace(rays, seeds, d, SKY, 3), abi, cam, cases)
    got = raw_samples(ctx, abi, cases, 2)
    ctx.close()
    K.parted(got, one, two, "jitter on the device")


def test_lens_divides_the_product(pkg, abi):
    """K.lens_cases on the device: where (p * defocusJitter) / W and p * (defocusJitter / W) give
    different lens offsets the raw samples are the former's (k_frame0's guaranteed form: DOF)."""
    _torch()
    desc, cam = K.lens_scene(pkg)
    cases = K.lens_cases(abi)
    ctx = open_ctx(pkg, desc, cam)
    one, two = K.lens_readings(lambda rays, seeds, d: ctx.trace(rays, seeds, d, SKY, 3), abi, cam, cases)
    got = raw_samples(ctx, abi, cases, 1)
    ctx.close()
    K.parted(got, one, two, "lens on the device")


def test_head_at_the_parameter_ends(pkg, abi):
    """K.head_cases on the device, inside K.box_scene as on the CPU: the raw samples of vpx_render
    (VPX_FLAG_NO_TONEMAP) equal head() -> vpx_trace on every pixel of the seven sizes, the wrapping
    seeds and the ends of AA strength, defocusJitter and focal distance; no pixel returns the sky."""
    _torch()
    sky = fbits(np.array(SKY, np.float32))
    ctxs = {}
    for W, H, flags, depth, frame, base, aa, jitter, focal in K.head_cases():
        scale = K.box_scale(jitter, W) if flags & DOF else 1.0
        cam = K.camera(pkg, W, H, focal, jitter, cam=K.BOX_CAM)
        if scale not in ctxs:
            ctxs[scale] = open_ctx(pkg, K.box_scene(pkg, scale)[0], cam)
        ctx = ctxs[scale]
        ctx.set_camera(cam)
        p = K.frame_params(abi, W, H, frame, base, flags, aa, depth)
        want, refused = K.head_through(lambda rays, seeds, d: ctx.trace(rays, seeds, d, SKY, 3), abi, cam, p)
        assert not refused
        p.flags |= abi.VPX_FLAG_NO_TONEMAP
        d_acc = dev(np.zeros(W * H * 4, np.uint32))
        _torch().cuda.synchronize()
        ctx.render(p, d_acc.data_ptr(), None)
        ctx.synchronize()
        got = host(d_acc).reshape(-1, 4)[:, :3]
        case = (W, H, flags, depth, frame, base, aa, jitter, focal)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (case, bad[:8], got[bad[0]], want[bad[0]])
        assert not (got == sky[None, :]).all(axis=1).any(), case
    for ctx in ctxs.values():
        ctx.close()


@pytest.mark.parametrize("name", K.FOCUS_NAMES)
def test_focus_distance(pkg, abi, name):
    _torch()
    desc, cam, W, H, want = K.focus_expected(pkg, name)
    ctx = open_ctx(pkg, desc, cam)
    got = np.float32(ctx.focus_distance(W, H))
    ctx.close()
    assert fbits(got) == fbits(want), (name, got, want)


# ------------------------------------------------------------------ tier B
W, H = 37, 21
PIX = W * H
LENS = dict(focal=1.3, jitter=2.0)
DEPTH = {"depth2": 2, "depth8": 8}


def flags_of(kind):
    return AA if kind == "lean" else AA | DOF


def kind_scene(pkg, kind):
    """The KAT room with what the kind's kernel needs: a spot light, an area light, a second
    (scaled, rotated) volume."""
    def make():
        sc, abi = pkg.scene, pkg.abi
        cells, mats, points, d = kat_scene(0)
        desc = to_oracle(pkg, None, cells, mats, points, d, [Vol(cells, N)])
        desc.width, desc.height, desc.max_bounces, desc.area_samples = W, H, DEPTH.get(kind, 0), 3
        if kind == "spot":
            desc.spots = [sc.spot_light((0.5, 0.6, -0.5), (0.0, -0.2, 1.0))]
        if kind == "area3":
            desc.areas = [sc.area_light((0.3, 0.8, -0.6), radius=0.3)]
        if kind == "two volumes":
            second = sc.volume(position=(0.55, 0.15, 0.1), scale=(0.5, 0.5, 0.5), rotation=(0.0, 0.4, 0.1))
            desc.volumes = (abi.Volume * 2)(desc.volumes[0], second)
        return desc
    return cached(("scene", kind), make)


def tb_camera(pkg, w=W, h=H):
    return K.camera(pkg, w, h, **LENS)


def tb_params(abi, kind, frame, w=W, h=H):
    p = K.frame_params(abi, w, h, frame, 0, flags_of(kind), 1.0, DEPTH.get(kind, 0))
    p.area_samples = 3
    return p


def heads(pkg, abi, flags, frame, w=W, h=H, pixels=None):
    """head() for the pixels (all by default) of a frame: (abi.Ray array, states); cached, as it depends
    on the camera, the flags and the frame only."""
    def make():
        cam = F.Cam(tb_camera(pkg, w, h))
        p = K.frame_params(abi, w, h, frame, 0, flags, 1.0, 0)
        rays, seeds = [], []
        for i in (range(w * h) if pixels is None else pixels):
            o, d, s = F.head(cam, p, int(i) % w, int(i) // w)  # a refusal (cr32_f64) raises: none is skipped
            rays.append((o, d, 1e34, False))
            seeds.append(s)
        return api_rays(abi, rays), np.array(seeds, np.uint32)
    return cached(("heads", flags, frame, w, h, None if pixels is None else tuple(pixels)), make)


def samples(pkg, abi, kind, frame):
    """head() composed with vpx_trace for every pixel: bits [PIX, 3]."""
    def make():
        ctx = open_ctx(pkg, kind_scene(pkg, kind), tb_camera(pkg))
        out = {}
        for f in range(5):
            rays, seeds = heads(pkg, abi, flags_of(kind), f)
            out[f] = np.ascontiguousarray(ctx.trace(rays, seeds, DEPTH.get(kind, 0), SKY, 3), np.float32).view(np.uint32)
        ctx.close()
        return out
    return cached(("samples", kind), make)[frame]


def folded(pkg, abi, kind, first, count=3):
    """Frames first .. first + count - 1 blended in order from a zero accumulator: (acc bits, RGB8)."""
    def make():
        acc = np.zeros((PIX, 4), np.uint32)
        for f in range(first, first + count):
            acc, rgb = E.reference(samples(pkg, abi, kind, f), acc, f)
        return acc, rgb
    return cached(("folded", kind, first, count), make)


@pytest.mark.parametrize("kind", ["spot", "area3"])
def test_composed_samples_equal_the_numpy_trace(pkg, abi, kind):
    """The expected samples of the "spot" and "area3" forms, head() composed with the device's
    vpx_trace, are also the numpy Trace's (frame 0): the lights of those scenes are ones
    test_kat_paths.Scene.illumination restates, read back here from the scene the device was given."""
    _torch()
    desc = kind_scene(pkg, kind)
    cells, mats, points, d = kat_scene(0)
    spots = [(tuple(s.position), tuple(s.direction), tuple(s.color), s.angle) for s in desc.spots]
    areas = [(tuple(a.position), tuple(a.color), a.color_multiplier, a.radius) for a in desc.areas]
    assert len(spots) + len(areas) == 1
    s = K.Scene([Vol(cells, N)], mats, points, d, sky=SKY, spots=spots, areas=areas)
    want = F.samples(s, tb_camera(pkg), tb_params(abi, kind, 0))
    got = samples(pkg, abi, kind, 0)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (kind, bad[:8], got[bad[0]], want[bad[0]])
    assert {p[0] for p in s.picks} == {"point", "spot" if spots else "area", "directional"}


@pytest.mark.parametrize("lanes", [0, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_head_in_vpx_render(pkg, abi, kind, lanes):
    """vpx_render, frames 0..2; on the serial context the kernel that ran is confirmed per frame."""
    _torch()
    want = folded(pkg, abi, kind, 0)
    hit = (samples(pkg, abi, kind, 0) != fbits(np.array(SKY, np.float32))[None, :]).any(axis=1)
    assert PIX // 8 <= hit.sum() <= PIX - PIX // 8, (kind, int(hit.sum()))  # hits and misses: the head matters
    ctx = open_ctx(pkg, kind_scene(pkg, kind), tb_camera(pkg), lanes)
    if lanes == 0:
        ctx.profile_enable(4096)
    d_acc, d_rgb = dev(np.zeros(PIX * 4, np.uint32)), dev(np.zeros(PIX, np.uint32))
    _torch().cuda.synchronize()
    for f in range(3):
        if lanes == 0:
            ctx.profile_read(reset=True)
        ctx.render(tb_params(abi, kind, f), d_acc.data_ptr(), d_rgb.data_ptr())
        if lanes == 0:
            form = ctx.last_frame_kernel()
            check_form(kind, form, {k: v[1] for k, v in ctx.profile_read(reset=True).items()}, f"{kind} frame {f}")
    ctx.synchronize()
    acc, rgb = host(d_acc), host(d_rgb)
    ctx.close()
    expect(acc, rgb, want[0], want[1], f"vpx_render {kind} lanes={lanes}")


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_head_in_render_tiles_accum(pkg, abi, kind, R):
    """vpx_render_tiles_accum, every rank of R, frames 0..2 into the rank's packed accumulator; the
    slots mapped to pixels with epilogue_ref.slot_pixels, padding slots 0 / 0."""
    torch = _torch()
    want_acc, want_rgb = folded(pkg, abi, kind, 0)
    L, slots = E.slot_pixels(W, H, R)
    ctx = open_ctx(pkg, kind_scene(pkg, kind), tb_camera(pkg))
    accs, rgbs = [], []
    for rank in range(R):
        d_acc, d_rgb = dev(np.zeros(L * 4, np.uint32)), dev(np.full(L, 0xDEADBEEF, np.uint32))
        torch.cuda.synchronize()
        for f in range(3):
            ctx.render_tiles_accum(tb_params(abi, kind, f), rank, R, d_acc.data_ptr(), d_rgb.data_ptr())
        ctx.synchronize()
        accs.append(host(d_acc).reshape(-1, 4))
        rgbs.append(host(d_rgb))
    ctx.close()
    acc, rgb = np.concatenate(accs), np.concatenate(rgbs)
    ok = slots >= 0
    assert sorted(slots[ok].tolist()) == list(range(PIX))
    wa, wr = np.zeros_like(acc), np.zeros(len(slots), np.uint32)
    wa[ok], wr[ok] = want_acc[slots[ok]], want_rgb[slots[ok]]
    expect(acc, rgb, wa, wr, f"vpx_render_tiles_accum {kind} R={R}")


@pytest.mark.parametrize("first,lanes", [(0, 0), (0, 2), (2, 0)])
@pytest.mark.parametrize("kind", KINDS)
def test_head_in_render_window(pkg, abi, kind, first, lanes):
    """vpx_render_window, 3 frames from frame_index 0 and from 2: the chain renders frame b in tile
    blocks [b * T, (b + 1) * T) (batch_tiles) and one blend folds them in frame order."""
    _torch()
    want = folded(pkg, abi, kind, first)
    ctx = open_ctx(pkg, kind_scene(pkg, kind), tb_camera(pkg), lanes)
    d_acc, d_rgb = dev(np.zeros(PIX * 4, np.uint32)), dev(np.zeros(PIX, np.uint32))
    _torch().cuda.synchronize()
    ctx.render_window(tb_params(abi, kind, first), 3, d_acc.data_ptr(), d_rgb.data_ptr())
    ctx.synchronize()
    acc, rgb = host(d_acc), host(d_rgb)
    ctx.close()
    expect(acc, rgb, want[0], want[1], f"vpx_render_window {kind} first={first} lanes={lanes}")


@pytest.mark.parametrize("entry", ["render", "window", "window rgb8 only"])
@pytest.mark.parametrize("kind", KINDS)
def test_head_on_a_device_set(pkg, abi, kind, entry):
    """The device set [0, 0] (tiles dealt to two members, gathered by device copies): vpx_render frame
    by frame, vpx_render_window of the three frames — a set keeps its camera in its members, so the
    window has to reach them before any check of the set's own state — and the window with accum
    NULL (the members' sharded accumulators, reset by frame_index 0; only RGB8 comes back)."""
    _torch()
    want = folded(pkg, abi, kind, 0)
    ctx = open_ctx(pkg, kind_scene(pkg, kind), tb_camera(pkg), devices=[0, 0])
    d_acc, d_rgb = dev(np.zeros(PIX * 4, np.uint32)), dev(np.zeros(PIX, np.uint32))
    _torch().cuda.synchronize()
    if entry == "render":
        for f in range(3):
            ctx.render(tb_params(abi, kind, f), d_acc.data_ptr(), d_rgb.data_ptr())
    else:
        ctx.render_window(tb_params(abi, kind, 0), 3, d_acc.data_ptr() if entry == "window" else None, d_rgb.data_ptr())
    ctx.synchronize()
    acc, rgb = host(d_acc), host(d_rgb)
    ctx.close()
    if entry == "window rgb8 only":
        assert not acc.any()
        bad = np.flatnonzero(rgb != want[1])
        assert bad.size == 0, (kind, bad[:8], hex(int(rgb[bad[0]])), hex(int(want[1][bad[0]])))
    else:
        expect(acc, rgb, want[0], want[1], f"device set {entry} {kind}")


# ------------------------------------------------------------------ the large window
BIG_W = BIG_H = 2048


def big_pixels():
    """At most 2048 pixel ids of the 2048x2048 frame: the corners, both sides of 16-pixel tile seams
    (and of the 8-pixel quadrant seams inside a tile) along two rows and two columns, the last row and
    column, the rest random with a fixed seed."""
    w, h = BIG_W, BIG_H
    px = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)}
    for s in (8, 16, 1024, 1040, 2032, 2040):
        for o in (s - 1, s):
            px |= {(o, 0), (o, 777), (0, o), (1500, o), (o, o)}
    rng = np.random.default_rng(20240613)
    px |= {(int(x), h - 1) for x in rng.integers(0, w, 24)} | {(w - 1, int(y)) for y in rng.integers(0, h, 24)}
    while len(px) < 1024:
        px.add((int(rng.integers(0, w)), int(rng.integers(0, h))))
    return sorted(y * w + x for x, y in px)


def test_big_window_chain(pkg, abi):
    """vpx_render_window of 4 frames at 2048x2048 on 2 lanes with an area light: chains of two frames
    whose own tail resolves and blends (k_finish_window; 16384 tiles a frame).  The sampled pixels'
    accumulators and RGB8 equal head() -> vpx_trace -> blend_ref, the head restated for them only.
    vpx_profile_read confirms the chains (two head and two tail launches for the four frames)."""
    torch = _torch()
    kind = "area3"
    desc = kind_scene(pkg, kind)
    assert (BIG_W // 16) * (BIG_H // 16) >= 16384 and len(desc.areas) == 1
    ids = big_pixels()
    assert len(ids) <= 2048
    cam = tb_camera(pkg, BIG_W, BIG_H)
    ctx = open_ctx(pkg, desc, cam)
    acc = np.zeros((len(ids), 4), np.uint32)
    for f in range(4):
        rays, seeds = heads(pkg, abi, flags_of(kind), f, BIG_W, BIG_H, ids)
        s = np.ascontiguousarray(ctx.trace(rays, seeds, 0, SKY, 3), np.float32).view(np.uint32)
        acc, rgb = E.reference(s, acc, f)
    ctx.close()
    ctx = open_ctx(pkg, desc, cam, lanes=2)
    ctx.profile_enable(256)
    d_acc = torch.zeros(BIG_W * BIG_H * 4, dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros(BIG_W * BIG_H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.profile_read(reset=True)
    ctx.render_window(tb_params(abi, kind, 0, BIG_W, BIG_H), 4, d_acc.data_ptr(), d_rgb.data_ptr())
    ctx.synchronize()
    # two chains of two frames, each one head and one tail launch, and no one-launch frame: what
    # vpx_profile_read can show.  It counts k_finish_window and k_resolve_finish under the same stage,
    # so which of the two tails ran rests on the launch condition the asserts above restate.
    launches = {k: v[1] for k, v in ctx.profile_read(reset=True).items()}
    assert (launches["primary"], launches["finish"], launches["frame"]) == (2, 2, 0), launches
    sel = torch.as_tensor(ids, device="cuda")
    got_acc, got_rgb = host(d_acc.view(-1, 4)[sel]), host(d_rgb[sel])
    ctx.close()
    expect(got_acc, got_rgb, acc, rgb, "2048x2048 window, 2 lanes, area light")
