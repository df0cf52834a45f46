"""The head of Renderer::Update and the focus ray of Tick: the oracle against tests/frame_head_ref.py.

oracle_render_pixels / oracle_render / oracle_focus_distance are compared bit for bit with the numpy
restatement of the frame head (seed, AA fma, thin lens, draw order) — composed with oracle_trace
where only the head is under test, and with test_kat_paths' numpy Trace and epilogue_ref's blend and
tonemap for whole frames, where no oracle code takes part in the expected value.  The GPU side
(tests/test_kat_frame_gpu.py) compares the device with the same expected values.

cr32_f64 refuses a sin / cos argument whose float32 rounding a 1-ulp double error could flip; a
refused pixel is counted, never skipped, and every test asserts a count of 0.
"""
import numpy as np
import pytest

import epilogue_ref as E
import frame_head_ref as F
import test_kat_lights as L
from test_kat_paths import N, NONE, Rng, Scene, Vol, _messy_volume, api_rays, fbits, kat_scene, to_oracle, v3

pytestmark = pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning", "ignore:invalid value:RuntimeWarning")

SKY = (0.392, 0.584, 0.829)
AA, DOF = F.FLAG_AA, F.FLAG_DOF
# The room from outside the cube, off every axis: with right and up along the axes each lane of
# P and of the lens origin has one non-zero term and the order of the two additions could not matter.
CAM = ((0.3, 0.8, -0.9), (0.55, 0.4, 0.5))


def refusing(fn, refused):
    """fn(), or None with the refusal counted (cr32_f64's double-rounding midpoints)."""
    try:
        return fn()
    except AssertionError as e:
        if "double-rounding midpoint" not in str(e):
            raise
        refused.append(str(e))
        return None


def camera(pkg, W, H, focal=1.0, jitter=2.0, cam=CAM):
    c = pkg.scene.look_at(cam[0], cam[1], W, H)
    c.focal_distance, c.defocus_jitter = float(focal), float(jitter)
    return c


def frame_params(abi, W, H, frame=0, seed_base=0, flags=0, aa=1.0, depth=0, samples=3):
    p = abi.FrameParams()
    p.width, p.height, p.max_bounces, p.frame_index, p.seed_base = W, H, depth, frame, seed_base
    p.flags, p.aa_strength, p.area_samples, p.sky = flags, aa, samples, abi.vec3(SKY)
    return p


def room(pkg, vols_of=lambda cells: [Vol(cells, N)], wall=0, lights=None):
    """The KAT room as a SceneDesc and as what Scene takes; lights: a test_kat_lights light set in place
    of the room's point light (the last element then holds the spots and areas for Scene)."""
    cells, mats, points, d = kat_scene(wall)
    vols = vols_of(cells)
    if lights is None:
        return to_oracle(pkg, None, cells, mats, points, d, vols), (cells, mats, points, d, vols)
    kw = L.lights_of(lights)
    points = kw.pop("points")
    return to_oracle(pkg, None, cells, mats, points, d, vols, **kw), (cells, mats, points, d, vols, kw)


def two_volumes(cells):
    return [Vol(cells, N), _messy_volume(cells)]


def head_through(trace, abi, cam, p):
    """Every pixel's sample as head() composed with `trace` (oracle_trace or vpx_trace): bits [W*H, 3]
    and the refusals."""
    refused, rays, seeds = [], [], []
    c = F.Cam(cam)
    for i in range(p.width * p.height):
        h = refusing(lambda: F.head(c, p, i % p.width, i // p.width), refused)
        o, d, s = h if h is not None else (v3(0, 0, 0), v3(0, 0, 1), 1)
        rays.append((o, d, 1e34, False))
        seeds.append(s)
    got = trace(api_rays(abi, rays), np.array(seeds, np.uint32), p.max_bounces)
    return np.ascontiguousarray(got, np.float32).view(np.uint32), refused


def wrap_frame(W, H, seed_base):
    """A frame_index whose frame * (W * H), together with seed_base, passes 2^32."""
    f = min(0xFFFFFFFF, (1 << 32) // (W * H) + 7)
    assert f * W * H + seed_base >= 1 << 32
    return f


# (W, H, flags, depth): the four measured sets, then 1x1, narrower than one 8-wide step, and 1/W exact
SIZES = [(19, 13, AA | DOF, 2), (24, 10, AA, 0), (17, 9, DOF, 0), (33, 7, 0, 0), (1, 1, AA | DOF, 1),
         (5, 3, AA | DOF, 1), (64, 16, AA | DOF, 0)]
AAS, JITTERS, FOCALS = (0.0, 0.37, 1.0), (0.0, 2.0, 50.0), (2.0 ** -10, 1.3, 1e4, -1.0)


def head_cases():
    """Every size at frames 0, 3 and a wrapping one, the parameter values dealt round-robin (each of
    them on at least three frames), then the full cross product of the values on the 5x3 frame.
    These cases see a wrong ray or a wrong state where it moves the hit point by more than the last
    bit or two; they are blind to most single-ulp readings (the jitter as mul + add instead of one fma,
    the lens as p * (defocusJitter / W)): only test_aa_jitter_is_one_rounding and
    test_lens_divides_the_product hold those, and neither is redundant."""
    out, k = [], 0
    for W, H, flags, depth in SIZES:
        for which in range(3):
            base = 0xFFFFFF00 if which == 2 else 977 * k
            frame = (0, 3, wrap_frame(W, H, 0xFFFFFF00))[which]
            aa = 0.37 if (W, H) == (24, 10) else AAS[k % 3]
            out.append((W, H, flags, depth, frame, base, aa, JITTERS[(k // 3 + k) % 3], FOCALS[k % 4]))
            k += 1
    for aa in AAS:
        for j in JITTERS:
            for fd in FOCALS:
                out.append((5, 3, AA | DOF, 0, 1, 12345, aa, j, fd))
    return out


BOX_CAM = ((0.45, 0.55, 0.4), (0.6, 0.45, 0.9))  # inside the box, off its centre and off every axis


def box_scene(pkg, scale=1.0, centre=(0.5, 0.5, 0.5)):
    """A closed box of the default material 20 (a one-cell shell of the 16^3 grid: DiffuseReflection
    and an unconditional Illumination) lit from inside by seven point lights, scaled by `scale` (a
    power of two: the matrices are exact) about its centre, which sits at `centre` in the world.  A
    ray that starts inside never sees the sky, whichever way it points, and its sample depends on
    where it lands.  Returns (desc, volumes)."""
    g = np.full((N, N, N), NONE, np.uint8)
    g[0], g[-1], g[:, 0], g[:, -1], g[:, :, 0], g[:, :, -1] = 20, 20, 20, 20, 20, 20
    cells = g.reshape(-1)
    _, mats, _, d = kat_scene(0)
    S, c = float(scale), np.array(centre, np.float64)
    t = c - 0.5 * S
    m, inv = np.eye(4), np.eye(4)
    m[:3, :3], m[:3, 3] = np.eye(3) * S, t
    inv[:3, :3], inv[:3, 3] = np.eye(3) / S, -t / S
    vols = [Vol(cells, N, matrix=m.reshape(-1).astype(np.float32), inv=inv.reshape(-1).astype(np.float32))]
    points = [(v3(*(t + S * np.array([0.2 + 0.1 * k, 0.85 - 0.1 * k, 0.2 + 0.09 * k]))), v3(1.0, 0.95, 0.9))
              for k in range(7)]
    return to_oracle(pkg, None, cells, mats, points, d, vols), vols


def box_scale(jitter, W):
    """The box scale at which the lens (radius defocusJitter / W) stays inside the box around
    BOX_CAM: 1 up to a radius of 1 / 4, else the power of two that brings it back to that."""
    s = 1.0
    while jitter / W > 0.25 * s:
        s *= 2.0
    return s


def test_head_composed_with_oracle_trace_equals_render_pixels(pkg, orc, abi):
    """oracle_render_pixels == head() -> oracle_trace on every pixel of every case: the seed, the
    AA fma (draws spent at strength 0 too), the lens, the draw order and the state handed to Trace.
    Every case runs inside box_scene, scaled so that the lens stays inside: no pixel of any case —
    a focal distance of -1, which turns the ray round, and the widest lens included — returns the
    constant sky, on which the comparison would hold whatever head() produced, and most are lit."""
    cases = head_cases()
    assert {c[6] for c in cases} >= set(AAS) and {c[7] for c in cases} >= set(JITTERS) and {c[8] for c in cases} >= set(FOCALS)
    oracles = {}
    sky = fbits(np.array(SKY, np.float32))
    refused, pixels = [], 0
    for W, H, flags, depth, frame, base, aa, jitter, focal in cases:
        scale = box_scale(jitter, W) if flags & DOF else 1.0
        if scale not in oracles:
            oracles[scale] = orc.Oracle(abi, box_scene(pkg, scale)[0])
        o = oracles[scale]
        cam = camera(pkg, W, H, focal, jitter, cam=BOX_CAM)
        p = frame_params(abi, W, H, frame, base, flags, aa, depth)
        o.set_camera(cam)
        want, r = head_through(lambda rays, seeds, d: o.trace(rays, seeds, d, SKY, 3)[0], abi, cam, p)
        refused += r
        got, _ = o.render_pixels(p, np.arange(W * H, dtype=np.uint32), threads=2)
        got = np.ascontiguousarray(got[:, :3]).view(np.uint32)
        case = (W, H, flags, depth, frame, base, aa, jitter, focal)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (case, bad[:8], got[bad[0]], want[bad[0]])
        # no sky anywhere; Illumination picks one of the seven point lights 7 times in 8 (the
        # directional light never reaches the inside), so ask for half the pixels lit where there
        # are enough pixels for that to be a fair demand
        assert not (got == sky[None, :]).all(axis=1).any(), case
        lit = (got != 0).any(axis=1).sum()
        assert lit >= (W * H) // 2 or W * H < 15, (case, int(lit))
        pixels += W * H
    assert len(refused) == 0, refused[:3]
    assert pixels >= 1742


# ------------------------------------------------------------------ one rounding or two
JITTER_W = JITTER_H = 2
JITTER_FRAMES = 160
JITTER_AA = 0.37


def mul_add32(a, b, c):
    """a * b + c rounded twice: NOT the reference's jitter."""
    return np.float32(np.float32(a * b) + c)


def lens_scaled(p, jitter, W):
    """p * (defocusJitter / SCRWIDTH): NOT camera.h:75's operand order."""
    return np.float32(p * np.float32(jitter / np.float32(W)))


class reading:
    """`with reading("fma32", mul_add32):` — head() under another reading of one of its steps."""

    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def __enter__(self):
        self.kept = getattr(F, self.name)
        setattr(F, self.name, self.fn)

    def __exit__(self, *a):
        setattr(F, self.name, self.kept)


def jitter_cases(abi):
    """The frames of a 2x2 AA frame (strength 0.37) and, of their pixels, those where the jitter
    rounded twice (mul, then add) lands on another float than the fma: x or y is 1 there, so the sum's
    ulp is 2^-23 against the product's 2^-25 or less, and about one pixel in six parts the readings —
    where whole frames part them once in several hundred pixels, and then only if the ulp survives
    to the sample.  Returns [(params, [pixel ids])]."""
    out = []
    for f in range(JITTER_FRAMES):
        p = frame_params(abi, JITTER_W, JITTER_H, f, 0, AA, JITTER_AA, 0)
        ids = []
        for i in range(JITTER_W * JITTER_H):
            x, y = i % JITTER_W, i // JITTER_W
            g = Rng(F.pixel_seed(0, f, JITTER_W, JITTER_H, x, y))
            rx, ry, aa = g.rf(), g.rf(), np.float32(JITTER_AA)
            if F.fma32(rx, aa, x) != mul_add32(rx, aa, np.float32(x)) or F.fma32(ry, aa, y) != mul_add32(ry, aa, np.float32(y)):
                ids.append(i)
        out.append((p, ids))
    return out


def jitter_scene(pkg):
    """box_scene centred on the world's origin, where the camera stands (as lens_scene): the direction
    P - camPos is P itself, so the last bit of the jittered coordinate is not rounded away on the way to
    the ray, and every pixel's sample depends on its hit point."""
    return box_scene(pkg, 1.0, (0.0, 0.0, 0.0))[0], camera(pkg, JITTER_W, JITTER_H, cam=LENS_CAM, **FORCED_LENS)


def two_readings(trace, abi, cam, cases, name, other):
    """The listed pixels' samples, head() composed with `trace`, as the restatement reads step `name`
    and under the `other` reading of it: (bits, bits)."""
    c = F.Cam(cam)
    out = []
    for fn in (getattr(F, name), other):
        rays, seeds = [], []
        with reading(name, fn):
            for p, ids in cases:
                for i in ids:
                    o, d, s = F.head(c, p, i % p.width, i // p.width)
                    rays.append((o, d, 1e34, False))
                    seeds.append(s)
        out.append(np.ascontiguousarray(trace(api_rays(abi, rays), np.array(seeds, np.uint32), 0), np.float32).view(np.uint32))
    return out


def jitter_readings(trace, abi, cam, cases):
    return two_readings(trace, abi, cam, cases, "fma32", mul_add32)


def parted(got, one, two, what):
    """The samples are the restatement's reading's, and the other reading's differ on enough of the
    parting pixels (one would tell them apart; a tenth is asked for) that the wrong one could not pass."""
    print(what, "parting pixels", len(one), "samples that differ", int((one != two).any(axis=1).sum()))
    assert np.array_equal(got, one), what
    assert len(one) >= 40 and (got != two).any(axis=1).sum() >= len(one) // 10, what


def rendered(o, cases):
    return np.concatenate([np.ascontiguousarray(o.render_pixels(p, np.array(ids, np.uint32))[0][:, :3]).view(np.uint32)
                           for p, ids in cases if ids])


def test_aa_jitter_is_one_rounding(pkg, orc, abi):
    """fma(rand, aa, x) against rand * aa + x: on the pixels where the two land on different floats the
    oracle's sample is the fma's, and the other reading's sample differs on enough of them that the
    comparison could not pass with the wrong one."""
    desc, cam = jitter_scene(pkg)
    o = orc.Oracle(abi, desc)
    o.set_camera(cam)
    cases = jitter_cases(abi)
    one, two = jitter_readings(lambda rays, seeds, d: o.trace(rays, seeds, d, SKY, 3)[0], abi, cam, cases)
    parted(rendered(o, cases), one, two, "jitter")


# ------------------------------------------------------------------ the lens: (p * jitter) / W
LENS_W, LENS_H, LENS_FRAMES = 3, 2, 40
LENS_CAM = ((0.0, 0.0, 0.0), (0.06, -0.05, 1.0))
LENS_OPTICS = dict(focal=2.0 ** -10, jitter=0.003)  # a lens radius of 1e-3 around a focal distance of 1e-3


def lens_scene(pkg):
    """box_scene centred on the world's origin, where the camera stands: camPos + right * jx keeps
    every bit of jx (a camera at 0.5 would round the last bits of a 1e-3 offset away), and with the
    focal point as near as the lens is wide the direction focal - origin turns with them; the walls
    are 0.4 away."""
    return box_scene(pkg, 1.0, (0.0, 0.0, 0.0))[0], camera(pkg, LENS_W, LENS_H, cam=LENS_CAM, **LENS_OPTICS)


def lens_cases(abi):
    """The frames of a 3x2 DOF frame and, of their pixels, those where (p * defocusJitter) / W and
    p * (defocusJitter / W) differ in a lane.  Returns [(params, [pixel ids])]."""
    out = []
    dj = np.float32(LENS_OPTICS["jitter"])
    for f in range(LENS_FRAMES):
        p = frame_params(abi, LENS_W, LENS_H, f, 0, DOF, 1.0, 0)
        ids = []
        for i in range(LENS_W * LENS_H):
            g = Rng(F.pixel_seed(0, f, LENS_W, LENS_H, i % LENS_W, i // LENS_W))
            r = np.float32(np.sqrt(g.rf()))
            theta = np.float32(g.rf() * np.float32(np.float32(2) * F.PI))
            lanes = (np.float32(F.cosf(theta) * r), np.float32(F.sinf(theta) * r))
            if any(F.lens_offset(q, dj, LENS_W) != lens_scaled(q, dj, LENS_W) for q in lanes):
                ids.append(i)
        out.append((p, ids))
    return out


def lens_readings(trace, abi, cam, cases):
    return two_readings(trace, abi, cam, cases, "lens_offset", lens_scaled)


def test_lens_divides_the_product(pkg, orc, abi):
    """camera.h:75, p * defocusJitter / SCRWIDTH, is (p * defocusJitter) / W: on the pixels where
    p * (defocusJitter / W) gives another offset the oracle's sample is the former's, and the latter's
    differs on enough of them."""
    desc, cam = lens_scene(pkg)
    o = orc.Oracle(abi, desc)
    o.set_camera(cam)
    cases = lens_cases(abi)
    one, two = lens_readings(lambda rays, seeds, d: o.trace(rays, seeds, d, SKY, 3)[0], abi, cam, cases)
    parted(rendered(o, cases), one, two, "lens")


# ------------------------------------------------------------------ forced draws
def forced_scene(pkg, name):
    """A wall across the whole cube at z = 12..13, seen from inside the cube by a 1x1 frame whose
    whole view it fills, and nothing else in the world.  The wall is of the default material 20
    (DiffuseReflection and an unconditional Illumination: the sample depends on the hit point) —
    except under the all-zero state, where DiffuseReflection's rejection loop would never end:
    there it is of material 0, whose Schlick draw of 0.0 takes the specular arm (sample 0)."""
    cells = np.full(N * N * N, NONE, np.uint8)
    cells.reshape(N, N, N)[12:14, :, :] = 0 if name == "all-zero state" else 20
    _, mats, _, d = kat_scene(0)
    # seven point lights in front of the wall: Illumination's pick is the directional light (whose
    # term does not depend on the hit point) only for a draw of 7/8 or more
    points = [(v3(0.2 + 0.1 * k, 0.9 - 0.1 * k, 0.2 + 0.05 * k), v3(1.0, 0.95, 0.9)) for k in range(7)]
    vols = [Vol(cells, N)]
    return to_oracle(pkg, None, cells, mats, points, d, vols), (cells, mats, points, d, vols)


FORCED_CAM = ((0.5, 0.5, 0.5), (0.53, 0.47, 1.0))
FORCED_LENS = dict(focal=0.25, jitter=0.03125)  # W = 1: the lens radius is defocusJitter itself


def back(state, draws):
    for _ in range(draws):
        state = F.inv_xorshift(state)
    return state


# name -> (initial state of the 1x1 frame's pixel, what the draws must then be)
FORCED = {
    "first draw 0xFFFFFFFF": back(0xFFFFFFFF, 1),
    "first draw 1": back(1, 1),
    "all-zero state": 0,
    "third draw r = 1": back(0xFFFFFFC1, 3),
    "fourth draw theta = 2 pi": back(0xFFFFFF93, 4),
}


def forced_params(abi, name, depth=0):
    base = F.seed_base_for(FORCED[name], 0, 1, 1, 0, 0)
    return frame_params(abi, 1, 1, 0, base, AA | DOF, 1.0, depth)


def test_forced_states_are_what_they_say():
    g = Rng(FORCED["first draw 0xFFFFFFFF"])
    assert g.rf() == 1.0 and g.s == 0xFFFFFFFF  # (float)0xFFFFFFFF = 2^32, times 2^-32
    g = Rng(FORCED["first draw 1"])
    assert g.rf() == np.float32(2.0 ** -32) and g.s == 1
    g = Rng(FORCED["all-zero state"])
    assert [g.rf() for _ in range(6)] == [0.0] * 6
    g = Rng(FORCED["third draw r = 1"])
    assert [g.rf() for _ in range(3)][2] == 1.0 and g.s >= 0xFFFFFF80
    g = Rng(FORCED["fourth draw theta = 2 pi"])
    assert [g.rf() for _ in range(4)][3] == 1.0 and g.s >= 0xFFFFFF80
    for s in (1, 0x12345678, 0xFFFFFFFF, 0x80000000):
        assert F.inv_xorshift(F.xorshift(s)) == s and F.xorshift(F.inv_xorshift(s)) == s
        assert F.wang_hash(F.inv_wang_hash(s)) == s


def test_forced_draws(pkg, orc, abi):
    """The five edge draws on a 1x1 AA+DOF frame: fx = x + aa exactly, the smallest draw, all zeros,
    r = 1 and theta = float(2 pi); the oracle's pixel equals head() -> oracle_trace, and (no oracle
    code in the expected value) head() -> numpy Trace -> blend -> tonemap equals oracle_render."""
    cam = camera(pkg, 1, 1, cam=FORCED_CAM, **FORCED_LENS)
    refused, seen = [], {}
    for name in FORCED:
        desc, (cells, mats, points, d, vols) = forced_scene(pkg, name)
        o = orc.Oracle(abi, desc)
        o.set_camera(cam)
        p = forced_params(abi, name)
        assert F.pixel_seed(p.seed_base, 0, 1, 1, 0, 0) == FORCED[name]
        want, r = head_through(lambda rays, seeds, dd: o.trace(rays, seeds, dd, SKY, 3)[0], abi, cam, p)
        refused += r
        got, _ = o.render_pixels(p, np.zeros(1, np.uint32))
        assert np.array_equal(np.ascontiguousarray(got[:, :3]).view(np.uint32), want), name
        s = Scene(vols, mats, points, d, sky=SKY)
        acc, rgb = refusing(lambda: F.frame(s, cam, p, np.zeros((1, 4), np.uint32)), refused)
        seen[name] = tuple(int(v) for v in acc[0, :3])
        oacc, orgb, _ = o.render(p)
        bad, left_out = E.compare(fbits(oacc), orgb, acc, rgb)
        assert not bad and left_out == 0, (name, fbits(oacc), acc)
    assert len(refused) == 0, refused
    # every case hits the wall: black under the all-zero state, lit and different everywhere else
    sky = tuple(int(v) for v in fbits(np.array(SKY, np.float32)))
    assert seen.pop("all-zero state") == (0, 0, 0)
    assert len(set(seen.values())) == 4 and sky not in seen.values() and (0, 0, 0) not in seen.values(), seen


# ------------------------------------------------------------------ whole frames
FRAME_W, FRAME_H = 19, 13
FRAME_SCENES = {"room": lambda cells: [Vol(cells, N)], "two volumes": two_volumes,
                "mixed lights": lambda cells: [Vol(cells, N)]}
# which -> (light set, area samples): the scenes whose lights are not the room's own point light.  "wide
# lights" (18 lights and the directional one, 15 samples) is no FRAME_SCENES entry: it has one frame at depth 2.
# "mixed lights, 1 sample" is the mixed set with one shadow slot per path, which the device's one-launch
# depth-0 frame kernel requires.
FRAME_LIGHTS = {"mixed lights": (L.LIGHT_SETS["mixed"], 3), "wide lights": (L.LIGHT_SETS["wide"], 15),
                "mixed lights, 1 sample": (L.LIGHT_SETS["mixed"], 1)}
FRAME_LENS = dict(focal=1.3, jitter=2.0)
_FRAMES = {}


def frame_samples(which):
    return FRAME_LIGHTS[which][1] if which in FRAME_LIGHTS else 3


def expected_frames(pkg, abi, which, depth, frames=3):
    """Frames 0..frames-1 of the 19x13 AA+DOF scene accumulated from a zero accumulator by F.frame
    (numpy only): (desc, camera, [per frame (accumulator bits, RGB8, shadow rays, DDA cells, the
    picks)], refusals).  Computed once and shared with the GPU tests."""
    key = (which, depth, frames)
    if key not in _FRAMES:
        lights, samples = FRAME_LIGHTS.get(which, (None, 3))
        desc, (cells, mats, points, d, vols, *kw) = room(pkg, FRAME_SCENES.get(which, FRAME_SCENES["room"]), lights=lights)
        desc.area_samples = samples
        cam = camera(pkg, FRAME_W, FRAME_H, **FRAME_LENS)
        acc = np.zeros((FRAME_W * FRAME_H, 4), np.uint32)
        out, refused = [], []
        for f in range(frames):
            p = frame_params(abi, FRAME_W, FRAME_H, f, 0, AA | DOF, 1.0, depth, samples)
            s = Scene(vols, mats, points, d, sky=SKY, **(kw[0] if kw else {}))
            s.area_samples = samples
            r = refusing(lambda: F.frame(s, cam, p, acc), refused)
            if r is None:
                break
            acc, rgb = r
            out.append((acc, rgb, s.shadows, s.cells, s.picks))
        _FRAMES[key] = (desc, cam, out, refused)
    return _FRAMES[key]


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("which", list(FRAME_SCENES))
def test_whole_frames_equal_oracle_render(pkg, orc, abi, which, depth):
    """oracle_render over three accumulated frames equals head -> numpy Trace -> blend_ref ->
    tonemap_ref: accumulator bits and RGB8 under epilogue_ref.compare."""
    desc, cam, frames, refused = expected_frames(pkg, abi, which, depth)
    assert len(refused) == 0 and len(frames) == 3, refused
    o = orc.Oracle(abi, desc)
    o.set_camera(cam)
    acc = None
    for f, (want_acc, want_rgb, shadows, cells, _) in enumerate(frames):
        acc, rgb, st = o.render(frame_params(abi, FRAME_W, FRAME_H, f, 0, AA | DOF, 1.0, depth, frame_samples(which)),
                                accum=acc, threads=2)
        bad, left_out = E.compare(fbits(acc), rgb, want_acc, want_rgb)
        assert not bad and left_out == 0, (which, depth, f, len(bad), bad[:8])
        assert (st.shadow_rays, st.dda_cells) == (shadows, cells), (which, depth, f)
    hit = (frames[0][0][:, :3] != fbits(np.array(SKY, np.float32))[None, :]).any(axis=1)
    assert 40 <= hit.sum() <= FRAME_W * FRAME_H - 20  # both hits and misses, not a constant image


def frame_picks(frames):
    """(kind, index within the kind, randLightIndex, outcome) of every Illumination call of the frames."""
    return [p for fr in frames for p in fr[4]]


def test_light_frames_draw_every_light(pkg, abi):
    """What the frames with light sets stand on, from the restatement alone: every light of the mixed
    set is drawn at depth 0 and at depth 2, spots fall outside, lit and occluded, area samples are
    rejected, occluded and lit; the wide frame draws every one of its 19 lights, picks that share a
    bucket modulo 16, and an area light with all 15 samples lit (every slot bit)."""
    for depth in (0, 2):
        _, _, frames, refused = expected_frames(pkg, abi, "mixed lights", depth)
        assert not refused and len(frames) == 3
        picks = frame_picks(frames)
        assert {p[2] for p in picks} == set(range(7)), depth
        assert {p[3] for p in picks if p[0] == "spot"} == {"outside", "lit", "occluded"}, depth
        assert {o for p in picks if p[0] == "area" for o in p[3]} == {"rejected", "occluded", "lit"}, depth
    _, _, frames, refused = expected_frames(pkg, abi, "wide lights", 2, frames=1)
    assert not refused and len(frames) == 1
    picks = frame_picks(frames)
    idx = {p[2] for p in picks}
    assert idx == set(range(19)) and {0, 16} <= idx
    assert any(p[0] == "area" and set(p[3]) == {"lit"} and len(p[3]) == 15 for p in picks)
    assert any(p[0] == "area" and len(set(p[3])) == 3 for p in picks)  # one pick with all three outcomes


def test_wide_light_frame_equals_oracle_render(pkg, orc, abi):
    """One 19x13 frame at depth 2 with the wide light set and 15 area samples."""
    desc, cam, frames, refused = expected_frames(pkg, abi, "wide lights", 2, frames=1)
    assert not refused and len(frames) == 1
    o = orc.Oracle(abi, desc)
    o.set_camera(cam)
    acc, rgb, st = o.render(frame_params(abi, FRAME_W, FRAME_H, 0, 0, AA | DOF, 1.0, 2, 15), threads=2)
    bad, left_out = E.compare(fbits(acc), rgb, frames[0][0], frames[0][1])
    assert not bad and left_out == 0, (len(bad), bad[:8])
    assert (st.shadow_rays, st.dda_cells) == (frames[0][2], frames[0][3])


# ------------------------------------------------------------------ focus ray
def focus_cases(pkg):
    """name -> (desc, volumes, camera pose, W, H, what the distance must be)."""
    cells, mats, points, d = kat_scene(0)
    solid = cells.copy()
    solid.reshape(N, N, N)[4:8, 6:10, 6:10] = 20  # the camera of "inside a solid cell" sits in here
    ident, messy = [Vol(cells, N)], [Vol(cells, N), _messy_volume(cells)]
    mk = lambda c, vols: to_oracle(pkg, None, c, mats, points, d, vols)  # noqa: E731
    return {
        "hit": (mk(cells, ident), ident, CAM, 20, 12, "hit"),
        "miss": (mk(cells, ident), ident, ((0.5, 0.5, -1.0), (0.5, 3.0, -2.0)), 20, 12, "miss"),
        "inside a solid cell": (mk(solid, [Vol(solid, N)]), [Vol(solid, N)], ((0.5, 0.5, 0.375), (0.5, 0.5, 1.0)), 20, 12, "zero"),
        "second volume transformed": (mk(cells, messy), messy, ((0.45, 0.55, -0.8), (0.5, 0.4, 0.5)), 20, 12, "hit"),
        "odd W and H": (mk(cells, ident), ident, ((0.3, 0.7, -0.9), (0.55, 0.35, 0.5)), 19, 13, "hit"),
    }


def focus_expected(pkg, name):
    desc, vols, pose, W, H, kind = focus_cases(pkg)[name]
    cam = camera(pkg, W, H, cam=pose)
    t = F.focus_distance(cam, W, H, vols)
    assert {"hit": 0 < t < 1e4, "miss": t == np.float32(1e4), "zero": t == 0}[kind], (name, t)
    return desc, cam, W, H, t


FOCUS_NAMES = ["hit", "miss", "inside a solid cell", "second volume transformed", "odd W and H"]


@pytest.mark.parametrize("name", FOCUS_NAMES)
def test_focus_distance(pkg, orc, abi, name):
    """oracle_focus_distance equals the restated Tick ray: integer centre, no lens draw, every volume
    walked in world space, clamp(t, -1, 1e4)."""
    desc, cam, W, H, want = focus_expected(pkg, name)
    o = orc.Oracle(abi, desc)
    o.set_camera(cam)
    got = np.float32(o.focus_distance(W, H))
    assert fbits(got) == fbits(want), (name, got, want)
    if name == "second volume transformed":  # the transform is ignored: the same distance without it
        plain = [Vol(v.cells, N, b0=v.b0, b1=v.b1) for v in focus_cases(pkg)[name][1]]
        assert fbits(F.focus_distance(cam, W, H, plain)) == fbits(want)
