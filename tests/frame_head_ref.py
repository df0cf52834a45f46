"""The head of a moving-camera frame, restated in numpy float32 from the reference text.

What Renderer::Update does to a pixel before Trace takes its random stream over, and the focus
ray of Renderer::Tick, one rounded float32 operation per step in the reference's operand order
(the build's -ffp-contract=off reading of /fp:fast, as tests/test_kat_paths.py):

  Renderer::Update        renderer.cpp:1646-1891   the AA jitter _mm256_fmadd_ps(rand, aa, x) (one
                                                   rounding), r = sqrt(rand), theta = rand * (2 * PI),
                                                   (cos theta * r, sin theta * r), normalize, Trace
  Camera::GetPrimaryRay   template/camera.h:68-83  u = x * (1.0f / SCRWIDTH), P, the thin lens:
                                                   p * defocusJitter / SCRWIDTH (BOTH lanes by the width)
  WangHash / InitSeed     template/tmpl8math.cpp:16-38
  RandomUInt / RandomFloat template/tmpl8math.cpp:119-133 (test_kat_paths.Rng)
  the focus ray           renderer.cpp:1987-1991   Scene::FindNearest on the WORLD-space ray per volume

A plain helper module without fixtures.  Nothing here calls the oracle or the library; the only
self-check is seed_base_for's, against this module's own pixel_seed.  tests/test_kat_frame.py
pins the oracle to it, tests/test_kat_frame_gpu.py the device (no oracle in between).

Decided elsewhere and taken as decided: the reference draws a row's random numbers
eight pixels at a time from one thread's stream; the build gives every pixel its own stream, seeded
from InitSeed's formula with k = seed_base + frame * (W * H) + y * W + x, and spends it in the
order the reference's vectors are filled: [AA: x, y][DOF: r, theta], then Trace.  A flag that is
off spends no draws.  sin / cos are correctly rounded (_mm256_sin_ps / _mm256_cos_ps are SVML).
The focus ray is GetPrimaryRay's at the integer centre without the lens sample, i.e. from camPos
through P.

Not covered, on purpose:
  - the head under VPX_ARITH_X86_HOST (D = dir * rsqrtps(dot(dir, dir))): vpx_trace normalises the
    direction it is given exactly, so head() composed with it cannot carry an rsqrt-normalised D,
    and the numpy Trace has no FastReciprocal;
  - GetPrimaryRayNoDOF paths (the static camera, vpx_render_ids, vpx_pick_pixel): restated in
    tests/test_kat_reproject.py and tests/reproject_ids_ref.py.
Spot and area lights are inside the numpy Trace (test_kat_paths.Scene.illumination; tests/test_kat_lights.py
pins the oracle to it): whole frames with them are compared with head -> numpy Trace like the others, and
the GPU tests' composition of head() with the device's vpx_trace remains for depth 8 and as a second check.

The device flushes subnormals and numpy does not: every intermediate is asserted to be zero or
normal, so that the restatement never silently depends on one.
"""
from fractions import Fraction

import numpy as np

import epilogue_ref as E
from test_kat_paths import NONE, PI, Ray, Rng, Vol, add, cosf, cr32, dsign, f32, mul, normalize, sinf, sub, v3

FLAG_AA, FLAG_DOF = 0x1, 0x2  # VPX_FLAG_AA / VPX_FLAG_DOF
M32 = 0xFFFFFFFF
TINY = f32(2.0 ** -126)


def normal(x):
    """x, after asserting that no lane is subnormal."""
    a = np.abs(np.asarray(x, np.float32))
    assert not np.any((a > 0) & (a < TINY)), ("subnormal intermediate", x)
    return x


# ------------------------------------------------------------------------ seeds
def wang_hash(s):  # WangHash (tmpl8math.cpp:20-27), uint32
    s &= M32
    s = (s ^ 61) ^ (s >> 16)
    s = (s * 9) & M32
    s = s ^ (s >> 4)
    s = (s * 0x27D4EB2D) & M32
    return s ^ (s >> 15)


def pixel_seed(seed_base, frame, W, H, x, y):
    """seed = 0x12345678 + WangHash((k + 1) * 17) (InitSeed on a fresh thread_local seed), uint32."""
    k = (seed_base + frame * (W * H) + y * W + x) & M32
    return (0x12345678 + wang_hash(((k + 1) & M32) * 17)) & M32


def xorshift(s):  # RandomUInt
    s ^= (s << 13) & M32
    s ^= s >> 17
    s ^= (s << 5) & M32
    return s


def inv_xorshift(s):
    """The state before a RandomUInt that leaves `s`."""
    s ^= (s << 5) & M32   # x ^= x << 5 undone: shifts 5, 10, 20
    s ^= (s << 10) & M32
    s ^= (s << 20) & M32
    s ^= s >> 17          # x ^= x >> 17 is its own inverse (34 >= 32)
    s ^= (s << 13) & M32  # x ^= x << 13 undone: shifts 13, 26
    s ^= (s << 26) & M32
    return s


def inv_wang_hash(h):
    h ^= h >> 15
    h ^= h >> 30
    h = (h * pow(0x27D4EB2D, -1, 1 << 32)) & M32
    h ^= h >> 4
    h ^= h >> 8
    h ^= h >> 16
    h = (h * pow(9, -1, 1 << 32)) & M32
    return h ^ 61 ^ (h >> 16)  # the high half passes through (s ^ 61) ^ (s >> 16) unchanged


def seed_base_for(state0, frame, W, H, x, y):
    """The seed_base with pixel_seed(seed_base, frame, W, H, x, y) == state0: WangHash, * 17 and
    the additions are bijections on uint32."""
    k1 = (inv_wang_hash((state0 - 0x12345678) & M32) * pow(17, -1, 1 << 32)) & M32
    base = (k1 - 1 - frame * (W * H) - y * W - x) & M32
    assert pixel_seed(base, frame, W, H, x, y) == state0 & M32
    return base


# ------------------------------------------------------------------------- head
class Cam:
    """The six vectors and two scalars of Camera that GetPrimaryRay reads, from any object with
    vpx_camera's field names."""

    def __init__(self, c):
        self.pos, self.tl, self.tr, self.bl = v3(*c.cam_pos), v3(*c.top_left), v3(*c.top_right), v3(*c.bottom_left)
        self.right, self.up = v3(*c.right), v3(*c.up)
        self.focal, self.jitter = f32(c.focal_distance), f32(c.defocus_jitter)


def fma32(a, b, c):
    """a * b + c rounded once: the float32 nearest to the exact rational."""
    return cr32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def screen_point(cam, W, H, fx, fy):  # camera.h:71-73
    u = normal(f32(fx * normal(f32(f32(1.0) / f32(W)))))
    v = normal(f32(fy * normal(f32(f32(1.0) / f32(H)))))
    across, down = normal(sub(cam.tr, cam.tl)), normal(sub(cam.bl, cam.tl))
    return normal(add(normal(add(cam.tl, normal(mul(across, u)))), normal(mul(down, v))))


def lens_offset(p, jitter, W):
    """One lane of p * defocusJitter / SCRWIDTH (camera.h:75): the product first, then the divide."""
    return normal(f32(normal(f32(p * jitter)) / f32(W)))


def head(camera, params, x, y):
    """Pixel (x, y) of the frame: (origin, direction as GetPrimaryRay leaves it — unnormalised —,
    the xorshift32 state Trace starts from)."""
    cam = camera if isinstance(camera, Cam) else Cam(camera)
    W, H = int(params.width), int(params.height)
    g = Rng(pixel_seed(int(params.seed_base), int(params.frame_index), W, H, x, y))
    fx, fy = f32(x), f32(y)
    if params.flags & FLAG_AA:  # renderer.cpp:1682-1685, 1699-1707
        aa = f32(params.aa_strength)
        rx = g.rf()
        ry = g.rf()
        fx, fy = normal(fma32(rx, aa, fx)), normal(fma32(ry, aa, fy))
    if params.flags & FLAG_DOF:  # renderer.cpp:1688-1697
        r = normal(f32(np.sqrt(g.rf())))
        theta = normal(f32(g.rf() * f32(f32(2) * PI)))
        px, py = normal(f32(cosf(theta) * r)), normal(f32(sinf(theta) * r))
    P = screen_point(cam, W, H, fx, fy)
    if not params.flags & FLAG_DOF:
        # the build's reading of "no DOF": the lens term is left out (GetPrimaryRayNoDOF's ray)
        return cam.pos.copy(), normal(sub(P, cam.pos)), g.s
    jx, jy = lens_offset(px, cam.jitter, W), lens_offset(py, cam.jitter, W)  # both lanes by SCRWIDTH
    to_p = normal(normalize(normal(sub(P, cam.pos))))
    focal = normal(add(cam.pos, normal(mul(to_p, cam.focal))))             # :79
    origin = normal(add(normal(add(cam.pos, normal(mul(cam.right, jx)))), normal(mul(cam.up, jy))))  # :80
    return origin, normal(sub(focal, origin)), g.s                          # :82


# ------------------------------------------------------------------- focus ray
def focus_distance(camera, W, H, vols):
    """Renderer::Tick's focus ray (renderer.cpp:1987-1991): the ray of the integer centre
    (W / 2, H / 2), Scene::FindNearest (scene.cpp:751-811) of every volume on the world-space
    ray — no volume's transform is applied, the reference's quirk — then clamp(t, -1, 1e4)."""
    cam = camera if isinstance(camera, Cam) else Cam(camera)
    P = screen_point(cam, W, H, f32(W // 2), f32(H // 2))
    ray = Ray(cam.pos, sub(P, cam.pos))
    rD = v3(*[f32(f32(1) / ray.D[k]) for k in range(3)])  # Ray::Ray (scene.cpp:83-93)
    for v in vols:
        s = v.setup(ray.O, ray.D, rD, dsign(ray.D))
        if s is None:
            continue
        while s["t"] < ray.t:
            if v.cell(s["X"], s["Y"], s["Z"]) != NONE and s["t"] < ray.t:
                ray.t = f32(s["t"])
                break
            if not Vol.advance(s, v.n):
                break
    t = ray.t if ray.t < f32(1e4) else f32(1e4)   # clamp: fmaxf(a, fminf(f, b))
    return t if t > f32(-1.0) else f32(-1.0)


# ------------------------------------------------------------------------ frame
def samples(scene, camera, params, pixels=None):
    """Trace(primary ray, maxBounces) per pixel id (all of the frame by default): bit patterns [n, 3].
    scene: a test_kat_paths.Scene (its sky is the frame's)."""
    cam = Cam(camera)
    W, H = int(params.width), int(params.height)
    ids = range(W * H) if pixels is None else pixels
    out = np.zeros((len(ids), 3), np.float32)
    for i, p in enumerate(ids):
        o, d, state = head(cam, params, int(p) % W, int(p) // W)
        out[i] = scene.trace(Ray(o, d), int(params.max_bounces), Rng(state))
    return out.view(np.uint32)


def frame(scene, camera, params, acc_bits):
    """One Renderer::Update: head -> Trace -> blend -> tonemap, no oracle and no library.
    acc_bits: the accumulator before the frame, bit patterns [W * H, 4].
    Returns (accumulator bits [W * H, 4], RGB8 [W * H])."""
    return E.reference(samples(scene, camera, params), acc_bits, int(params.frame_index))


__all__ = ["Cam", "FLAG_AA", "FLAG_DOF", "focus_distance", "fma32", "frame", "head", "inv_xorshift", "lens_offset",
           "pixel_seed", "samples", "seed_base_for", "xorshift"]
