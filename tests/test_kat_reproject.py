"""Known answers for the static-camera (reprojection) branch of Renderer::Tick.

The expected values come from a restatement written here in numpy float32 straight from the
reference text, independent of oracle/vpx_oracle.c and of the kernels.  It builds on the
machinery of test_kat_paths.py (Scene, Vol, Ray, Rng, the float32 helpers): every operation
is the reference's, in its operand order, rounded to float32 after each step.  The oracle's
oracle_render_reproject is compared with it bit for bit on the CPU, and the device's
vpx_render_reproject is compared with it directly (no oracle in between) on the GPU.

  Renderer::Tick, static branch            renderer.cpp:1996-2101 (both pixel loops, the
                                           material weight switch :2050-2083)
  TraceReproject and its helpers           renderer.cpp:1330-1585 (TraceMetal, TraceNonMetal,
                                           TraceDialectric, TraceSmoke, TraceEmmision,
                                           TraceModelMaterials), AlbedoIlluminationData /
                                           GetColor / GetRayInfo renderer.h:10-34
  SampleSkyReproject                       renderer.cpp:2328-2333 (constant sky: {colour, 1})
  IsValid / IsValidScreen                  renderer.cpp:1635-1643
  IsOccludedPrevFrame                      renderer.cpp:767-774
  SampleHistory                            renderer.cpp:777-830
  RGBToYCoCg / YCoCgToRGB / ClampHistory   renderer.cpp:833-910
  Camera::PointToUV / SetFrustumNormals    template/camera.h:34-66, HALF_PIXEL_W / _H :7-8
  Camera::GetPrimaryRayNoDOF               template/camera.h:103-110
  Camera::HandleInput(0), no key down      template/camera.h:121-178
  Renderer::CopyToPrevCamera               renderer.cpp:1893-1902
  lerp / clamp / fminf / fmaxf / cross     template/tmpl8math.h:2220-2223, 2105-2138, 401-409, 2496-2499
  ApplyReinhardJodie / RGBF32_to_RGB8      reused from test_kat_reference.ref_tonemap

Three points are taken as decided, not derived from the reference:
  * the per-pixel RNG state is vpx_pixel_seed(seed_base, frame_index, W, H, x, y), the
    project's own choice, pinned by test_cpu_oracle.test_wang_hash_and_pixel_seed;
  * the history holds finite values only: the reference leaves NaN / inf history undefined
    under /fp:fast, so no case feeds one;
  * no subnormal intermediates: the oracle and the device run with FTZ / DAZ and numpy does
    not, so the restatement asserts that no operand or result of pass 2's own arithmetic
    (reprojection, sampling, clamp, blend, the tonemap's input) is subnormal.  The occlusion
    walk of pass 2 is Renderer::IsOccluded as test_kat_paths.py restates and pins it.
The history is a float4 per pixel whose w lane is not the reference's (its buffers are
float3): the lane is never read and is written as 0.

The module's wall time on the CPU (the restatement of 8 pass-1 and 15 pass-2 frames of at
most 256 pixels, computed once and shared by all tests) is about 35 s; the device spends well
under a second on the same frames.
"""
import numpy as np
import pytest

from test_cpu_oracle import wang_py
from test_kat_paths import (N, NONE, Ray, Rng, Scene, Vol, add, dot, expf, f32, fbits, kat_scene, length, mul,
                            normalize, offset_ray, reflect, refract, schlick, std_max, std_min, sub, to_oracle,
                            trunc_i32, v3)
from test_kat_reference import ref_tonemap

pytestmark = [pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning"),   # 1/0 = inf, as the reference
              pytest.mark.filterwarnings("ignore:invalid value:RuntimeWarning"),    # sky points: normalize(0) = NaN
              pytest.mark.filterwarnings("ignore:overflow:RuntimeWarning")]         # sky points: |1e34|^2 = inf

TINY = f32(2.0 ** -126)
SKY = (0.392, 0.584, 0.829)
SENTINEL = f32(-7777.0)  # the history's unused w lane on entry


def nz(x):
    """x, after asserting that it holds no subnormal (the oracle's and the device's FTZ / DAZ
    would flush it and this restatement would not)."""
    a = np.abs(np.asarray(x, np.float32))
    assert not np.any((a > 0) & (a < TINY)), ("subnormal in pass 2", x)
    return x


def fadd(a, b):
    return nz((nz(a) + nz(b)).astype(np.float32))


def fsub(a, b):
    return nz((nz(a) - nz(b)).astype(np.float32))


def fmul(a, b):
    return nz((np.asarray(nz(a), np.float32) * np.asarray(nz(b), np.float32)).astype(np.float32))


def fdiv(a, b):
    return nz((np.asarray(nz(a), np.float32) / np.asarray(nz(b), np.float32)).astype(np.float32))


def fdot(a, b):  # dot with the subnormal check on every product and sum
    return fadd(fadd(fmul(a[0], b[0]), fmul(a[1], b[1])), fmul(a[2], b[2]))


def t_fminf(a, b):  # tmpl8math.h:401-404
    return a if a < b else b


def t_fmaxf(a, b):  # tmpl8math.h:406-409
    return a if a > b else b


def cross(a, b):  # tmpl8math.h:2496-2499
    return v3(f32(a[1] * b[2]) - f32(a[2] * b[1]), f32(a[2] * b[0]) - f32(a[0] * b[2]),
              f32(a[0] * b[1]) - f32(a[1] * b[0]))


def pixel_seed(seed_base, frame_index, w, h, x, y):  # the project's per-pixel seed (see the docstring)
    k = (seed_base + frame_index * (w * h) + y * w + x) & 0xFFFFFFFF
    return (0x12345678 + wang_py(((k + 1) * 17) & 0xFFFFFFFF)) & 0xFFFFFFFF


# ------------------------------------------------------------------------ camera
class Camera:
    """Camera::HandleInput(0) with no key down (camera.h:121-178), then SetFrustumNormals
    (:53-66); ASPECT = float(W) / float(H) (:183)."""

    def __init__(self, pos, target, w, h):
        self.w, self.h = w, h
        pos, tgt = v3(*pos), v3(*target)
        tmp_up = v3(0, 1, 0)
        ahead = normalize(sub(tgt, pos))               # :121-124
        right = normalize(cross(tmp_up, ahead))
        up = normalize(cross(ahead, right))
        ahead = normalize(sub(tgt, pos))               # :163-165
        right = normalize(cross(tmp_up, ahead))
        up = normalize(cross(ahead, right))
        tgt = add(pos, ahead)                          # :172-175
        ahead = normalize(sub(tgt, pos))
        up = normalize(cross(ahead, right))
        right = normalize(cross(up, ahead))
        aspect = f32(f32(w) / f32(h))
        ar = mul(right, aspect)
        a2 = mul(ahead, f32(2))
        self.pos, self.ahead, self.right, self.up = pos, ahead, right, up
        self.top_left = add(sub(add(pos, a2), ar), up)      # :176-178, left to right
        self.top_right = add(add(add(pos, a2), ar), up)
        self.bottom_left = sub(sub(add(pos, a2), ar), up)
        lf, rf = sub(a2, ar), add(a2, ar)                   # SetFrustumNormals
        tf, bf = add(a2, up), sub(a2, up)
        self.left_n = cross(up, lf)
        self.right_n = cross(rf, up)
        self.top_n = cross(right, tf)
        self.bottom_n = cross(bf, right)

    def primary_ray(self, x, y):  # GetPrimaryRayNoDOF (camera.h:103-110) + Ray(O, D)
        u = f32(f32(x) * f32(f32(1.0) / f32(self.w)))
        v = f32(f32(y) * f32(f32(1.0) / f32(self.h)))
        tl = self.top_left
        p = add(add(tl, mul(sub(self.top_right, tl), u)), mul(sub(self.bottom_left, tl), v))
        return Ray(self.pos, sub(p, self.pos))

    def point_to_uv(self, point):  # PointToUV (camera.h:34-49)
        delta = fsub(point, self.pos)
        ld, rd = fdot(self.left_n, delta), fdot(self.right_n, delta)
        td, bd = fdot(self.top_n, delta), fdot(self.bottom_n, delta)
        return fdiv(ld, fadd(ld, rd)), fdiv(td, fadd(td, bd))


# ------------------------------------------------------------------------ pass 1
class RScene(Scene):
    """test_kat_paths.Scene plus Renderer::TraceReproject; counts FindNearest calls and the
    volume-0 smoke probes on top of the base class's shadow rays and DDA cells."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.nearest = 0
        self.probes = 0

    def find_nearest(self, ray):
        self.nearest += 1
        return super().find_nearest(ray)

    def color(self, ray, depth, g):  # TraceReproject(...).GetColor() = albedo * illumination
        a, i = self.trace_reproject(ray, depth, g)
        return mul(a, i)

    def trace_reproject(self, ray, depth, g):  # renderer.cpp:1521-1585 -> (albedo, illumination)
        if depth < 0:
            return v3(0, 0, 0), v3(0, 0, 0)
        vox = self.find_nearest(ray)
        m = ray.mat
        if m == NONE:
            return self.sky.copy(), v3(1, 1, 1)  # SampleSkyReproject, constant sky
        mat = self.mats[m]
        if 5 <= m <= 7:  # TraceMetal :1330-1340: nothing multiplied at this level
            refl = reflect(ray.D, ray.N)
            nr = Ray(offset_ray(ray.point(), ray.N), add(refl, mul(g.sphere_sample(), f32(mat["roughness"]))))
            return self.albedo(m), self.color(nr, depth - 1, g)
        if m <= 4:  # TraceNonMetal :1342-1357: the Lambertian vector first, no Schlick draw
            rdir = add(ray.N, g.sphere_sample())
            inc = self.illumination(ray, g)
            nr = Ray(offset_ray(ray.point(), ray.N), rdir)
            il = add(v3(0, 0, 0), inc)
            il = add(il, self.color(nr, depth - 1, g))
            return self.albedo(m), il
        if m == 8:  # TraceDialectric :1359-1423
            color = v3(1, 1, 1)
            in_glass = ray.inside
            ior = f32(mat["ior"])
            ratio = ior if in_glass else f32(f32(1.0) / ior)
            inside_volume = True
            if in_glass:
                color = self.albedo(m)
                inside_volume = self.exit_march(vox, ray, glass=True)
            if not inside_volume:
                ray.O = add(ray.O, mul(ray.D, ray.t))
                ray.t = f32(0)
            c = std_min(dot(-ray.D, ray.N), f32(1.0))
            s = f32(np.sqrt(f32(f32(1.0) - f32(c * c))))
            cannot = f32(ratio * s) > f32(1.0)
            if cannot or schlick(c, ratio) > g.rf():
                rdir, rn = reflect(ray.D, ray.N), ray.N
            else:
                rdir, rn = refract(ray.D, ray.N, ratio), -ray.N
                in_glass = not in_glass
            nr = Ray(offset_ray(ray.point(), rn), rdir)
            nr.inside = in_glass
            return color, self.color(nr, depth - 1, g)
        if m <= 14:  # TraceSmoke :1425-1501
            color = v3(1, 1, 1)
            in_glass = ray.inside
            inside_volume = True
            intensity, dist = f32(0), f32(0)
            if vox == 0:  # the player: the probe Illumination runs first (its result only sets inLight)
                self.probes += 1
                self.illumination(ray, g)
            if in_glass:
                intensity = f32(mat["emissive"])
                color = self.albedo(m)
                inside_volume = self.exit_march(vox, ray, glass=False)
                dist = ray.t
            threshold = f32(f32(g.rf() * f32(100)) - intensity)
            if f32(g.rf() * dist) > threshold:
                lo, hi = f32(ray.t * f32(0.45)), ray.t
                tt = f32(lo + f32(g.rf() * f32(hi - lo)))
                ray.O = add(ray.O, mul(ray.D, tt))
                ray.D = g.random_direction()
                ray.t = f32(0)
            e = mul(sub(v3(1, 1, 1), color), f32(f32(-dist) * intensity))
            color = v3(expf(e[0]), expf(e[1]), expf(e[2]))
            if not inside_volume:
                ray.O = add(ray.O, mul(ray.D, ray.t))
                ray.t = f32(0)
            rdir = refract(ray.D, ray.N, f32(1.0))
            nr = Ray(offset_ray(ray.point(), -ray.N), rdir)
            nr.inside = not in_glass
            return color, self.color(nr, depth - 1, g)
        if m == 15:  # TraceEmmision :1503-1506
            return mul(self.albedo(m), f32(mat["emissive"])), v3(1, 1, 1)
        rdir = g.diffuse_reflection(ray.N)  # TraceModelMaterials :1508-1518
        inc = self.illumination(ray, g)
        nr = Ray(offset_ray(ray.point(), ray.N), rdir)
        il = add(inc, self.color(nr, depth - 1, g))
        return self.albedo(m), il


# --------------------------------------------------------------------- the scene
PINK = dict(albedo=(0.9, 0.5, 0.7), roughness=0.4, emissive=0.0, ior=1.5)  # NON_METAL_PINK (4)


def reproject_scene():
    """The kat_scene room with its back wall split into patches of every weight class; the
    glass and the smoke block stay in front, the floor is the model material."""
    cells, mats, points, d = kat_scene(0)
    idx = lambda x, y, z: x + y * N + z * N * N
    patches = {(0, 1): 0, (1, 1): 6, (2, 1): 15, (0, 0): 20, (1, 0): 4, (2, 0): 0}
    for x in range(3, 13):
        for y in range(3, 13):
            px = 0 if x < 5 else (1 if x < 11 else 2)  # the middle patches are 3 x 3 pixels at 20 x 12
            for z in (12, 13):
                cells[idx(x, y, z)] = patches[(px, 1 if y >= 8 else 0)]
    mats = dict(mats)
    mats[4] = PINK
    return cells, mats, points, d


_PASS1 = {}
MIXED = "mixed"  # test_kat_lights' mixed light set in place of the room's point light


def scene_lights(lights):
    """(points, Scene's spots / areas keywords) of reproject_scene() under `lights` (None: its own)."""
    if lights is None:
        return reproject_scene()[2], {}
    from test_kat_lights import LIGHT_SETS, lights_of

    kw = lights_of(LIGHT_SETS[lights])
    return kw.pop("points"), kw


def pass1(w, h, depth, frame_index, cam_pt, lights=None):
    """The first pixel loop (renderer.cpp:2003-2022): albedo, illumination, GetRayInfo's
    intersection point and material per pixel, and the loop's counts."""
    key = (w, h, depth, frame_index, cam_pt, lights)
    if key in _PASS1:
        return _PASS1[key]
    cells, mats, _, d = reproject_scene()
    points, kw = scene_lights(lights)
    cam = Camera(cam_pt[0], cam_pt[1], w, h)
    s = RScene([Vol(cells, N)], mats, points, d, sky=SKY, **kw)
    alb, ill, ip = (np.zeros((w * h, 3), np.float32) for _ in range(3))
    mat = np.zeros(w * h, np.int64)
    for y in range(h):
        for x in range(w):
            g = Rng(pixel_seed(0, frame_index, w, h, x, y))
            ray = cam.primary_ray(x, y)
            a, i = s.trace_reproject(ray, depth, g)
            k = x + y * w
            alb[k], ill[k] = a, i
            ip[k], mat[k] = ray.point(), ray.mat  # GetRayInfo on the ray as TraceReproject leaves it
    out = dict(alb=alb, ill=ill, ip=ip, mat=mat, nearest=s.nearest, shadows=s.shadows, cells=s.cells,
               probes=s.probes, picks=s.picks)
    _PASS1[key] = out
    return out


# ------------------------------------------------------------------------ pass 2
def ycocg(c):  # RGBToYCoCg (renderer.cpp:833-839)
    k = fdiv(fmul(f32(0.5), f32(256.0)), f32(255.0))
    y = fmul(fdot(c, v3(1, 2, 1)), f32(0.25))
    co = fadd(fmul(fdot(c, v3(2, 0, -2)), f32(0.25)), k)
    cg = fadd(fmul(fdot(c, v3(-1, 2, -1)), f32(0.25)), k)
    return v3(y, co, cg)


def ycocg_to_rgb(c):  # YCoCgToRGB (renderer.cpp:842-851)
    k = fdiv(fmul(f32(0.5), f32(256.0)), f32(255.0))
    y, co, cg = c[0], fsub(c[1], k), fsub(c[2], k)
    return v3(fsub(fadd(y, co), cg), fadd(y, cg), fsub(fsub(y, co), cg))


def on_screen(x, y, w, h):  # IsValidScreen on int2 -> float2 (renderer.cpp:1640-1643)
    return f32(x) >= f32(0.0) and f32(x) < f32(w) and f32(y) >= f32(0.0) and f32(y) < f32(h)


def weight_of(m):  # the switch of renderer.cpp:2050-2083 -> (w, class)
    if m <= 4:
        return f32(0.8), "non_metal"
    if m <= 7:
        return f32(0.5), "metal"
    if m == 8:
        return f32(0.5), "glass"
    if m <= 14:
        return f32(0.9), "smoke"
    if m == 15:
        return f32(0.0), "emissive"
    return f32(0.9), "none" if m == NONE else "default"


def pass2(p1, w, h, prev, hist):
    """The second pixel loop (renderer.cpp:2023-2100) -> new history (float4, w = 0), RGB8
    words, (shadow rays, DDA cells) of IsOccludedPrevFrame, and the arms taken."""
    cells, mats, points, d = reproject_scene()
    s = RScene([Vol(cells, N)], mats, points, d, sky=SKY)
    arms = set()
    new = np.zeros((w * h, 4), np.float32)
    rgb = np.zeros(w * h, np.uint32)
    hw = fdiv(fdiv(f32(1.0), f32(w)), f32(2.0))  # HALF_PIXEL_W / HALF_PIXEL_H (camera.h:7-8)
    hh = fdiv(fdiv(f32(1.0), f32(h)), f32(2.0))
    ill = p1["ill"]
    for y in range(h):
        for x in range(w):
            k = x + y * w
            ip, ns, m = p1["ip"][k], ill[k], int(p1["mat"][k])
            u, v = prev.point_to_uv(ip)
            uu, vv = fadd(u, hw), fadd(v, hh)
            valid = uu >= f32(0.0) and uu < f32(1.0) and vv >= f32(0.0) and vv < f32(1.0)  # IsValid
            if not valid:
                for name, c in (("u<0", uu < 0), ("u>=1", uu >= 1), ("v<0", vv < 0), ("v>=1", vv >= 1)):
                    if c:
                        arms.add(("invalid", name))
            use = valid
            if valid:  # IsOccludedPrevFrame (renderer.cpp:767-774)
                dn = nz(normalize(fsub(ip, prev.pos)))
                pos = nz(offset_ray(ip, -dn))
                occ = Ray(prev.pos, dn, t=nz(length(fsub(pos, prev.pos))))
                use = not s.is_occluded(occ)
                arms.add(("valid", "visible" if use else "occluded"))
            fin = ns
            if use:
                # SampleHistory (renderer.cpp:777-830)
                ptx, pty = fmul(fsub(uu, hw), f32(w)), fmul(fsub(vv, hh), f32(h))
                tlx, tly = trunc_i32(ptx), trunc_i32(pty)
                fx, fy = fsub(ptx, f32(tlx)), fsub(pty, f32(tly))
                gx, gy = fsub(f32(1), fx), fsub(f32(1), fy)
                taps = [(tlx, tly, gx, gy), (tlx + 1, tly, fx, gy), (tlx, tly + 1, gx, fy), (tlx + 1, tly + 1, fx, fy)]
                ok = [on_screen(tx, ty, w, h) for tx, ty, _, _ in taps]
                wt = [fmul(a, b) if o else f32(0.0) for (_, _, a, b), o in zip(taps, ok)]
                total = fadd(fadd(fadd(wt[0], wt[1]), wt[2]), wt[3])
                rtw = fdiv(f32(1.0), total)
                wt = [fmul(q, rtw) for q in wt]
                hs = v3(0, 0, 0)
                for (tx, ty, _, _), o, q in zip(taps, ok, wt):
                    if o:
                        hs = fadd(hs, fmul(hist[ty * w + tx, :3], q))
                if ptx < 0 and tlx == 0:
                    arms.add(("tap0", "negative x"))
                if pty < 0 and tly == 0:
                    arms.add(("tap0", "negative y"))
                if tlx + 1 == w and ok == [True, False, True, False]:
                    arms.add(("tap off", "right"))
                if tly + 1 == h and ok == [True, True, False, False]:
                    arms.add(("tap off", "bottom"))
                # ClampHistory (renderer.cpp:856-910)
                nsy, hy = ycocg(ns), ycocg(hs)
                nvalid = 1
                avg, var = nsy, fmul(nsy, nsy)
                for ox, oy in ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)):
                    qx, qy = x + ox, y + oy
                    if on_screen(qx, qy, w, h):
                        fe = ycocg(ill[qx + qy * w])
                        avg = fadd(avg, fe)
                        var = fadd(var, fmul(fe, fe))
                        nvalid += 1
                arms.add(("neighbourhood", nvalid))
                inv = fdiv(f32(1.0), f32(nvalid))
                avg, var = fmul(avg, inv), fmul(var, inv)
                out = []
                for ch, name in enumerate(("Y", "Co", "Cg")):
                    dv = fsub(var[ch], fmul(avg[ch], avg[ch]))
                    if dv < 0:
                        arms.add(("variance clamped",))
                    sg = nz(f32(np.sqrt(std_max(f32(0.0), dv))))  # max(0.0f, .)
                    lo, hi = fsub(avg[ch], fmul(f32(0.75), sg)), fadd(avg[ch], fmul(f32(0.75), sg))
                    mn = t_fminf(hy[ch], hi)                       # clamp = fmaxf(a, fminf(f, b))
                    r = t_fmaxf(lo, mn)
                    arms.add(("clamp", name, "low" if lo > mn else ("inactive" if hy[ch] < hi else "high")))
                    out.append(r)
                hr = ycocg_to_rgb(v3(*out))
                hz = v3(*[t_fmaxf(q, f32(0.0)) for q in hr])       # fmaxf(historySample, 0.0f)
                if np.any(fbits(hz) != fbits(hr)):
                    arms.add(("fmaxf changed",))
                wgt, cls = weight_of(m)
                arms.add(("weight", cls))
                fin = fadd(ns, fmul(fsub(hz, ns), wgt))            # lerp: a + t * (b - a)
            new[k, :3] = fin
            rgb[k] = ref_tonemap(fmul(p1["alb"][k], fin))
    return new, rgb, (s.shadows, s.cells), arms


# ------------------------------------------------------------------------- cases
KAT_CAM = ((0.5, 0.5, -1.0), (0.5, 0.5, 0.5))
PX = 0.125  # one 20x12 / 16x16 pixel at the target's distance (1.5): 2 / 12 * 1.5 / 2


def _cam(dp=(0, 0, 0), dt=(0, 0, 0)):
    return (tuple(a + b for a, b in zip(KAT_CAM[0], dp)), tuple(a + b for a, b in zip(KAT_CAM[1], dt)))


OFF_CAM = ((0.52, 0.51, -1.0), (0.52, 0.51, 0.5))

# name: (W, H, depth, previous camera (pos, target), frames[, live camera: KAT_CAM])
CASES = {
    "a_depth-1": (20, 12, -1, KAT_CAM, 1),
    "a_depth0": (20, 12, 0, KAT_CAM, 1),
    "a_depth1": (20, 12, 1, KAT_CAM, 1),
    "a_depth2": (20, 12, 2, KAT_CAM, 1),
    "a_16x16": (16, 16, 1, KAT_CAM, 1),
    "b_subpixel": (20, 12, 1, _cam((0.004, -0.003, 0.002), (0.3 * PX, -0.3 * PX, 0)), 3),
    "b_subpixel_back": (20, 12, 1, _cam((-0.004, 0.003, -0.002), (-0.3 * PX, 0.3 * PX, 0)), 1),
    "c_diagonal": (20, 12, 1, _cam((0.02, -0.01, 0), (3.4 * PX, -2.3 * PX, 0)), 1),
    "c_mirrored": (20, 12, 1, _cam((-0.02, 0.01, 0), (-3.4 * PX, 2.3 * PX, 0)), 1),
    "d_occluded": (20, 12, 1, ((1.05, 0.62, -0.7), (0.3, 0.3, 0.6)), 1),
    "d_occluded_0": (20, 12, 0, ((-0.1, 0.3, -0.8), (0.7, 0.4, 0.6)), 1),
    "e_away": (20, 12, 1, ((0.5, 0.5, -1.0), (1.5, 0.5, -1.0)), 1),
    # a live camera beside the KAT position, so that no pixel centre lies on a cell boundary: the
    # 3 x 3 metal pixels all reflect the sky, a uniform neighbourhood whose variance term is < 0
    "f_uniform_metal": (20, 12, 1, OFF_CAM, 1, OFF_CAM),
    # TraceReproject's Illumination calls with spot and area lights (3 samples), two frames
    "g_mixed_lights": (20, 12, 1, _cam((0.004, -0.003, 0.002), (0.3 * PX, -0.3 * PX, 0)), 2),
}
LIGHTS = {"g_mixed_lights": MIXED}


def crafted_history(w, h):
    """uniform [0, 8) from a fixed seed; whole rows at 0 and at 1e4; rows of small values on
    the gamut's edge (one channel exactly 0); the unused w lane holds a sentinel."""
    rng = np.random.default_rng(20241)
    hist = rng.uniform(0, 8, (h, w, 4)).astype(np.float32)
    small = rng.uniform(0.001, 0.05, (h, w, 3)).astype(np.float32)
    for y in range(h):
        if y % 6 == 1:
            hist[y, :, :3] = 0
        elif y % 6 == 4:
            hist[y, :, :3] = 1e4
        elif y % 6 in (2, 3):
            hist[y, :, :3] = small[y]
            hist[y, :, 2 - (y // 6) % 3] = 0
    hist[:, :, 3] = SENTINEL
    return hist.reshape(w * h, 4)


_EXPECTED = {}


def live_of(name):
    return CASES[name][5] if len(CASES[name]) > 5 else KAT_CAM


def expected_case(name):
    """Per frame: the history on entry, the new history, RGB8, (shadow, bounce, cells), probes;
    and the union of the arms.  Computed once per process."""
    if name in _EXPECTED:
        return _EXPECTED[name]
    w, h, depth, prev_pt, frames = CASES[name][:5]
    live = live_of(name)
    prev = Camera(prev_pt[0], prev_pt[1], w, h)
    hist = crafted_history(w, h)
    out, arms = [], set()
    for f in range(frames):
        p1 = pass1(w, h, depth, f, live, LIGHTS.get(name))
        new, rgb, (sh2, cells2), a = pass2(p1, w, h, prev, hist)
        arms |= a
        bounce = p1["nearest"] - (w * h if depth >= 0 else 0)  # vpx_stats: FindNearest calls past the primary
        out.append(dict(hist_in=hist.copy(), hist=new, rgb=rgb, ill=p1["ill"], probes=p1["probes"],
                        counts=(p1["shadows"] + sh2, bounce, p1["cells"] + cells2)))
        hist = new.copy()  # illuminationHistoryBuffer = tempIlluminationBuffer
    _EXPECTED[name] = (out, arms)
    return _EXPECTED[name]


@pytest.fixture(scope="module")
def expected():
    return {name: expected_case(name) for name in CASES}


def scene_desc(pkg, w, h, depth, live=KAT_CAM, lights=None):
    cells, mats, _, d = reproject_scene()
    points, kw = scene_lights(lights)
    desc = to_oracle(pkg, None, cells, mats, points, d, [Vol(cells, N)], **kw)
    desc = desc.with_size(w, h)
    desc._cam_pos, desc._cam_target = live
    desc.camera = pkg.scene.look_at(live[0], live[1], w, h)
    desc.max_bounces = depth
    desc.flags = 0
    desc.sky = SKY
    return desc


# ------------------------------------------------------------------------- tests
CAMERA_PAIRS = [
    KAT_CAM,
    ((0.37, 1.9, -0.4), (0.52, 0.1, 0.3)),        # steeply down
    ((0.5, 0.5, -1.0), (1.5, 0.5, -1.0)),         # ahead = (1, 0, 0): zero components
    ((1.25, 0.9, -0.35), (0.45, 0.15, 0.55)),
    ((-0.3, 0.21, 0.77), (0.9, 0.63, -0.18)),     # looking towards -z
    ((0.513, 0.497, -1.003), (0.5375, 0.4625, 0.5)),
    ((2.1, 0.05, 1.4), (-0.6, 0.35, 0.2)),
]


@pytest.mark.parametrize("w,h", [(20, 12), (16, 16)])
def test_camera_basis_and_frustum_normals(pkg, w, h):
    """vpx_camera_look_at and vpx_prev_camera_look_at equal Camera::HandleInput(0) +
    SetFrustumNormals + CopyToPrevCamera bit for bit."""
    for pos, tgt in CAMERA_PAIRS:
        want = Camera(pos, tgt, w, h)
        cam = pkg.scene.look_at(pos, tgt, w, h)
        pc = pkg.scene.prev_camera(pos, tgt, w, h)
        for got, exp, what in ((cam.cam_pos, want.pos, "camPos"), (cam.top_left, want.top_left, "topLeft"),
                               (cam.top_right, want.top_right, "topRight"),
                               (cam.bottom_left, want.bottom_left, "bottomLeft"), (cam.right, want.right, "right"),
                               (cam.up, want.up, "up"), (pc.cam_pos, want.pos, "prev camPos"),
                               (pc.left_normal, want.left_n, "leftNormal"),
                               (pc.right_normal, want.right_n, "rightNormal"),
                               (pc.top_normal, want.top_n, "topNormal"),
                               (pc.bottom_normal, want.bottom_n, "bottomNormal")):
            assert np.array_equal(fbits(np.array(got[:], np.float32)), fbits(exp)), (pos, tgt, what, got[:], exp)
    steep = Camera(*CAMERA_PAIRS[1], w, h)
    assert steep.ahead[1] < -0.9 and np.any(Camera(*CAMERA_PAIRS[2], w, h).ahead == 0)


def _prev_struct(pkg, name):
    w, h, _, prev_pt, _ = CASES[name][:5]
    return pkg.scene.prev_camera(prev_pt[0], prev_pt[1], w, h)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_restatement(pkg, orc, expected, name):
    """oracle_render_reproject: the same history bits, RGB8 words and shadow / bounce / cell
    counts as the restatement, frame after frame with the history fed back."""
    w, h, depth, _, frames = CASES[name][:5]
    desc = scene_desc(pkg, w, h, depth, live_of(name), LIGHTS.get(name))
    o = orc.Oracle(pkg.abi, desc)
    prev = _prev_struct(pkg, name)
    out, _ = expected[name]
    hist = out[0]["hist_in"].copy()
    for f in range(frames):
        rgb, st = o.render_reproject(desc.frame_params(f), prev, hist)
        e = out[f]
        print(name, f, "counts", (st.shadow_rays, st.bounce_rays, st.dda_cells), e["counts"])
        bad = np.flatnonzero(np.any(fbits(hist) != fbits(e["hist"]), axis=1))
        assert bad.size == 0, (name, f, "history", bad[:8], hist[bad[:4]], e["hist"][bad[:4]])
        assert np.array_equal(rgb, e["rgb"]), (name, f, "rgb8")
        assert (st.shadow_rays, st.bounce_rays, st.dda_cells) == e["counts"], (name, f)


def test_away_history_is_pass1_illumination(expected):
    """Set-up (e): no pixel is valid, so the new history is pass 1's illumination exactly."""
    out, arms = expected["e_away"]
    assert np.array_equal(fbits(out[0]["hist"][:, :3]), fbits(out[0]["ill"]))
    assert not any(a[0] == "valid" for a in arms)


NEED = ({("valid", "visible"), ("valid", "occluded"),
         ("invalid", "u<0"), ("invalid", "u>=1"), ("invalid", "v<0"), ("invalid", "v>=1"),
         ("tap0", "negative x"), ("tap0", "negative y"), ("tap off", "right"), ("tap off", "bottom"),
         ("neighbourhood", 4), ("neighbourhood", 6), ("neighbourhood", 9),
         ("fmaxf changed",), ("variance clamped",)}
        | {("clamp", ch, arm) for ch in ("Y", "Co", "Cg") for arm in ("low", "high", "inactive")}
        | {("weight", c) for c in ("non_metal", "metal", "glass", "smoke", "emissive", "default", "none")})


def test_reprojection_arms_are_covered(expected):
    """A condition on the case set, not a measurement: the restatement alone reaches every
    arm the cases exist for."""
    arms = set()
    for name in CASES:
        arms |= expected[name][1]
    assert NEED <= arms, sorted(NEED - arms, key=str)
    # the weight classes come from the materials the frame sees, material 4 among the non-metals
    mats = set(int(m) for m in pass1(20, 12, 1, 0, KAT_CAM)["mat"])
    assert {0, 4, 6, 8, 11, 15, 20, NONE} <= mats, mats
    assert expected["a_depth1"][0][0]["probes"] > 0
    # the mixed set: every light drawn in pass 1, by the smoke probe too, with every area outcome
    picks = [p for f in range(2) for p in pass1(20, 12, 1, f, KAT_CAM, MIXED)["picks"]]
    assert {p[2] for p in picks} == set(range(7)), sorted({p[2] for p in picks})
    assert {o for p in picks if p[0] == "area" for o in p[3]} == {"rejected", "occluded", "lit"}
    assert {p[3] for p in picks if p[0] == "spot"} == {"outside", "lit", "occluded"}
    assert expected["g_mixed_lights"][0][0]["probes"] > 0


GPU_PIPELINED = "b_subpixel"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES) + [GPU_PIPELINED + "+pipeline2"])
def test_device_equals_restatement(pkg, expected, name):
    """vpx_render_reproject on the GPU: history bits, RGB8, the three counts and the player
    light's probe count equal the restatement's (no oracle in between); one case again with
    frames in flight (vpx_set_pipeline(2)), which must not change a static-camera frame."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    name, _, pipe = name.partition("+")
    w, h, depth, _, frames = CASES[name][:5]
    desc = scene_desc(pkg, w, h, depth, live_of(name), LIGHTS.get(name))
    prev = _prev_struct(pkg, name)
    out, _ = expected[name]
    ctx = pkg.context.Context(0)
    try:
        ctx.load_scene(desc)
        if pipe:
            ctx.set_pipeline(2)
        hist = torch.from_numpy(out[0]["hist_in"].copy()).cuda().reshape(-1)
        rgb = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for f in range(frames):
            ctx.player_light(reset=True)
            st = ctx.render_reproject(desc.frame_params(f), prev, hist.data_ptr(), rgb.data_ptr(), stats=True)
            ctx.synchronize()
            e = out[f]
            got = hist.cpu().numpy().reshape(-1, 4)
            print(name, f, "counts", (st.shadow_rays, st.bounce_rays, st.dda_cells), e["counts"])
            bad = np.flatnonzero(np.any(fbits(got) != fbits(e["hist"]), axis=1))
            assert bad.size == 0, (name, f, "history", bad[:8], got[bad[:4]], e["hist"][bad[:4]])
            assert np.array_equal(rgb.cpu().numpy().view(np.uint32), e["rgb"]), (name, f, "rgb8")
            assert (st.shadow_rays, st.bounce_rays, st.dda_cells) == e["counts"], (name, f)
            assert ctx.player_light().probes == e["probes"], (name, f)
    finally:
        ctx.close()
