"""The analytic geometry restated in numpy float32 straight from the reference text.

Independent of oracle/vpx_oracle.c and of the kernels; built on the machinery of
test_kat_paths.py (Scene, Vol, Ray, Rng and the float32 helpers).  Every operation is the
reference's, in its operand order, rounded to float32 after each step.  A plain module: the
CPU file test_kat_shapes.py compares the oracle with it, the GPU file test_kat_shapes_gpu.py
the device, bit for bit.

  Sphere::Hit / IsHit            src/BVH/Shapes.h:12-63
  Triangle::Hit / IsHit          src/BVH/Shapes.h:79-139 (position added to each vertex first)
  Renderer::FindNearest          renderer.cpp:995-1016, the shape stage: a fresh Ray{O, D}
                                 (D normalised again, t = 1e34, scene.cpp:83-93), spheres then
                                 triangles, taken only if ray.t > sphereHit.t
  Renderer::IsOccluded           renderer.cpp:231-240: IsHit over spheres, then triangles, on
                                 the caller's ray
  BasicBVH::IntersectTri / IntersectAABB / IntersectBVH   src/BVH/BasicBVH.cpp:18-61
  cross / sqrLength / float3 operators   template/tmpl8math.h:2496-2499, 2304-2307, 1755-1763,
                                 1962-1965; min / max are std::min / std::max (precomp.h:34)

Taken as decided, not derived from the reference:
  * a shape win (voxel index -1) that reaches the glass or smoke branch with the inside flag
    set runs no exit march (the reference would index voxelVolumes[-1]); DESIGN.md section 3;
  * no subnormal intermediates: the oracle and the device flush them (FTZ / DAZ) and numpy
    does not, so every operation here asserts that neither its operands nor its result are
    subnormal.  That is a condition on the inputs of a case, not a tolerance.
"""
import numpy as np

from test_kat_paths import BIG, NONE, Ray, Scene, f32, std_max, std_min, v3

TINY = f32(2.0 ** -126)
EPS = f32(0.0001)  # the 0.0001f of Shapes.h:89, 98, 130 and BasicBVH.cpp:24, 33


# ------------------------------------------------------- checked float32 arithmetic
def nz(x):
    """x, after asserting that it holds no subnormal."""
    a = np.abs(np.asarray(x, np.float32))
    assert not np.any((a > 0) & (a < TINY)), ("subnormal intermediate: choose other inputs", x)
    return x


def fa(a, b):
    return nz((np.asarray(nz(a), np.float32) + np.asarray(nz(b), np.float32)).astype(np.float32))


def fs(a, b):
    return nz((np.asarray(nz(a), np.float32) - np.asarray(nz(b), np.float32)).astype(np.float32))


def fm(a, b):
    return nz((np.asarray(nz(a), np.float32) * np.asarray(nz(b), np.float32)).astype(np.float32))


def fd(a, b):
    return nz((np.asarray(nz(a), np.float32) / np.asarray(nz(b), np.float32)).astype(np.float32))


def fsqrt(a):
    return nz(np.sqrt(np.asarray(nz(a), np.float32)).astype(np.float32))


def cdot(a, b):  # tmpl8math.h: a.x*b.x + a.y*b.y + a.z*b.z, left to right
    return f32(fa(fa(fm(a[0], b[0]), fm(a[1], b[1])), fm(a[2], b[2])))


def ccross(a, b):  # tmpl8math.h:2496-2499
    return v3(fs(fm(a[1], b[2]), fm(a[2], b[1])), fs(fm(a[2], b[0]), fm(a[0], b[2])),
              fs(fm(a[0], b[1]), fm(a[1], b[0])))


def cnormalize(v):  # v * rsqrtf(dot(v, v)), rsqrtf = 1.0f / sqrtf (tmpl8math.h:411-414, 2350-2354)
    return fm(v, fd(f32(1.0), fsqrt(cdot(v, v))))


def make_ray(o, d, t=BIG, inside=False, raw=False):
    """Ray(origin, direction) (scene.cpp:83-93), t and isInsideGlass then set by the caller;
    raw: the five-argument constructor (scene.cpp:29-37), D used as given."""
    r = Ray(o, d, t, bool(inside))
    if raw:
        r.D = np.asarray(d, np.float32).copy()
    else:
        assert np.array_equal(r.D.view(np.uint32), cnormalize(np.asarray(d, np.float32)).view(np.uint32))
    nz(r.O), nz(r.D), nz(r.t)
    return r


# ------------------------------------------------------------------------ shapes
def sphere(center, radius, material):
    return (v3(*center), f32(radius), int(material))


def triangle(position, v0, v1, v2, material):
    return (v3(*position), v3(*v0), v3(*v1), v3(*v2), int(material))


def _sphere_len(sp, r, arms, fn):
    """The shared head of Sphere::Hit / IsHit (Shapes.h:14-25, 46-57): rayLength, or None."""
    center, radius, _ = sp
    to = fs(r.O, center)
    b = cdot(to, r.D)
    c = f32(fs(cdot(to, to), fm(radius, radius)))
    disc = f32(fs(fm(b, b), c))
    if c > f32(0.0) and b > f32(0.0):
        arms.add((fn, "behind"))
        return None
    arms.add((fn, "not behind", "c <= 0" if not c > f32(0.0) else "b <= 0"))
    if disc < 0:
        arms.add((fn, "disc < 0"))
        return None
    arms.add((fn, "disc >= 0"))
    return f32(fs(-b, fsqrt(disc)))


def sphere_hit(sp, r, arms):  # Sphere::Hit, Shapes.h:12-42
    center, radius, material = sp
    ln = _sphere_len(sp, r, arms, "sphere_hit")
    if ln is None:
        return
    if ln > r.t:
        arms.add(("sphere_hit", "len > t"))
        return
    arms.add(("sphere_hit", "len <= t", "tie" if ln == r.t else "nearer"))
    if ln < 0:
        arms.add(("sphere_hit", "len < 0"))
        return
    arms.add(("sphere_hit", "len >= 0"))
    ip = fa(r.O, fm(r.D, ln))
    outn = fd(fs(ip, center), radius)
    outside = bool(cdot(r.D, outn) < 0)
    arms.add(("sphere_hit", "outside" if outside else "inside"))
    r.N = outn if outside else -outn
    r.inside = not outside
    r.t = ln
    r.mat = material


def sphere_is_hit(sp, r, arms):  # Sphere::IsHit, Shapes.h:44-63
    ln = _sphere_len(sp, r, arms, "sphere_is_hit")
    if ln is None:
        return False
    if ln < 0:
        arms.add(("sphere_is_hit", "len < 0"))
        return False
    arms.add(("sphere_is_hit", "len >= 0"))
    if ln > r.t:
        arms.add(("sphere_is_hit", "len > t"))
        return False
    arms.add(("sphere_is_hit", "len <= t", "tie" if ln == r.t else "nearer"))
    return True


def _tri_t(tr, r, arms, fn, raw_edges=False):
    """The shared head of Triangle::Hit / IsHit (Shapes.h:81-97, 113-129): (t, edge1, edge2) or
    None.  raw_edges forms the edges from the vertices without the position: NOT the
    reference; the tests use it to show that their rows tell the two readings apart."""
    pos, v0, v1, v2, _ = tr
    p1, p2, p3 = fa(pos, v0), fa(pos, v1), fa(pos, v2)
    e1, e2 = (fs(v1, v0), fs(v2, v0)) if raw_edges else (fs(p2, p1), fs(p3, p1))
    h = ccross(r.D, e2)
    a = cdot(e1, h)
    if a > -EPS and a < EPS:
        arms.add((fn, "parallel"))
        return None
    arms.add((fn, "not parallel", "a <= -eps" if not a > -EPS else "a >= eps"))
    f = f32(fd(f32(1), a))
    s = fs(r.O, p1)
    u = f32(fm(f, cdot(s, h)))
    if u < 0 or u > 1:
        arms.add((fn, "u < 0" if u < 0 else "u > 1"))
        return None
    arms.add((fn, "u in"))
    q = ccross(s, e1)
    v = f32(fm(f, cdot(r.D, q)))
    if v < 0 or f32(fa(u, v)) > 1:
        arms.add((fn, "v < 0" if v < 0 else "u + v > 1"))
        return None
    arms.add((fn, "v in"))
    return f32(fm(f, cdot(e2, q))), e1, e2


def tri_hit(tr, r, arms, raw_edges=False):  # Triangle::Hit, Shapes.h:79-109
    got = _tri_t(tr, r, arms, "tri_hit", raw_edges)
    if got is None:
        return
    t, e1, e2 = got
    if t > EPS:
        arms.add(("tri_hit", "t > eps"))
        if r.t > t:
            arms.add(("tri_hit", "nearer"))
            r.t = t
            r.mat = tr[4]
            n = cnormalize(ccross(e1, e2))
            outside = bool(cdot(r.D, n) < 0)
            arms.add(("tri_hit", "front" if outside else "back"))
            r.N = n if outside else -n
        else:
            arms.add(("tri_hit", "not nearer", "tie" if r.t == t else "farther"))
    else:
        arms.add(("tri_hit", "t <= eps", "t == eps" if t == EPS else "t < eps"))


def tri_is_hit(tr, r, arms, raw_edges=False):  # Triangle::IsHit, Shapes.h:111-139
    got = _tri_t(tr, r, arms, "tri_is_hit", raw_edges)
    if got is None:
        return False
    t = got[0]
    if t < EPS:
        arms.add(("tri_is_hit", "t < eps"))
        return False
    arms.add(("tri_is_hit", "t >= eps", "t == eps" if t == EPS else "t > eps"))
    if t > r.t:
        arms.add(("tri_is_hit", "t > ray.t"))
        return False
    arms.add(("tri_is_hit", "t <= ray.t", "tie" if t == r.t else "nearer"))
    return True


# Every early-out and both outcomes of every branch of the four functions.
ALL_ARMS = {
    ("sphere_hit", "behind"), ("sphere_hit", "not behind", "c <= 0"), ("sphere_hit", "not behind", "b <= 0"),
    ("sphere_hit", "disc < 0"), ("sphere_hit", "disc >= 0"), ("sphere_hit", "len > t"),
    ("sphere_hit", "len <= t", "tie"), ("sphere_hit", "len <= t", "nearer"), ("sphere_hit", "len < 0"),
    ("sphere_hit", "len >= 0"), ("sphere_hit", "outside"), ("sphere_hit", "inside"),
    ("sphere_is_hit", "behind"), ("sphere_is_hit", "not behind", "c <= 0"), ("sphere_is_hit", "not behind", "b <= 0"),
    ("sphere_is_hit", "disc < 0"), ("sphere_is_hit", "disc >= 0"), ("sphere_is_hit", "len < 0"),
    ("sphere_is_hit", "len >= 0"), ("sphere_is_hit", "len > t"), ("sphere_is_hit", "len <= t", "tie"),
    ("sphere_is_hit", "len <= t", "nearer"),
    ("tri_hit", "parallel"), ("tri_hit", "not parallel", "a <= -eps"), ("tri_hit", "not parallel", "a >= eps"),
    ("tri_hit", "u < 0"), ("tri_hit", "u > 1"), ("tri_hit", "u in"), ("tri_hit", "v < 0"), ("tri_hit", "u + v > 1"),
    ("tri_hit", "v in"), ("tri_hit", "t > eps"), ("tri_hit", "t <= eps", "t == eps"), ("tri_hit", "t <= eps", "t < eps"),
    ("tri_hit", "nearer"), ("tri_hit", "not nearer", "tie"), ("tri_hit", "not nearer", "farther"),
    ("tri_hit", "front"), ("tri_hit", "back"),
    ("tri_is_hit", "parallel"), ("tri_is_hit", "not parallel", "a <= -eps"), ("tri_is_hit", "not parallel", "a >= eps"),
    ("tri_is_hit", "u < 0"), ("tri_is_hit", "u > 1"), ("tri_is_hit", "u in"), ("tri_is_hit", "v < 0"),
    ("tri_is_hit", "u + v > 1"), ("tri_is_hit", "v in"), ("tri_is_hit", "t < eps"),
    ("tri_is_hit", "t >= eps", "t == eps"), ("tri_is_hit", "t >= eps", "t > eps"), ("tri_is_hit", "t > ray.t"),
    ("tri_is_hit", "t <= ray.t", "tie"), ("tri_is_hit", "t <= ray.t", "nearer"),
}


# ------------------------------------------------------------------------- scene
class ShapeScene(Scene):
    """test_kat_paths.Scene plus Renderer::spheres / triangles (renderer.h:207-208).

    shapes=False leaves the shape stage out (VPX_QUERY_NO_SHAPES); second_normalize=False and
    raw_edges are NOT the reference: they exist to show that the tests' rows are sensitive to
    those readings."""

    def __init__(self, vols, mats, points=(), spheres=(), triangles=(), shapes=True, second_normalize=True,
                 raw_edges=False, **kw):
        super().__init__(vols, mats, points, **kw)
        self.spheres, self.triangles = list(spheres), list(triangles)
        self.shapes = shapes
        self.second_normalize, self.raw_edges = second_normalize, raw_edges
        self.shape_arms = set()
        self.guards = 0

    def find_nearest(self, ray):  # Renderer::FindNearest, renderer.cpp:946-1018
        vox = super().find_nearest(ray)  # the volume loop, :952-993
        self.volume_stage = (ray.t, ray.N, ray.mat, vox, ray.inside)  # what the entries give without the shapes
        self.shape_t = None
        if not self.shapes:
            return vox
        sh = make_ray(ray.O, ray.D, raw=not self.second_normalize)  # :997 Ray sphereHit{ray.O, ray.D}
        for sp in self.spheres:
            sphere_hit(sp, sh, self.shape_arms)
        for tr in self.triangles:
            tri_hit(tr, sh, self.shape_arms, self.raw_edges)
        self.shape_t = sh.t  # 1e34: no shape on the ray
        if ray.t > sh.t:  # :1008
            ray.t, ray.mat, ray.N, ray.inside = sh.t, sh.mat, sh.N, sh.inside
            vox = -1
        return vox

    def is_occluded(self, ray):  # Renderer::IsOccluded, renderer.cpp:209-243
        self.volume_occluded = super().is_occluded(ray)  # the volume loop, :211-228
        if self.volume_occluded:
            return True
        if not self.shapes:
            return False
        for sp in self.spheres:
            if sphere_is_hit(sp, ray, self.shape_arms):
                return True
        for tr in self.triangles:
            if tri_is_hit(tr, ray, self.shape_arms, self.raw_edges):
                return True
        return False

    def exit_march(self, vox, ray, glass):
        """Scene.trace's FindMaterialExit / FindSmokeExit call.  A shape win has no volume to
        march through (the reference would index voxelVolumes[-1]): decided as no march, the ray
        untouched and insideVolume left true.  Python would index the last volume instead."""
        if vox < 0:
            assert vox == -1
            self.guards += 1
            self.arms.add(("guard", "glass" if glass else "smoke"))
            return True
        return super().exit_march(vox, ray, glass)


# --------------------------------------------------------------------------- BVH
def bvh_arrays(nodes, tri_idx, tris, used):
    """ctypes arrays of vpx_bvh_build_host as numpy: (aabb_min, aabb_max, left_first, tri_count,
    tri_idx, vertices[n, 3, 3])."""
    nd = np.frombuffer(nodes, np.uint32).reshape(-1, 8)[:used]
    v = np.frombuffer(tris, np.float32).reshape(-1, 3, 3).copy()
    return (nd[:, 0:3].copy().view(np.float32), nd[:, 3:6].copy().view(np.float32), nd[:, 6].copy(), nd[:, 7].copy(),
            np.array(tri_idx[:len(v)], np.uint32), v)


def intersect_tri(ray, v0, v1, v2):  # BasicBVH::IntersectTri, BasicBVH.cpp:18-34
    e1, e2 = fs(v1, v0), fs(v2, v0)
    h = ccross(ray.D, e2)
    a = cdot(e1, h)
    if a > -EPS and a < EPS:
        return
    f = f32(fd(f32(1), a))
    s = fs(ray.O, v0)
    u = f32(fm(f, cdot(s, h)))
    if u < 0 or u > 1:
        return
    q = ccross(s, e1)
    v = f32(fm(f, cdot(ray.D, q)))
    if v < 0 or f32(fa(u, v)) > 1:
        return
    t = f32(fm(f, cdot(e2, q)))
    if t > EPS:
        ray.t = std_min(ray.t, t)


def _fmin(a, b):  # NaN-dropping, symmetric: NOT the reference's std::min
    return f32(np.fmin(a, b))


def _fmax(a, b):
    return f32(np.fmax(a, b))


def intersect_aabb(ray, bmin, bmax, symmetric=False):  # BasicBVH::IntersectAABB, BasicBVH.cpp:36-45
    """symmetric evaluates min / max as NaN-dropping hardware operations: NOT the reference;
    the tests use it to show that their rays tell the operand order apart."""
    mn, mx = (_fmin, _fmax) if symmetric else (std_min, std_max)
    tx1, tx2 = f32(fd(fs(bmin[0], ray.O[0]), ray.D[0])), f32(fd(fs(bmax[0], ray.O[0]), ray.D[0]))
    tmin, tmax = mn(tx1, tx2), mx(tx1, tx2)
    ty1, ty2 = f32(fd(fs(bmin[1], ray.O[1]), ray.D[1])), f32(fd(fs(bmax[1], ray.O[1]), ray.D[1]))
    tmin, tmax = mx(tmin, mn(ty1, ty2)), mn(tmax, mx(ty1, ty2))
    tz1, tz2 = f32(fd(fs(bmin[2], ray.O[2]), ray.D[2])), f32(fd(fs(bmax[2], ray.O[2]), ray.D[2]))
    tmin, tmax = mx(tmin, mn(tz1, tz2)), mn(tmax, mx(tz1, tz2))
    return bool(tmax >= tmin and tmin < ray.t and tmax > 0)


def bvh_intersect(arrays, ray, symmetric=False):
    """BasicBVH::IntersectBVH(ray, 0) (BasicBVH.cpp:47-61): returns (ray.t, high-water mark).
    The mark belongs to a model of an explicit stack that holds the root, pops a node, and on
    an interior node pushes the right child, then the left, so that the left is popped first:
    the order of the recursion."""
    bmin, bmax, left_first, tri_count, tri_idx, verts = arrays
    state = {"sp": 1, "high": 1}

    def visit(i):
        state["sp"] -= 1  # pop
        if not intersect_aabb(ray, bmin[i], bmax[i], symmetric):
            return
        if tri_count[i] > 0:  # isLeaf
            for k in range(int(tri_count[i])):
                tv = verts[tri_idx[int(left_first[i]) + k]]
                intersect_tri(ray, tv[0], tv[1], tv[2])
        else:
            state["sp"] += 2  # push right, push left
            state["high"] = max(state["high"], state["sp"])
            visit(int(left_first[i]))
            visit(int(left_first[i]) + 1)

    visit(0)
    assert state["sp"] == 0
    return ray.t, state["high"]


__all__ = ["ALL_ARMS", "EPS", "NONE", "ShapeScene", "bvh_arrays", "bvh_intersect", "intersect_aabb", "make_ray",
           "sphere", "sphere_hit", "sphere_is_hit", "tri_hit", "tri_is_hit", "triangle"]
