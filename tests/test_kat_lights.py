"""Spot lights, area lights and the light pick: the oracle against test_kat_paths' numpy Trace (CPU).

Scene.illumination restates Renderer::Illumination (renderer.cpp:738-764: point, then AREA, then
spot, then directional), SpotLightEvaluate (:133-159) and AreaLightEvaluation (:161-207) from the
reference text.  Here oracle_trace is compared with it bit for bit (a NaN's sign and payload apart),
together with the shadow-ray and DDA-cell counts, in the 16^3 KAT room over the rays of
test_kat_paths.CASES that reach a lit material: the floor ("default"), the wall ("non_metal") and
the smoke block, whose probe in volume 0 draws a light and discards the result ("smoke_outside").

  light sets   mixed (2 point + 2 area + 2 spot + directional), areas only, spots only, and a wide set
               of 18 lights + directional whose indices share buckets modulo 16
  samples      1, 3, 15, and 0 (0 / 0: the path carries NaN)
  depths       1 over SEEDS; test_kat_paths.DEPTHS over SEEDS[:8] (the stream after an area light's draws)
  spot edges   positions derived from the restated hit point: cos == angle, alpha == 1, cos one ulp to
               either side of angle, a spot on the far side of the floor
  dst = 0      a point light and a spot exactly at the hit point (CPU only: non-finite directions)
  two volumes  the mixed set with a second, rotated and scaled volume

test_light_arms_are_covered is a condition on the case set, computed from the restatement alone.
Every expected value is computed once per process and shared with tests/test_kat_lights_gpu.py.
"""
import numpy as np
import pytest

from test_kat_paths import (CASES, DEPTHS, N, SEEDS, Ray, Rng, Scene, Vol, _messy_volume, api_rays, dot, f32, fbits,
                            kat_scene, length, normalize, sub, to_oracle, v3)

pytestmark = [pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning"),   # 1 / 0 = inf, as the reference
              pytest.mark.filterwarnings("ignore:invalid value:RuntimeWarning")]    # 0 / 0, 0 * inf = NaN, as the reference

SKY = (0.392, 0.584, 0.829)
RAYS = {c[0]: c[2] for c in CASES if c[0] in ("default", "non_metal", "smoke_outside")}
FIRST = {"default": 20, "non_metal": 0, "smoke_outside": 11}  # the material each ray reaches first
WHITE = (1.0, 0.95, 0.9)


def unit(*a):
    return tuple(float(x) for x in normalize(v3(*a)))


# ------------------------------------------------------------------------- light sets
# The hit points: the floor at about (0.50, 0.125, 0.58), normal +y, behind the gap between the glass
# block (x in [3/16, 6/16)) and the smoke block (x in [9/16, 12/16)), both y in [2/16, 5/16), z in
# [6/16, 9/16); the wall at about (0.49, 0.52, 0.75), normal -z; the smoke block's front at about
# (0.66, 0.24, 0.375), normal -z.  RandomDirection draws from the positive octant only, so an area
# light's samples lie in center + radius * [0, 1]^3.
P_ROOM = ((0.5, 0.9, 0.2), WHITE)                       # kat_scene's own point light
P_LOW = ((0.1, 0.2, 0.45), (0.8, 0.9, 1.0))             # behind the glass block, seen from the floor point
A_FRONT = ((0.3, 0.8, -0.6), (1.0, 1.0, 1.0), 1.2, 0.3)  # in front of the room: nothing in the way
A_FLOOR = ((0.5, 0.0, 0.2), (1.0, 0.9, 0.8), 1.5, 0.25)  # straddles the floor's plane: samples below it are rejected
A_BACK = ((0.45, 0.45, 0.9), (0.9, 1.0, 0.9), 2.0, 0.1)  # behind the wall: every sample rejected from the wall and the smoke
A_SIDE = ((0.8, 0.12, 0.4), (1.0, 0.8, 0.9), 1.1, 0.12)  # beside the smoke block: some samples behind it from the floor
S_FRONT = ((0.5, 0.6, -0.5), unit(0.0, 0.1, -1.0), (1.5, 1.4, 1.3), 0.9)   # wide: every hit point inside the cone
S_GLASS = ((0.2, 0.2, 0.2), unit(-0.6, 0.15, -0.75), (1.2, 1.3, 1.5), 0.5)  # the glass block shadows the floor point
S_NARROW = ((0.2, 0.5, 0.1), unit(-0.4, -0.02, -0.9), (1.5, 1.5, 1.5), 0.995)  # aimed at the wall point only


def wide_lights():
    """Six lights of each kind placed round the room by formula: 18 + the directional light, so the
    randLightIndex values 0..2 and 16..18 share the buckets 0..2."""
    points = [((0.15 + 0.14 * k, 0.35 + 0.09 * k, 0.05 + 0.11 * (k % 3)), (1.0 - 0.05 * k, 0.9, 0.8 + 0.03 * k)) for k in range(6)]
    areas = [A_FRONT, A_FLOOR, A_BACK, A_SIDE, ((0.1, 0.5, 0.1), WHITE, 0.9, 0.2), ((0.6, 0.7, -0.2), WHITE, 1.3, 0.15)]
    spots = [S_FRONT, S_GLASS, S_NARROW, ((0.8, 0.3, 0.1), unit(0.3, 0.2, -0.9), WHITE, 0.8),
             ((0.5, 0.95, 0.5), unit(0.0, 1.0, -0.1), WHITE, 0.7), ((0.7, 0.2, 0.2), unit(0.1, -0.1, -1.0), WHITE, 0.97)]
    return dict(points=points, areas=areas, spots=spots)


LIGHT_SETS = {
    "mixed": dict(points=[P_ROOM, P_LOW], areas=[A_FRONT, A_FLOOR], spots=[S_FRONT, S_GLASS]),
    "areas": dict(points=[], areas=[A_FRONT, A_BACK, A_SIDE], spots=[]),
    "spots": dict(points=[], areas=[], spots=[S_FRONT, S_GLASS, S_NARROW]),
    "wide": wide_lights(),
}
SAMPLES = (1, 3, 15, 0)
# (light set, area samples, second volume): depth 1 over SEEDS for every row; the rows of DEEP again at DEPTHS
SHALLOW = [(s, n, False) for s in LIGHT_SETS for n in SAMPLES if not (s == "spots" and n != 3)] + [("mixed", 3, True)]
DEEP = SHALLOW
RUNS = [(cfg, 1) for cfg in SHALLOW] + [(cfg, d) for cfg in DEEP for d in DEPTHS]


def seeds_of(depth):
    return SEEDS if depth == 1 else SEEDS[:8]


def lights_of(lights):
    """A light set as the restatement holds it: points as (v3, v3), the rest as Scene takes them."""
    return dict(points=[(v3(*p), v3(*c)) for p, c in lights["points"]], spots=list(lights["spots"]), areas=list(lights["areas"]))


def volumes(cells, second):
    return [Vol(cells, N), _messy_volume(cells)] if second else [Vol(cells, N)]


def build(pkg, lights, second=False):
    """(SceneDesc, a factory of fresh restatement scenes) of the KAT room (wall of material 0) with the
    light set: one scene for all three rays, so that a device call can batch them."""
    cells, mats, _, d = kat_scene(0)
    L = lights_of(lights)
    vols = volumes(cells, second)
    desc = None if pkg is None else to_oracle(pkg, None, cells, mats, L["points"], d, vols, spots=L["spots"], areas=L["areas"])

    def fresh(samples):
        s = Scene(vols, mats, L["points"], d, sky=SKY, spots=L["spots"], areas=L["areas"])
        s.area_samples = samples
        return s
    return desc, fresh


def restate(fresh, samples, rays, depth, seeds):
    """The numpy Trace over rays x seeds (ray-major): radiance [n, 3], shadow rays, DDA cells, the
    picks per path and the arms."""
    rad, shadows, cells, picks, arms = [], 0, 0, [], set()
    for o, dd, inside in rays:
        for seed in seeds:
            s = fresh(samples)
            rad.append(s.trace(Ray(v3(*o), v3(*dd), inside=inside), depth, Rng(seed)))
            shadows, cells = shadows + s.shadows, cells + s.cells
            picks.append(s.picks)
            arms |= s.arms
    return dict(rad=np.array(rad, np.float32), shadows=shadows, cells=cells, picks=picks, arms=arms)


_EXPECTED = {}


def expected(cfg, depth):
    """restate() of a RUNS row over the three rays, computed once per process."""
    key = (cfg, depth)
    if key not in _EXPECTED:
        name, samples, second = cfg
        _, fresh = build(None, LIGHT_SETS[name], second)
        _EXPECTED[key] = restate(fresh, samples, list(RAYS.values()), depth, seeds_of(depth))
    return _EXPECTED[key]


def batch(abi, rays, seeds):
    """rays x seeds, ray-major, as restate() orders them: (abi.Ray array, uint32 states)."""
    return (api_rays(abi, [(o, dd, 1e34, inside) for o, dd, inside in rays for _ in seeds]),
            np.array(list(seeds) * len(rays), np.uint32))


def same_radiance(got, want, what):
    """Bit for bit, a NaN's sign and payload apart."""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert g.shape == w.shape, what
    gn, wn = np.isnan(g), np.isnan(w)
    bad = np.argwhere((gn != wn) | ((fbits(g) != fbits(w)) & ~gn))
    assert not len(bad), (what, len(bad), bad[:4], g[bad[0][0]], w[bad[0][0]])


def run_id(run):
    (name, samples, second), depth = run
    return f"{name}{'+vol2' if second else ''}-s{samples}-d{depth}"


# ------------------------------------------------------------------ oracle == restatement
@pytest.mark.parametrize("run", RUNS, ids=[run_id(r) for r in RUNS])
def test_oracle_equals_restatement(pkg, orc, run):
    """oracle_trace over the three rays x the run's seeds: radiance, shadow rays and DDA cells."""
    cfg, depth = run
    name, samples, second = cfg
    desc, _ = build(pkg, LIGHT_SETS[name], second)
    o = orc.Oracle(pkg.abi, desc)
    for case, (org, dirn, inside) in RAYS.items():
        h = o.find_nearest(api_rays(pkg.abi, [(org, dirn, 1e34, inside)]))[0]
        assert h.material == FIRST[case], (case, h.material)
    e = expected(cfg, depth)
    rays, seeds = batch(pkg.abi, list(RAYS.values()), seeds_of(depth))
    got, st = o.trace(rays, seeds, depth, SKY, samples)
    same_radiance(got, e["rad"], run_id(run))
    assert (st.shadow_rays, st.dda_cells) == (e["shadows"], e["cells"]), run_id(run)
    if samples == 0 and name != "spots":  # an area light was picked somewhere: 0 / 0
        assert np.isnan(e["rad"]).any() and not np.isnan(e["rad"]).all(), run_id(run)


# ------------------------------------------------------------------------- spot edges
def hit_point(case):
    """The restated hit point and normal of a RAYS ray in the room."""
    cells, mats, points, d = kat_scene(0)
    s = Scene([Vol(cells, N)], mats, points, d)
    o, dd, inside = RAYS[case]
    r = Ray(v3(*o), v3(*dd), inside=inside)
    s.find_nearest(r)
    return r.point(), r.N


def spot_cos(ip, pos, direction):
    """cosTheta as SpotLightEvaluate computes it for the hit point ip."""
    dr = sub(v3(*pos), ip)
    dn = (dr / length(dr)).astype(np.float32)
    return dn, dot(dn, v3(*direction))


def edge_sets():
    """name -> (lights, the ray, the outcome every pick of the spot must have, alpha == 1).  Each set
    holds one spot (and the directional light, so lightCount is 2); the positions come from the floor
    ray's restated hit point."""
    ip, n = hit_point("default")
    assert np.array_equal(n, v3(0, 1, 0))
    above = (ip[0], f32(ip[1] + f32(0.5)), ip[2])  # dir = (0, dy, 0) exactly, so dn = (0, 1, 0)
    below = (ip[0], f32(ip[1] - f32(0.5)), ip[2])  # the far side of the floor: dn = (0, -1, 0)
    dn, c = spot_cos(ip, above, (0, 1, 0))
    assert np.array_equal(dn, v3(0, 1, 0)) and c == f32(1.0)
    dn, c = spot_cos(ip, below, (0, -1, 0))
    assert np.array_equal(dn, v3(0, -1, 0)) and c == f32(1.0)
    # a spot in general position whose cosTheta has many bits
    pos, direction = (0.42, 0.7, 0.3), unit(-0.1, 0.8, -0.5)
    _, c = spot_cos(ip, pos, direction)
    assert f32(0.5) < c < f32(1.0)
    spot = lambda p, dr, a: dict(points=[], areas=[], spots=[(p, dr, (1.5, 1.4, 1.3), a)])  # noqa: E731
    return {
        "cos == angle == 1": (spot(above, (0, 1, 0), 1.0), "outside", False),
        "straight on, alpha == 1": (spot(above, (0, 1, 0), 0.25), "lit", True),
        "cos == angle": (spot(pos, direction, c), "outside", False),
        "cos one ulp below angle": (spot(pos, direction, np.nextafter(c, f32(2))), "outside", False),
        "cos one ulp above angle": (spot(pos, direction, np.nextafter(c, f32(-2))), "lit", False),
        "far side of the floor": (spot(below, (0, -1, 0), 0.25), "occluded", False),
    }


_EDGES = {}


def edge_expected(name):
    if name not in _EDGES:
        lights, outcome, alpha_one = edge_sets()[name]
        _, fresh = build(None, lights)
        e = restate(fresh, 3, [RAYS["default"]], 1, SEEDS)
        got = [p[3] for path in e["picks"] for p in path[:1] if p[0] == "spot"]  # the floor's own pick, not the bounce's
        assert len(got) >= 6 and set(got) == {outcome}, (name, got)
        if alpha_one:  # lightIntensity * k * 1: the spot's term is col * albedo / dst^2 * lightCount exactly
            s = fresh(3)
            ip, _ = hit_point("default")
            col, dst = v3(*lights["spots"][0][2]), f32(f32(lights["spots"][0][0][1]) - ip[1])
            want = ((col / f32(dst * dst)).astype(np.float32) * s.albedo(20)).astype(np.float32)
            assert np.array_equal(s.spot_light(_floor_ray(), s.spots[0]), want), name
        _EDGES[name] = e
    return _EDGES[name]


def _floor_ray():
    cells, mats, points, d = kat_scene(0)
    o, dd, inside = RAYS["default"]
    r = Ray(v3(*o), v3(*dd), inside=inside)
    Scene([Vol(cells, N)], mats, points, d).find_nearest(r)
    return r


EDGE_NAMES = ["cos == angle == 1", "straight on, alpha == 1", "cos == angle", "cos one ulp below angle",
              "cos one ulp above angle", "far side of the floor"]


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_spot_edges(pkg, orc, name):
    """One spot placed from the restated hit point: the reject is cos <= angle (a < would give
    1 - 0 / 0 at angle 1), alpha is exactly 1 straight on, and a spot behind the surface sends its
    shadow ray (no N.L test), which starts into the solid."""
    e = edge_expected(name)
    desc, _ = build(pkg, edge_sets()[name][0])
    o = orc.Oracle(pkg.abi, desc)
    rays, seeds = batch(pkg.abi, [RAYS["default"]], SEEDS)
    got, st = o.trace(rays, seeds, 1, SKY, 3)
    same_radiance(got, e["rad"], name)
    assert not np.isnan(e["rad"]).any(), name
    assert (st.shadow_rays, st.dda_cells) == (e["shadows"], e["cells"]), name


def test_light_at_the_hit_point(pkg, orc):
    """dst = 0 (CPU only): a point light and a spot exactly at the floor ray's hit point.  dir / 0 is
    NaN, no reject fires on a NaN cosine, and the oracle follows the restatement through it."""
    ip, _ = hit_point("default")
    here = tuple(ip)
    lights = dict(points=[(here, WHITE)], areas=[], spots=[(here, (0.0, 1.0, 0.0), (1.5, 1.4, 1.3), 0.5)])
    desc, fresh = build(pkg, lights)
    e = restate(fresh, 3, [RAYS["default"]], 1, SEEDS)
    first = [path[0][0] for path in e["picks"]]
    assert first.count("point") >= 4 and first.count("spot") >= 4, first
    nan = np.isnan(e["rad"]).any(axis=1)
    assert np.array_equal(nan, np.array([k != "directional" for k in first])), (nan, first)
    o = orc.Oracle(pkg.abi, desc)
    rays, seeds = batch(pkg.abi, [RAYS["default"]], SEEDS)
    got, st = o.trace(rays, seeds, 1, SKY, 3)
    same_radiance(got, e["rad"], "dst = 0")
    assert (st.shadow_rays, st.dda_cells) == (e["shadows"], e["cells"])


# ---------------------------------------------------------------------- coverage gate
def test_light_arms_are_covered():
    """From the restatement alone, over every run above: every kind is picked and, within each kind,
    every index of every set; a spot is outside its cone, lit and occluded; an area sample is
    rejected, occluded and lit; some pick has every sample rejected and some has all 15 lit; in the
    wide set two picked lights share a bucket modulo 16; and the runs with a second volume, with 0
    samples and past depth 1 draw area lights."""
    arms, by_set = set(), {}
    all_rejected = all_15_lit = False
    for cfg, depth in RUNS:
        e = expected(cfg, depth)
        arms |= e["arms"]
        seen = by_set.setdefault(cfg[0], set())
        area = 0
        for path in e["picks"]:
            for kind, k, idx, outcome in path:
                seen.add((kind, k, idx))
                if kind == "area":
                    area += 1
                    assert len(outcome) == cfg[1]
                    all_rejected |= len(outcome) >= 3 and set(outcome) == {"rejected"}
                    all_15_lit |= len(outcome) == 15 and set(outcome) == {"lit"}
        if LIGHT_SETS[cfg[0]]["areas"]:
            assert area >= 4, (cfg, depth, area)
    for name, L in LIGHT_SETS.items():
        want = ({("point", k) for k in range(len(L["points"]))} | {("area", k) for k in range(len(L["areas"]))}
                | {("spot", k) for k in range(len(L["spots"]))} | {("directional", 0)})
        got = {(kind, k) for kind, k, _ in by_set[name]}
        assert want == got, (name, sorted(want - got))
    need = ({("spot", o) for o in ("outside", "lit", "occluded")} | {("area sample", o) for o in ("rejected", "occluded", "lit")}
            | {("light", k, 0) for k in ("point", "area", "spot", "directional")})
    assert need <= arms, sorted(need - arms)
    assert all_rejected and all_15_lit, (all_rejected, all_15_lit)
    idx = {i for _, _, i in by_set["wide"]}
    assert len(LIGHT_SETS["wide"]["points"]) + len(LIGHT_SETS["wide"]["areas"]) + len(LIGHT_SETS["wide"]["spots"]) >= 17
    assert any(i + 16 in idx for i in idx), sorted(idx)
    # the pick order: in the mixed set the indices 2, 3 are the areas and 4, 5 the spots
    assert {(k, i) for k, _, i in by_set["mixed"]} == {("point", 0), ("point", 1), ("area", 2), ("area", 3), ("spot", 4),
                                                       ("spot", 5), ("directional", 6)}
    # deeper than one bounce some path draws again after an area light's draws
    after = 0
    for cfg in DEEP:
        for depth in DEPTHS:
            for path in expected(cfg, depth)["picks"]:
                kinds = [p[0] for p in path]
                after += int("area" in kinds[:-1])
    assert after >= 10, after
