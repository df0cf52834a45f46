"""The player light probe (Renderer::inLight, renderer.h:231) without a GPU: the C-ABI
additions, the numpy reference the GPU tests compare with, and the sharded reduce.

The probe: a path that reaches smoke (materials 9..14) in volume 0 runs
Illumination(ray, incLight) and sets inLight when sqrLength(incLight) > 16
(Trace renderer.cpp:1228-1240, TraceSmoke :1438-1450).  The reference for it is
test_kat_paths' numpy restatement of Trace, whose smoke branch already makes the call:
ProbeScene below records what that call returns.
"""
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from test_kat_paths import CASES, N, SEEDS, Ray, Rng, Scene, Vol, f32, kat_scene, v3

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLD = f32(16.0)  # sqrThreshold, renderer.cpp:1233, 1443


# ------------------------------------------------------------------- header and library
def test_header_declares_and_library_exports(pkg):
    text = open(os.path.join(REPO, "include", "vpx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("vpx_get_player_light", "vpx_trace_probe"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in pkg.abi.SIGNATURES
    assert re.search(r"#define\s+VPX_PLAYER_LIGHT_SQR\s+16\.0f", code)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (vpx_\w+)", out))
    assert {"vpx_get_player_light", "vpx_trace_probe"} <= exported
    assert pkg.abi.PLAYER_LIGHT_SQR == 16.0


def test_struct_sizes_and_fields(pkg):
    abi = pkg.abi
    assert C.sizeof(abi.PlayerLight) == 24 and C.sizeof(abi.RayProbe) == 16
    assert abi.STRUCT_SIZES[abi.PlayerLight] == 24 and abi.STRUCT_SIZES[abi.RayProbe] == 16
    assert [(n, getattr(abi.PlayerLight, n).offset) for n, _ in abi.PlayerLight._fields_] == [
        ("probes", 0), ("lit", 8), ("max_sqr", 16), ("in_light", 20)]
    assert [(n, getattr(abi.RayProbe, n).offset) for n, _ in abi.RayProbe._fields_] == [
        ("probes", 0), ("lit", 4), ("max_sqr", 8), ("reserved", 12)]
    # the header's own layout, through the compiler
    src = ('#include <cstddef>\n#include "vpx.h"\n'
           "static_assert(sizeof(vpx_player_light) == 24, \"vpx_player_light\");\n"
           "static_assert(sizeof(vpx_ray_probe) == 16, \"vpx_ray_probe\");\n"
           "static_assert(offsetof(vpx_player_light, max_sqr) == 16, \"max_sqr\");\n"
           "static_assert(offsetof(vpx_player_light, in_light) == 20, \"in_light\");\n"
           "static_assert(VPX_PLAYER_LIGHT_SQR == 16.0f && VPX_ABI_VERSION == 2, \"constants\");\n")
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(REPO, "include"), "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_arguments_and_abi_version(pkg):
    lib = pkg.load_library()
    pl = pkg.abi.PlayerLight()
    assert lib.vpx_get_player_light(None, C.byref(pl), 0) == pkg.abi.VPX_E_INVALID
    assert lib.vpx_get_player_light(None, None, 1) == pkg.abi.VPX_E_INVALID
    pr = (pkg.abi.RayProbe * 1)()
    assert lib.vpx_trace_probe(None, None, None, 0, 0, None, 3, None, pr) == pkg.abi.VPX_E_INVALID
    assert lib.vpx_abi_version() == pkg.abi.ABI_VERSION == 2


def test_python_surface(pkg):
    assert callable(pkg.context.Context.player_light) and callable(pkg.context.Context.trace_probe)
    assert callable(pkg.dist.ShardedAccumFrame.player_light)


# --------------------------------------------------------- the reference of the GPU tests
class ProbeScene(Scene):
    """test_kat_paths.Scene that records the probe: inside trace(), illumination() is called
    with a smoke material (9..14) by the probe alone (the shaded materials are 0..4 and >= 16)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.sqr = []

    def illumination(self, ray, g):
        inc = super().illumination(ray, g)
        if 9 <= ray.mat <= 14:  # sqrLength (tmpl8math.h): x*x + y*y + z*z, left to right
            self.sqr.append(f32(f32(f32(inc[0] * inc[0]) + f32(inc[1] * inc[1])) + f32(inc[2] * inc[2])))
        return inc


SMOKE_RAYS = [c[2] for c in CASES if c[0].startswith("smoke_")]
DEPTHS = (0, 1, 3)
COLOURS = (4.0, 4.5)  # the point light's (c, 0.95c, 0.9c): either side of the threshold


def probe_scene(c):
    """kat_scene(0) with the point light's colour (c, 0.95c, 0.9c)."""
    cells, mats, points, d = kat_scene(0)
    points = [(points[0][0], v3(c, 0.95 * c, 0.9 * c))]
    return cells, mats, points, d


MIXED = "mixed"  # in place of a colour: test_kat_lights' mixed set (2 point + 2 area + 2 spot + directional)


def probe_lights(c):
    """(cells, mats, points, directional light, Scene's spots / areas keywords) of a reference scene."""
    if c != MIXED:
        return probe_scene(c) + ({},)
    from test_kat_lights import LIGHT_SETS, lights_of

    cells, mats, _, d = kat_scene(0)
    kw = lights_of(LIGHT_SETS[MIXED])
    return cells, mats, kw.pop("points"), d, kw


def probe_rays():
    """(origin, direction, inside, seed) of the 48 reference rays: the two smoke rays x SEEDS."""
    return [(o, dd, inside, seed) for (o, dd, inside) in SMOKE_RAYS for seed in SEEDS]


_REF = {}


def reference(c, depth):
    """Per ray (probes, lit, bits of max_sqr) from the numpy restatement; computed once."""
    if (c, depth) not in _REF:
        cells, mats, points, d, kw = probe_lights(c)
        rows, rad, picks = [], [], []
        for o, dd, inside, seed in probe_rays():
            s = ProbeScene([Vol(cells, N)], mats, points, d, **kw)
            rad.append(s.trace(Ray(v3(*o), v3(*dd), inside=inside), depth, Rng(seed)))
            picks.append(s.picks[0])  # the first Illumination of either smoke ray is the probe's
            ok = [v for v in s.sqr if v == v]
            mx = max(ok) if ok else f32(0)
            rows.append((len(s.sqr), sum(1 for v in s.sqr if v > THRESHOLD), int(np.float32(mx).view(np.uint32))))
        _REF[(c, depth)] = np.array(rows, np.uint64)
        _RAD[(c, depth)] = (np.array(rad, np.float32), picks)
    return _REF[(c, depth)]


_RAD = {}


def reference_paths(c, depth):
    """Per ray the radiance of the same paths (what the stream gives after the probe's draws) and
    the probe's pick (kind, index, randLightIndex, outcome)."""
    reference(c, depth)
    return _RAD[(c, depth)]


def test_reference_is_not_empty():
    """The counts the GPU test stands on: probes at depth 0 and 3, none lit at c = 4.0 and some
    lit at 4.5, the maxima either side of 16, and rays that probe more than once."""
    want = {(4.0, 0): (48, 0, 13.4533), (4.0, 3): (120, 0, 13.4542),
            (4.5, 0): (48, 12, 17.0268), (4.5, 3): (120, 26, 17.0280)}
    for (c, depth), (probes, lit, mx) in want.items():
        r = reference(c, depth)
        assert (int(r[:, 0].sum()), int(r[:, 1].sum())) == (probes, lit), (c, depth)
        got = float(np.uint32(r[:, 2].max()).view(np.float32))
        assert abs(got - mx) < 1e-4, (c, depth, got)
    assert int((reference(4.5, 3)[:, 0] > 1).sum()) == 37
    assert int((reference(4.0, 3)[:, 0] > 1).sum()) == 37


@pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning")  # 1 / 0 = inf, as the reference
def test_probe_draws_area_lights(pkg, orc):
    """The probe with test_kat_lights' mixed set: a third of the probes or so draw an area light, whose
    rejection loops advance the stream that the smoke branch draws its threshold, its scatter and
    its direction from afterwards.  oracle_trace at depth 0, 1 and 3 equals the restatement on the
    same 48 rays bit for bit; the probes' own values are what the GPU test compares."""
    from test_kat_paths import api_rays, fbits, to_oracle

    cells, mats, points, d, kw = probe_lights(MIXED)
    o = orc.Oracle(pkg.abi, to_oracle(pkg, None, cells, mats, points, d, [Vol(cells, N)], **kw))
    rr = probe_rays()
    rays = api_rays(pkg.abi, [(org, dd, 1e34, inside) for org, dd, inside, _ in rr])
    seeds = np.array([s for *_, s in rr], np.uint32)
    for depth in DEPTHS:
        rows = reference(MIXED, depth)
        rad, picks = reference_paths(MIXED, depth)
        area = [p for p in picks if p[0] == "area"]
        assert len(area) >= 8 and {p[1] for p in area} == {0, 1}, picks
        assert any("lit" in p[3] for p in area) and any("rejected" in p[3] for p in area)
        assert {p[0] for p in picks} == {"point", "area", "spot", "directional"}
        assert int(rows[:, 0].sum()) >= len(rr) and 4 <= int(rows[:, 1].sum()) <= int(rows[:, 0].sum()) - 4, rows[:, :2].sum(0)
        got, _ = o.trace(rays, seeds, depth, (0.392, 0.584, 0.829), 3)
        assert not np.isnan(rad).any()
        assert np.array_equal(fbits(got), fbits(rad)), (depth, np.argwhere(fbits(got) != fbits(rad))[:4])
    # past depth 0 the radiance depends on the draws after the probe: the paths part (many end in the
    # one sky colour, so a quarter of the 48 being distinct is asked for)
    assert len({tuple(r) for r in fbits(reference_paths(MIXED, 3)[0])}) >= 12


# ---------------------------------------------------------------------- sharded reduce
class _StubCtx:
    """Stands in for the vpx context: a fixed record per rank."""

    def __init__(self, pkg, rec):
        self.pkg, self.rec, self.stream_handle, self.resets = pkg, rec, None, []

    def packed_len(self, w, h, n):
        return self.pkg.dist.packed_len(w, h, n)

    def player_light(self, reset=False):
        self.resets.append(reset)
        pl = self.pkg.abi.PlayerLight()
        pl.probes, pl.lit, pl.max_sqr = self.rec
        pl.in_light = 1 if pl.lit else 0
        return pl


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    sys.path.insert(0, REPO)
    import torch
    import torch.distributed as dist

    import __graft_entry__ as entry

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pkg = entry.load_package()
        desc = pkg.scene.model_scene("monu3", 64, 40, 24, 1)
        ctx = _StubCtx(pkg, [(5, 0, 3.0), (7, 2, 20.0)][rank])
        fr = pkg.dist.ShardedAccumFrame(ctx, desc, rank, world, torch.device("cpu"), host_gather=True)
        r = fr.player_light()
        q.put((rank, r["probes"], r["lit"], r["max_sqr"], r["in_light"], ctx.resets))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sharded_player_light_two_ranks_gloo():
    import torch.multiprocessing as mp

    q = mp.get_context("spawn").Queue()
    mp.start_processes(_worker, args=(2, _free_port(), q), nprocs=2, join=True, start_method="spawn")
    got = sorted(q.get(timeout=60) for _ in range(2))
    assert got == [(0, 12, 2, 20.0, 1, [True]), (1, 12, 2, 20.0, 1, [True])], got


# ---------------------------------------------- the two-volume scene of the GPU tests (B, C)
PLAYER_C = (0.6, 0.2125, 0.45)  # the player's centre in the room


def player_scene(pkg, width=72, height=40, max_bounces=0):
    """Volume 0: the golden player model (396 cells of SMOKE_PLAYER, 2 emissive) in a 16^3 grid,
    scaled to 0.3 and standing in the room; volume 1: a 32^3 room with a floor and a block of
    smoke (material 11) that is NOT the player.  One light of each kind, so lightCount is 4."""
    sc, abi = pkg.scene, pkg.abi
    z = np.load(os.path.join(REPO, "tests", "golden", "player.npz"))
    player = sc.load_model_grid(z["size"].astype(np.int64), z["voxels"].astype(np.uint8), 16)
    n = 32
    room = np.full((n, n, n), abi.MAT_NONE, np.uint8)  # [z][y][x]
    room[:, :2, :] = 20
    room[18:26, 2:12, 4:12] = 11
    mats = sc.default_materials()
    mats[20].albedo[0], mats[20].albedo[1], mats[20].albedo[2] = 0.45, 0.6, 0.35
    # LoadModel's palette override gives the player's smoke its colour (MaterialSetUp leaves it black)
    mats[14].albedo[0], mats[14].albedo[1], mats[14].albedo[2] = 0.8, 0.75, 0.7
    # the cube [pos, pos + 1] scaled about its centre: the player's box is PLAYER_C +- 0.15, on the floor
    vols = [sc.volume(tuple(c - 0.5 for c in PLAYER_C), (0.3, 0.3, 0.3)), sc.volume(grid_id=1)]
    pts = [sc.point_light((0.62, 0.55, 0.0), (1.6, 1.5, 1.4))]
    sps = [sc.spot_light((0.6, 0.9, 0.45), (0.0, 1.0, 0.0), (0.3, 0.28, 0.26), angle=0.8)]  # dot(to light, direction) > angle
    ars = [sc.area_light((1.3, 0.5, 0.4), (1.0, 0.95, 0.9), 1.2, 0.2)]
    dl = sc.dir_light((-0.3, -1.0, 0.4), (0.9, 0.9, 1.0))
    return sc._scene("player_light", [sc.GridSpec(n=16, dense=player), sc.GridSpec(n=n, dense=room.reshape(-1))],
                     vols, mats, pts, sps, ars, dl, (0.75, 0.45, -0.55), (0.52, 0.2, 0.45), width, height,
                     max_bounces=max_bounces, area_samples=3)


def player_rays(n_player=1500, n_block=500, seed=11):
    """Rays from around the room aimed at the player's box and at the room's smoke block, with
    an xorshift32 state each."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_player + n_block):
        if k < n_player:
            tgt = np.array(PLAYER_C) + rng.uniform(-0.13, 0.13, 3)
            th, ph = rng.uniform(0, 2 * np.pi), rng.uniform(0.05, 1.3)
            org = tgt + 0.9 * np.array([np.cos(th) * np.cos(ph), np.sin(ph), np.sin(th) * np.cos(ph)])
        else:
            tgt = np.array([0.125, 0.0625, 0.5625]) + rng.uniform(0.02, 0.23, 3) * np.array([1.0, 1.25, 1.0])
            org = np.array([rng.uniform(-0.4, 0.6), rng.uniform(0.5, 1.2), rng.uniform(-0.5, 0.3)])
        out.append((org.astype(np.float32), (tgt - org).astype(np.float32)))
    seeds = (0x9E3779B9 * (np.arange(len(out), dtype=np.uint64) + 1) % (1 << 32)).astype(np.uint32) | np.uint32(1)
    return out, seeds


# Illumination's order of the evaluators (renderer.cpp:742-760): point, area, spot, directional;
# oracle_kat_light's kinds: 0 point, 1 spot, 2 area, 3 directional.
KAT_KIND = {0: 0, 1: 2, 2: 1, 3: 3}


def player_expected(pkg, orc, desc, rays, seeds):
    """Per ray (probes, lit, bits of max_sqr, evaluator or -1, hit material, vox_index) at depth 0,
    from oracle pieces only: oracle_find_nearest for the hit; a probe exists when the hit is
    smoke (9..14) in volume 0; then idx = int(RandomFloat * lightCount) and the evaluator
    (oracle_kat_light) with the running RNG state, * lightCount, sqrLength."""
    from test_kat_paths import api_rays

    abi = pkg.abi
    o = orc.Oracle(abi, desc)
    lib = o.lib
    P = C.POINTER
    F3 = P(C.c_float)
    lib.oracle_kat_light.argtypes = [C.c_void_p, C.c_int, C.c_uint32, F3, F3, C.c_float, F3, C.c_uint32, C.c_int32,
                                     P(C.c_uint32), F3]
    arr = api_rays(abi, [(org, d, 1e34, False) for org, d in rays])
    hits = o.find_nearest(arr)
    lc = len(desc.points) + len(desc.spots) + len(desc.areas) + 1
    rows = []
    for i, (org, d) in enumerate(rays):
        h = hits[i]
        row = [0, 0, 0, -1, int(h.material), int(h.vox_index)]
        if h.vox_index == 0 and 9 <= h.material <= 14:
            s = C.c_uint32(int(seeds[i]))
            idx = int(f32(f32(lib.oracle_random_float(C.byref(s))) * f32(lc)))
            out = np.zeros(3, np.float32)
            oo, dd = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(d, np.float32)
            nn = np.array(h.normal[:], np.float32)
            assert lib.oracle_kat_light(o.ptr, KAT_KIND[idx], 0, oo.ctypes.data_as(F3), dd.ctypes.data_as(F3),
                                        C.c_float(h.t), nn.ctypes.data_as(F3), h.material, desc.area_samples,
                                        C.byref(s), out.ctypes.data_as(F3)) == 0
            inc = (out * f32(lc)).astype(np.float32)
            v = f32(f32(f32(inc[0] * inc[0]) + f32(inc[1] * inc[1])) + f32(inc[2] * inc[2]))
            row[:4] = [1, int(v > THRESHOLD), int(np.float32(v if v == v else 0).view(np.uint32)), idx]
        rows.append(row)
    return np.array(rows, np.int64)


_PLAYER = {}


def player_case(pkg, orc):
    """(desc, rays, seeds, expected) of GPU test B; computed once."""
    if not _PLAYER:
        desc = player_scene(pkg)
        rays, seeds = player_rays()
        _PLAYER["v"] = (desc, rays, seeds, player_expected(pkg, orc, desc, rays, seeds))
    return _PLAYER["v"]


def test_player_scene_conditions(pkg, orc):
    """What GPU test B stands on: every evaluator drawn by at least 20 probes, at least 20 probes
    lit and 20 unlit, and at least 100 rays that end in volume 1's smoke (no probe there)."""
    desc, rays, seeds, e = player_case(pkg, orc)
    probes = e[e[:, 0] == 1]
    for idx in range(4):
        assert int((probes[:, 3] == idx).sum()) >= 20, (idx, np.bincount(probes[:, 3], minlength=4))
    assert int(probes[:, 1].sum()) >= 20 and int((probes[:, 1] == 0).sum()) >= 20
    other = e[(e[:, 5] == 1) & (e[:, 4] >= 9) & (e[:, 4] <= 14)]
    assert len(other) >= 100 and int(other[:, 0].sum()) == 0
