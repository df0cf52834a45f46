"""Filtered ray queries on the device (vpx_find_nearest_filtered / vpx_is_occluded_filtered):
every filter of scene S against the oracle on the filtered grids (tests/test_ray_filter.py
explains and pins that reference), the identities with the unfiltered entries, the refusals,
the raw direction, the zone scene's player rays through the TLAS, and the C++ mirror.
Everything is compared bit for bit: t, normal, index, material, cells, inside_glass.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

from cases import bits  # noqa: E402
from test_ray_filter import (N_RAYS, NO_RANGE, SMOKE, case_s, expected, expected_occluded, hit_rows, make_rays,  # noqa: E402
                             normalize32)

pytestmark = pytest.mark.gpu
X86 = os.uname().machine in ("x86_64", "i686")  # hosts that have VPX_ARITH_X86_HOST (tests/test_x86_arith.py)


@pytest.fixture(scope="module")
def s(pkg, orc):
    """Scene S on the device, its rays, and a cache of expected records."""
    desc, o, d, tmax = case_s(pkg, orc)
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    yield dict(desc=desc, o=o, d=d, tmax=tmax, rays=make_rays(pkg.abi, o, d, tmax), ctx=ctx)
    ctx.close()


def same(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def x86_mode(pkg, orc, ctx, on):
    orc.set_x86_approx(pkg.abi, on)
    ctx.set_arithmetic(pkg.abi.VPX_ARITH_X86_HOST if on else pkg.abi.VPX_ARITH_EXACT)


FILTERS = {  # name: (first_volume, material range, shapes)
    "player": (1, SMOKE, False),
    "player_shapes": (1, SMOKE, True),
    "all_volumes": (0, SMOKE, True),
    "last_volume": (2, NO_RANGE, False),
}


@pytest.mark.parametrize("name", list(FILTERS))
def test_filters_equal_oracle(pkg, orc, s, name):
    first, rng_mat, shapes = FILTERS[name]
    want = expected(pkg, orc, s["desc"], s["rays"], first, rng_mat, shapes)
    got = hit_rows(s["ctx"].find_nearest_filtered(s["rays"], first, rng_mat, shapes), N_RAYS)
    print(name, "hits", int((want[:, 4] >= 0).sum()), "shapes", int((want[:, 4] == -1).sum()), "cells", int(want[:, 6].sum()))
    same(got, want, name)


def test_no_volume_visited(pkg, s):
    """first_volume = count and above: -2, t = tmax, nothing read; with the shapes, theirs."""
    abi = pkg.abi
    for first in (3, 4, 0xFFFFFFFF):
        got = hit_rows(s["ctx"].find_nearest_filtered(s["rays"], first, SMOKE, shapes=False), N_RAYS)
        assert (got[:, 4] == -2).all() and (got[:, 0] == bits(s["tmax"])).all()
        assert (got[:, 5] == abi.MAT_NONE).all() and (got[:, 6] == 0).all() and (got[:, 1:4] == 0).all()
    got = hit_rows(s["ctx"].find_nearest_filtered(s["rays"], 3, SMOKE, shapes=True), N_RAYS)
    assert set(np.unique(got[:, 4])) == {-2, -1} and int((got[:, 4] == -1).sum()) >= 50
    miss = got[:, 4] == -2
    assert (got[miss, 0] == bits(s["tmax"])[miss]).all() and (got[:, 6] == 0).all()


@pytest.mark.skipif(not X86, reason="VPX_ARITH_X86_HOST needs an x86 host")
def test_player_filter_x86_arithmetic(pkg, orc, s):
    """FastReciprocal (renderer.cpp:1043) in the filtered FindNearest; the occlusion keeps 1 / D."""
    exact = expected(pkg, orc, s["desc"], s["rays"], 1, SMOKE, False)
    occ_want = expected_occluded(pkg, orc, s["desc"], s["rays"], 1, False)
    try:
        x86_mode(pkg, orc, s["ctx"], True)
        want = expected(pkg, orc, s["desc"], s["rays"], 1, SMOKE, False)
        got = hit_rows(s["ctx"].find_nearest_filtered(s["rays"], 1, SMOKE, shapes=False), N_RAYS)
        occ = s["ctx"].is_occluded_filtered(s["rays"], 1, shapes=False)
    finally:
        x86_mode(pkg, orc, s["ctx"], False)
    assert int((want[:, 0] != exact[:, 0]).sum()) >= 1  # the mode matters for these rays
    same(got, want, "player filter, x86 arithmetic")
    assert np.array_equal(occ, occ_want)


def test_one_ray_and_none(pkg, orc, s):
    abi, ctx = pkg.abi, s["ctx"]
    i = int(np.flatnonzero(expected(pkg, orc, s["desc"], s["rays"], 1, SMOKE, False)[:, 4] >= 0)[0])
    one = make_rays(abi, s["o"][i:i + 1], s["d"][i:i + 1], s["tmax"][i:i + 1])
    same(hit_rows(ctx.find_nearest_filtered(one, 1, SMOKE, shapes=False), 1), expected(pkg, orc, s["desc"], one, 1, SMOKE, False),
         "n = 1")
    assert np.array_equal(ctx.is_occluded_filtered(one, 1, shapes=False), expected_occluded(pkg, orc, s["desc"], one, 1, False))
    f = ctx.ray_filter(1, SMOKE, shapes=False)
    assert ctx.lib.vpx_find_nearest_filtered(ctx.h, None, 0, C.byref(f), None) == abi.VPX_OK
    f = ctx.ray_filter(1, None, shapes=False)
    assert ctx.lib.vpx_is_occluded_filtered(ctx.h, None, 0, C.byref(f), None) == abi.VPX_OK
    assert len(ctx.is_occluded_filtered((abi.Ray * 0)(), 1)) == 0


def test_neutral_filter_is_the_unfiltered_entry(pkg, s):
    """{0, 1, 0, 0} equals vpx_find_nearest and vpx_is_occluded bit for bit."""
    ctx = s["ctx"]
    f = pkg.abi.RayFilter(0, 1, 0, 0)
    same(hit_rows(ctx.find_nearest_filtered(s["rays"], filter=f), N_RAYS), hit_rows(ctx.find_nearest(s["rays"]), N_RAYS),
         "neutral filter")
    assert np.array_equal(ctx.is_occluded_filtered(s["rays"], filter=f), ctx.is_occluded(s["rays"]))


def test_occlusion_from_volume_one(pkg, orc, s):
    ctx, desc, rays = s["ctx"], s["desc"], s["rays"]
    want = {sh: expected_occluded(pkg, orc, desc, rays, 1, sh) for sh in (False, True)}
    assert (want[False] != want[True]).any()  # the shapes alone occlude some of these rays
    assert 0 < int(want[False].sum()) < N_RAYS
    for sh in (False, True):
        assert np.array_equal(ctx.is_occluded_filtered(rays, 1, shapes=sh), want[sh]), sh
    assert not ctx.is_occluded_filtered(rays, 3, shapes=False).any()


def test_refusals(pkg, s):
    """VPX_E_INVALID, with rays and with n == 0: no filter, a range end above 255 (unless the range
    is empty), unknown flag bits, and any material range for the occlusion entry."""
    abi, ctx = pkg.abi, s["ctx"]
    lib, h = ctx.lib, ctx.h
    rays = make_rays(abi, s["o"][:4], s["d"][:4], s["tmax"][:4])
    hits, occ = (abi.Hit * 4)(), (C.c_uint8 * 4)()
    for n, r, ho, oo in ((4, rays, hits, occ), (0, None, None, None)):
        assert lib.vpx_find_nearest_filtered(h, r, n, None, ho) == abi.VPX_E_INVALID
        assert lib.vpx_is_occluded_filtered(h, r, n, None, oo) == abi.VPX_E_INVALID
        for bad in ((0, 9, 256, 0), (0, 0, 0xFFFFFFFF, 0), (0, 256, 256, 0), (0, 1, 0, 4), (0, 9, 14, 0x80000000)):
            assert lib.vpx_find_nearest_filtered(h, r, n, C.byref(abi.RayFilter(*bad)), ho) == abi.VPX_E_INVALID, bad
        for bad in ((1, 9, 14, 1), (0, 0, 0, 0), (0, 255, 255, 0), (0, 1, 0, 8)):
            assert lib.vpx_is_occluded_filtered(h, r, n, C.byref(abi.RayFilter(*bad)), oo) == abi.VPX_E_INVALID, bad
        assert lib.vpx_last_error(h)
        for ok in ((0, 256, 255, 0), (0, 0xFFFFFFFF, 0, 3), (7, 0, 255, 0)):  # empty ranges; the whole range
            assert lib.vpx_find_nearest_filtered(h, r, n, C.byref(abi.RayFilter(*ok)), ho) == abi.VPX_OK, ok
        assert lib.vpx_is_occluded_filtered(h, r, n, C.byref(abi.RayFilter(0, 300, 299, 3)), oo) == abi.VPX_OK
    assert lib.vpx_find_nearest_filtered(h, None, 4, C.byref(abi.RayFilter(0, 1, 0, 0)), hits) == abi.VPX_E_INVALID
    assert lib.vpx_is_occluded_filtered(h, rays, 4, C.byref(abi.RayFilter(0, 1, 0, 0)), None) == abi.VPX_E_INVALID
    with pytest.raises(abi.VpxError):
        ctx.find_nearest_filtered(rays, 0, (0, 300))
    # every material excepted: nothing can be hit
    got = hit_rows(ctx.find_nearest_filtered(s["rays"], 0, (0, 255), shapes=False), N_RAYS)
    assert (got[:, 4] == -2).all() and int(got[:, 6].sum()) > 0


def test_device_set_forwards(pkg, orc, s):
    """The first 512 rays on a device set of [0, 0]."""
    abi = pkg.abi
    rays = make_rays(abi, s["o"][:512], s["d"][:512], s["tmax"][:512])
    ctx = pkg.context.Context(devices=[0, 0])
    try:
        ctx.load_scene(s["desc"])
        same(hit_rows(ctx.find_nearest_filtered(rays, 1, SMOKE, shapes=False), 512),
             expected(pkg, orc, s["desc"], rays, 1, SMOKE, False), "device set")
        assert np.array_equal(ctx.is_occluded_filtered(rays, 1, shapes=False),
                              expected_occluded(pkg, orc, s["desc"], rays, 1, False))
        assert ctx.lib.vpx_find_nearest_filtered(ctx.h, rays, 512, None, (abi.Hit * 512)()) == abi.VPX_E_INVALID
    finally:
        ctx.close()


def test_raw_direction(pkg, s):
    """dn = normalize(d) as the reference normalises (tmpl8math.h:2350-2354).  The flagged call on
    dn is the unflagged call on d; the unflagged call on dn normalises twice, which moves low bits
    of D for some rays and with them t (PlayerCharacter::GetRay normalises by itself and then uses
    the constructor that does not, src/Game/PlayerCharacter.cpp:11-18)."""
    abi, ctx = pkg.abi, s["ctx"]
    dn = normalize32(s["d"])
    assert (bits(normalize32(dn)) != bits(dn)).any()
    rays_n = make_rays(abi, s["o"], dn, s["tmax"])
    plain = hit_rows(ctx.find_nearest_filtered(s["rays"], 1, SMOKE, shapes=False), N_RAYS)
    raw = hit_rows(ctx.find_nearest_filtered(rays_n, 1, SMOKE, shapes=False, raw_direction=True), N_RAYS)
    same(raw, plain, "raw direction on dn")
    twice = hit_rows(ctx.find_nearest_filtered(rays_n, 1, SMOKE, shapes=False), N_RAYS)
    assert int((twice[:, 0] != plain[:, 0]).sum()) >= 1
    for sh in (False, True):
        assert np.array_equal(ctx.is_occluded_filtered(rays_n, 1, shapes=sh, raw_direction=True),
                              ctx.is_occluded_filtered(s["rays"], 1, shapes=sh))
    # with the shapes on as well (they take D as it stands)
    same(hit_rows(ctx.find_nearest_filtered(rays_n, 0, SMOKE, raw_direction=True), N_RAYS),
         hit_rows(ctx.find_nearest_filtered(s["rays"], 0, SMOKE), N_RAYS), "raw direction, shapes")


# ------------------------------------------------------------------------------ the zone
EPS = np.float32(1e-6)  # EPSILON, template/common.h:11
WASD = {"W": (EPS, EPS, -1.0), "D": (-1.0, EPS, EPS), "S": (EPS, EPS, 1.0), "A": (1.0, EPS, EPS)}  # PlayerCharacter.cpp:61-90
PLAYER_LEN = 3.0  # PlayerCharacter.h:24


def zone_rays():
    """Player rays (PlayerCharacter::GetRay, direction - up) from a 9 x 9 lattice over the first
    zone's floor (x, z in [-1.9, 2.9], y = 0.5; the smoke ball around (0.5, 0.8, 0.5) holds
    some of the origins), the four WASD directions and up in +-x, +-y, +-z."""
    ups = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    o, d = [], []
    for x in np.linspace(-1.9, 2.9, 9):
        for z in np.linspace(-1.9, 2.9, 9):
            for w in WASD.values():
                for up in ups:
                    o.append((x, 0.5, z))
                    d.append(np.asarray(w, np.float32) - np.asarray(up, np.float32))
    return np.array(o, np.float32), np.array(d, np.float32)


@pytest.fixture(scope="module")
def zone(pkg):
    desc = pkg.scene.zone_scene(64, 48, 0, sky=False)
    r = pkg.renderer.Renderer(desc, 0).Init()
    yield desc, r
    r.ctx.close()


@pytest.mark.parametrize("arith", ["exact", "x86"])
def test_zone_player_rays(pkg, orc, zone, arith):
    """21 volumes, so the TLAS carries the volume loop; the smoke ball is volume 5, the player 0."""
    if arith == "x86" and not X86:
        pytest.skip("VPX_ARITH_X86_HOST needs an x86 host")
    abi = pkg.abi
    desc, r = zone
    assert len(desc.volumes) == 21
    o, d = zone_rays()
    n = len(o)
    plain = make_rays(abi, o, d, PLAYER_LEN)
    raw = make_rays(abi, o, normalize32(d), PLAYER_LEN)
    try:
        x86_mode(pkg, orc, r.ctx, arith == "x86")
        want = expected(pkg, orc, desc, plain, 1, SMOKE, False)
        unfiltered = expected(pkg, orc, desc, plain, 1, NO_RANGE, False)
        occ_want = expected_occluded(pkg, orc, desc, plain, 1, False)
        got = hit_rows(r.ctx.find_nearest_filtered(raw, 1, SMOKE, shapes=False, raw_direction=True), n)
        occ = r.ctx.is_occluded_filtered(raw, 1, shapes=False, raw_direction=True)
    finally:
        x86_mode(pkg, orc, r.ctx, False)
    through = (unfiltered[:, 5] >= 9) & (unfiltered[:, 5] <= 14)
    print(arith, "rays", n, "hits", int((want[:, 4] >= 0).sum()), "through the smoke ball", int(through.sum()),
          "volumes", sorted(set(want[:, 4])))
    assert int(through.sum()) >= 100 and int((through & (want[:, 4] >= 0)).sum()) >= 20
    assert len(set(want[want[:, 4] >= 0, 4])) >= 2 and not (want[:, 4] == 5).any()
    same(got, want, "zone " + arith)
    assert np.array_equal(occ, occ_want)


def test_zone_python_mirror(pkg, orc, zone):
    """Renderer.FindNearestPlayer / IsOccludedPlayerClimbable on a ray that starts inside the
    smoke ball, passes through it and meets the floor (volume 1)."""
    abi, ren = pkg.abi, pkg.renderer
    desc, r = zone
    o = np.array([[0.5, 0.5, 0.5]], np.float32)
    d = (np.asarray(WASD["W"], np.float32) - np.array([0, 1, 0], np.float32))[None]
    want = expected(pkg, orc, desc, make_rays(abi, o, d, PLAYER_LEN), 1, SMOKE, False)[0]
    unf = expected(pkg, orc, desc, make_rays(abi, o, d, PLAYER_LEN), 1, NO_RANGE, False)[0]
    assert want[4] == 1 and unf[4] == 5 and 9 <= unf[5] <= 14
    ray = ren.Ray(o[0], normalize32(d)[0], PLAYER_LEN)
    r.currentChunk = 0
    assert r.FindNearestPlayer(ray) == 1
    assert int(bits(np.float32(ray.t)).reshape(-1)[0]) == want[0] and ray.t < PLAYER_LEN
    assert [int(b) for b in bits(np.array(ray.rayNormal, np.float32))] == list(want[1:4]) and ray.indexMaterial == want[5]
    assert r.IsOccludedPlayerClimbable(ren.Ray(o[0], normalize32(d)[0], PLAYER_LEN)) is True
    up = ren.Ray(o[0], (0.0, 1.0, 0.0), 0.25)  # ends inside the smoke ball: smoke occludes, but is no hit
    assert r.IsOccludedPlayerClimbable(up) is True and r.FindNearestPlayer(up) == -2 and up.t == 0.25
    r.currentChunk = 2  # renderer.cpp:1068-1069: a miss becomes -1
    assert r.FindNearestPlayer(up) == -1
    assert r.FindNearestPlayer(ren.Ray(o[0], normalize32(d)[0], PLAYER_LEN)) == 1
    r.currentChunk = 0


def test_cpp_mirror_casts_the_player_rays(pkg, zone):
    """host/vpx_demo in its 'w' mode builds the zone's volumes in C++ and casts the four WASD rays
    from (0.5, 0.5, 0.5) with up = +y through host/vpx_renderer.cpp: the same index, t, normal and
    material as the same rays from Python."""
    ren = pkg.renderer
    desc, r = zone
    exe = os.path.join(os.path.dirname(pkg.__file__), "host", "vpx_demo")
    p = subprocess.run([exe, "64", "64", "48", "1", "0", "-", "w"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    rows = json.loads(lines[0])["player_rays"]
    assert [x["key"] for x in rows] == list(WASD)
    hit = 0
    for x in rows:
        d = normalize32((np.asarray(WASD[x["key"]], np.float32) - np.array([0, 1, 0], np.float32))[None])[0]
        ray = ren.Ray((0.5, 0.5, 0.5), d, PLAYER_LEN)
        vox = r.FindNearestPlayer(ray)
        got = (x["vox"], x["t_bits"], x["normal_bits"], x["material"], bool(x["occluded"]))
        want = (vox, int(bits(np.float32(ray.t)).reshape(-1)[0]), [int(b) for b in bits(np.array(ray.rayNormal, np.float32))],
                ray.indexMaterial, r.IsOccludedPlayerClimbable(ren.Ray((0.5, 0.5, 0.5), d, PLAYER_LEN)))
        print(x["key"], got)
        assert got == want, x["key"]
        hit += vox >= 0
    assert hit == 4  # each meets the floor under the smoke ball
