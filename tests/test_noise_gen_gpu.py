"""GPU suite of the noise generators: vpx_grid_generate_noise (Scene::GenerateSomeNoise /
GenerateSomeSmoke on the device, one call, no host grid) against the host path of the same code
and the numpy restatement, read back with vpx_grid_read_box; the levels after a generation through
the distance-field planes and frames; resizing, frames in flight, a device set, the refusals
and the C++ mirror."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from cases import bits  # noqa: E402
from test_noise_gen import BLOCK, CASES, DRAW, SEED, host_generate, noise_restated  # noqa: E402, F401

SCAN_PASS = 256  # block counts the prefix workgroup takes per pass (noise::kScanPass)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.context.Context(0)
    yield c
    c.close()


def checksum(pkg, orc, cells):
    cells = np.ascontiguousarray(cells, np.uint8).reshape(-1)
    return orc._lib(pkg.abi).oracle_grid_checksum(cells.ctypes.data, cells.size)


def gen_mode(pkg, mode):
    return pkg.abi.GEN_NOISE if mode == "noise" else pkg.abi.GEN_SMOKE


def device_generate(pkg, ctx, gid, mode, n, f, seed=SEED):
    res = ctx.grid_generate_noise(gid, n, gen_mode(pkg, mode), f, seed)
    return ctx.grid_read_box(gid, (0, 0, 0), (n, n, n)).reshape(-1), res


# ---------------------------------------------------------------------- placement
@pytest.mark.parametrize("mode,n,f", CASES, ids=[f"{m}-{n}-{f}" for m, n, f in CASES])
def test_device_equals_host_and_restatement(pkg, orc, ctx, noise_restated, mode, n, f):
    want, seed, noise_seed, draws = noise_restated(mode, n, f)[:4]
    dev, res = device_generate(pkg, ctx, 7, mode, n, f)
    host, hres = host_generate(pkg, mode, n, f)
    assert np.array_equal(dev, host)
    assert np.array_equal(dev, want)
    assert bytes(res) == bytes(hres)
    assert (res.seed, res.noise_seed, res.draws) == (seed, noise_seed, draws)
    assert ctx.grid_checksum(7) == checksum(pkg, orc, want)


def test_more_blocks_than_one_scan_pass(pkg, orc, ctx, noise_restated):
    """128^3 cells are 512 blocks of 4096: the prefix workgroup, which takes 256 block counts per
    pass, carries its sum over a pass boundary, with drawers on both sides of it."""
    n, f = 128, .03
    assert n ** 3 // BLOCK > SCAN_PASS
    want, seed, noise_seed, draws, cls = noise_restated("noise", n, f)
    per_block = np.bincount(np.nonzero(cls == DRAW)[0] // BLOCK, minlength=n ** 3 // BLOCK)
    assert per_block[:SCAN_PASS].sum() > 0 and per_block[SCAN_PASS:].sum() > 0
    dev, res = device_generate(pkg, ctx, 7, "noise", n, f)
    assert np.array_equal(dev, want)
    assert (res.seed, res.noise_seed, res.draws) == (seed, noise_seed, draws)
    assert not (dev == 254).any()  # no marker survives


def test_256_equals_host(pkg, orc, ctx):
    for mode, f in (("noise", .03), ("smoke", .167)):
        dev, res = device_generate(pkg, ctx, 7, mode, 256, f)
        host, hres = host_generate(pkg, mode, 256, f)
        assert np.array_equal(dev, host) and bytes(res) == bytes(hres), mode
        assert (dev != 255).any()
    ctx.grid_generate_noise(7, 16)  # give the memory back


# ------------------------------------------------------------------------- levels
def _render(r, frames):
    r.ResetAccumulator()
    stats = [r.Tick(0.0, stats=True) for _ in range(frames)]
    torch.cuda.synchronize()
    counters = [{k: v for k, v in st.as_dict().items() if not k.endswith("_ms")} for st in stats]
    return r.accumulator_host().reshape(-1, 4).copy(), r.screen_host().reshape(-1).copy(), counters


def _same_frames(a, b):
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    assert a[2] == b[2]
    assert a[1].any() and a[2][0]["dda_cells"] > 0


@pytest.mark.parametrize("mode,f", [("noise", .03), ("smoke", .167)])
def test_levels_after_a_generation(pkg, mode, f):
    """The walkers read the occupancy levels and the distance field: after the device call they
    are those of a grid that vpx_upload_grid filled with the same bytes, plane for plane and frame
    for frame (accumulator bits, RGB8, ray and cell counters)."""
    sc, ren = pkg.scene, pkg.renderer
    n = 64
    cells, hres = host_generate(pkg, mode, n, f)
    sizes = ((64, 48), (70, 50)) if mode == "noise" else ((64, 48),)
    for w, h in sizes:
        desc = sc.model_scene("monu3", n, w, h, 2, city_lights=True)
        r = ren.Renderer(desc, 0).Init()
        res = (r.GenerateSomeNoise if mode == "noise" else r.GenerateSomeSmoke)(0, f)
        assert bytes(res) == bytes(hres) and r.seed == hres.seed
        desc2 = sc.model_scene("monu3", n, w, h, 2, city_lights=True)
        desc2.grids[0].dense = cells
        r2 = ren.Renderer(desc2, 0).Init()
        assert r.ctx.grid_checksum(0) == r2.ctx.grid_checksum(0)
        assert np.array_equal(r.ctx.grid_wide_planes(0, n), r2.ctx.grid_wide_planes(0, n))
        _same_frames(_render(r, 2), _render(r2, 2))
        r.ctx.close()
        r2.ctx.close()


def test_zone_scene_checkpoint_smoke(pkg, noise_restated):
    """voxelVolumes[5].GenerateSomeSmoke(0.167f) (renderer.cpp:626) on the zone scene through the
    Renderer mirror, against zone_scene(smoke="noise"), whose grid the host generated."""
    sc, ren = pkg.scene, pkg.renderer
    r = ren.Renderer(sc.zone_scene(64, 48, 2), 0).Init()
    res = r.GenerateSomeSmoke(5, 0.167)
    want, seed, _, draws = noise_restated("smoke", 64, .167)
    assert (res.seed, res.draws) == (seed, draws) and r.seed == seed
    desc2 = sc.zone_scene(64, 48, 2, smoke="noise")
    r2 = ren.Renderer(desc2, 0).Init()
    gid = desc2.volumes[5].grid_id
    assert np.array_equal(r.ctx.grid_read_box(gid, (0, 0, 0), (64, 64, 64)).reshape(-1), want)
    _same_frames(_render(r, 1), _render(r2, 1))
    r.ctx.close()
    r2.ctx.close()


# ---------------------------------------------------------------------- lifecycle
def test_creation_resizing_and_refusals(pkg, orc, ctx, noise_restated):
    abi, lib = pkg.abi, pkg.load_library()
    out = np.zeros(8, np.uint8)
    assert lib.vpx_grid_read_box(ctx.h, 11, out.ctypes.data, 0, 0, 0, 1, 1, 1) == abi.VPX_E_INVALID  # no grid 11 yet
    seed = SEED
    for n in (64, 16, 33):  # created, then regenerated at other sizes; the seed carried along
        mode, f = ("noise", .03) if n != 33 else ("noise", .167)
        dev, res = device_generate(pkg, ctx, 11, mode, n, f, seed)
        host, hres = host_generate(pkg, mode, n, f, seed)
        assert np.array_equal(dev, host) and bytes(res) == bytes(hres)
        if seed == SEED:
            assert np.array_equal(dev, noise_restated(mode, n, f)[0])
        seed = res.seed
    assert lib.vpx_grid_read_box(ctx.h, 11, out.ctypes.data, 32, 32, 32, 2, 1, 1) == abi.VPX_E_INVALID  # 33^3 now
    before = ctx.grid_checksum(11)
    res = abi.NoiseResult()

    def call(g, n=33, r=res):
        return lib.vpx_grid_generate_noise(ctx.h, 11, n, None if g is None else C.byref(g), None if r is None else C.byref(r))

    assert call(None) == abi.VPX_E_INVALID
    bad = abi.noise_gen()
    bad.reserved = 7
    assert call(bad) == abi.VPX_E_INVALID and b"reserved" in lib.vpx_last_error(ctx.h)
    assert call(abi.noise_gen(mode=2)) == abi.VPX_E_INVALID
    assert call(abi.noise_gen(), n=0) == abi.VPX_E_INVALID
    assert call(abi.noise_gen(), n=4097) == abi.VPX_E_INVALID
    for f in (float("nan"), float("inf"), -float("inf")):
        assert call(abi.noise_gen(frequency=f)) == abi.VPX_E_INVALID
    assert call(abi.noise_gen(frequency=2.0 ** 25)) == abi.VPX_E_INVALID  # 32 * 2^25 = 2^30
    assert call(abi.noise_gen(frequency=-2.0 ** 25)) == abi.VPX_E_INVALID
    assert ctx.grid_checksum(11) == before  # refused calls changed nothing
    assert call(abi.noise_gen(frequency=.167, seed=SEED), r=None) == abi.VPX_OK  # out may be NULL
    assert ctx.grid_checksum(11) == checksum(pkg, orc, noise_restated("noise", 33, .167)[0])


def test_generation_waits_for_frames_in_flight(pkg):
    """Three frames queued on three lanes, a generation, three more: the call must not change the
    world under the queued frames, so the accumulator equals the serial run's."""
    sc, ren = pkg.scene, pkg.renderer
    accs = []
    for depth in (0, 3):
        r = ren.Renderer(sc.model_scene("monu3", 64, 64, 40, 1, city_lights=True), 0).Init()
        r.ctx.set_pipeline(depth)
        for _ in range(3):
            r.Tick(0.0)
        r.GenerateSomeNoise(0, .03)
        for _ in range(3):
            r.Tick(0.0)
        r.ctx.synchronize()
        torch.cuda.synchronize()
        accs.append((r.accumulator_host().copy(), r.screen_host().copy()))
        r.ctx.close()
    assert np.array_equal(bits(accs[0][0]), bits(accs[1][0])) and np.array_equal(accs[0][1], accs[1][1])
    assert np.isfinite(accs[0][0]).all() and accs[0][1].any()


def test_device_set(pkg, noise_restated):
    """A set that repeats the device: the generation goes to every member, the read-back to the
    first; frames equal one device's."""
    sc, ren = pkg.scene, pkg.renderer
    want, seed = noise_restated("noise", 64, .03)[:2]
    out = []
    for devices in (None, [0, 0]):
        desc = sc.model_scene("monu3", 64, 64, 40, 1, city_lights=True)
        torch.cuda.set_device(0)
        c = pkg.context.Context(0) if devices is None else pkg.context.Context(devices=devices)
        r = ren.Renderer(desc, 0, ctx=c).Init()
        res = r.GenerateSomeNoise(0, .03)
        assert res.seed == seed
        assert np.array_equal(c.grid_read_box(0, (0, 0, 0), (64, 64, 64)).reshape(-1), want)
        out.append(_render(r, 2))
        c.close()
    _same_frames(out[0], out[1])


def test_cpp_mirror_runs_the_generators(pkg, orc, noise_restated):
    """host/vpx_demo in its 'g' mode: GenerateSomeNoise(0.03f), then GenerateSomeSmoke(0.167f) from
    the seed the first left, through host/vpx_renderer.cpp; checksums, draws and seeds are the
    Python path's."""
    exe = os.path.join(os.path.dirname(pkg.__file__), "host", "vpx_demo")
    p = subprocess.run([exe, "64", "64", "48", "1", "0", "-", "g"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    got = json.loads(lines[0])
    noise, seed1, _, draws1 = noise_restated("noise", 64, .03)[:4]
    smoke, hres = pkg.scene.generate_some_smoke(64, 0.167, seed1)
    assert got["n"] == 64
    assert (int(got["noise"]["checksum"]), got["noise"]["draws"], got["noise"]["seed"]) == (checksum(pkg, orc, noise), draws1, seed1)
    assert (int(got["smoke"]["checksum"]), got["smoke"]["draws"], got["smoke"]["seed"]) == (checksum(pkg, orc, smoke),
                                                                                             hres.draws, hres.seed)
