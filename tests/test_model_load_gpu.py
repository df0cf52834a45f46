"""GPU suite of the model loaders: vpx_model_upload + vpx_grid_load_model (Scene::LoadModel /
LoadModelPartial / LoadModelRandomMaterials on the device, one call, no host grid) against the
host path of the same code and the oracle, read back with vpx_grid_read_box; the levels after a
load through frames; frames in flight, device sets and the C++ mirror."""
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
from test_model_load import oracle_full, oracle_partial, place_host, scale_rule, sequential_random  # noqa: E402


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.context.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models(pkg):
    got = {}

    def get(name):
        if name not in got:
            got[name] = pkg.scene.load_model(name)
        return got[name]

    return get


def checksum(pkg, orc, cells):
    cells = np.ascontiguousarray(cells, np.uint8).reshape(-1)
    return orc._lib(pkg.abi).oracle_grid_checksum(cells.ctypes.data, cells.size)


FULL, PARTIAL, RANDOM = 0, 1, 2
PLACE_CASES = [
    (FULL, "monu2", 32, {}), (FULL, "SmallBuilding02", 32, {}), (FULL, "TallBuilding01", 16, {}), (FULL, "monu2", 64, {}),
    (FULL, "roomGlass", 100, {}),  # n % 16 != 0: one thread per cell
    (PARTIAL, "monu2", 64, dict(columns=16, thickness=16)), (PARTIAL, "monu2", 64, dict(columns=32, thickness=16)),
    (PARTIAL, "monu2", 64, dict(columns=64, thickness=16)), (PARTIAL, "monu2", 64, dict(columns=3, thickness=13)),
    (RANDOM, "Text", 32, dict(seed=0x12345678)),
    (RANDOM, "monu2", 32, dict(seed=0x12345678, rand_lo=9.0, rand_hi=15.0)),
]


@pytest.mark.parametrize("mode,name,n,kw", PLACE_CASES,
                         ids=[f"{'FPR'[c[0]]}-{c[1]}-{c[2]}-{c[3].get('columns', '')}" for c in PLACE_CASES])
def test_device_placement(pkg, orc, ctx, models, mode, name, n, kw):
    size, vox, _ = models(name)
    ctx.model_upload(3, size, vox)
    res = ctx.grid_load_model(7, n, 3, mode=mode, **kw)
    dev = ctx.grid_read_box(7, (0, 0, 0), (n, n, n)).reshape(-1)
    host, hres = place_host(pkg, size, vox, n, mode=mode, **kw)
    if mode == FULL:
        want = oracle_full(pkg, orc, size, vox, n)
    elif mode == PARTIAL:
        want = oracle_partial(pkg, orc, size, vox, n, kw["columns"], kw["thickness"])
        if kw["columns"] == 3:
            assert (want == 255).all()  # the empty slice
    else:
        want, state = sequential_random(pkg, orc, size, vox, n, kw["seed"], kw.get("rand_lo", 12.0),
                                        kw.get("rand_hi", 13.0))
        assert res.seed == state
    assert np.array_equal(dev, host)
    assert np.array_equal(dev, want)
    assert ctx.grid_checksum(7) == checksum(pkg, orc, want)
    assert bytes(res) == bytes(hres)
    assert np.array_equal(np.array(res.scale_model[:], np.float32).view(np.uint32), scale_rule(size, n).view(np.uint32))


def test_creation_and_resizing(pkg, orc, ctx, models):
    abi, lib = pkg.abi, pkg.load_library()
    size, vox, _ = models("monu3")
    ctx.model_upload(4, size, vox)
    out = np.zeros(8, np.uint8)
    assert lib.vpx_grid_read_box(ctx.h, 9, out.ctypes.data, 0, 0, 0, 1, 1, 1) == abi.VPX_E_INVALID  # no grid 9 yet
    ctx.grid_load_model(9, 16, 4)  # created
    assert np.array_equal(ctx.grid_read_box(9, (0, 0, 0), (16, 16, 16)).reshape(-1), oracle_full(pkg, orc, size, vox, 16))
    ctx.grid_load_model(9, 48, 4)  # resized
    assert np.array_equal(ctx.grid_read_box(9, (0, 0, 0), (48, 48, 48)).reshape(-1), oracle_full(pkg, orc, size, vox, 48))
    assert lib.vpx_grid_read_box(ctx.h, 9, out.ctypes.data, 47, 47, 47, 2, 1, 1) == abi.VPX_E_INVALID
    ctx.grid_load_model(9, 16, 4)  # and back
    assert ctx.grid_checksum(9) == checksum(pkg, orc, oracle_full(pkg, orc, size, vox, 16))
    # argument errors of the device entry
    ld = abi.model_load()
    assert lib.vpx_grid_load_model(ctx.h, 9, 16, 4, None, None) == abi.VPX_E_INVALID
    assert lib.vpx_grid_load_model(ctx.h, 9, 16, 99, C.byref(ld), None) == abi.VPX_E_INVALID  # unknown model
    assert lib.vpx_grid_load_model(ctx.h, 9, 0, 4, C.byref(ld), None) == abi.VPX_E_INVALID
    assert lib.vpx_grid_load_model(ctx.h, 9, 4097, 4, C.byref(ld), None) == abi.VPX_E_INVALID
    assert lib.vpx_grid_load_model(ctx.h, 9, 16, 4, C.byref(abi.model_load(mode=3)), None) == abi.VPX_E_INVALID
    assert lib.vpx_grid_load_model(ctx.h, 9, 16, 4, C.byref(abi.model_load(mode=RANDOM, rand_lo=5.0, rand_hi=4.0)),
                                   None) == abi.VPX_E_INVALID
    assert lib.vpx_model_upload(ctx.h, 5, vox.ctypes.data, 257, 1, 1) == abi.VPX_E_INVALID
    assert lib.vpx_model_upload(ctx.h, 5, vox.ctypes.data, 4, 0, 1) == abi.VPX_E_INVALID
    ctx.model_upload(4, None, None)  # removed
    assert lib.vpx_grid_load_model(ctx.h, 9, 16, 4, C.byref(ld), None) == abi.VPX_E_INVALID
    assert ctx.grid_checksum(9) == checksum(pkg, orc, oracle_full(pkg, orc, size, vox, 16))  # refused calls changed nothing


def test_read_box(pkg, ctx):
    abi, lib = pkg.abi, pkg.load_library()
    n = 20
    grid = np.random.default_rng(11).integers(0, 256, (n, n, n), dtype=np.uint8)
    ctx.lib.vpx_upload_grid(ctx.h, 2, grid.ctypes.data_as(C.c_void_p), n)
    assert np.array_equal(ctx.grid_read_box(2, (0, 0, 0), (n, n, n)), grid)
    for (x0, y0, z0), (dz, dy, dx) in (((3, 5, 7), (4, 9, 13)), ((0, 0, 19), (1, 20, 20)), ((19, 19, 19), (1, 1, 1)),
                                       ((0, 2, 0), (20, 3, 20)), ((1, 0, 4), (6, 20, 17))):
        assert np.array_equal(ctx.grid_read_box(2, (x0, y0, z0), (dz, dy, dx)), grid[z0:z0 + dz, y0:y0 + dy, x0:x0 + dx])
    out = np.zeros(n ** 3, np.uint8)
    for box in ((0, 0, 0, 21, 1, 1), (19, 0, 0, 2, 1, 1), (0, 20, 0, 1, 1, 1), (0, 0, 5, 1, 1, 16), (0xFFFFFFFF, 0, 0, 2, 1, 1)):
        assert lib.vpx_grid_read_box(ctx.h, 2, out.ctypes.data, *box) == abi.VPX_E_INVALID, box
    assert lib.vpx_grid_read_box(ctx.h, 2, None, 0, 0, 0, 1, 1, 1) == abi.VPX_E_INVALID
    assert lib.vpx_grid_read_box(ctx.h, 63, out.ctypes.data, 0, 0, 0, 1, 1, 1) == abi.VPX_E_INVALID


def _render_on(r, frames=1):
    r.ResetAccumulator()
    for _ in range(frames):
        r.Tick(0.0)
    torch.cuda.synchronize()
    return r.accumulator_host().reshape(-1, 4).copy(), r.screen_host().reshape(-1).copy()


def test_levels_after_a_load(pkg, orc, models):
    """The walkers read the occupancy levels and the distance field, so a frame equals the oracle's
    on the loaded cells only if the load rebuilt them: a monu3 world replaced by monu2 (LoadModel),
    then three prop edits on the same grid, the last compared with the old flow too."""
    sc, ren = pkg.scene, pkg.renderer
    n = 64
    desc = sc.model_scene("monu3", n, 64, 40, 1, city_lights=True)
    size, vox, pal = models("monu2")
    r = ren.Renderer(desc, 0).Init()
    r.UploadModel(0, size, vox, pal)
    r.LoadModel(0, 0)  # the palette override lands in desc.materials, which the oracle reads
    assert bytes(desc.materials) == bytes(sc.palette_materials(sc.palette_materials(
        sc.default_materials(), *sc.load_model("monu3")[1:]), vox, pal))
    full = oracle_full(pkg, orc, size, vox, n)
    assert not np.array_equal(full, desc.grids[0].dense)
    assert r.ctx.grid_checksum(0) == checksum(pkg, orc, full)
    acc_g, rgb_g = _render_on(r)
    acc_o, rgb_o, _ = orc.Oracle(pkg.abi, desc, grid_cells=[full]).render(desc.frame_params(0))
    assert np.array_equal(bits(acc_g), bits(acc_o)) and np.array_equal(rgb_g, rgb_o)
    prop = ren.ModifyingProp(r, 0, 0, 16, 16)
    for index in (16, 32, 48):
        assert prop.index == index
        prop.Update()
    assert prop.index == 64
    part = oracle_partial(pkg, orc, size, vox, n, 48, 16)
    assert r.ctx.grid_checksum(0) == checksum(pkg, orc, part)
    acc_g, rgb_g = _render_on(r)
    acc_o, rgb_o, _ = orc.Oracle(pkg.abi, desc, grid_cells=[part]).render(desc.frame_params(0))
    assert np.array_equal(bits(acc_g), bits(acc_o)) and np.array_equal(rgb_g, rgb_o)
    # the old flow in a second context: host loop, ResetGrid, dirty-box upload
    r2 = ren.Renderer(desc, 0).Init()
    grid, box = sc.load_model_partial(size, vox, n, 48, 16)
    x0, y0, z0, x1, y1, z1 = box
    r2.ctx.grid_fill(0, 255)
    r2.ctx.grid_write_box(0, grid.reshape(n, n, n)[z0:z1, y0:y1, x0:x1], (x0, y0, z0))
    acc_2, rgb_2 = _render_on(r2)
    assert np.array_equal(bits(acc_g), bits(acc_2)) and np.array_equal(rgb_g, rgb_2)
    prop.Update()  # index 64, then the wrap: 80 > 64 -> 16
    assert prop.index == 16
    assert r.ctx.grid_checksum(0) == checksum(pkg, orc, oracle_partial(pkg, orc, size, vox, n, 64, 16))
    r.ctx.close()
    r2.ctx.close()


def test_random_materials_through_the_renderer(pkg, orc, models):
    """Renderer.LoadModelRandomMaterials draws Rand(12, 13) from, and advances, Renderer.seed."""
    sc, ren = pkg.scene, pkg.renderer
    desc = sc.model_scene("Text", 32, 64, 40, 0, city_lights=True)
    size, vox, _ = models("Text")
    r = ren.Renderer(desc, 0).Init()
    r.UploadModel(1, size, vox)
    assert r.seed == 0x12345678
    r.LoadModelRandomMaterials(0, 1)
    g1, s1 = sc.load_model_random(size, vox, 32, 0x12345678)
    assert r.seed == s1 and r.ctx.grid_checksum(0) == checksum(pkg, orc, g1)
    r.LoadModelRandomMaterials(0, 1)
    g2, s2 = sc.load_model_random(size, vox, 32, s1)
    assert r.seed == s2 and r.ctx.grid_checksum(0) == checksum(pkg, orc, g2)
    r.ctx.close()


def test_load_waits_for_frames_in_flight(pkg, models):
    """Three frames queued on three lanes, a load, three more: the load must not change the world
    under the queued frames, so the accumulator equals the serial run's."""
    sc, ren = pkg.scene, pkg.renderer
    size, vox, pal = models("monu2")
    accs = []
    for depth in (0, 3):
        desc = sc.model_scene("monu3", 64, 64, 40, 1, city_lights=True)
        r = ren.Renderer(desc, 0).Init()
        r.ctx.set_pipeline(depth)
        r.UploadModel(0, size, vox, pal)
        for _ in range(3):
            r.Tick(0.0)
        r.LoadModelPartial(0, 0, 32, 16)
        for _ in range(3):
            r.Tick(0.0)
        r.ctx.synchronize()
        torch.cuda.synchronize()
        accs.append((r.accumulator_host().copy(), r.screen_host().copy()))
        r.ctx.close()
    assert np.array_equal(bits(accs[0][0]), bits(accs[1][0])) and np.array_equal(accs[0][1], accs[1][1])
    assert np.isfinite(accs[0][0]).all() and accs[0][1].any()


def test_device_set(pkg, orc, models):
    """A set that repeats the device: the model and the load go to every member, the read-back
    to the first; frames equal one device's."""
    sc, ren = pkg.scene, pkg.renderer
    size, vox, pal = models("monu2")
    out = []
    for devices in (None, [0, 0]):
        desc = sc.model_scene("monu3", 64, 64, 40, 1, city_lights=True)
        torch.cuda.set_device(0)
        c = pkg.context.Context(0) if devices is None else pkg.context.Context(devices=devices)
        r = ren.Renderer(desc, 0, ctx=c).Init()
        r.UploadModel(0, size, vox, pal)
        r.LoadModelPartial(0, 0, 32, 16)
        cells = c.grid_read_box(0, (0, 0, 0), (64, 64, 64)).reshape(-1)
        assert np.array_equal(cells, oracle_partial(pkg, orc, size, vox, 64, 32, 16))
        out.append(_render_on(r, 2))
        c.close()
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(out[0][1], out[1][1])


def test_cpp_mirror_runs_the_prop_edits(pkg, orc):
    """host/vpx_demo in its 'm' mode: five ModifyingProp edits, a LoadModel and a
    LoadModelRandomMaterials of its synthetic model through host/vpx_renderer.cpp; the checksums
    are the oracle's for the same calls, Scene::scaleModel multiplied once more by every load."""
    sc = pkg.scene
    sx, sy, sz, n = 96, 40, 72, 64
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    vox = np.where((7 * x + 13 * y + 5 * z) % 11 < 4, 1 + (x + 3 * y + 5 * z) % 200, 0).astype(np.uint8).reshape(-1)
    size = (sx, sy, sz)
    exe = os.path.join(os.path.dirname(pkg.__file__), "host", "vpx_demo")
    p = subprocess.run([exe, "64", "64", "48", "1", "0", "-", "m"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    got = json.loads(lines[0])
    scale = np.ones(3, np.float32)
    assert [e["index"] for e in got["prop_edits"]] == [16, 32, 48, 64, 16]
    for e in got["prop_edits"]:
        want = oracle_partial(pkg, orc, size, vox, n, e["index"], 16, tuple(scale))
        assert int(e["checksum"]) == checksum(pkg, orc, want), e
        scale = scale_rule(size, n, scale)
    assert int(got["full"]) == checksum(pkg, orc, oracle_full(pkg, orc, size, vox, n, tuple(scale)))
    scale = scale_rule(size, n, scale)
    grid, seed = sc.load_model_random(size, vox, n, 0x12345678, scale_model=tuple(scale))
    assert int(got["random"]) == checksum(pkg, orc, grid) and got["seed"] == seed
