"""CPU suite of the model loaders (Scene::LoadModel / LoadModelPartial / LoadModelRandomMaterials,
template/scene.cpp:449-683): vpx_model_place_host — the host path of the code the device kernel
runs (csrc/vpx_model.hpp) — against the oracle's loops and the numpy restatements, the
xorshift32 jump against looped steps, the palette override, the argument errors, and the
stand-alone native test of the shared header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "raytracer-voxpopuli_amd", "csrc")
ONE = (1.0, 1.0, 1.0)


def place_host(pkg, size, vox, n, **kw):
    """vpx_model_place_host -> (grid, abi.ModelResult)."""
    lib, abi = pkg.load_library(), pkg.abi
    sx, sy, sz = (int(v) for v in size)
    ld = abi.model_load(**kw)
    out = np.full(n ** 3, 77, np.uint8)
    res = abi.ModelResult()
    rc = lib.vpx_model_place_host(vox.ctypes.data, sx, sy, sz, n, C.byref(ld), out.ctypes.data, C.byref(res))
    assert rc == abi.VPX_OK, rc
    return out, res


def oracle_full(pkg, orc, size, vox, n, scale=ONE):
    sx, sy, sz = (int(v) for v in size)
    out = np.empty(n ** 3, np.uint8)
    orc._lib(pkg.abi).oracle_load_model(vox.ctypes.data, sx, sy, sz, n, (C.c_float * 3)(*scale), out.ctypes.data)
    return out


def oracle_partial(pkg, orc, size, vox, n, columns, thickness, scale=ONE):
    sx, sy, sz = (int(v) for v in size)
    out = np.empty(n ** 3, np.uint8)
    orc._lib(pkg.abi).oracle_load_model_partial(vox.ctypes.data, sx, sy, sz, n, (C.c_float * 3)(*scale), columns,
                                                thickness, out.ctypes.data)
    return out


def scale_rule(size, n, scale=ONE):
    """Scene::scaleModel after a loader call (scene.cpp:488-494), in float32."""
    s = np.array(scale, np.float32)
    if int(size[0]) > n:
        s = s * (np.float32(n) / np.array([int(v) for v in size], np.float32))
    return s


def writes(size, vox, n, scale=ONE):
    """The loop's writes in loop order: (target cell index, value) of the non-empty voxels that land
    in the grid, and the number that land outside it."""
    sx, sy, sz = (int(v) for v in size)
    s = scale_rule(size, n, scale)
    zz, yy, xx = np.nonzero(vox.reshape(sz, sy, sx))  # z-major, then y, then x: the loop's order
    gx = (xx.astype(np.float32) * s[0]).astype(np.int64)
    gy = (zz.astype(np.float32) * s[1]).astype(np.int64)
    gz = (yy.astype(np.float32) * s[2]).astype(np.int64)
    ok = (gx >= 0) & (gy >= 0) & (gz >= 0) & (gx < n) & (gy < n) & (gz < n)
    return (gx + gy * n + gz * n * n)[ok], vox.reshape(sz, sy, sx)[zz, yy, xx][ok], int((~ok).sum())


def first_writer_grid(size, vox, n):
    tgt, val, _ = writes(size, vox, n)
    g = np.full(n ** 3, 255, np.uint8)
    cells, first = np.unique(tgt, return_index=True)
    g[cells] = val[first]
    return g


# model, n, downscaled, cells with more than one source (None: not counted), cells whose first and
# last writer differ, non-empty voxels that land outside the grid (of how many)
FULL_CASES = [("monu2", 32, True, 14666, 1240, (0, None)),
              ("SmallBuilding02", 32, True, None, 152, (6721, 9172)),
              ("TallBuilding01", 16, False, 0, 0, (123, None)),
              ("monu3", 16, True, None, 71, (0, None)),
              ("monu2", 64, False, 0, 0, (0, None))]


@pytest.mark.parametrize("name,n,down,multi,differ,outside", FULL_CASES, ids=[f"{c[0]}-{c[1]}" for c in FULL_CASES])
def test_full_equals_oracle(pkg, orc, name, n, down, multi, differ, outside):
    sc = pkg.scene
    size, vox, _ = sc.load_model(name)
    want = oracle_full(pkg, orc, size, vox, n)
    got, res = place_host(pkg, size, vox, n)
    assert np.array_equal(got, want)
    assert np.array_equal(got, sc.load_model_grid(size, vox, n))
    # what the case is here for
    assert (int(size[0]) > n) == down
    tgt, _, out = writes(size, vox, n)
    _, counts = np.unique(tgt, return_counts=True)
    first = first_writer_grid(size, vox, n)
    if multi is not None:
        assert int((counts > 1).sum()) == multi
    assert int((first != want).sum()) == differ
    assert out == outside[0]
    if outside[1] is not None:
        assert int((vox != 0).sum()) == outside[1]
    if name == "monu2" and n == 32:
        assert not np.array_equal(want, first)  # order matters: a first-writer-wins grid is another grid
    if name == "monu2" and n == 64:  # the identity placement: every voxel its own cell, y and z swapped
        sx, sy, sz = (int(v) for v in size)
        ident = np.where(vox == 0, np.uint8(255), vox).reshape(sz, sy, sx).transpose(1, 0, 2)
        assert np.array_equal(want.reshape(n, n, n), ident)
    # Scene::scaleModel afterwards, and a second call fed the returned scale multiplies again
    s1 = scale_rule(size, n)
    assert np.array_equal(np.array(res.scale_model[:], np.float32).view(np.uint32), s1.view(np.uint32))
    got2, res2 = place_host(pkg, size, vox, n, scale_model=tuple(res.scale_model))
    s2 = scale_rule(size, n, s1)
    assert np.array_equal(np.array(res2.scale_model[:], np.float32).view(np.uint32), s2.view(np.uint32))
    assert np.array_equal(got2, oracle_full(pkg, orc, size, vox, n, tuple(s1)))
    assert res.seed == 0 and res2.seed == 0  # not RANDOM: the seed given


PARTIAL_CASES = [("monu2", 64, 16, 16), ("monu2", 64, 64, 16), ("monu2", 64, 30, 6), ("monu2", 64, 3, 13),
                 ("monu2", 32, 30, 6), ("monu2", 32, 16, 16), ("monu2", 32, 64, 16), ("monu2", 32, 3, 13),
                 ("SmallBuilding02", 32, 30, 6), ("monu3", 16, 30, 6), ("TallBuilding01", 16, 3, 13)]


@pytest.mark.parametrize("name,n,columns,thickness", PARTIAL_CASES)
def test_partial_equals_oracle(pkg, orc, name, n, columns, thickness):
    sc = pkg.scene
    size, vox, _ = sc.load_model(name)
    want = oracle_partial(pkg, orc, size, vox, n, columns, thickness)
    got, res = place_host(pkg, size, vox, n, mode=pkg.abi.LOAD_PARTIAL, columns=columns, thickness=thickness)
    assert np.array_equal(got, want)
    assert np.array_equal(got, sc.load_model_partial(size, vox, n, columns, thickness)[0])
    if (columns, thickness) == (3, 13):  # the lower bound wraps to 0xfffffff6: no column passes
        assert (got == 255).all()
    else:
        assert (got != 255).any() and not np.array_equal(got, oracle_full(pkg, orc, size, vox, n))
    assert np.array_equal(np.array(res.scale_model[:], np.float32).view(np.uint32), scale_rule(size, n).view(np.uint32))
    s1 = tuple(res.scale_model)
    got2, _ = place_host(pkg, size, vox, n, mode=pkg.abi.LOAD_PARTIAL, columns=columns, thickness=thickness,
                         scale_model=s1)
    assert np.array_equal(got2, oracle_partial(pkg, orc, size, vox, n, columns, thickness, s1))


def sequential_random(pkg, orc, size, vox, n, seed, lo, hi, scale=ONE):
    """Scene::LoadModelRandomMaterials as written (scene.cpp:636-679) with the oracle's RandomFloat:
    one draw per voxel in loop order, empty ones included, last write stays."""
    ol = orc._lib(pkg.abi)
    sx, sy, sz = (int(v) for v in size)
    s = scale_rule(size, n, scale)
    state = C.c_uint32(seed)
    ref = C.byref(state)
    draw = ol.oracle_random_float
    r = np.array([draw(ref) for _ in range(sx * sy * sz)], np.float32)  # one per voxel, in loop order
    mats = (np.float32(lo) + r * (np.float32(hi) - np.float32(lo))).astype(np.uint8)  # Rand(lo, hi) -> MatType
    grid = np.full(n ** 3, 255, np.uint8)
    gxs = [int(np.float32(x) * s[0]) for x in range(sx)]
    gys = [int(np.float32(z) * s[1]) for z in range(sz)]
    gzs = [int(np.float32(y) * s[2]) for y in range(sy)]
    for i in np.nonzero(vox)[0].tolist():  # ascending i: the loop's order, a later write replaces an earlier one
        x, y, z = i % sx, (i // sx) % sy, i // (sx * sy)
        if 0 <= gxs[x] < n and 0 <= gys[z] < n and 0 <= gzs[y] < n:
            grid[gxs[x] + gys[z] * n + gzs[y] * n * n] = mats[i]
    return grid, state.value


@pytest.fixture(scope="module")
def random_models(pkg):
    sc = pkg.scene
    return {name: sc.load_model(name)[:2] for name in ("Text", "monu2")}


@pytest.mark.parametrize("seed", [0x12345678, 1, 0])
@pytest.mark.parametrize("name", ["Text", "monu2"])
def test_random_equals_sequential(pkg, orc, random_models, name, seed):
    n = 32
    size, vox = random_models[name]
    want, state = sequential_random(pkg, orc, size, vox, n, seed, 9.0, 15.0)
    got, res = place_host(pkg, size, vox, n, mode=pkg.abi.LOAD_RANDOM, seed=seed, rand_lo=9.0, rand_hi=15.0)
    assert np.array_equal(got, want)
    assert res.seed == state
    g2, s2 = pkg.scene.load_model_random(size, vox, n, seed, 9.0, 15.0)
    assert np.array_equal(g2, want) and s2 == state
    if seed:
        assert len(np.unique(want[want != 255])) >= 5  # the range is used
        if name == "monu2":  # collisions: the last draw stays, not the first
            tgt, _, _ = writes(size, vox, n)
            assert len(np.unique(tgt)) < len(tgt)
    else:
        assert set(np.unique(want)) == {9, 255}  # the zero state stays zero: every draw is rand_lo


def xorshift32_inverse(s):
    """The state one step before s (each of the three xor-shifts undone)."""
    def unshl(v, k):
        r = v
        for _ in range(32 // k + 1):
            r = v ^ ((r << k) & 0xFFFFFFFF)
        return r

    def unshr(v, k):
        r = v
        for _ in range(32 // k + 1):
            r = v ^ (r >> k)
        return r

    return unshl(unshr(unshl(s, 5), 17), 13)


def test_random_reference_range_reaches_13(pkg, orc, random_models):
    """Rand(12, 13) gives 13 only when RandomFloat() rounds to 1.0f, a draw of at least
    0xFFFFFF80: a seed inverted from such a state at a non-empty voxel that keeps its cell."""
    n = 32
    size, vox = random_models["Text"]
    assert int(size[0]) <= n  # identity placement: every non-empty voxel owns its cell
    i = int(np.nonzero(vox)[0][len(np.nonzero(vox)[0]) // 2])
    seed = 0xFFFFFFC3
    ol = orc._lib(pkg.abi)
    for _ in range(i + 1):
        seed = xorshift32_inverse(seed)
    chk = C.c_uint32(seed)
    for _ in range(i + 1):
        ol.oracle_xorshift32(C.byref(chk))
    assert chk.value == 0xFFFFFFC3
    want, state = sequential_random(pkg, orc, size, vox, n, seed, 12.0, 13.0)
    assert set(np.unique(want)) == {12, 13, 255}
    got, res = place_host(pkg, size, vox, n, mode=pkg.abi.LOAD_RANDOM, seed=seed, rand_lo=12.0, rand_hi=13.0)
    assert np.array_equal(got, want) and res.seed == state
    g2, s2 = pkg.scene.load_model_random(size, vox, n, seed)
    assert np.array_equal(g2, want) and s2 == state


def test_xorshift32_jump(pkg, orc):
    lib, ol = pkg.load_library(), orc._lib(pkg.abi)
    ks = [0, 1, 2, 31, 32, 33, 147, 558, 2 ** 18, 2 ** 24 - 1]
    tris = (pkg.abi.BvhTri * 64)()
    for s in (0, 1, 0x12345678, 0xFFFFFFFF, 0x80000000, 2463534242):
        st, done = C.c_uint32(s), 0
        for k in ks:
            # the oracle's looped steps: 576 per call of its BasicBVH triangle draw (64 triangles of
            # 9 RandomFloat each, BasicBVH.cpp:4-16), the rest one at a time
            while k - done >= 576:
                st.value = ol.oracle_bvh_random_tris(st.value, tris)
                done += 576
            for _ in range(k - done):
                ol.oracle_xorshift32(C.byref(st))
            done = k
            assert lib.vpx_xorshift32_jump(s, k) == st.value, (s, k)
        assert int(pkg.scene.xorshift32_stream(s, 2 ** 18)[-1]) == lib.vpx_xorshift32_jump(s, 2 ** 18)
        if s:
            assert lib.vpx_xorshift32_jump(s, 2 ** 32 - 1) == s  # the period: T^(2^32 - 1) is the identity
            assert lib.vpx_xorshift32_jump(s, 2 ** 32 + 146) == lib.vpx_xorshift32_jump(s, 147)
        else:
            assert lib.vpx_xorshift32_jump(0, 2 ** 32 - 1) == 0  # the zero state is a fixed point


@pytest.mark.parametrize("name", ["player", "Text"])
def test_palette_materials(pkg, name):
    lib, abi, sc = pkg.load_library(), pkg.abi, pkg.scene
    _, vox, pal = sc.load_model(name)
    want = sc.palette_materials(sc.default_materials(), vox, pal)
    got = sc.default_materials()
    pal = np.ascontiguousarray(pal, np.uint8)
    assert lib.vpx_model_palette_materials(got, vox.ctypes.data, vox.size, pal.ctypes.data) == abi.VPX_OK
    assert bytes(got) == bytes(want)
    assert bytes(got) != bytes(sc.default_materials())
    assert lib.vpx_model_palette_materials(None, vox.ctypes.data, vox.size, pal.ctypes.data) == abi.VPX_E_INVALID
    assert lib.vpx_model_palette_materials(got, None, vox.size, pal.ctypes.data) == abi.VPX_E_INVALID
    assert lib.vpx_model_palette_materials(got, vox.ctypes.data, vox.size, None) == abi.VPX_E_INVALID


def test_argument_errors(pkg):
    lib, abi = pkg.load_library(), pkg.abi
    vox = np.ones(4 * 3 * 2, np.uint8)
    cells = np.zeros(8 ** 3, np.uint8)
    res = abi.ModelResult()

    def call(ld, sx=4, sy=3, sz=2, n=8, v=vox, c=cells):
        return lib.vpx_model_place_host(None if v is None else v.ctypes.data, sx, sy, sz, n,
                                        None if ld is None else C.byref(ld), None if c is None else c.ctypes.data,
                                        C.byref(res))

    assert call(abi.model_load()) == abi.VPX_OK
    assert lib.vpx_model_place_host(vox.ctypes.data, 4, 3, 2, 8, C.byref(abi.model_load()), cells.ctypes.data,
                                    None) == abi.VPX_OK  # out may be NULL
    assert call(None) == abi.VPX_E_INVALID
    assert call(abi.model_load(), v=None) == abi.VPX_E_INVALID
    assert call(abi.model_load(), c=None) == abi.VPX_E_INVALID
    bad = abi.model_load()
    bad.reserved = 1
    assert call(bad) == abi.VPX_E_INVALID
    assert call(abi.model_load(mode=3)) == abi.VPX_E_INVALID
    for dims in ((0, 3, 2), (4, 0, 2), (4, 3, 0), (257, 1, 1), (1, 257, 1), (1, 1, 257)):
        assert call(abi.model_load(), *dims) == abi.VPX_E_INVALID, dims
    assert call(abi.model_load(), n=0) == abi.VPX_E_INVALID
    assert call(abi.model_load(), n=4097) == abi.VPX_E_INVALID
    nan = float("nan")
    for lo, hi in ((-1.0, 5.0), (5.0, 4.0), (0.0, 256.0), (nan, 5.0), (1.0, nan), (-0.5, -0.25)):
        assert call(abi.model_load(mode=abi.LOAD_RANDOM, rand_lo=lo, rand_hi=hi)) == abi.VPX_E_INVALID, (lo, hi)
        assert call(abi.model_load(mode=abi.LOAD_FULL, rand_lo=lo, rand_hi=hi)) == abi.VPX_OK  # RANDOM's rule only
    for lo, hi in ((0.0, 0.0), (0.0, 255.0), (255.0, 255.0), (12.0, 13.0)):
        assert call(abi.model_load(mode=abi.LOAD_RANDOM, rand_lo=lo, rand_hi=hi)) == abi.VPX_OK, (lo, hi)


def test_non_monotone_and_nan_scales(pkg, orc):
    """Negative, NaN and overflowing scales: the truncation gives INT_MIN (or a negative cell) and
    the write is dropped, axis by axis, as in the oracle's loop."""
    size, vox, _ = pkg.scene.load_model("TallBuilding01")
    nan = float("nan")
    for scale in ((-1.0, 1.0, 1.0), (1.0, nan, 1.0), (1.0, 1.0, 3e9), (0.5, 0.25, 2.0), (0.0, 0.0, 0.0), (1.0, 1.0, -0.1)):
        want = oracle_full(pkg, orc, size, vox, 16, scale)
        got, _ = place_host(pkg, size, vox, 16, scale_model=scale)
        assert np.array_equal(got, want), scale


def test_native_model_place(tmp_path):
    """tests/native/model_place_test.cpp: the shared header against a naive triple loop, built
    with g++ alone (no HIP)."""
    exe = tmp_path / "model_place_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(HERE, "native", "model_place_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("bad=0"), r.stdout
