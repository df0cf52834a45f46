"""Model stamps on the CPU (csrc/vpx_stamp.hpp through vpx_stamp_apply_host).

Against tests/stamp_ref.py, which never computes a model index: all 48 orientations of a 3x5x7
model with distinct bytes in a 16^3 grid, inside it and clipped through each of its six faces,
a stamp wholly outside, the filters, CONSTANT with a material and with 255, GRID_BYTES with a
model that holds byte 0, a default-convention model that holds byte 255, two overlapping stamps
whose result depends on their order, the counts, every refusal and the struct sizes.  The GPU
side is tests/test_stamp_gpu.py.
"""
import ctypes as C

import numpy as np
import pytest

from stamp_ref import CONSTANT, GRID_BYTES, ORIENTATIONS, numpy_stamps, oriented
from test_brush import world

N = 16
SIZE = (3, 5, 7)


def distinct_model(size=SIZE):
    """Bytes 1 .. sx*sy*sz, index x + y*sx + z*sx*sy: no two voxels alike, none empty."""
    return size, np.arange(1, size[0] * size[1] * size[2] + 1, dtype=np.uint8)


def check(pkg, cells, n, models, stamps, what):
    want, changed, flipped = numpy_stamps(cells, n, models, stamps)
    got = np.ascontiguousarray(cells, np.uint8).reshape(-1).copy()
    res = pkg.scene.apply_stamps(got, n, models, stamps)
    assert np.array_equal(got, want), what
    assert (res.changed, res.flipped, res.reserved) == (changed, flipped, 0), (what, res.changed, res.flipped, changed, flipped)
    return want, changed, flipped


def test_reference_tells_the_orientations_apart(pkg):
    sc = pkg.scene
    rng = np.random.default_rng(5)
    size, vox = SIZE, rng.integers(1, 255, 105).astype(np.uint8)
    images = {oriented(size, vox, sc.orient(a, f)).tobytes() + bytes(oriented(size, vox, sc.orient(a, f)).shape) for a, f in ORIENTATIONS}
    assert len(ORIENTATIONS) == 48 == len(images)
    assert sc.orient() == pkg.abi.ORIENT_IDENTITY == 0x24 and sc.orient((0, 2, 1)) == pkg.abi.ORIENT_LOAD_MODEL == 0x18
    # the header's per-cell formula, written out, on one orientation: x <- z mirrored, y <- x, z <- y
    t = oriented(size, vox, sc.orient((2, 0, 1), (True, False, False)))
    sx, sy, sz = size
    assert t.shape == (sy, sx, sz)
    for gz, gy, gx in ((0, 0, 0), (4, 2, 6), (1, 2, 3)):
        m = {2: sz - 1 - gx, 0: gy, 1: gz}
        assert t[gz, gy, gx] == vox[m[0] + m[1] * sx + m[2] * sx * sy]


# inside the grid, then pushed through each face: low x, high x, low y, ...
PLACES = [("inside", (5, 4, 6))] + [(f"{'xyz'[q]} {'low' if low else 'high'}",
                                      tuple((-2 if low else N - 2) if k == q else (5, 4, 6)[k] for k in range(3)))
                                     for q in range(3) for low in (True, False)]


@pytest.mark.parametrize("place,origin", PLACES, ids=[p[0] for p in PLACES])
def test_all_orientations(pkg, place, origin):
    sc = pkg.scene
    models = [distinct_model()]
    cells = world(N)
    seen = set()
    for axes, flips in ORIENTATIONS:
        want, changed, _ = check(pkg, cells, N, models, [sc.stamp(0, origin, sc.orient(axes, flips))], (place, axes, flips))
        assert changed > 0
        seen.add(want.tobytes())
    assert len(seen) == 48  # no two orientations leave the same grid, clipped or not


def test_outside_the_grid(pkg):
    sc = pkg.scene
    models = [distinct_model()]
    cells = world(N)
    for origin in ((N, 0, 0), (0, -7, 0), (0, 0, N + 100), (-3, 2, 2), (2 ** 31 - 1, 0, 0), (-2 ** 31, -2 ** 31, -2 ** 31)):
        _, changed, flipped = check(pkg, cells, N, models, [sc.stamp(0, origin)], origin)
        assert (changed, flipped) == (0, 0), origin
    # one cell of the model's far corner still lands in the grid
    _, changed, _ = check(pkg, cells, N, models, [sc.stamp(0, (-2, -4, -6), match=(255, 255))], "far corner")
    assert changed <= 1


def test_filters_and_constant(pkg):
    sc = pkg.scene
    size, vox = distinct_model()
    vox = vox.copy()
    vox[::4] = 0  # empty voxels leave their cells alone
    models = [(size, vox)]
    base = np.full((N, N, N), 255, np.uint8)
    base[4:9, 4:8, 4:6] = 3  # [z, y, x]: half of the stamp's box is solid
    for match in ((0, 255), (255, 255), (0, 254), (3, 3), (4, 200)):
        for flags, value in ((0, 0), (CONSTANT, 9), (CONSTANT, 255), (CONSTANT, 3)):
            st = sc.stamp(0, (4, 4, 4), flags=flags, value=value, match=match)
            _, changed, _ = check(pkg, base, N, models, [st], (match, flags, value))
            if match == (4, 200):
                assert changed == 0
    solid = int((vox != 0).sum())
    assert check(pkg, base, N, models, [sc.stamp(0, (4, 4, 4))], "all")[1] == solid
    # digging the model's shape out flips the brick it empties; a repaint flips nothing
    block = np.full((N, N, N), 255, np.uint8)
    block[4:8, 4:8, 4:8] = 3
    full = [((4, 4, 4), np.ones(64, np.uint8))]
    assert check(pkg, block, N, full, [sc.stamp(0, (4, 4, 4), flags=CONSTANT, value=255)], "dig")[1:] == (64, 1)
    assert check(pkg, block, N, full, [sc.stamp(0, (4, 4, 4), flags=CONSTANT, value=6, match=(0, 254))], "repaint")[1:] == (64, 0)
    assert check(pkg, block, N, full, [sc.stamp(0, (4, 4, 4), match=(255, 255))], "nothing empty there")[1:] == (0, 0)


def test_byte_conventions(pkg):
    sc = pkg.scene
    size = (4, 3, 2)
    vox = np.array([0, 255, 7, 0, 255, 1, 0, 9] * 3, np.uint8)
    models = [(size, vox)]
    cells = np.full(N ** 3, 4, np.uint8)
    # GRID_BYTES: 255 is empty and byte 0 is a material that is written
    want, changed, _ = check(pkg, cells, N, models, [sc.stamp(0, (1, 2, 3), flags=GRID_BYTES)], "grid bytes")
    assert changed == int((vox != 255).sum()) and (want == 0).sum() == int((vox == 0).sum()) and not (want == 255).any()
    # default: 0 is empty and a voxel byte 255 writes NONE
    want, changed, _ = check(pkg, cells, N, models, [sc.stamp(0, (1, 2, 3))], "model bytes")
    assert changed == int((vox != 0).sum()) and (want == 255).sum() == int((vox == 255).sum()) and not (want == 0).any()
    for flags in (GRID_BYTES | CONSTANT, CONSTANT):
        check(pkg, cells, N, models, [sc.stamp(0, (1, 2, 3), sc.orient((1, 2, 0), (True, False, True)), flags, 0)], flags)


def test_order_matters(pkg):
    sc = pkg.scene
    models = [((6, 6, 6), np.full(216, 7, np.uint8)), ((5, 5, 5), np.full(125, 8, np.uint8))]
    base = np.full(N ** 3, 255, np.uint8)
    a, b = sc.stamp(0, (2, 2, 2), match=(255, 255)), sc.stamp(1, (6, 6, 6), match=(255, 255))
    ab, _, _ = check(pkg, base, N, models, [a, b], "a then b")
    ba, _, _ = check(pkg, base, N, models, [b, a], "b then a")
    assert not np.array_equal(ab, ba)
    # a later stamp's filter sees what the earlier one left
    c = sc.stamp(1, (2, 2, 2), flags=CONSTANT, value=255, match=(7, 7))
    _, changed, flipped = check(pkg, base, N, models, [a, c], "place then dig")
    assert changed == 216 + 125 and flipped > 0


def test_several_models_and_counts(pkg):
    sc = pkg.scene
    rng = np.random.default_rng(11)
    models = [distinct_model(), ((33, 2, 2), rng.integers(0, 256, 132).astype(np.uint8)), ((1, 1, 1), np.array([5], np.uint8)),
              ((2, 3, 33), rng.integers(0, 4, 198).astype(np.uint8))]
    for n in (37, 64):
        cells = world(n)
        stamps = [sc.stamp(1, (-1, 3, 3)), sc.stamp(1, (n - 20, 9, 3), sc.orient((0, 1, 2), (True, False, False))),
                  sc.stamp(2, (0, 0, 0)), sc.stamp(2, (n - 1, n - 1, n - 1), match=(255, 255)),
                  sc.stamp(3, (3, 20, 10), sc.orient((2, 1, 0))), sc.stamp(3, (n - 9, 20, 20), sc.orient((2, 0, 1), (True, True, False))),
                  sc.stamp(0, (10, 0, 10), flags=CONSTANT, value=255), sc.stamp(0, (12, 1, 12), pkg.abi.ORIENT_LOAD_MODEL, GRID_BYTES)]
        _, changed, flipped = check(pkg, cells, n, models, stamps, n)
        assert changed > 0 and flipped > 0


def test_struct_sizes_and_validation(pkg):
    abi, sc = pkg.abi, pkg.scene
    lib = pkg.load_library()
    assert C.sizeof(abi.Stamp) == 32 == abi.STRUCT_SIZES[abi.Stamp]
    assert C.sizeof(abi.StampSource) == 24 == abi.STRUCT_SIZES[abi.StampSource]
    assert (abi.Stamp.origin.offset, abi.Stamp.orient.offset, abi.Stamp.flags.offset, abi.Stamp.value.offset,
            abi.Stamp.reserved.offset, abi.Stamp.reserved2.offset) == (4, 16, 20, 24, 27, 28)
    assert abi.StampSource.sx.offset == 8 and abi.StampSource.reserved.offset == 20
    n = 8
    cells = np.full(n ** 3, 255, np.uint8)
    vox = np.ones(8, np.uint8)
    src = (abi.StampSource * 1)(abi.StampSource(vox.ctypes.data, 2, 2, 2, 0))
    good = sc.stamp(0, (0, 0, 0))

    def call(stamps, count=None, c=cells, size=n, models=src, n_models=1):
        arr = (abi.Stamp * max(1, len(stamps)))(*stamps) if stamps is not None else None
        return lib.vpx_stamp_apply_host(None if c is None else c.ctypes.data, size, models, n_models, arr,
                                        len(stamps) if count is None else count, None)

    assert call([good]) == abi.VPX_OK and (cells != 255).sum() == 8
    assert call(None, 1) == abi.VPX_E_INVALID
    assert call([good], 0) == abi.VPX_E_INVALID
    assert call([good] * 257) == abi.VPX_E_INVALID
    assert call([good] * 256) == abi.VPX_OK
    assert call([good], c=None) == abi.VPX_E_INVALID
    assert call([good], size=0) == abi.VPX_E_INVALID
    assert call([good], models=None) == abi.VPX_E_INVALID
    assert call([good], n_models=0) == abi.VPX_E_INVALID
    assert call([good, sc.stamp(1, (0, 0, 0))]) == abi.VPX_E_INVALID  # unknown model
    for bad_src in (abi.StampSource(None, 2, 2, 2, 0), abi.StampSource(vox.ctypes.data, 0, 2, 2, 0),
                    abi.StampSource(vox.ctypes.data, 2, 257, 2, 0), abi.StampSource(vox.ctypes.data, 2, 2, 2, 1)):
        assert call([good], models=(abi.StampSource * 1)(bad_src)) == abi.VPX_E_INVALID
    # orient: axes that are no permutation, an axis 3, stray bits
    for orient in (0x00, 0x14, 0x25, 0x3C, 0x27, 0x24 | 0x40, 0x24 | 0x80, 0x24 | 0x800, 0x24 | 1 << 31):
        bad = sc.stamp(0, (0, 0, 0))
        bad.orient = orient
        assert call([good, bad]) == abi.VPX_E_INVALID, hex(orient)
    for axes, flips in ((a, f) for a in ((0, 1, 2), (2, 0, 1)) for f in ((False,) * 3, (True,) * 3)):
        assert call([sc.stamp(0, (0, 0, 0), sc.orient(axes, flips))]) == abi.VPX_OK
    for field, value in (("flags", 4), ("flags", 0x80000001), ("reserved", 1), ("reserved2", 1)):
        bad = sc.stamp(0, (0, 0, 0))
        setattr(bad, field, value)
        assert call([good, bad]) == abi.VPX_E_INVALID, field
    assert call([sc.stamp(0, (0, 0, 0), match=(5, 4))]) == abi.VPX_E_INVALID
    assert call([sc.stamp(0, (0, 0, 0), flags=GRID_BYTES | CONSTANT, value=255, match=(4, 4))]) == abi.VPX_OK
