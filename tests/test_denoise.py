"""The plane-keyed a-trous filter on the host (vpx_denoise_host) against its numpy restatement
(tests/denoise_ref.py), bit for bit, on synthetic ID buffers; then the filter's properties: invalid
keys pass through, .w is untouched, a NaN or an infinity on one plane never reaches another, a
constant colour comes back exactly, rgb8 is the frame's tonemap, and the refusals.  No GPU.

The patterns, the colours and the cached references are shared with tests/test_denoise_gpu.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref
import epilogue_ref

SIZES = ((67, 35), (16, 16), (5, 3), (1, 1))
PASSES = (1, 2, 5)
SIGMAS = (0.0, 0.5)
FIELDS = ("vox_index", "material", "face_axis", "face_sign", "coord")
PATTERNS = ("one_plane", "stripes1", "stripes3", "checker") + tuple("field_" + f for f in FIELDS) + (
    "invalid", "coord_extremes")


def pack_ids(rng, v, mat, face, coord):
    """An ID buffer [H, W, 4] from per-pixel fields as vpx_render_ids packs them: v = vox_index + 2,
    material, face, and the plane coordinate, stored in the cell component of the face's axis.  The
    other two cell components and the bits of t are random: the key must not read them."""
    h, w = v.shape
    axis = np.where((face >= 1) & (face <= 6), (np.maximum(face, 1) - 1) >> 1, 0)
    cell = rng.integers(0, 4096, (3, h, w)).astype(np.uint32)
    for a in range(3):
        cell[a] = np.where(axis == a, coord, cell[a])
    ids = np.empty((h, w, 4), np.uint32)
    ids[..., 0] = rng.integers(0, 2**32, (h, w), dtype=np.uint64).astype(np.uint32)
    ids[..., 1] = (v.astype(np.uint32) & 0xFFFF) | (mat.astype(np.uint32) << 16) | (face.astype(np.uint32) << 24)
    ids[..., 2] = cell[0] | (cell[1] << 16)
    ids[..., 3] = cell[2]
    return ids


def pattern_fields(name, w, h):
    """(v, material, face, coord, region) per pixel; region numbers the areas the pattern tells apart."""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    one = np.ones((h, w), np.int64)
    v, mat, face, coord = 2 * one, 3 * one, 1 * one, 7 * one
    region = 0 * one
    if name == "one_plane":
        pass
    elif name in ("stripes1", "stripes3"):
        region = (x // (1 if name == "stripes1" else 3)) % 2
        coord = 7 + region
    elif name == "checker":
        region = (x + y) % 2
        mat = 3 + region
    elif name.startswith("field_"):
        region = (x > w // 2 + (y % 3) - 1).astype(np.int64)  # a wobbling vertical border
        f = name[len("field_"):]
        if f == "vox_index":
            v = 2 + region
        elif f == "material":
            mat = 3 + region
        elif f == "face_axis":
            face = 1 + 2 * region  # the same coordinate value, read from another cell component
        elif f == "face_sign":
            face = 1 + region
        else:
            coord = 7 + region
    elif name == "invalid":
        # the upper three fifths one plane; below it a miss, a shape win, a face 0 and a face 7
        band = np.minimum(x * 4 // max(w, 1), 3) + 1
        region = np.where(y * 5 < h * 3, 0, band)
        v = np.select([region == 1, region == 2], [0 * one, 1 * one], 2 * one)
        mat = np.where(region == 1, 255, 3)
        face = np.select([region == 1, region == 2, region == 3, region == 4], [0 * one, 2 * one, 0 * one, 7 * one], one)
    elif name == "coord_extremes":
        region = np.minimum(x * 6 // max(w, 1), 5)  # per axis a band at coordinate 0 and one at 4095
        face = 1 + 2 * (region // 2)
        coord = np.where(region % 2 == 0, 0, 4095)
    else:
        raise KeyError(name)
    return v, mat, face, coord, region


@functools.lru_cache(maxsize=None)
def pattern(name, w, h):
    """(ids uint32 [H, W, 4], image float32 [H, W, 4], region [H, W]): colours 2^u, u uniform in
    [-6, 6]; .w any bit pattern at all."""
    rng = np.random.default_rng([PATTERNS.index(name), w, h])
    v, mat, face, coord, region = pattern_fields(name, w, h)
    ids = pack_ids(rng, v, mat, face, coord)
    img = np.empty((h, w, 4), np.float32)
    img[..., :3] = np.exp2(rng.uniform(-6.0, 6.0, (h, w, 3))).astype(np.float32)
    img[..., :3] = np.clip(img[..., :3], np.float32(2.0**-6), np.float32(2.0**6))
    img[..., 3] = rng.integers(0, 2**32, (h, w), dtype=np.uint64).astype(np.uint32).view(np.float32)
    for a in (ids, img, region):
        a.setflags(write=False)
    return ids, img, region


@functools.lru_cache(maxsize=None)
def reference(name, w, h, sigma_l):
    """denoise_ref.run over five passes, computed once: ([out_1 .. out_5], pass 0's tap counts)."""
    ids, img, _ = pattern(name, w, h)
    outs, taps = denoise_ref.run(ids, img, max(PASSES), sigma_l)
    for a in outs + [taps]:
        a.setflags(write=False)
    return outs, taps


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what):
    """Bit equality of float images; NaN payloads apart (the project's known exception)."""
    g, w = u32(got), u32(want)
    gn, wn = np.isnan(np.asarray(got)), np.isnan(np.asarray(want))
    bad = (gn != wn) | (~wn & (g != w))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def poisoned(img, region, value):
    """img with every colour of region 1 replaced by `value`."""
    out = img.copy()
    out[..., :3][region == 1] = value
    return out


POISON = ("stripes1", "checker", "field_material", "field_coord")


# ------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", PATTERNS)
def test_host_equals_restatement(pkg, name, size):
    w, h = size
    ids, img, _ = pattern(name, w, h)
    ka, kb = denoise_ref.keys(ids)
    for sigma_l in SIGMAS:
        outs, taps = reference(name, w, h, sigma_l)
        if size == (67, 35):  # "everything passed through" must not be a passing result
            assert int(((kb != 0) & (taps >= 2)).sum()) * 2 >= w * h, (name, "too few filtered pixels")
        for passes in PASSES:
            got = pkg.context.denoise_host(w, h, ids, img, passes, sigma_l)
            want = outs[passes - 1]
            assert np.array_equal(u32(got), u32(want)), (name, size, passes, sigma_l, int((u32(got) != u32(want)).sum()))
            assert np.array_equal(u32(got)[..., 3], u32(img)[..., 3]), ".w is untouched"
            assert np.array_equal(u32(got)[kb == 0], u32(img)[kb == 0]), "invalid keys pass through"
    if size == (1, 1):
        # no tap but the centre: out = (9/64 * c) / (9/64), the input up to the one rounding of 9 * c
        # (exactly the input where 9 * c needs no rounding; the restatement decides the bits)
        assert taps.tolist() == [[1]] and np.allclose(got[..., :3], img[..., :3], rtol=2.0**-22, atol=0)


def test_patterns_are_what_they_claim():
    """The field patterns differ in exactly one key field; the invalid pattern's four lower regions
    have the invalid key, for four different reasons; coordinates 0 and 4095 are valid keys."""
    for f in FIELDS:
        ids, _, region = pattern("field_" + f, 67, 35)
        ka, kb = denoise_ref.keys(ids)
        a = {(int(ka[region == r][0]), int(kb[region == r][0])) for r in (0, 1)}
        assert len(a) == 2 and (kb != 0).all()
        assert len(np.unique(ka[region == 0])) == 1 and len(np.unique(kb[region == 1])) == 1
        (a0, b0), (a1, b1) = sorted(a)
        diff = [(a0 ^ a1) & 0xFFFF, (a0 ^ a1) >> 16 & 0xFF, (a0 ^ a1) >> 24, b0 ^ b1]
        want = {"vox_index": [1, 0, 0, 0], "material": [0, 1, 0, 0], "face_axis": [0, 0, 1, 0], "face_sign": [0, 0, 1, 0],
                "coord": [0, 0, 0, 1]}[f]
        assert [int(bool(d)) for d in diff] == want, (f, diff)
    ids, _, region = pattern("invalid", 67, 35)
    ka, kb = denoise_ref.keys(ids)
    assert (kb[region == 0] != 0).all() and not ka[region > 0].any() and not kb[region > 0].any()
    assert sorted(np.unique(region).tolist()) == [0, 1, 2, 3, 4]
    y = ids[..., 1]
    assert (y[region == 2] & 0xFFFF == 1).all() and (y[region == 3] >> 24 == 0).all() and (y[region == 4] >> 24 == 7).all()
    ids, _, region = pattern("coord_extremes", 67, 35)
    ka, kb = denoise_ref.keys(ids)
    assert sorted(set((kb & 0x7FFFFFFF).reshape(-1).tolist())) == [0, 4095] and (kb >> 31 == 1).all()
    assert len({(int(a), int(b)) for a, b in zip(ka.reshape(-1), kb.reshape(-1))}) == 6


# -------------------------------------------------------------------------- 2. properties
@pytest.mark.parametrize("name", POISON)
def test_nan_and_inf_stay_on_their_plane(pkg, name):
    for w, h in ((67, 35), (16, 16)):
        ids, img, region = pattern(name, w, h)
        assert (region == 1).any() and (region == 0).any()
        for sigma_l in SIGMAS:
            for passes in (1, 5):
                clean = pkg.context.denoise_host(w, h, ids, img, passes, sigma_l)
                for value in (np.nan, np.inf):
                    got = pkg.context.denoise_host(w, h, ids, poisoned(img, region, value), passes, sigma_l)
                    assert np.array_equal(u32(got)[region == 0], u32(clean)[region == 0]), (name, passes, sigma_l, value)
                    assert not np.isfinite(got[..., :3][region == 1]).any()


@pytest.mark.parametrize("c", (1.0, 0.75))
@pytest.mark.parametrize("name", ("one_plane", "stripes3", "field_face_sign"))
def test_constant_colour_comes_back(pkg, name, c):
    """sigma_l == 0: wsum is an exact dyadic and so is every w * c and their sum: acc / wsum == c."""
    w, h = 67, 35
    ids, img, _ = pattern(name, w, h)
    flat = img.copy()
    flat[..., :3] = np.float32(c)
    for passes in PASSES:
        got = pkg.context.denoise_host(w, h, ids, flat, passes, 0.0)
        assert np.array_equal(u32(got), u32(flat)), (name, c, passes)


@pytest.mark.parametrize("name", ("field_material", "invalid"))
def test_rgb8_is_the_tonemap_of_out(pkg, name):
    w, h = 67, 35
    ids, img, _ = pattern(name, w, h)
    out, rgb = pkg.context.denoise_host(w, h, ids, img, 2, 0.5, rgb=True)
    assert np.array_equal(u32(out), u32(reference(name, w, h, 0.5)[0][1]))
    want = np.array([epilogue_ref.tonemap_ref(px[:3].astype(np.float64)) for px in out.reshape(-1, 4)], np.uint32)
    assert np.array_equal(rgb.reshape(-1), want)
    assert len(np.unique(rgb)) > 100


def refusals(abi, call, ids, src, out):
    """Every refusal of the two entries; call(width, height, ids, in, out, denoise or None) -> status."""
    ok = abi.Denoise(2, 0.5, 0, 0)
    assert call(67, 35, ids, src, out, ok) == abi.VPX_OK
    for bad in ((67, 35, None, src, out, ok), (67, 35, ids, None, out, ok), (67, 35, ids, src, None, ok),
                (67, 35, ids, src, out, None),
                (0, 35, ids, src, out, ok), (67, 0, ids, src, out, ok), (32769, 1, ids, src, out, ok),
                (1, 32769, ids, src, out, ok), (32768, 32768, ids, src, out, ok),
                (67, 35, ids, src, src, ok), (67, 35, ids, src, ids, ok)):
        assert call(*bad) == abi.VPX_E_INVALID, bad[:2]
    for d in (abi.Denoise(0, 0.0, 0, 0), abi.Denoise(6, 0.0, 0, 0), abi.Denoise(0xFFFFFFFF, 0.0, 0, 0),
              abi.Denoise(2, -0.5, 0, 0), abi.Denoise(2, float("nan"), 0, 0), abi.Denoise(2, float("inf"), 0, 0),
              abi.Denoise(2, float("-inf"), 0, 0), abi.Denoise(2, 0.5, 1, 0), abi.Denoise(2, 0.5, 0, 1)):
        assert call(67, 35, ids, src, out, d) == abi.VPX_E_INVALID, (d.passes, d.sigma_l, d.flags, d.reserved)


def test_refusals(pkg):
    abi, lib = pkg.abi, pkg.load_library()
    ids, img, _ = pattern("one_plane", 67, 35)
    ids, img = ids.copy(), img.copy()
    out = np.zeros_like(img)

    def call(w, h, i, s, o, d):
        return lib.vpx_denoise_host(w, h, None if i is None else i.ctypes.data, None if s is None else s.ctypes.data,
                                    None if o is None else o.ctypes.data, None, C.byref(d) if d is not None else None)

    refusals(abi, call, ids, img, out)
    out[:] = 0
    assert call(67, 35, ids, img, out, abi.Denoise(6, 0.0, 0, 0)) == abi.VPX_E_INVALID and not out.any()
