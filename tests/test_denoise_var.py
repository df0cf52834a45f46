"""The variance-guided denoise on the host (vpx_denoise_var_host, vpx_reproject_moments_host) against
the numpy restatements (tests/denoise_var_ref.py, tests/reproject_moments_ref.py), bit for bit, on
tests/test_denoise.py's patterns and tests/test_reproject_ids.py's cases; then the properties: NaN
and infinity stay on their plane (colour and variance alike), a constant colour with zero variance
comes back exactly, the refusals, and the two claims the filter is built on:

1. an edge the history vouches for survives: one plane, a luminance step dl, moments that say zero
   variance.  Then tol = epsilon, a tap across the edge weighs at most h * (epsilon / dl)^2
   (w = h / (1 + dd^2) < h / dd^2), those h sum to at most 55/64, wsum >= 9/64 (the centre), so
   |out - in| <= (55/9) * (epsilon / dl)^2 * dc per channel, dc the colour step; the plane-key
   filter at sigma_l = 0 moves the edge pixels by more than that.
2. a large uniform variance V gives the sigma_l = 0 result back: dd <= dmax / T with
   T = sigma_v * sqrt(Vmin), so w = h * (1 - e), 0 <= e <= delta = (dmax / T)^2, and for colours in
   [0, cmax] |sum(w c) / sum(w) - sum(h c) / sum(h)| <= cmax * delta / (1 - delta); the roundings of
   the two results (at most 2 x 51 operations of relative error 2^-24 on positive terms) add at
   most 2^-17 * cmax.

No GPU.  The patterns, the moments and the cached references are shared with
tests/test_denoise_var_gpu.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref
import denoise_var_ref
import reproject_ids_ref
import reproject_moments_ref
import test_reproject_ids as tri
from test_denoise import PASSES, PATTERNS, POISON, SIZES, pattern, poisoned, same_bits, u32

pytestmark = [pytest.mark.filterwarnings("ignore:invalid value:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:overflow:RuntimeWarning")]

F = np.float32
SIGMA_V, EPSILON, MIN_HISTORY = 4.0, 2.0 ** -4, 4  # inside denoise_var_ref's tested ranges
VAR = dict(sigma_v=SIGMA_V, epsilon=EPSILON, min_history=MIN_HISTORY)
LENGTHS = np.array([0.0, 1.0, 2.0, 3.0, 3.0, 4.0, 4.0, 5.0, 32.0, 65536.0, np.nan, -7.0], F)


@functools.lru_cache(maxsize=None)
def with_moments(name, w, h):
    """(image, moments) for the calls with mom given: the pattern's image with history lengths from
    LENGTHS in .w (half of them below MIN_HISTORY, a NaN and a negative one among them), and moments
    m1 = lum * 2^u, u in [-1/4, 1/4]; m2 = m1^2 + 2^v, v in [-8, 2], but a tenth of them
    m2 = 0.9 * m1^2: a negative variance, clamped to zero."""
    ids, img, _ = pattern(name, w, h)
    rng = np.random.default_rng([77, PATTERNS.index(name), w, h])
    img = img.copy()
    img[..., 3] = LENGTHS[rng.integers(0, len(LENGTHS), (h, w))]
    m1 = (denoise_ref.lum(img).astype(np.float64) * np.exp2(rng.uniform(-0.25, 0.25, (h, w)))).astype(F)
    m2 = (m1.astype(np.float64) ** 2 + np.exp2(rng.uniform(-8.0, 2.0, (h, w)))).astype(F)
    m2 = np.where(rng.uniform(0, 1, (h, w)) < 0.1, (0.9 * m1.astype(np.float64) ** 2).astype(F), m2)
    mom = np.stack([m1, m2], axis=2).astype(F)
    img.setflags(write=False)
    mom.setflags(write=False)
    return img, mom


def inputs(name, w, h, given):
    """(ids, image, moments or None) of one call."""
    ids, img, _ = pattern(name, w, h)
    if not given:
        return ids, img, None
    return (ids,) + with_moments(name, w, h)


@functools.lru_cache(maxsize=None)
def reference(name, w, h, given):
    """denoise_var_ref.run over five passes, computed once: ([out_1 .. out_5], variances, temporal mask)."""
    ids, img, mom = inputs(name, w, h, given)
    outs, variances, temporal = denoise_var_ref.run(ids, img, mom, max(PASSES), **VAR)
    for a in outs + variances + [temporal]:
        a.setflags(write=False)
    return outs, variances, temporal


# ------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", PATTERNS)
def test_host_equals_restatement(pkg, name, size):
    w, h = size
    for given in (False, True):
        ids, img, mom = inputs(name, w, h, given)
        ka, kb = denoise_ref.keys(ids)
        outs, variances, temporal = reference(name, w, h, given)
        if given and w * h >= 256 and (kb != 0).any():
            spatial = (kb != 0) & ~temporal
            assert temporal.sum() * 8 >= (kb != 0).sum() and spatial.sum() * 8 >= (kb != 0).sum(), "both arms occur"
            assert (variances[0][temporal] == 0).any() and (variances[0][temporal] > 0).any()
        if not given:
            assert not temporal.any()
        for passes in PASSES:
            got = pkg.context.denoise_var_host(w, h, ids, img, mom, passes=passes, **VAR)
            same_bits(got, outs[passes - 1], (name, size, passes, given))
            assert np.array_equal(u32(got)[..., 3], u32(img)[..., 3]), ".w is the input's"
            assert np.array_equal(u32(got)[kb == 0], u32(img)[kb == 0]), "invalid keys pass through"


def test_the_variance_does_something(pkg):
    """The restatement's variance is neither zero nor constant, and the result is not the plane-key
    filter's with any one sigma_l: the per-pixel tolerance is what the bits depend on."""
    w, h = 67, 35
    outs, variances, _ = reference("stripes3", w, h, True)
    assert len(np.unique(variances[0])) > 100 and len(np.unique(variances[5])) > 100
    assert (variances[5] < variances[0]).sum() * 2 > w * h, "filtering lowers the variance"
    ids, img, mom = inputs("stripes3", w, h, True)
    plain = pkg.context.denoise_host(w, h, ids, img, 5, 0.0)
    assert not np.array_equal(u32(plain), u32(outs[4]))


def test_rgb8_is_the_tonemap_of_out(pkg):
    w, h = 67, 35
    ids, img, mom = inputs("field_material", w, h, True)
    out, rgb = pkg.context.denoise_var_host(w, h, ids, img, mom, passes=2, rgb=True, **VAR)
    import epilogue_ref
    want = np.array([epilogue_ref.tonemap_ref(px[:3].astype(np.float64)) for px in out.reshape(-1, 4)], np.uint32)
    assert np.array_equal(rgb.reshape(-1), want) and len(np.unique(rgb)) > 100


# -------------------------------------------------------------- 2. the moments' reprojection
def moments_for(c, seed):
    """A moments image for a reprojection case: both in [2^-6, 2^6]."""
    rng = np.random.default_rng([91, seed, c["w"], c["h"]])
    return np.exp2(rng.uniform(-6.0, 6.0, (c["h"], c["w"], 2))).astype(F)


@pytest.mark.parametrize("size", ((67, 35), (33, 17), (1, 1)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", ("translation", "yaw", "dolly"))
def test_reproject_moments_host(pkg, pair, size):
    w, h = size
    c = tri.case(pair, w, h)
    mom_in = moments_for(c, 0)
    cam, prev = tri.cameras(pkg, c)
    got, mom, rgb = pkg.context.reproject_moments_host(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], mom_in,
                                                       cam, prev, rgb=True)
    plain, plain_rgb = tri.host(pkg, c, rgb=True)
    assert np.array_equal(u32(got), u32(plain)) and np.array_equal(rgb, plain_rgb), "hist_out and rgb8 are vpx_reproject_ids'"
    want_hist, want_mom, arm = reproject_moments_ref.run(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], mom_in,
                                                         c["cam"], c["prev"])
    same_bits(got, want_hist, (pair, size))
    same_bits(mom, want_mom, (pair, size, "moments"))
    if size == (67, 35):
        assert (arm == reproject_ids_ref.HISTORY).sum() >= 200 and (arm != reproject_ids_ref.HISTORY).sum() >= 200
    # no previous frame: the sample's own moments
    got0, mom0 = pkg.context.reproject_moments_host(w, h, c["ids_cur"], None, c["cur"], None, None, cam, prev)
    _, want0, _ = reproject_moments_ref.run(w, h, c["ids_cur"], None, c["cur"], None, None, c["cam"], c["prev"])
    same_bits(mom0, want0, "no previous frame")
    assert np.array_equal(u32(got0), u32(tri.host(pkg, c, ids_prev=None, hist_in=None)))


def test_reproject_moments_host_moving_volume(pkg):
    w, h = 33, 17
    c = tri.moving_case(w, h)
    mom_in = moments_for(c, 1)
    cam, prev = tri.cameras(pkg, c)
    cv, pv = tri.moving_volumes(c, "moved")
    got, mom = pkg.context.reproject_moments_host(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], mom_in, cam,
                                                  prev, cur_volumes=cv, prev_volumes=pv)
    assert np.array_equal(u32(got), u32(tri.host(pkg, c, cur_volumes=cv, prev_volumes=pv)))
    want_hist, want_mom, arm = reproject_moments_ref.run(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], mom_in,
                                                         c["cam"], c["prev"], 32, (1, 0), c["cur_ref"], c["prev_ref"])
    same_bits(got, want_hist, "moving volume")
    same_bits(mom, want_mom, "moving volume, moments")
    box = (c["ids_cur"][..., 1] & 0xFFFF) == 3
    assert (arm[box] == reproject_ids_ref.HISTORY).sum() >= 10, "the moved box finds its history"
    static = pkg.context.reproject_moments_host(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], mom_in, cam, prev)[1]
    assert not np.array_equal(u32(mom)[box], u32(static)[box])


def test_moments_of_a_standing_camera_are_the_running_means(pkg):
    """Eight frames from a standing camera: where the history holds, m1 is the mean luminance of the
    frames so far and m2 - m1^2 their variance, to a few ulp of the largest term."""
    w, h = 16, 16
    c = tri.case("identical", w, h)
    cam, prev = tri.cameras(pkg, c)
    rng = np.random.default_rng(3)
    hist = mom = None
    lums = []
    for f in range(8):
        cur = np.concatenate([rng.uniform(0.25, 1.0, (h, w, 3)).astype(F), np.zeros((h, w, 1), F)], axis=2)
        lums.append(denoise_ref.lum(cur).astype(np.float64))
        hist, mom = pkg.context.reproject_moments_host(w, h, c["ids_cur"], None if hist is None else c["ids_prev"], cur,
                                                       hist, mom, cam, prev)
    full = hist[..., 3] == 8.0
    assert full.sum() >= 50
    lums = np.array(lums)
    assert np.allclose(mom[..., 0][full], lums.mean(axis=0)[full], rtol=1e-5, atol=0)
    assert np.allclose((mom[..., 1].astype(np.float64) - mom[..., 0].astype(np.float64) ** 2)[full], lums.var(axis=0)[full],
                       rtol=0, atol=1e-5)


# -------------------------------------------------------------------------- 3. properties
@pytest.mark.parametrize("name", POISON)
def test_nan_and_inf_stay_on_their_plane(pkg, name):
    for w, h in ((67, 35), (16, 16)):
        _, _, region = pattern(name, w, h)
        assert (region == 1).any() and (region == 0).any()
        for given in (False, True):
            ids, img, mom = inputs(name, w, h, given)
            for passes in (1, 5):
                clean = reference(name, w, h, given)[0][passes - 1]
                for value in (np.nan, np.inf):
                    got = pkg.context.denoise_var_host(w, h, ids, poisoned(img, region, value), mom, passes=passes, **VAR)
                    assert np.array_equal(u32(got)[region == 0], u32(clean)[region == 0]), (name, passes, given, value)
                    assert not np.isfinite(got[..., :3][region == 1]).any()
                    if given:  # the variance alone: the moments of region 1
                        bad = mom.copy()
                        bad[region == 1] = value
                        got = pkg.context.denoise_var_host(w, h, ids, img, bad, passes=passes, **VAR)
                        assert np.array_equal(u32(got)[region == 0], u32(clean)[region == 0]), (name, passes, "mom", value)


@pytest.mark.parametrize("c", (1.0, 0.75))
@pytest.mark.parametrize("name", ("one_plane", "stripes3", "field_face_sign"))
def test_constant_colour_with_zero_variance_comes_back(pkg, name, c):
    """Zero variance: tol = epsilon; a constant colour: dd = 0 and w = h, exact dyadics as in
    vpx_denoise_host's sigma_l == 0 case, so acc / wsum == c."""
    w, h = 67, 35
    ids, img, _ = pattern(name, w, h)
    flat = img.copy()
    flat[..., :3] = F(c)
    flat[..., 3] = F(8.0)
    m1 = denoise_ref.lum(flat)
    mom = np.stack([m1, np.multiply(m1, m1, dtype=F)], axis=2)
    for passes in PASSES:
        for m in (mom, None):
            got = pkg.context.denoise_var_host(w, h, ids, flat, m, passes=passes, **VAR)
            assert np.array_equal(u32(got), u32(flat)), (name, c, passes, m is None)


def step_image(w, h, lo, hi):
    """One plane, a vertical luminance step in the middle: grey lo on the left, grey hi on the right;
    history length 8; moments that say zero variance."""
    ids, _, _ = pattern("one_plane", w, h)
    img = np.empty((h, w, 4), F)
    img[..., :3] = F(lo)
    img[:, w // 2:, :3] = F(hi)
    img[..., 3] = F(8.0)
    m1 = denoise_ref.lum(img)
    mom = np.stack([m1, np.multiply(m1, m1, dtype=F)], axis=2)
    return ids, img, mom


def test_an_edge_the_history_vouches_for_survives(pkg):
    w, h = 33, 17
    lo, hi, eps = 0.25, 0.75, 2.0 ** -10
    ids, img, mom = step_image(w, h, lo, hi)
    lum_img = denoise_ref.lum(img)
    dl = float(lum_img[0, w - 1]) - float(lum_img[0, 0])
    dc = hi - lo
    bound = (55.0 / 9.0) * (eps / dl) ** 2 * dc
    got = pkg.context.denoise_var_host(w, h, ids, img, mom, passes=1, sigma_v=4.0, epsilon=eps, min_history=4)
    moved = np.abs(got[..., :3].astype(np.float64) - img[..., :3].astype(np.float64))
    print("edge: largest move", moved.max(), "bound", bound)
    assert moved.max() <= bound
    plain = pkg.context.denoise_host(w, h, ids, img, 1, 0.0)
    edge = np.zeros((h, w), bool)
    edge[:, w // 2 - 1:w // 2 + 1] = True
    moved_plain = np.abs(plain[..., :3].astype(np.float64) - img[..., :3].astype(np.float64))
    print("edge: the plane-key filter moves the edge pixels by at least", moved_plain[edge].min())
    assert (moved_plain[edge] > bound).all()


def test_a_large_uniform_variance_gives_the_plane_key_filter(pkg):
    w, h = 33, 17
    ids, _, _ = pattern("stripes3", w, h)
    rng = np.random.default_rng(11)
    img = np.empty((h, w, 4), F)
    img[..., :3] = rng.uniform(0.25, 1.0, (h, w, 3)).astype(F)
    img[..., 3] = F(8.0)
    m1 = denoise_ref.lum(img)
    big = F(2.0 ** 20)
    mom = np.stack([m1, np.add(np.multiply(m1, m1, dtype=F), big, dtype=F)], axis=2)
    vmin = 2.0 ** 20 - 1.0  # m2 - m1^2 with m1^2 <= 1, each rounded at 2^-3
    cmax, dmax, sigma_v = 1.0, 0.75 * 1.0001, 4.0
    delta = (dmax / (sigma_v * np.sqrt(vmin))) ** 2
    bound = cmax * delta / (1.0 - delta) + 2.0 ** -17 * cmax
    got = pkg.context.denoise_var_host(w, h, ids, img, mom, passes=1, sigma_v=sigma_v, epsilon=2.0 ** -10, min_history=4)
    plain = pkg.context.denoise_host(w, h, ids, img, 1, 0.0)
    diff = np.abs(got[..., :3].astype(np.float64) - plain[..., :3].astype(np.float64)).max()
    print("large variance: largest difference", diff, "bound", bound)
    assert diff <= bound
    assert np.abs(plain[..., :3] - img[..., :3]).max() > 0.05, "the filter did filter"


# ---------------------------------------------------------------------------- 4. refusals
def denoise_var_refusals(abi, call, ids, src, mom, out):
    """Every refusal of the two entries; call(width, height, ids, in, mom, out, params or None) -> status."""
    ok = abi.denoise_var(2, 4.0, 2.0 ** -10, 4)
    assert call(67, 35, ids, src, mom, out, ok) == abi.VPX_OK
    assert call(67, 35, ids, src, None, out, ok) == abi.VPX_OK
    for bad in ((67, 35, None, src, mom, out, ok), (67, 35, ids, None, mom, out, ok), (67, 35, ids, src, mom, None, ok),
                (67, 35, ids, src, mom, out, None),
                (0, 35, ids, src, mom, out, ok), (67, 0, ids, src, mom, out, ok), (32769, 1, ids, src, mom, out, ok),
                (1, 32769, ids, src, mom, out, ok), (32768, 32768, ids, src, mom, out, ok),
                (67, 35, ids, src, mom, src, ok), (67, 35, ids, src, mom, ids, ok), (67, 35, ids, src, mom, mom, ok)):
        assert call(*bad) == abi.VPX_E_INVALID, bad[:2]
    nan, inf = float("nan"), float("inf")

    def params(passes=2, sigma_v=4.0, epsilon=2.0 ** -10, min_history=4.0, flags=0, reserved=(0, 0, 0)):
        return abi.DenoiseVar(passes, sigma_v, epsilon, min_history, flags, (C.c_uint32 * 3)(*reserved))

    for d in (params(passes=0), params(passes=6), params(passes=0xFFFFFFFF),
              params(sigma_v=0.0), params(sigma_v=-1.0), params(sigma_v=nan), params(sigma_v=inf),
              params(epsilon=0.0), params(epsilon=-1.0), params(epsilon=nan), params(epsilon=inf),
              params(min_history=0.0), params(min_history=0.5), params(min_history=1.5), params(min_history=65537.0),
              params(min_history=-1.0), params(min_history=nan), params(min_history=inf),
              params(flags=1), params(reserved=(1, 0, 0)), params(reserved=(0, 1, 0)), params(reserved=(0, 0, 1))):
        assert call(67, 35, ids, src, mom, out, d) == abi.VPX_E_INVALID, (d.passes, d.sigma_v, d.epsilon, d.min_history, d.flags)
    for d in (params(passes=1), params(passes=5), params(min_history=1.0), params(min_history=65536.0)):
        assert call(67, 35, ids, src, mom, out, d) == abi.VPX_OK


def test_denoise_var_refusals(pkg):
    abi, lib = pkg.abi, pkg.load_library()
    ids, img, mom = (a.copy() for a in inputs("one_plane", 67, 35, True))
    out = np.zeros_like(img)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(w, h, i, s, m, o, d):
        return lib.vpx_denoise_var_host(w, h, p(i), p(s), p(m), p(o), None, C.byref(d) if d is not None else None)

    denoise_var_refusals(abi, call, ids, img, mom, out)
    out[:] = 0
    assert call(67, 35, ids, img, mom, out, abi.denoise_var(6)) == abi.VPX_E_INVALID and not out.any()


def reproject_moments_refusals(pkg, call, c, bufs):
    """vpx_reproject_ids' refusals through the moments entry (tri.refusals), then the moments' own.
    call(width, height, ids_cur, ids_prev, cur, hist_in, mom_in, hist_out, mom_out, r, cur_volumes, prev_volumes);
    bufs: ids_cur, ids_prev, cur, hist_in, mom_in, hist_out, mom_out."""
    abi = pkg.abi
    ids_cur, ids_prev, cur, hist_in, mom_in, hist_out, mom_out = bufs
    cam, prev = tri.cameras(pkg, c)
    vols = (abi.Volume * 2)(pkg.scene.volume(), pkg.scene.volume())

    def as_ids(w, h, ic, ip, cu, hi, ho, r, cv, pv):  # mom_in goes with hist_in
        return call(w, h, ic, ip, cu, hi, mom_in if hi is not None else None, ho, mom_out, r, cv, pv)

    tri.refusals(pkg, as_ids, ids_cur, ids_prev, cur, hist_in, hist_out, cam, prev, vols)
    r = pkg.context.reproject_desc(cam, prev)[0]
    good = dict(w=67, h=35, ic=ids_cur, ip=ids_prev, cu=cur, hi=hist_in, mi=mom_in, ho=hist_out, mo=mom_out)

    def with_(**kw):
        a = dict(good)
        a.update(kw)
        return (a["w"], a["h"], a["ic"], a["ip"], a["cu"], a["hi"], a["mi"], a["ho"], a["mo"], r, None, None)

    assert call(*with_()) == abi.VPX_OK
    for bad in (with_(mo=None), with_(mi=None), with_(ip=None, hi=None), with_(mo=ids_cur), with_(mo=ids_prev),
                with_(mo=cur), with_(mo=hist_in), with_(mo=mom_in), with_(mo=hist_out), with_(ho=mom_in)):
        assert call(*bad) == abi.VPX_E_INVALID
    assert call(*with_(ip=None, hi=None, mi=None)) == abi.VPX_OK
    assert call(*with_()) == abi.VPX_OK


def test_reproject_moments_refusals(pkg):
    lib = pkg.load_library()
    c = tri.case("translation", 67, 35)
    bufs = [c[k].copy() for k in ("ids_cur", "ids_prev", "cur", "hist_in")] + [moments_for(c, 0)]
    bufs += [np.zeros_like(bufs[2]), np.zeros((35, 67, 2), F)]
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(w, h, ic, ip, cu, hi, mi, ho, mo, r, cv, pv):
        return lib.vpx_reproject_moments_host(w, h, p(ic), p(ip), p(cu), p(hi), p(mi), p(ho), p(mo), None,
                                              C.byref(r) if r is not None else None, cv, pv)

    reproject_moments_refusals(pkg, call, c, bufs)
    same_bits(bufs[5], tri.reference("translation", 67, 35)[0], "the normal call after the refusals")
