"""The plane-keyed reprojection on the host (vpx_reproject_ids_host) against its numpy restatement
(tests/reproject_ids_ref.py), bit for bit, on synthetic ID buffers; then the pass's properties and
the refusals.  No GPU.

The synthetic world is a floor, a wall that ends below the top of the view (above it: sky) and a
box, all axis-aligned in their volume's object space.  Per pixel the ray of the camera restatement
(test_kat_reproject.Camera) is intersected with them in float64; t, the volume, the material, the
entry face and the plane's cell coordinate are packed as k_ids packs them.  One patch of pixels is
overwritten with a shape win (v = 1) and one with a first-cell hit (face 0).  The pass itself
never sees the world: t is just an input, and the hit point is what the pass computes from it.

The cases, the cameras and the cached references are shared with tests/test_reproject_ids_gpu.py.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import reproject_ids_ref as ref
from test_kat_reproject import Camera

pytestmark = [pytest.mark.filterwarnings("ignore:invalid value:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning")]

F = np.float32
SIZES = ((67, 35), (33, 17), (16, 16), (1, 1))
POS, TARGET = (0.0, 1.2, -1.5), (0.2, 0.8, 3.0)
# name -> ((previous pos, target), (current pos, target))
PAIRS = {
    "identical": ((POS, TARGET), (POS, TARGET)),
    "translation": ((POS, TARGET), ((0.07, 1.23, -1.45), (0.27, 0.83, 3.05))),
    "yaw": ((POS, TARGET), (POS, (0.9, 0.8, 3.0))),
    "dolly": ((POS, TARGET), ((0.0, 1.3, -2.7), (0.2, 0.8, 3.0))),  # backwards: the rim was not in the previous view
    "behind": (((0.0, 1.2, -1.5), (-0.2, 1.6, -6.0)), (POS, TARGET)),  # the previous camera looked the other way
}
MAT_FLOOR, MAT_WALL, MAT_BOX = 3, 4, 5
BOX_AT = (0.3, 0.0, 3.0)  # the box's object-space origin in the world


def translation(t):
    m = np.eye(4)
    m[:3, 3] = t
    return m


def box_surfaces(vol):
    """The box in its object space: [-0.6, 0.6] x [0, 1] x [-0.6, 0.6], no bottom."""
    s = [dict(vol=vol, axis=1, plane=1.0, lo=(-0.6, -0.6), hi=(0.6, 0.6), mat=MAT_BOX, coord=40)]
    for plane, coord in ((-0.6, 30), (0.6, 39)):
        s.append(dict(vol=vol, axis=0, plane=plane, lo=(0.0, -0.6), hi=(1.0, 0.6), mat=MAT_BOX, coord=coord))
        s.append(dict(vol=vol, axis=2, plane=plane, lo=(-0.6, 0.0), hi=(0.6, 1.0), mat=MAT_BOX, coord=coord + 100))
    return s


WORLD = [dict(vol=0, axis=1, plane=0.0, lo=(-50.0, -50.0), hi=(50.0, 50.0), mat=MAT_FLOOR, coord=1),
         dict(vol=0, axis=2, plane=6.0, lo=(-50.0, 0.0), hi=(50.0, 2.5), mat=MAT_WALL, coord=12)]


def synth_ids(w, h, pos, target, box_vol=0, box_matrix=None, patches=True):
    """The ID buffer [H, W, 4] of the synthetic world seen from (pos, target).  box_vol / box_matrix:
    the volume that holds the box and its object -> world matrix (float64 4x4)."""
    cam = Camera(pos, target, w, h)
    mats = {0: np.eye(4), box_vol: np.eye(4) @ (translation(BOX_AT) if box_matrix is None else box_matrix)}
    if box_vol == 0:  # one volume holds everything: the box's object space is the world's, shifted
        surfaces = WORLD + [dict(s, shift=np.array(BOX_AT)) for s in box_surfaces(0)]
        mats[0] = np.eye(4)
    else:
        surfaces = WORLD + box_surfaces(box_vol)
    inv = {k: np.linalg.inv(m) for k, m in mats.items()}
    tl, tr, bl, o = (np.asarray(a, np.float64) for a in (cam.top_left, cam.top_right, cam.bottom_left, cam.pos))
    ids = np.zeros((h, w, 4), np.uint32)
    for y in range(h):
        for x in range(w):
            d = tl + (tr - tl) * (x / w) + (bl - tl) * (y / h) - o
            d /= np.linalg.norm(d)
            best = None
            for s in surfaces:
                shift = s.get("shift", np.zeros(3))
                oo = inv[s["vol"]][:3, :3] @ o + inv[s["vol"]][:3, 3] - shift
                dd = inv[s["vol"]][:3, :3] @ d
                a = s["axis"]
                if abs(dd[a]) < 1e-9:
                    continue
                t = (s["plane"] - oo[a]) / dd[a]
                if t <= 1e-3 or (best is not None and t >= best[0]):
                    continue
                p = oo + t * dd
                others = [k for k in range(3) if k != a]
                if all(s["lo"][i] <= p[k] <= s["hi"][i] for i, k in enumerate(others)):
                    best = (t, s, p, dd[a] < 0)
            if best is None:  # sky: a miss
                ids[y, x] = (F(1e34).view(np.uint32), 255 << 16, 0, 0)
                continue
            t, s, p, neg = best
            face = 1 + 2 * s["axis"] + int(neg)
            cell = [int(np.clip(math.floor(c * 8) + 2048, 0, 4095)) for c in p]
            cell[s["axis"]] = s["coord"]
            ids[y, x] = (F(t).view(np.uint32), (s["vol"] + 2) | s["mat"] << 16 | face << 24, cell[0] | cell[1] << 16, cell[2])
    if patches:
        ys, xs = np.mgrid[0:h, 0:w]
        shape_win = (xs * 10 >= w) & (xs * 10 < 2 * w) & (ys * 10 >= 6 * h) & (ys * 10 < 8 * h)
        first_cell = (xs * 10 >= 7 * w) & (xs * 10 < 8 * w) & (ys * 10 >= 7 * h) & (ys * 10 < 9 * h)
        ids[..., 1][shape_win] = 1 | 7 << 16                       # v = 1: a sphere or a triangle won
        ids[..., 1][first_cell] = 2 | MAT_FLOOR << 16              # face 0: hit in the ray's first cell
    return ids


def colours(rng, h, w):
    """2^u, u uniform in [-6, 6]."""
    c = np.exp2(rng.uniform(-6.0, 6.0, (h, w, 3))).astype(F)
    return np.clip(c, F(2.0 ** -6), F(2.0 ** 6))


LENGTHS = np.array([0.0, 0.5, np.nan, 1.0, 1.0, 2.0, 3.0, 7.0, 31.0, 32.0, 100.0, 65536.0], F)


@functools.lru_cache(maxsize=None)
def case(pair, w, h):
    """One synthetic call: the two ID buffers, this frame's samples (.w any bits) and a history whose
    lengths are drawn from LENGTHS: a quarter of them (0, 0.5, NaN) make their tap unusable."""
    (ppos, ptgt), (cpos, ctgt) = PAIRS[pair]
    rng = np.random.default_rng([sorted(PAIRS).index(pair), w, h])
    cur = np.empty((h, w, 4), F)
    cur[..., :3] = colours(rng, h, w)
    cur[..., 3] = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32).view(F)
    hist = np.empty((h, w, 4), F)
    hist[..., :3] = colours(rng, h, w)
    hist[..., 3] = LENGTHS[rng.integers(0, len(LENGTHS), (h, w))]
    c = dict(w=w, h=h, ids_cur=synth_ids(w, h, cpos, ctgt), ids_prev=synth_ids(w, h, ppos, ptgt), cur=cur, hist_in=hist,
             cam=Camera(cpos, ctgt, w, h), prev=Camera(ppos, ptgt, w, h), cam_args=(cpos, ctgt), prev_args=(ppos, ptgt))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(pair, w, h, max_history=32, nohist=(1, 0)):
    c = case(pair, w, h)
    res = ref.run(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], c["cam"], c["prev"], max_history, nohist)
    for a in res:
        a.setflags(write=False)
    return res


def cameras(pkg, c):
    """(vpx_camera of the current view, vpx_prev_camera of the previous one) of a case."""
    return (pkg.scene.look_at(*c["cam_args"], c["w"], c["h"]), pkg.scene.prev_camera(*c["prev_args"], c["w"], c["h"]))


def host(pkg, c, **kw):
    cam, prev = cameras(pkg, c)
    a = dict(ids_prev=c["ids_prev"], cur=c["cur"], hist_in=c["hist_in"])
    a.update({k: kw.pop(k) for k in list(kw) if k in a})
    return pkg.context.reproject_host(c["w"], c["h"], c["ids_cur"], a["ids_prev"], a["cur"], a["hist_in"], cam, prev, **kw)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what):
    """Bit equality of float images; NaN payloads apart (the project's known exception)."""
    g, w = u32(got), u32(want)
    gn, wn = np.isnan(np.asarray(got)), np.isnan(np.asarray(want))
    bad = (gn != wn) | (~wn & (g != w))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def ulp_distance(a, b):
    """Of positive finite float32 arrays."""
    return np.abs(u32(a).astype(np.int64) - u32(b).astype(np.int64))


# ------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", ("identical", "translation", "yaw", "dolly"))
def test_host_equals_restatement(pkg, pair, size):
    w, h = size
    c = case(pair, w, h)
    want, arm, mask = reference(pair, w, h)
    got, rgb = host(pkg, c, rgb=True)
    same_bits(got, want, (pair, size))
    none = arm != ref.HISTORY
    assert np.array_equal(u32(got)[none][:, :3], u32(c["cur"])[none][:, :3]) and (got[..., 3][none] == 1.0).all()
    import epilogue_ref
    flat = got.reshape(-1, 4)
    pick = range(0, len(flat), max(1, len(flat) // 200))
    assert [int(rgb.reshape(-1)[i]) for i in pick] == [int(epilogue_ref.tonemap_ref(flat[i, :3].astype(np.float64))) for i in pick]


def test_the_cases_cover_the_definition():
    """Asserted on the restatement alone, the translation pair at 67 x 35: at least half of the
    valid-key pixels take history, each of the 15 non-empty usable-tap masks occurs; and the arms
    the other pairs are there for."""
    w, h = 67, 35
    c = case("translation", w, h)
    _, arm, mask = reference("translation", w, h)
    valid = arm != ref.INVALID_KEY
    assert int(valid.sum()) * 2 >= w * h, "most of the frame is on voxels"
    assert int((arm == ref.HISTORY).sum()) * 2 >= int(valid.sum()), (int((arm == ref.HISTORY).sum()), int(valid.sum()))
    assert sorted(set(mask[arm == ref.HISTORY].tolist())) == list(range(1, 16))
    assert (arm == ref.INVALID_KEY).sum() >= 100 and (arm == ref.NO_TAP).any()
    y = c["ids_cur"][..., 1]
    assert ((y & 0xFFFF) == 0).any() and ((y & 0xFFFF) == 1).any() and (((y & 0xFFFF) == 2) & (y >> 24 == 0)).any()
    assert len({int(v) for v in y[arm == ref.HISTORY]}) >= 4, "floor, wall and two faces of the box at the least"
    _, arm_dolly, _ = reference("dolly", w, h)
    assert (arm_dolly == ref.OUTSIDE).sum() >= 50 and (arm_dolly == ref.HISTORY).sum() >= 200
    _, arm_yaw, _ = reference("yaw", w, h)
    assert (arm_yaw == ref.OUTSIDE).any() and (arm_yaw == ref.HISTORY).sum() >= 200


# -------------------------------------------------------------------------- 2. properties
def test_max_history_one_gives_cur_back(pkg):
    c = case("translation", 33, 17)
    got = host(pkg, c, max_history=1)
    assert np.array_equal(u32(got)[..., :3], u32(c["cur"])[..., :3]) and (got[..., 3] == 1.0).all()
    want, arm, _ = reference("translation", 33, 17, 1)
    same_bits(got, want, "max_history 1")
    assert (arm == ref.CAP_ONE).any() and not (arm == ref.HISTORY).any()


def test_cap_is_reached_and_held(pkg):
    """40 frames from a standing camera, max_history 32: the length of a pixel that keeps its
    history grows by one per frame up to 32 and stays."""
    w, h = 16, 16
    c = case("identical", w, h)
    rng = np.random.default_rng(5)
    hist, lengths = None, []
    for f in range(40):
        cur = np.concatenate([colours(rng, h, w), np.zeros((h, w, 1), F)], axis=2)
        prev_hist = hist
        hist = host(pkg, c, cur=cur, ids_prev=None if hist is None else c["ids_prev"], hist_in=hist, max_history=32)
        lengths.append(hist[..., 3].copy())
    lengths = np.array(lengths)
    assert (lengths[0] == 1.0).all()
    steady = (lengths[1:] > 1.0).all(axis=0)  # interior voxel pixels: all four taps on their plane every frame
    assert steady.sum() >= 50
    grow = np.minimum(np.arange(1, 41), 32).astype(F)
    assert (lengths[:, steady] <= grow[:, None]).all() and (lengths.max(axis=(1, 2)) == grow).all()
    assert (lengths[31:].max(axis=(1, 2)) == 32.0).all() and (lengths <= 32.0).all()
    want, _, _ = ref.run(w, h, c["ids_cur"], c["ids_prev"], cur, prev_hist, c["cam"], c["prev"], 32)
    same_bits(hist, want, "frame 40 of the chain")


def test_constant_colour_per_plane_comes_back(pkg):
    """A constant per plane in cur and hist_in: within 16 ulp per channel (the ten roundings of
    steps 5-6: up to four products and four sums, the division, the blend's three; nothing here is
    dyadic, so it is not exact)."""
    w, h = 67, 35
    c = case("translation", w, h)
    table = {}

    def paint(ids):
        import denoise_ref
        ka, kb = denoise_ref.keys(ids)
        img = np.ones((h, w, 4), F)
        for yy in range(h):
            for xx in range(w):
                k = (int(ka[yy, xx]), int(kb[yy, xx]))
                if k not in table:
                    table[k] = np.random.default_rng(len(table)).uniform(0.05, 5.0, 3).astype(F)
                img[yy, xx, :3] = table[k]
        return img

    cur, hist = paint(c["ids_cur"]), paint(c["ids_prev"])
    hist[..., 3] = c["hist_in"][..., 3]
    got = host(pkg, c, cur=cur, hist_in=hist)
    _, arm, _ = reference("translation", w, h)
    took = arm == ref.HISTORY
    assert took.sum() >= 500 and (got[..., 3][took] >= 2.0).all()
    assert int(ulp_distance(got[..., :3][took], cur[..., :3][took]).max()) <= 16
    assert np.array_equal(u32(got)[..., :3][~took], u32(cur)[..., :3][~took])


@functools.lru_cache(maxsize=None)
def poison_case(w, h, value):
    """The translation case with `value` in the history colour and length of every pixel that is not
    on the floor, and arbitrary bits in those pixels' previous ids where the key does not read."""
    c = dict(case("translation", w, h))
    floor_prev = (c["ids_prev"][..., 1] >> 16 & 255 == MAT_FLOOR) & (c["ids_prev"][..., 1] >> 24 > 0)
    hist = c["hist_in"].copy()
    hist[~floor_prev] = value
    ids_prev = c["ids_prev"].copy()
    ids_prev[..., 0][~floor_prev] = F(value).view(np.uint32)
    c["hist_in"], c["ids_prev"] = hist, ids_prev
    return c


@pytest.mark.parametrize("value", (np.nan, np.inf))
def test_poison_stays_off_the_floor(pkg, value):
    for w, h in ((67, 35), (33, 17)):
        c = poison_case(w, h, value)
        clean, arm, _ = reference("translation", w, h)
        got = host(pkg, c)
        floor = (c["ids_cur"][..., 1] >> 16 & 255 == MAT_FLOOR) & (c["ids_cur"][..., 1] >> 24 > 0)
        assert (arm[floor] == ref.HISTORY).sum() >= 100
        assert np.array_equal(u32(got)[floor], u32(clean)[floor]), value
        assert np.isfinite(got[floor]).all()


def test_short_and_nan_lengths_make_a_tap_unusable(pkg):
    w, h = 33, 17
    c = case("translation", w, h)
    _, arm, _ = reference("translation", w, h)
    for bad in (0.0, 0.5, np.nan):
        hist = c["hist_in"].copy()
        hist[..., 3] = bad
        got = host(pkg, c, hist_in=hist)
        assert np.array_equal(u32(got)[..., :3], u32(c["cur"])[..., :3]) and (got[..., 3] == 1.0).all(), bad
    hist = c["hist_in"].copy()
    hist[..., 3] = 1.0
    got = host(pkg, c, hist_in=hist)
    full = ref.run(w, h, c["ids_cur"], c["ids_prev"], c["cur"], hist, c["cam"], c["prev"])
    same_bits(got, full[0], "every length 1")
    assert (got[..., 3][full[1] == ref.HISTORY] == 2.0).all() and (full[1] == ref.HISTORY).sum() >= (arm == ref.HISTORY).sum()


def test_behind_the_previous_camera_takes_no_history(pkg):
    w, h = 33, 17
    c = case("behind", w, h)
    want, arm, _ = reference("behind", w, h)
    assert (arm == ref.OUTSIDE).sum() >= 200 and not (arm == ref.HISTORY).any()
    got = host(pkg, c)
    same_bits(got, want, "behind")
    assert np.array_equal(u32(got)[..., :3], u32(c["cur"])[..., :3]) and (got[..., 3] == 1.0).all()


@pytest.mark.parametrize("nohist", ((MAT_BOX, MAT_BOX), (MAT_WALL, MAT_BOX), (0, 255), (5, 14), (6, 5)))
def test_nohist_ranges(pkg, nohist):
    w, h = 33, 17
    c = case("translation", w, h)
    want, arm, _ = reference("translation", w, h, 32, nohist)
    got = host(pkg, c, nohist=nohist)
    same_bits(got, want, nohist)
    mat = c["ids_cur"][..., 1] >> 16 & 255
    inside = (mat >= nohist[0]) & (mat <= nohist[1]) & (arm != ref.INVALID_KEY)
    assert (arm[inside] == ref.NOHIST_MATERIAL).all() and (got[..., 3][inside] == 1.0).all()
    if nohist[0] <= nohist[1]:
        assert inside.any()
    else:
        same_bits(got, reference("translation", w, h)[0], "an empty range")
    if nohist != (0, 255):
        assert (arm == ref.HISTORY).any()


def test_without_a_previous_frame(pkg):
    w, h = 33, 17
    c = case("translation", w, h)
    got = host(pkg, c, ids_prev=None, hist_in=None)
    assert np.array_equal(u32(got)[..., :3], u32(c["cur"])[..., :3]) and (got[..., 3] == 1.0).all()
    want, arm, _ = ref.run(w, h, c["ids_cur"], None, c["cur"], None, c["cam"], c["prev"])
    same_bits(got, want, "no previous frame")
    assert (arm == ref.NO_PREVIOUS).any()


# ----------------------------------------------------------------------- 3. moving volumes
def volume_pair(pkg, position, yaw):
    """(abi.Volume, its float64 matrix, (matrix, inv_matrix) float32 for the restatement)."""
    v = pkg.scene.volume(position=position, rotation=(0.0, yaw, 0.0))
    m = np.array(list(v.matrix), F)
    return v, m.astype(np.float64).reshape(4, 4), (m, np.array(list(v.inv_matrix), F))


@functools.lru_cache(maxsize=None)
def moving_case(w, h):
    """The box is volume 1, translated and turned between the frames; floor and wall are volume 0;
    the camera moves as in the translation pair."""
    import __graft_entry__ as entry
    pkg = entry.load_package()
    (ppos, ptgt), (cpos, ctgt) = PAIRS["translation"]
    base = dict(case("translation", w, h))
    world = volume_pair(pkg, (0.0, 0.0, 0.0), 0.0)
    box_prev = volume_pair(pkg, BOX_AT, 0.0)
    box_cur = volume_pair(pkg, (BOX_AT[0] + 0.25, BOX_AT[1], BOX_AT[2] - 0.2), 0.2)
    base["ids_prev"] = synth_ids(w, h, ppos, ptgt, 1, box_prev[1])
    base["ids_cur"] = synth_ids(w, h, cpos, ctgt, 1, box_cur[1])
    base["cur_volumes"] = (world[0], box_cur[0])
    base["prev_volumes"] = (world[0], box_prev[0])
    base["cur_ref"] = (world[2], box_cur[2])
    base["prev_ref"] = (world[2], box_prev[2])
    return base


@functools.lru_cache(maxsize=None)
def moving_reference(w, h, mode):
    """mode: 'moved' (both volumes given), 'static' (n_volumes 0), 'short' (volume 0 only),
    'equal' (both given, the current matrices for both frames)."""
    c = moving_case(w, h)
    cv, pv = {"moved": (c["cur_ref"], c["prev_ref"]), "static": (None, None), "short": (c["cur_ref"][:1], c["prev_ref"][:1]),
              "equal": (c["cur_ref"], c["cur_ref"])}[mode]
    return ref.run(w, h, c["ids_cur"], c["ids_prev"], c["cur"], c["hist_in"], c["cam"], c["prev"], 32, (1, 0), cv, pv)


def moving_volumes(c, mode):
    return {"moved": (c["cur_volumes"], c["prev_volumes"]), "static": (None, None),
            "short": (c["cur_volumes"][:1], c["prev_volumes"][:1]), "equal": (c["cur_volumes"], c["cur_volumes"])}[mode]


@pytest.mark.parametrize("size", ((67, 35), (33, 17)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_moving_volumes(pkg, size):
    w, h = size
    c = moving_case(w, h)
    got = {}
    for mode in ("moved", "static", "short", "equal"):
        cv, pv = moving_volumes(c, mode)
        got[mode] = host(pkg, c, cur_volumes=cv, prev_volumes=pv)
        same_bits(got[mode], moving_reference(w, h, mode)[0], (mode, size))
    box = (c["ids_cur"][..., 1] & 0xFFFF) == 3
    keyed = moving_reference(w, h, "static")[1] != ref.INVALID_KEY
    assert (box & keyed).sum() >= (100 if size == (67, 35) else 20)
    arm_moved, arm_static = moving_reference(w, h, "moved")[1], moving_reference(w, h, "static")[1]
    # the moved surface finds its history; without the matrices it looks where the box no longer is
    assert (arm_moved[box & keyed] == ref.HISTORY).sum() * 2 >= (box & keyed).sum()
    assert (arm_moved[box & keyed] == ref.HISTORY).sum() > (arm_static[box & keyed] == ref.HISTORY).sum()
    assert not np.array_equal(u32(got["moved"])[box], u32(got["static"])[box])
    # the static volume's bits are the static-world call's
    assert np.array_equal(u32(got["moved"])[~box], u32(got["static"])[~box])
    # v >= n_volumes takes no history
    assert (moving_reference(w, h, "short")[1][box & keyed] == ref.VOLUME_RANGE).all()
    assert np.array_equal(u32(got["short"])[box][:, :3], u32(c["cur"])[box][:, :3]) and (got["short"][..., 3][box] == 1.0).all()
    assert np.array_equal(u32(got["short"])[~box], u32(got["static"])[~box])
    # equal matrices leave every bit of the static call
    assert np.array_equal(u32(got["equal"]), u32(got["static"]))


# ---------------------------------------------------------------------------- 4. refusals
def refusals(pkg, call, ids_cur, ids_prev, cur, hist_in, hist_out, cam, prev, volumes):
    """Every refusal of the two entries, then a normal call.
    call(width, height, ids_cur, ids_prev, cur, hist_in, hist_out, vpx_reproject or None, cur_volumes, prev_volumes)."""
    abi = pkg.abi
    desc = pkg.context.reproject_desc

    def r(**kw):
        d = desc(cam, prev, kw.pop("max_history", 32), kw.pop("nohist", (1, 0)))[0]
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    ok = r()
    good = (67, 35, ids_cur, ids_prev, cur, hist_in, hist_out, ok, None, None)
    assert call(*good) == abi.VPX_OK

    def with_(**kw):
        names = ("width", "height", "ids_cur", "ids_prev", "cur", "hist_in", "hist_out", "r", "cur_volumes", "prev_volumes")
        a = dict(zip(names, good))
        a.update(kw)
        return tuple(a[n] for n in names)

    for bad in (with_(ids_cur=None), with_(cur=None), with_(hist_out=None), with_(r=None),
                with_(ids_prev=None), with_(hist_in=None),
                with_(width=0), with_(height=0), with_(width=32769, height=1), with_(width=1, height=32769),
                with_(width=32768, height=32768),
                with_(hist_out=ids_cur), with_(hist_out=ids_prev), with_(hist_out=cur), with_(hist_out=hist_in)):
        assert call(*bad) == abi.VPX_E_INVALID, [type(b).__name__ for b in bad]
    for d in (r(max_history=0), r(max_history=0.5), r(max_history=1.5), r(max_history=65537), r(max_history=-1),
              r(max_history=float("nan")), r(max_history=float("inf")), r(nohist=(5, 256)), r(nohist=(0, 0xFFFFFFFF)),
              r(flags=1), r(reserved=1), r(n_volumes=65535), r(n_volumes=2)):
        assert call(*with_(r=d)) == abi.VPX_E_INVALID, (d.max_history, d.nohist_lo, d.nohist_hi, d.flags, d.n_volumes)
    two = r(n_volumes=2)
    assert call(*with_(r=two, cur_volumes=volumes)) == abi.VPX_E_INVALID
    assert call(*with_(r=two, prev_volumes=volumes)) == abi.VPX_E_INVALID
    # what is allowed: a range that is empty whatever its bounds, both history arguments absent, the
    # limits of max_history, volumes
    for d in (r(nohist=(300, 256)), r(max_history=1), r(max_history=65536)):
        assert call(*with_(r=d)) == abi.VPX_OK
    assert call(*with_(ids_prev=None, hist_in=None)) == abi.VPX_OK
    assert call(*with_(r=two, cur_volumes=volumes, prev_volumes=volumes)) == abi.VPX_OK
    assert call(*good) == abi.VPX_OK


def test_refusals(pkg):
    lib = pkg.load_library()
    c = case("translation", 67, 35)
    ids_cur, ids_prev, cur, hist_in = (c[k].copy() for k in ("ids_cur", "ids_prev", "cur", "hist_in"))
    out = np.zeros_like(cur)
    cam, prev = cameras(pkg, c)
    vols = (pkg.abi.Volume * 2)(pkg.scene.volume(), pkg.scene.volume())
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(w, h, ic, ip, cu, hi, ho, r, cv, pv):
        return lib.vpx_reproject_ids_host(w, h, p(ic), p(ip), p(cu), p(hi), p(ho), None, C.byref(r) if r is not None else None,
                                          cv, pv)

    refusals(pkg, call, ids_cur, ids_prev, cur, hist_in, out, cam, prev, vols)
    same_bits(out, reference("translation", 67, 35)[0], "the normal call after the refusals")
    out[:] = 0
    bad = pkg.context.reproject_desc(cam, prev, 0.5)[0]
    assert call(67, 35, ids_cur, ids_prev, cur, hist_in, out, bad, None, None) == pkg.abi.VPX_E_INVALID and not out.any()
