"""The device's accumulate / tonemap / pack epilogues at special values and weight edges.

Every site that writes the blend fma(1-w, acc, px*w), the Reinhard-Jodie tonemap and the
(uint32_t)(int64_t) pack is driven with the rows of tests/epilogue_ref.py's generator — one row per
pixel of a 37x21 frame (3x2 tiles, partial right and bottom tiles) — and compared per pixel with
oracle_accumulate_tonemap, which tests/test_epilogue.py pins to the exact model on the same rows:
device -> oracle -> exact model on identical inputs.  The comparison is epilogue_ref.compare: NaN
masks equal, every other accumulator lane bit-equal, RGB8 equal wherever the int64 cast is defined.

Which kernel a case runs (launch_render / render_window_impl / render_tiles_impl in
csrc/vpx_kernels.hip), confirmed per case with vpx_debug_last_frame_kernel and vpx_profile_read's
stage launches:
  composite_tiles / composite_rgb8     vpx_composite_tiles / vpx_composite_rgb8
  k_frame0 lean (form 2)               depth 0, one volume, point light
  k_frame0 guaranteed (form 1)         the same with a spot light
  k_shadow_finish<true>                depth 2, one volume (serial frames keep the tile kernels)
  k_shadow_finish<false>               depth 0, two volumes (k_primary + k_instances_list first)
  k_resolve_finish                     an area light with area_samples = 3 (the shadow pool)
  k_tail + k_finish                    depth 8 (the deep levels in one launch, then the fold)
  finish_path<kFinishPackedAccum>      vpx_render_tiles_accum (inside k_frame0 / k_resolve_finish)
  blend_packed                         vpx_render_tiles_accum with 2 lanes
  blend_window                         vpx_render_window / vpx_render_tiles_accum_window, 0 and 2 lanes
k_finish_window needs a chain of at least 16384 tiles a frame with lanes and an area light; a 6-tile
frame cannot reach it (the 2048x1600 two-launch path has its own test).

The flush-boundary rows (results within an ulp of 2^-126, where "flush what is below 2^-126 after
rounding" and "round onto the subnormal grid, then flush" part) are compared under the parameter
id "boundary"; every other row under "rows".
"""
import dataclasses

import numpy as np
import pytest

import epilogue_ref as E
from test_epilogue import COUNT, MAX_LEFT_OUT, SEED, oracle_rows

pytestmark = pytest.mark.gpu

W, H = 37, 21
assert COUNT == W * H
NAN_BITS = 0x7FC00000
MAT_EMISSIVE = 15  # VPX_MAT_EMISSIVE
CAMERA = ((0.5, 0.5, -0.25), (0.5, 0.5, 0.5))  # the unit volume fills the view
PARTS = ["rows", "boundary"]
RANKS = [1, 2, 4]

_CACHE = {}


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def rows():
    return cached("rows", lambda: E.cases(SEED, COUNT))


def part_mask(part):
    m = np.zeros(COUNT, bool)
    m[E.N_TABLE:E.N_TABLE + E.N_BOUNDARY] = True
    return m if part == "boundary" else ~m


def dev(bits):
    """A device buffer with these bit patterns (int32 words: no float ever touches them)."""
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint32).view(np.int32).reshape(-1).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


def f32s(bits):
    """Bit patterns as Python floats (for vpx_frame_params.sky and the materials)."""
    return tuple(E.f32(int(b)) for b in bits)


def expect(got_acc, got_rgb, want_acc, want_rgb, mask, what):
    """epilogue_ref.compare on the rows of `mask`, with the first differing row spelled out."""
    idx = np.flatnonzero(mask)
    ga = np.asarray(got_acc).reshape(-1, 4)[idx]
    wa = np.asarray(want_acc).reshape(-1, 4)[idx]
    gr = None if got_rgb is None else np.asarray(got_rgb).reshape(-1)[idx]
    wr = None if got_rgb is None else np.asarray(want_rgb).reshape(-1)[idx]
    bad, left_out = E.compare(ga, gr, wa, wr)
    assert left_out <= MAX_LEFT_OUT, (what, left_out)
    if bad:
        i = bad[0]
        msg = (f"{what}: {len(bad)} of {len(idx)} rows differ; first at {idx[i]}: got {[hex(v) for v in ga[i]]} "
               f"want {[hex(v) for v in wa[i]]}")
        if gr is not None:
            msg += f" rgb got {int(gr[i]):#x} want {int(wr[i]):#x}"
        raise AssertionError(msg)


def params(abi, frame):
    """The frame parameters the composites read: size and frame_index."""
    p = abi.FrameParams()
    p.width, p.height, p.frame_index = W, H, frame
    return p


# ------------------------------------------------------------------ composite
def oracle_blend(orc, abi, sample_bits, acc_bits, frame):
    return oracle_rows(orc._lib(abi), sample_bits, acc_bits, frame)


def gathered_of(R, sample_bits):
    """R packed buffers back to back from the header's formula: the pixels' samples in their slots,
    NaN in every sample's .w and in every padding slot."""
    L, slots = E.slot_pixels(W, H, R)
    g = np.full((R * L, 4), NAN_BITS, np.uint32)
    ok = slots >= 0
    g[ok, :3] = sample_bits[slots[ok]]
    return g


def composite(pkg, R, frame):
    def run():
        s, a = rows()
        g = gathered_of(R, s)
        ctx = pkg.context.Context(0)
        p = params(pkg.abi, frame)
        out = []
        for with_rgb in (True, False):
            d_g, d_acc, d_rgb = dev(g), dev(a), dev(np.full(COUNT, 0xDEADBEEF, np.uint32))
            _torch().cuda.synchronize()
            ctx.composite_tiles(p, R, d_g.data_ptr(), d_acc.data_ptr(), d_rgb.data_ptr() if with_rgb else None)
            ctx.synchronize()
            out.append((host(d_acc).reshape(-1, 4), host(d_rgb)))
        ctx.close()
        return out
    return cached(("composite", R, frame), run)


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("frame", E.FRAMES)
@pytest.mark.parametrize("R", RANKS)
def test_composite_tiles(pkg, orc, abi, R, frame, part):
    """composite_tiles: every pixel its own generator row, unpacked from a `gathered` built from the
    header's formula; neither a sample's .w nor a padding slot (both NaN) reaches the image; with
    rgb8 NULL the accumulator is the same and nothing else is written."""
    _torch()
    s, a = rows()
    want = cached(("blend", frame), lambda: oracle_blend(orc, abi, s, a, frame))
    (acc, rgb), (acc0, rgb0) = composite(pkg, R, frame)
    expect(acc, rgb, want[0], want[1], part_mask(part), f"composite_tiles R={R} frame={frame}")
    expect(acc0, None, want[0], None, part_mask(part), f"composite_tiles R={R} frame={frame}, rgb8 NULL")
    assert np.all(rgb0 == 0xDEADBEEF)


@pytest.mark.parametrize("R", RANKS)
def test_composite_rgb8_is_the_formulas_permutation(pkg, abi, R):
    _torch()
    L, slots = E.slot_pixels(W, H, R)
    g = np.arange(R * L, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(0x9E3779B9)  # distinct words
    assert len(set(g.tolist())) == R * L
    want = np.zeros(COUNT, np.uint32)
    want[slots[slots >= 0]] = g[slots >= 0]
    ctx = pkg.context.Context(0)
    d_g, d_rgb = dev(g), dev(np.zeros(COUNT, np.uint32))
    _torch().cuda.synchronize()
    ctx.composite_rgb8(params(abi, 0), R, d_g.data_ptr(), d_rgb.data_ptr())
    ctx.synchronize()
    got = host(d_rgb)
    ctx.close()
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ vpx_render
# (sky triple as table bit patterns, frame_index): every FRAMES entry, every kind of table value.
B = E.fbits
SKIES = [
    ((B(0.5), 0x3F7FFFFF, B(3.0)), 0),
    ((0x7FC00000, B(1.0), B(-0.5)), 1),
    ((0x7F800000, E.NORM_MIN, B(1e19)), 2),
    ((E.SUB_MIN, 0x80000000, 0x7F7FFFFF), 7),
    ((B(-1.0), B(-3.5), B(255.0)), 2**24 - 1),
    ((B(1e-30), 0x3F800001, B(1e10)), 2**24),
    ((0x80000000 | E.NORM_MIN, E.SUB_MAX, 0x01000000), 2**32 - 1),
    ((B(0.5), 0x80000000 | E.SUB_MIN, B(1.0)), 2**24 - 1),
]
# albedo[15] (bit patterns), emissive, sky, frame; boundary: the product itself sits on the flush boundary
SLABS = [
    dict(albedo=(B(0.5), 0x3F7FFFFF, B(3.0)), emissive=2.0, sky=SKIES[0][0], frame=2, boundary=False),
    # 2^-100 * 2^-30: a subnormal product, read as zero
    dict(albedo=(B(2.0**-100), B(1.0), B(2.0**-96)), emissive=2.0**-30, sky=SKIES[5][0], frame=1, boundary=False),
    # FLT_MAX * 1e30, 1e19 * 1e30: the product overflows
    dict(albedo=(0x7F7FFFFF, B(1e19), B(-1.0)), emissive=1e30, sky=SKIES[2][0], frame=7, boundary=False),
    # 2^-126 * (1 - 2^-24) = 2^-126 - 2^-150: zero when flushed after rounding, 2^-126 on the subnormal grid
    dict(albedo=(E.NORM_MIN, B(2.0**-100), 0x01000000), emissive=1.0 - 2.0**-24, sky=SKIES[3][0], frame=0,
         boundary=True),
    # 0x81658f * 0xfd3c9a = 2^47 - 549882: the product is 2^-126 * (1 - 2^-27.9), below 2^-126 before
    # rounding and 2^-126 after it — kept by x86, zero under "flush what is tiny before rounding"
    dict(albedo=(0x0081658F, E.NORM_MIN, 0x01000000), emissive=E.f32(0x3F7D3C9A), sky=SKIES[3][0], frame=0,
         boundary=True),
]
KINDS = ["lean", "spot", "depth2", "two volumes", "area3", "depth8"]
# kind -> (vpx_debug_last_frame_kernel, stage launches that must be > 0, stage launches that must be 0)
FORMS = {
    "lean": (2, ("frame",), ("finish", "primary", "shadow")),
    "spot": (1, ("frame",), ("finish", "primary", "shadow")),
    "depth2": (0, ("primary", "shadow", "resolve", "bounce"), ("frame", "finish", "instances")),  # k_shadow_finish<true>
    "two volumes": (0, ("primary", "instances", "shadow"), ("frame", "finish")),                # k_shadow_finish<false>
    "area3": (0, ("primary", "shadow", "finish"), ("frame",)),                                     # k_resolve_finish
    "depth8": (0, ("primary", "bounce", "finish"), ("frame",)),                                    # k_tail, k_finish
}


def scene(pkg, kind, slab=None):
    """An 8^3 world of empty cells (every ray returns the frame's constant sky), or with a one-cell
    slab of material 15 across the left half of the view (those pixels return albedo[15] * emissive)."""
    sc = pkg.scene
    n = 8
    cells = np.full((n, n, n), 255, np.uint8)  # [z, y, x]
    mats = sc.default_materials()
    if slab is not None:
        cells[3, :, :4] = MAT_EMISSIVE
        for k in range(3):
            mats[MAT_EMISSIVE].albedo[k] = E.f32(slab["albedo"][k])
        mats[MAT_EMISSIVE].emissive = slab["emissive"]
    vols = [sc.volume()]
    if kind == "two volumes":
        vols.append(sc.volume(position=(1.5, 0.0, 0.0), scale=(0.5, 0.5, 0.5)))
    desc = sc._scene(f"epilogue-{kind}", [sc.GridSpec(n=n, dense=cells.reshape(-1).copy())], vols, mats,
                     [sc.point_light((0.5, 0.9, -0.5), (1.0, 1.0, 1.0))],
                     [sc.spot_light()] if kind == "spot" else [], [sc.area_light()] if kind == "area3" else [],
                     sc.dir_light(), CAMERA[0], CAMERA[1], W, H,
                     max_bounces={"depth2": 2, "depth8": 8}.get(kind, 0), area_samples=3)
    return desc


def with_sky(desc, sky_bits, flags=0):
    d = dataclasses.replace(desc, sky=f32s(sky_bits), flags=flags)
    d._cam_pos, d._cam_target = desc._cam_pos, desc._cam_target
    return d


def open_ctx(pkg, desc, lanes=0):
    ctx = pkg.context.Context(0)
    ctx.load_scene(desc)
    if np.all(desc.grids[0].dense == 255):
        ctx.grid_fill(0, 255)  # the empty world as Scene::ResetGrid leaves it
    ctx.set_pipeline(lanes)
    return ctx


def oracle_samples(pkg, orc, desc, frame):
    """The oracle's raw sample per pixel, as bit patterns [W*H, 3]."""
    o = orc.Oracle(pkg.abi, desc)
    s4, _ = o.render_pixels(desc.frame_params(frame), np.arange(COUNT, dtype=np.uint32), threads=2)
    return np.ascontiguousarray(s4).view(np.uint32)[:, :3].copy()


def render_cases(pkg, kind, slab_index=None):
    """Every SKIES case (or one SLABS case) of a configuration on one context: per case the device's
    accumulator and RGB8 from the generator's accumulator rows, the form and the stage launches."""
    def run():
        torch = _torch()
        _, a = rows()
        slab = None if slab_index is None else SLABS[slab_index]
        base = scene(pkg, kind, slab)
        ctx = open_ctx(pkg, base)
        ctx.profile_enable(4096)
        cases = SKIES if slab is None else [(slab["sky"], slab["frame"])]
        out = []
        for sky, frame in cases:
            desc = with_sky(base, sky)
            d_acc, d_rgb = dev(a), dev(np.zeros(COUNT, np.uint32))
            torch.cuda.synchronize()
            ctx.profile_read(reset=True)
            ctx.render(desc.frame_params(frame), d_acc.data_ptr(), d_rgb.data_ptr())
            form = ctx.last_frame_kernel()
            launches = {k: v[1] for k, v in ctx.profile_read(reset=True).items()}
            out.append((desc, frame, host(d_acc).reshape(-1, 4), host(d_rgb), form, launches))
        ctx.close()
        return out
    return cached(("render", kind, slab_index), run)


def check_form(kind, form, launches, what):
    want_form, ran, idle = FORMS[kind]
    assert form == want_form, (what, form)
    assert all(launches[s] > 0 for s in ran) and all(launches[s] == 0 for s in idle), (what, launches)


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("kind", KINDS)
def test_render_constant_sky(pkg, orc, abi, kind, part):
    """vpx_render over the empty world: one sky triple from the table and one FRAMES entry per case,
    the accumulator read-modify-written from the generator's rows.  Kernel per kind: the module
    docstring's table (FORMS states what vpx_profile_read must show for it)."""
    _torch()
    _, a = rows()
    for desc, frame, acc, rgb, form, launches in render_cases(pkg, kind):
        what = f"{kind} sky={[hex(int(np.float32(v).view(np.uint32))) for v in desc.sky]} frame={frame}"
        check_form(kind, form, launches, what)
        s = oracle_samples(pkg, orc, desc, frame)
        sky_bits = np.array([int(np.float32(v).view(np.uint32)) for v in desc.sky], np.uint32)
        assert np.all(s == sky_bits[None, :]), what  # every ray misses: the raw sample is the sky
        want = oracle_blend(orc, abi, s, a, frame)
        expect(acc, rgb, want[0], want[1], part_mask(part), what)


SLAB_PARTS = [(i, part) for i, c in enumerate(SLABS) for part in PARTS if part == "boundary" or not c["boundary"]]


@pytest.mark.parametrize("slab,part", SLAB_PARTS)
@pytest.mark.parametrize("kind", ["lean", "depth2", "area3"])
def test_render_emissive_slab(pkg, orc, abi, kind, slab, part):
    """The same with a slab of material 15 across half the view: those pixels return
    albedo[15] * emissive, a product set from the table — plain, subnormal (read as zero),
    overflowing, and one that sits on the flush boundary itself (compared under "boundary" with
    every pixel; the others split by row like every other case)."""
    _torch()
    _, a = rows()
    case = SLABS[slab]
    (desc, frame, acc, rgb, form, launches), = render_cases(pkg, kind, slab)
    what = f"{kind} slab {slab} frame={frame}"
    check_form(kind, form, launches, what)
    s = oracle_samples(pkg, orc, desc, frame)
    product = np.array([E.bits_of(E.mul(E.f32(case["albedo"][k]), float(np.float32(case["emissive"]))))
                        for k in range(3)], np.uint32)
    hit = np.all(s == product[None, :], axis=1)
    sky_bits = np.array([int(np.float32(v).view(np.uint32)) for v in desc.sky], np.uint32)
    miss = np.all(s == sky_bits[None, :], axis=1)
    assert 0 < hit.sum() < COUNT and np.all(hit | miss), (what, int(hit.sum()), int(miss.sum()))
    want = oracle_blend(orc, abi, s, a, frame)
    mask = np.ones(COUNT, bool) if case["boundary"] else part_mask(part)
    expect(acc, rgb, want[0], want[1], mask, what)


@pytest.mark.parametrize("kind", ["lean", "depth2", "area3", "depth8"])
def test_no_tonemap_writes_the_raw_sample(pkg, orc, abi, kind):
    """VPX_FLAG_NO_TONEMAP: accum is the oracle's raw sample (x, y, z, 0) whatever it held, under
    the same NaN rule; with a slab so that the samples are not all one value."""
    torch = _torch()
    _, a = rows()
    base = scene(pkg, kind, SLABS[2])
    ctx = open_ctx(pkg, base)
    for sky, frame in SKIES[:4]:
        desc = with_sky(base, sky, flags=abi.VPX_FLAG_NO_TONEMAP)
        d_acc = dev(a)
        torch.cuda.synchronize()
        ctx.render(desc.frame_params(frame), d_acc.data_ptr(), None)
        ctx.synchronize()
        want = np.zeros((COUNT, 4), np.uint32)
        want[:, :3] = oracle_samples(pkg, orc, desc, frame)
        expect(host(d_acc), None, want, None, np.ones(COUNT, bool), f"NO_TONEMAP {kind} frame={frame}")
    ctx.close()


# ------------------------------------------------------------------ packed accumulator
def packed_init(R):
    """A rank-major packed accumulator from the generator: a pixel's slot holds the pixel's row, a
    padding slot the row of its slot number."""
    _, a = rows()
    L, slots = E.slot_pixels(W, H, R)
    row = np.where(slots >= 0, slots, np.arange(R * L) % COUNT)
    return L, slots, a[row]


def packed_want(orc, abi, slots, init, samples_per_frame, first):
    """Valid slots: the oracle's blends in frame order; padding slots: accumulator 0 and RGB8 0."""
    ok = slots >= 0
    acc = init[ok]
    for b, s in enumerate(samples_per_frame):
        acc, rgb = oracle_blend(orc, abi, s[slots[ok]], acc, first + b)
    want_acc = np.zeros_like(init)
    want_rgb = np.zeros(len(slots), np.uint32)
    want_acc[ok], want_rgb[ok] = acc, rgb
    return want_acc, want_rgb


def slot_mask(slots, part):
    """A valid slot belongs to its pixel's part; the padding slots are compared under "rows"."""
    pm = part_mask(part)
    return np.where(slots >= 0, pm[np.maximum(slots, 0)], part == "rows")


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("lanes", [0, 2])
@pytest.mark.parametrize("kind", ["lean", "area3"])
def test_render_tiles_accum(pkg, orc, abi, kind, lanes, part):
    """vpx_render_tiles_accum, 3 ranks: finish_path<kFinishPackedAccum> (inside k_frame0 for "lean",
    k_resolve_finish for "area3"); with 2 lanes the frame renders packed samples on a lane and
    blend_packed folds them.  The packed accumulator starts from the generator, padding included."""
    torch = _torch()
    R = 3
    L, slots, init = packed_init(R)

    def run():
        base = scene(pkg, kind)
        ctx = open_ctx(pkg, base, lanes)
        out = []
        for sky, frame in SKIES[1::2]:
            desc = with_sky(base, sky)
            accs, rgbs = [], []
            for rank in range(R):
                d_acc = dev(init[rank * L:(rank + 1) * L])
                d_rgb = dev(np.full(L, 0xDEADBEEF, np.uint32))
                torch.cuda.synchronize()
                ctx.render_tiles_accum(desc.frame_params(frame), rank, R, d_acc.data_ptr(), d_rgb.data_ptr())
                ctx.synchronize()
                accs.append(host(d_acc).reshape(-1, 4))
                rgbs.append(host(d_rgb))
            out.append((desc, frame, np.concatenate(accs), np.concatenate(rgbs)))
        ctx.close()
        return out

    for desc, frame, acc, rgb in cached(("tiles_accum", kind, lanes), run):
        s = oracle_samples(pkg, orc, desc, frame)
        want = packed_want(orc, abi, slots, init, [s], frame)
        expect(acc, rgb, want[0], want[1], slot_mask(slots, part), f"tiles_accum {kind} lanes={lanes} frame={frame}")


# ------------------------------------------------------------------ windows
@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("lanes", [0, 2])
@pytest.mark.parametrize("first", [0, 2**24 - 2])
def test_render_window(pkg, orc, abi, first, lanes, part):
    """vpx_render_window, 3 frames from frame_index `first`: packed samples of the chain, then
    blend_window on the caller's stream (without lanes one chain of 3; with 2 lanes chains of 2 and
    1).  The result is three oracle blends in frame order; from 2^24 - 2 the weights are 1/(2^24 - 1),
    2^-24 and 2^-24 again ((float)2^24 + 1 rounds)."""
    torch = _torch()
    _, a = rows()
    sky = SKIES[0][0] if first == 0 else SKIES[6][0]

    def run():
        desc = with_sky(scene(pkg, "lean", SLABS[0]), sky)
        ctx = open_ctx(pkg, desc, lanes)
        d_acc, d_rgb = dev(a), dev(np.zeros(COUNT, np.uint32))
        torch.cuda.synchronize()
        ctx.render_window(desc.frame_params(first), 3, d_acc.data_ptr(), d_rgb.data_ptr())
        ctx.synchronize()
        out = (desc, host(d_acc).reshape(-1, 4), host(d_rgb))
        ctx.close()
        return out

    desc, acc, rgb = cached(("window", first, lanes), run)
    want_acc = a
    for b in range(3):
        want_acc, want_rgb = oracle_blend(orc, abi, oracle_samples(pkg, orc, desc, first + b), want_acc, first + b)
    expect(acc, rgb, want_acc, want_rgb, part_mask(part), f"render_window first={first} lanes={lanes}")


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("lanes", [0, 2])
@pytest.mark.parametrize("first", [0, 2**24 - 2])
def test_render_tiles_accum_window(pkg, orc, abi, first, lanes, part):
    """vpx_render_tiles_accum_window, 3 ranks, 3 frames: blend_window on a rank's packed accumulator
    (padding slots come back 0 / 0)."""
    torch = _torch()
    R = 3
    L, slots, init = packed_init(R)
    sky = SKIES[0][0] if first == 0 else SKIES[6][0]

    def run():
        desc = with_sky(scene(pkg, "lean", SLABS[0]), sky)
        ctx = open_ctx(pkg, desc, lanes)
        accs, rgbs = [], []
        for rank in range(R):
            d_acc = dev(init[rank * L:(rank + 1) * L])
            d_rgb = dev(np.full(L, 0xDEADBEEF, np.uint32))
            torch.cuda.synchronize()
            ctx.render_tiles_accum_window(desc.frame_params(first), 3, rank, R, d_acc.data_ptr(), d_rgb.data_ptr())
            ctx.synchronize()
            accs.append(host(d_acc).reshape(-1, 4))
            rgbs.append(host(d_rgb))
        ctx.close()
        return desc, np.concatenate(accs), np.concatenate(rgbs)

    desc, acc, rgb = cached(("tiles_window", first, lanes), run)
    samples = [oracle_samples(pkg, orc, desc, first + b) for b in range(3)]
    want = packed_want(orc, abi, slots, init, samples, first)
    expect(acc, rgb, want[0], want[1], slot_mask(slots, part), f"tiles_accum_window first={first} lanes={lanes}")
