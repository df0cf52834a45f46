"""The depth-0 frame kernel's work counters (csrc/vpx_wavefront.hpp: WgCounters), on the GPU.

k_frame0's waves add their sums (primary rays, FindNearest calls, shadow rays, DDA cells per
stage) to a record in the workgroup's LDS after the primary walks, the level-0 shade and the
shadow walks, and the workgroup flushes the record once, after the shadow walks' barrier, into its
stripe of the context's counters.  The counters must hold what they held when every wave flushed
three times: every case compares them with the oracle's, and the images bit for bit.

The 128^3 monu3 city from the cameras of test_frame_handoff_gpu.py:
  inside   every pixel walks, 64x48 and 70x50 (a ragged last tile: lanes without a pixel);
  partial  tiles with 0, a few and 256 walkers (waves that count primary rays and nothing else
           beside waves that count everything);
  away     no walker in any tile: only primary rays and the FindNearest calls are counted.
The per-stage cells (vpx_profile_read) are pinned through the lights: without lights the frame
walks its primary rays only, so that frame's cells are the PRIMARY stage's of the lit frame.
test_counts_and_images_match_oracle repeats test_frame_handoff_gpu.py::test_view_frames on the four
views they share (it passes before this change too); what is specific to the record are the
stage cells, the accumulation / reset / stats case and inside / away / inside without a reset.
"""
import numpy as np
import pytest

from cases import bits
from test_axis_boxes import _torch, check
from test_frame_handoff_gpu import ARITH, FRAMES, render_rank0, view, want_of
from test_frame_views_gpu import COUNTS, open_ctx, render_frames, replace, set_lights

pytestmark = pytest.mark.gpu

NAMES = ["inside", "inside ragged", "partial", "away"]


def counts_of(st):
    return tuple(int(getattr(st, k)) for k in COUNTS)


def times(counts, n):
    return tuple(n * c for c in counts)


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("how", ["serial", "lanes", "rank"])
@pytest.mark.parametrize("name", NAMES)
def test_counts_and_images_match_oracle(pkg, orc, name, how, arith):
    desc = view(pkg, name)
    want = want_of(pkg, orc, (name, arith), [desc] * FRAMES, x86=arith == "x86")
    primary, shadow, nearest, cells = want[2]
    assert primary > 0
    if name == "away":
        assert shadow == 0 and cells == 0, want[2]
    else:
        assert shadow > 0 and cells > 0, want[2]
    if how == "rank":
        shard, counts, forms = render_rank0(pkg, desc, arith)
        assert forms == [2] * (2 * FRAMES)
        ids = pkg.dist.rank_pixel_ids(desc.width, desc.height, 0, 2)
        ok = ids >= 0
        assert ok.sum() > 0
        assert np.array_equal(shard[0][ok], want[0][ids[ok]]), f"packed accumulator ({name}, {arith})"
        assert np.array_equal(shard[1][ok], want[1][ids[ok]]), f"packed RGB8 ({name}, {arith})"
        assert counts == want[2], (name, arith, counts, want[2])
        return
    got, forms = render_frames(pkg, [desc] * FRAMES, arith, 3 if how == "lanes" else 0)
    assert forms == [2] * FRAMES
    check(got, want, f"{name}, {arith}, {how}")


def one_frame(pkg, ctx, s, desc, acc, rgb):
    """One frame from zeroed counters: (counts, {stage: cells}, the kernel's form)."""
    torch = _torch()
    ctx.counters(reset=True)
    ctx.profile_read(reset=True)
    with torch.cuda.stream(s):
        ctx.render(desc.frame_params(0), acc.data_ptr(), rgb.data_ptr())
    form = ctx.last_frame_kernel()
    counts = counts_of(ctx.counters())
    stage = {k: int(v[2]) for k, v in ctx.profile_read(reset=True).items()}
    return counts, stage, form


def frame_buffers(desc):
    torch = _torch()
    acc = torch.zeros(desc.width * desc.height * 4, dtype=torch.float32, device="cuda")
    rgb = torch.zeros(desc.width * desc.height, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return acc, rgb


@pytest.mark.parametrize("name", ["inside", "partial"])
def test_stage_cells_through_the_lights(pkg, orc, name):
    """Lit, without lights, lit again on one context: the stages' cells add up to dda_cells; the
    frame without lights counts its primary walks only, and the lit frame's PRIMARY stage holds
    that same number; nothing is counted for the city's shade."""
    lit = view(pkg, name)
    dark = replace(lit, points=[], dir_light=pkg.scene.dir_light())
    want_lit = want_of(pkg, orc, (name, "exact", "one frame"), [lit])[2]
    want_dark = want_of(pkg, orc, (name, "exact", "one frame, no lights"), [dark])[2]
    assert want_dark[1] == 0 and 0 < want_dark[3] < want_lit[3], (want_dark, want_lit)
    ctx, s = open_ctx(pkg, lit)
    acc, rgb = frame_buffers(lit)
    for step, desc in enumerate([lit, dark, lit]):
        set_lights(pkg, ctx, desc)
        counts, stage, form = one_frame(pkg, ctx, s, desc, acc, rgb)
        print(name, step, "counts", counts, "stage cells", stage, "form", form)
        assert sum(stage.values()) == counts[3], (step, stage, counts)
        assert stage["shade"] == 0, (step, stage)
        assert stage["primary"] == want_dark[3], (step, stage, want_dark)
        if desc is lit:
            assert form == 2
            assert counts == want_lit, (step, counts, want_lit)
            assert stage["shadow"] == want_lit[3] - want_dark[3], (step, stage)
        else:
            assert counts == want_dark, (step, counts, want_dark)
            assert stage["shadow"] == 0, (step, stage)
    ctx.close()


def test_stage_cells_roomglass(pkg, orc):
    """A 64x48 depth-0 frame of the roomGlass city: the stages' cells add up to the oracle's
    dda_cells.  (On one MI355X: primary 247636 + shade 0 + shadow 88047 = 335683.)

    This does not cover a non-zero SHADE count, and no frame of this kernel can: the level-0
    shade starts outside every volume (shade_path's ray.inside = false), so the glass's exit march
    never runs at depth 0 and k_frame0's SHADE stage is always 0.  The SHADE add, and wg_flush's
    way from the record's word 4 to counter word 9, are therefore not exercised by any test."""
    _torch()
    desc = pkg.scene.city_scene("roomGlass", 128, 64, 48, 0)
    want = want_of(pkg, orc, ("roomGlass", "exact", "one frame"), [desc])
    ctx, s = open_ctx(pkg, desc)
    acc, rgb = frame_buffers(desc)
    counts, stage, form = one_frame(pkg, ctx, s, desc, acc, rgb)
    ctx.synchronize()
    print("roomGlass counts", counts, "stage cells", stage, "form", form)
    assert form == 2
    assert counts == want[2], (counts, want[2])
    assert sum(stage.values()) == want[2][3], (stage, want[2])
    assert stage["primary"] > 0 and stage["shadow"] > 0, stage
    got = (bits(acc.cpu().numpy().reshape(-1, 4)), rgb.cpu().numpy().view(np.uint32), counts)
    check(got, want, "roomGlass")
    ctx.close()


@pytest.mark.parametrize("how", ["serial", "lanes"])
@pytest.mark.parametrize("name", ["inside ragged", "partial"])
def test_accumulation_reset_and_stats(pkg, orc, name, how):
    """Three identical frames count three times one frame; a reset reads them and leaves zero;
    vpx_render's stats are the one frame's delta on top of what the counters already hold."""
    torch = _torch()
    desc = view(pkg, name)
    one = want_of(pkg, orc, (name, "exact", "one frame"), [desc])[2]
    ctx, s = open_ctx(pkg, desc, "exact", 3 if how == "lanes" else 0)
    acc, rgb = frame_buffers(desc)
    ctx.counters(reset=True)
    with torch.cuda.stream(s):
        for _ in range(3):
            ctx.render(desc.frame_params(0), acc.data_ptr(), rgb.data_ptr())
            assert ctx.last_frame_kernel() == 2
    assert counts_of(ctx.counters()) == times(one, 3)
    assert counts_of(ctx.counters(reset=True)) == times(one, 3)
    assert counts_of(ctx.counters()) == (0, 0, 0, 0)
    with torch.cuda.stream(s):
        ctx.render(desc.frame_params(0), acc.data_ptr(), rgb.data_ptr())
        st = ctx.render(desc.frame_params(0), acc.data_ptr(), rgb.data_ptr(), stats=True)
    assert counts_of(st) == one, (counts_of(st), one)
    assert counts_of(ctx.counters()) == times(one, 2)
    ctx.close()


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("how", ["serial", "lanes"])
def test_inside_away_inside_counts(pkg, orc, how, arith):
    """One context, the camera moving before every frame, the counters never reset: a record
    word left over from a frame that counted cells and shadow rays would be flushed again by the
    frame that counts none."""
    torch = _torch()
    inside, away = view(pkg, "inside"), view(pkg, "away")
    w_in = want_of(pkg, orc, ("inside", arith, "one frame"), [inside], x86=arith == "x86")[2]
    w_aw = want_of(pkg, orc, ("away", arith, "one frame"), [away], x86=arith == "x86")[2]
    assert w_aw[1] == 0 and w_aw[3] == 0 and w_in[1] > 0 and w_in[3] > 0
    ctx, s = open_ctx(pkg, inside, arith, 3 if how == "lanes" else 0)
    acc, rgb = frame_buffers(inside)
    ctx.counters(reset=True)
    total = (0, 0, 0, 0)
    for d, want in ((inside, w_in), (away, w_aw), (inside, w_in)):
        ctx.set_camera(d.camera)
        with torch.cuda.stream(s):
            st = ctx.render(d.frame_params(0), acc.data_ptr(), rgb.data_ptr(), stats=True)
        assert ctx.last_frame_kernel() == 2
        assert counts_of(st) == want, (counts_of(st), want)
        total = tuple(a + b for a, b in zip(total, want))
        assert counts_of(ctx.counters()) == total
    ctx.close()
