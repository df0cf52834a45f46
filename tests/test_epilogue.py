"""The frame epilogue (blend, tonemap, RGB8 pack) of the CPU restatement against the exact model.

oracle_accumulate_tonemap of BOTH oracle builds (liboracle.so, and liboracle_perf.so: the -O3
-march=x86-64-v3 build bench.py's CPU baseline times) must equal tests/epilogue_ref.py on every
generator row and every FRAMES entry: special values, the flush boundary, the weights at 2^24 and
2^32.  tests/test_epilogue_gpu.py runs the device against the oracle on the same rows, so the chain
is device -> oracle -> exact model on identical inputs.
"""
from fractions import Fraction

import numpy as np
import pytest

import epilogue_ref as E
import test_kat_reference as K

SEED, COUNT = 20241, 37 * 21  # the GPU test's rows: one per pixel of its 37x21 frame
MAX_LEFT_OUT = 0.02


@pytest.fixture(scope="module")
def rows():
    return E.cases(SEED, COUNT)


@pytest.fixture(scope="module")
def expected(rows):
    """The exact model's answer per FRAMES entry, computed once."""
    return {frame: E.reference(rows[0], rows[1], frame) for frame in E.FRAMES}


def oracle_rows(lib, sample_bits, acc_bits, frame):
    n = len(sample_bits)
    s4 = np.zeros((n, 4), np.uint32)
    s4[:, :3] = sample_bits
    acc = np.array(acc_bits, np.uint32)
    rgb = np.zeros(n, np.uint32)
    for i in range(n):
        lib.oracle_accumulate_tonemap(s4[i].ctypes.data, frame, acc[i].ctypes.data, rgb[i:].ctypes.data)
    return acc, rgb


def describe(i, frame, rows, got, want):
    return (f"row {i} frame {frame}: sample {[hex(v) for v in rows[0][i]]} acc {[hex(v) for v in rows[1][i]]} "
            f"got {[hex(v) for v in got[0][i]]} rgb {int(got[1][i]):#x} want {[hex(v) for v in want[0][i]]} "
            f"rgb {int(want[1][i]):#x}")


def test_generator_is_seeded_and_covers_the_table(rows):
    again = E.cases(SEED, COUNT)
    assert np.array_equal(rows[0], again[0]) and np.array_equal(rows[1], again[1])
    assert rows[0].shape == (COUNT, 3) and rows[1].shape == (COUNT, 4)
    table = set(E.TABLE_BITS)
    pairs = {(int(s), int(a)) for srow, arow in zip(rows[0][:E.N_TABLE], rows[1][:E.N_TABLE])
             for s, a in zip(srow, arow[:3])}
    assert pairs == {(s, a) for s in table for a in table}, "the table's full cross product"
    assert COUNT > E.N_TABLE + E.N_BOUNDARY + len(E.CAST_ROWS), "no random rows left"


@pytest.mark.parametrize("perf", [False, True], ids=["liboracle", "liboracle_perf"])
@pytest.mark.parametrize("frame", E.FRAMES)
def test_oracle_equals_exact_model(orc, abi, rows, expected, frame, perf):
    lib = orc._lib(abi, perf=perf)
    want = expected[frame]
    got = oracle_rows(lib, rows[0], rows[1], frame)
    bad, left_out = E.compare(got[0], got[1], want[0], want[1])
    assert left_out <= MAX_LEFT_OUT, left_out
    assert not bad, f"{len(bad)} rows differ; first: " + describe(bad[0], frame, rows, got, want)


def test_flush_rules_part_on_the_boundary_rows(rows, expected):
    """The boundary rows do separate "flush what is below 2^-126 after rounding with an unbounded
    exponent" from "round onto the subnormal grid, then flush": the model's own example, and a
    count over the rows (so the rows cannot lose that property unnoticed)."""
    m126 = float(np.float32(2.0**-126))
    assert E.fma(1.0 - 2.0**-24, m126, 0.0) == 0.0
    assert E.fma(1.0 - 2.0**-24, 2.0**-125, 0.0) == 2.0**-125 * (1.0 - 2.0**-24)
    assert E.mul(m126, 1.0 - 2.0**-24) == 0.0 and E.mul(-m126, 1.0 - 2.0**-24) == 0.0
    assert str(E.mul(-m126, 1.0 - 2.0**-24)) == "-0.0"
    lo, hi = E.N_TABLE, E.N_TABLE + E.N_BOUNDARY
    Q126 = Fraction(2) ** -126
    parted = 0
    for frame in E.FRAMES:
        w, iw = E.weights(frame)
        s = rows[0][lo:hi].view(np.float32).astype(np.float64)
        a = rows[1][lo:hi].view(np.float32).astype(np.float64)
        for i in range(hi - lo):
            for k in range(3):
                pw = E.mul(s[i][k], w)
                exact = Fraction(iw) * Fraction(E.daz(a[i][k])) + Fraction(pw)
                # the subnormal grid (spacing 2^-149) rounds these up to 2^-126; 24 bits with an
                # unbounded exponent keep them below it
                if Q126 - Fraction(2) ** -150 <= abs(exact) < Q126 - Fraction(2) ** -151:
                    parted += 1
                    assert expected[frame][0][lo + i][k] & 0x7FFFFFFF == 0
    assert parted >= 50, parted


def test_cast_rule():
    assert E.u32_of(255.0) == 255 and E.u32_of(254.99998474121094) == 254 and E.u32_of(-0.5) == 0
    assert E.u32_of(-1.0) == 0xFFFFFFFF and E.u32_of(-3.0) == 0xFFFFFFFD
    assert E.u32_of(-(2.0**32) - 5.0) == 0xFFFFFFFB
    assert E.u32_of(float("nan")) == 0 and E.u32_of(-(2.0**63)) == 0 and E.u32_of(2.0**63) == 0
    assert E.u32_of(float("-inf")) == 0
    assert E.smin(1.0, float("nan")) == 1.0  # a NaN channel packs 255
    assert E.tonemap_ref((float("nan"), 0.0, 0.0)) == 0xFFFFFF  # lum is NaN too: every channel 255


def test_cast_rows_leave_int32(rows, expected):
    """At frame 0 every CAST_ROWS row has a channel whose 255 * min(1, o) is below -2^31 and inside
    int64: the rows where (uint32_t)(int64_t) and a cast through int32 part."""
    lo = E.N_TABLE + E.N_BOUNDARY
    assert [tuple(int(v) for v in r) for r in rows[0][lo:lo + len(E.CAST_ROWS)]] == list(E.CAST_ROWS)
    parted = 0
    for acc in E.rows_as_floats(expected[0][0][lo:lo + len(E.CAST_ROWS)]):
        ch = E.tonemap_channels(acc[:3])
        assert any(-(2.0**63) <= v < -(2.0**31) for v in ch), ch
        # a cast through int32 saturates to 0x80000000 there (cvttss2si and v_cvt_i32_f32 alike); the
        # packed words differ where the int64's low bits survive the channel's shift
        sat = [(int(v) if abs(v) < 2.0**31 else -2**31) & 0xFFFFFFFF for v in ch]
        parted += E.pack_ref(ch) != ((sat[0] << 16) + (sat[1] << 8) + sat[2]) & 0xFFFFFFFF
    assert parted >= 4, parted


def test_weights_at_the_rounding_frames():
    f = lambda x: float(np.float32(x))
    assert E.weights(0) == (1.0, 0.0)
    assert E.weights(2**24 - 1) == (2.0**-24, 1.0 - 2.0**-24)
    assert E.weights(2**24) == (2.0**-24, 1.0 - 2.0**-24)  # (float)2^24 + 1 rounds to 2^24
    assert E.weights(2**32 - 1) == (2.0**-32, 1.0)         # (float)(2^32 - 1) is 2^32
    assert E.weights(2) == (f(1.0 / 3.0), f(1.0 - f(1.0 / 3.0)))


def test_exact_model_equals_the_known_answer_restatement():
    """On test_accumulate_tonemap_known_answers' own domain (uniform(0, 3) samples, frames up to
    15) the two restatements are one: its fmaf / ref_tonemap and this module's blend_ref /
    tonemap_ref cannot drift apart."""
    rng = np.random.default_rng(14)
    f = K.f
    for frame in (0, 1, 2, 7, 15):
        for _ in range(200):
            px = (rng.uniform(0, 3, 4) * (rng.random(4) < 0.9)).astype(np.float32)
            px[3] = 0
            acc = rng.uniform(0, 2, 4).astype(np.float32)
            acc[3] = 0
            w = f(1) / (f(frame) + f(1))
            iw = f(1) - w
            want_acc = np.array([K.fmaf(iw, acc[k], f(px[k] * w)) for k in range(4)], np.float32)
            got_acc = np.array(E.blend_ref(px[:3], frame, acc), np.float32)
            assert np.array_equal(got_acc.view(np.uint32), want_acc.view(np.uint32)), (frame, px, acc)
            assert E.tonemap_ref(got_acc[:3]) == K.ref_tonemap(want_acc[:3]), (frame, px, acc)


@pytest.mark.parametrize("n_ranks", [1, 2, 3, 4])
def test_packed_layout_formula_equals_dist(pkg, n_ranks):
    """dist.pack / dist.unpack / dist.packed_len against the header's layout sentence, at 37x21:
    3x2 tiles with partial right and bottom tiles; 4 ranks leave the last two a padding tile."""
    W, H = 37, 21
    L, slots = E.slot_pixels(W, H, n_ranks)
    assert L == pkg.dist.packed_len(W, H, n_ranks)
    assert sorted(slots[slots >= 0].tolist()) == list(range(W * H)), "every pixel has exactly one slot"
    img = np.arange(W * H * 4, dtype=np.float32).reshape(-1, 4) + 1.0
    want = np.zeros((n_ranks * L, 4), np.float32)
    want[slots >= 0] = img[slots[slots >= 0]]
    got = np.concatenate([pkg.dist.pack(img, W, H, r, n_ranks) for r in range(n_ranks)])
    assert np.array_equal(got, want)
    assert np.array_equal(pkg.dist.unpack(want, W, H, n_ranks), img)
    ids = np.concatenate([pkg.dist.rank_pixel_ids(W, H, r, n_ranks) for r in range(n_ranks)])
    assert np.array_equal(ids, slots)
