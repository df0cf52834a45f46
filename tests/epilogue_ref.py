"""Exact restatement of the frame epilogue: running-average blend, Reinhard-Jodie tonemap, RGB8 pack.

The arithmetic of oracle/vpx_oracle.c's oracle_accumulate_tonemap / tonemap_pack and of
csrc/vpx_wavefront.hpp's blend / tonemap_pack, restated on integers so that special values,
the flush boundary and the weights at 2^24 and 2^32 have an answer that no floating-point unit
produced.  A plain helper module: tests import it (tests/test_epilogue.py pins both oracle builds
to it, tests/test_epilogue_gpu.py runs the device on the same rows).

The model (x86 under MXCSR FTZ | DAZ, which the oracle sets; the device builds with
-fgpu-flush-denormals-to-zero and is held to the same rule):
  - every operation rounds ONCE to float32, nearest-even (an fma is one operation);
  - a subnormal input is read as a zero of its sign (DAZ);
  - a result whose magnitude is below 2^-126 AFTER rounding to 24 bits with an unbounded exponent
    becomes a zero of its sign (FTZ; tininess after rounding).  2^-126 * (1 - 2^-25) therefore
    rounds to 2^-126 and stays, where "round onto the subnormal grid, then flush" also keeps it,
    but fma(1 - 2^-24, 2^-126, 0) = 2^-126 - 2^-150 exactly rounds (unbounded) to
    2^-126 * (1 - 2^-24) < 2^-126 and flushes, where the naive rule rounds up to 2^-126 first;
  - the float -> uint32 cast is (uint32_t)(int64_t): truncate to int64, 0x8000000000000000 for a
    NaN or a value outside int64 (cvttss2si's integer indefinite), keep the low 32 bits.
Values are Python floats that hold float32 values exactly.
"""
import math
import struct

import numpy as np

FRAMES = (0, 1, 2, 7, 2**24 - 1, 2**24, 2**32 - 1)
TWO_M126 = math.ldexp(1.0, -126)
NAN = math.nan
INF = math.inf
LUM = tuple(float(np.float32(x)) for x in (0.2126, 0.7152, 0.0722))  # GetLuminance


def f32(bits):
    """The float32 with this bit pattern, as a Python float."""
    return struct.unpack("<f", struct.pack("<I", bits & 0xFFFFFFFF))[0]


def bits_of(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def daz(x):
    """Subnormal -> zero of the same sign; everything else unchanged."""
    if x != x or x == 0.0 or abs(x) >= TWO_M126:
        return x
    return math.copysign(0.0, x)


def _neg(x):
    return math.copysign(1.0, x) < 0


def _dy(x):
    """A finite float32 as (m, e) with x == m * 2**e exactly, m a signed integer."""
    m, e = math.frexp(x)
    return int(math.ldexp(m, 24)), e - 24


def _round(neg, n, d):
    """+-n/d (n, d positive integers) rounded once to float32, then FTZ, overflow to inf."""
    e = n.bit_length() - d.bit_length()
    shift = 26 - e  # quotient gets 26 or 27 bits
    if shift >= 0:
        q, r = divmod(n << shift, d)
    else:
        q, r = divmod(n, d << -shift)
    extra = q.bit_length() - 24
    low = q & ((1 << extra) - 1)
    q >>= extra
    half = 1 << (extra - 1)
    if low > half or (low == half and (r or (q & 1))):
        q += 1
    k = extra - shift  # |value| = q * 2**k with q <= 2**24: a float32 with an unbounded exponent
    if q.bit_length() + k <= -126:  # below 2^-126 after rounding: flushed
        mag = 0.0
    elif q.bit_length() + k > 128:
        mag = INF
    else:
        mag = math.ldexp(q, k)
    return -mag if neg else mag


def _sum(terms):
    """Exact sum of dyadic terms (m, e) -> (M, E)."""
    E = min(e for _, e in terms)
    return sum(m << (e - E) for m, e in terms), E


def _round_dy(M, E, zero):
    """M * 2**E rounded; `zero` is the result when the exact value is zero."""
    if M == 0:
        return zero
    return _round(M < 0, abs(M) << E, 1) if E >= 0 else _round(M < 0, abs(M), 1 << -E)


def add(a, b):
    a, b = daz(a), daz(b)
    if a != a or b != b:
        return NAN
    if math.isinf(a) or math.isinf(b):
        if math.isinf(a) and math.isinf(b) and a != b:
            return NAN
        return a if math.isinf(a) else b
    if a == 0.0 and b == 0.0:
        return -0.0 if _neg(a) and _neg(b) else 0.0
    M, E = _sum([_dy(x) for x in (a, b) if x != 0.0])
    return _round_dy(M, E, 0.0)  # exact cancellation: +0 in round-to-nearest


def sub(a, b):
    return add(a, -b) if b == b else NAN


def mul(a, b):
    a, b = daz(a), daz(b)
    if a != a or b != b:
        return NAN
    neg = _neg(a) != _neg(b)
    if math.isinf(a) or math.isinf(b):
        if a == 0.0 or b == 0.0:
            return NAN
        return -INF if neg else INF
    if a == 0.0 or b == 0.0:
        return -0.0 if neg else 0.0
    (ma, ea), (mb, eb) = _dy(a), _dy(b)
    return _round_dy(ma * mb, ea + eb, 0.0)


def div(a, b):
    a, b = daz(a), daz(b)
    if a != a or b != b:
        return NAN
    neg = _neg(a) != _neg(b)
    if math.isinf(a):
        return NAN if math.isinf(b) else (-INF if neg else INF)
    if math.isinf(b):
        return -0.0 if neg else 0.0
    if b == 0.0:
        return NAN if a == 0.0 else (-INF if neg else INF)
    if a == 0.0:
        return -0.0 if neg else 0.0
    (ma, ea), (mb, eb) = _dy(a), _dy(b)
    n, d, e = abs(ma), abs(mb), ea - eb
    return _round(neg, n << e, d) if e >= 0 else _round(neg, n, d << -e)


def fma(a, b, c):
    """a * b + c with one rounding."""
    a, b, c = daz(a), daz(b), daz(c)
    if a != a or b != b or c != c:
        return NAN
    pneg = _neg(a) != _neg(b)
    if math.isinf(a) or math.isinf(b):
        if a == 0.0 or b == 0.0:
            return NAN
        p = -INF if pneg else INF
        return NAN if math.isinf(c) and c != p else p
    if math.isinf(c):
        return c
    if a == 0.0 or b == 0.0:
        if c == 0.0:
            return -0.0 if pneg and _neg(c) else 0.0
        return c
    (ma, ea), (mb, eb) = _dy(a), _dy(b)
    terms = [(ma * mb, ea + eb)]
    if c != 0.0:
        terms.append(_dy(c))
    M, E = _sum(terms)
    return _round_dy(M, E, 0.0)


def smin(a, b):
    """std::min: (b < a) ? b : a — a NaN b gives a."""
    return b if b < a else a


def u32_of(v):
    """(uint32_t)(int64_t)v as x86 computes it."""
    if v != v or v >= 2.0**63 or v < -(2.0**63):
        return 0  # low half of the integer indefinite
    return int(v) & 0xFFFFFFFF


def weights(frame_index):
    """w = 1 / ((float)n + 1), 1 - w."""
    n = float(np.float32(np.uint32(frame_index)))  # uint32 -> float32, nearest-even
    w = div(1.0, add(n, 1.0))
    return w, sub(1.0, w)


def blend_ref(sample3, frame_index, acc4):
    """acc' = fma(1-w, acc, px*w) per channel, px*w rounded first; w channel: fma(1-w, acc.w, 0*w)."""
    w, iw = weights(frame_index)
    px = (float(sample3[0]), float(sample3[1]), float(sample3[2]), 0.0)
    return tuple(fma(iw, float(acc4[k]), mul(px[k], w)) for k in range(4))


def tonemap_channels(acc3):
    """The three floats 255 * min(1, o) that the pack casts."""
    c = [float(acc3[0]), float(acc3[1]), float(acc3[2])]
    lum = add(add(mul(c[0], LUM[0]), mul(c[1], LUM[1])), mul(c[2], LUM[2]))  # dot, left to right
    d = add(1.0, lum)
    out = []
    for k in range(3):
        rh = div(c[k], add(1.0, c[k]))
        la = div(c[k], d)
        o = add(la, mul(rh, sub(rh, la)))
        out.append(mul(255.0, smin(1.0, o)))
    return out


def pack_ref(v3):
    r, g, b = (u32_of(v) for v in v3)
    return ((r << 16) + (g << 8) + b) & 0xFFFFFFFF


def tonemap_ref(acc3):
    return pack_ref(tonemap_channels(acc3))


def cast_defined(acc3):
    """False where a channel's 255 * min(1, o) is below -2^63: (int64_t) of it is undefined in C."""
    return all(not (v < -(2.0**63)) for v in tonemap_channels(acc3))


# ------------------------------------------------------------------ rows
SUB_MIN, SUB_MAX, NORM_MIN = 0x00000001, 0x007FFFFF, 0x00800000


def fbits(x):
    return int(np.float32(x).view(np.uint32))


TABLE_BITS = (
    0x00000000, 0x80000000,           # +-0
    SUB_MIN, 0x80000000 | SUB_MIN,    # +-smallest subnormal
    SUB_MAX,                          # largest subnormal
    NORM_MIN, 0x80000000 | NORM_MIN,  # +-2^-126
    0x01000000,                       # 2^-125
    fbits(1e-30), fbits(0.5),
    0x3F7FFFFF,                       # 1 - 2^-24
    fbits(1.0),
    0x3F800001,                       # 1 + 2^-23
    fbits(3.0), fbits(255.0), fbits(1e10), fbits(1e19),
    0x7F7FFFFF, 0xFF7FFFFF,           # +-FLT_MAX
    0x7F800000, 0xFF800000,           # +-inf
    0x7FC00000,                       # NaN
    fbits(-0.5), fbits(-1.0), fbits(-3.5), fbits(-4e16),
)


def _table_rows(rng):
    """Every (sample value, accumulator value) pair of the table once, three pairs to a row."""
    pairs = [(s, a) for s in TABLE_BITS for a in TABLE_BITS]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    while len(pairs) % 3:
        pairs.append(pairs[0])
    return [([p[0] for p in pairs[i:i + 3]], [p[1] for p in pairs[i:i + 3]]) for i in range(0, len(pairs), 3)]


def boundary_rows():
    """Accumulator and sample within a few ulp of 2^-126 and 2^-125, and the products that land
    within an ulp of 2^-126 for the weights of FRAMES (1/2, 1/3, 1/8, 2^-24, 2^-32 and 1 - those):
    the rows where "flush after rounding with an unbounded exponent" and "round onto the
    subnormal grid, then flush" part.  Returns (sample bits [n,3], accum bits [n,4])."""
    near = [NORM_MIN + d for d in (0, 1, 2, 3)] + [SUB_MAX, SUB_MAX - 1] + [0x01000000 + d for d in (-2, -1, 0, 1, 2)]
    # x with x * w or x * (1-w) next to 2^-126 for w = 1/3, 1/8, 1/2, 2^-24, 2^-32
    scaled = []
    for frame in FRAMES[1:]:
        w, iw = weights(frame)
        for m in (w, iw):
            x0 = bits_of(div(TWO_M126, m))
            scaled += [x0 + d for d in (-2, -1, 0, 1, 2)]
    vals = near + scaled
    vals += [v | 0x80000000 for v in vals]
    s, a = [], []
    zero = 0
    for i, v in enumerate(vals):
        o = vals[(i + 1) % len(vals)]
        s.append([zero, v, o])       # blend of 0 with a boundary value; boundary sample alone
        a.append([v, zero, o, v])    # ... and both near the boundary
        s.append([v, v ^ 0x80000000, NORM_MIN])
        a.append([v, v, v ^ 0x80000000, o])
    return np.array(s, np.uint32), np.array(a, np.uint32)


# Samples whose tonemap leaves a channel's 255 * min(1, o) below -2^31 yet inside int64 (with a zero
# accumulator at frame 0 the blend returns the sample): one channel at -0.99, so that color / (1 +
# color) is -99, and another tuned until 1 + luminance is one or two ulp from zero.  A cast through
# int32 differs there; random rows never reach it.
CAST_ROWS = (
    (0xBF7D70A4, 0xBF8D4D5B, 0), (0xBF7D70A4, 0xBF8D4D5E, 0), (0, 0xBF7D70A4, 0xC08165A1), (0, 0xBF7D70A4, 0xC081659E),
    (0xC08BC23B, 0, 0xBF7D70A4), (0xC08BC23D, 0, 0xBF7D70A4), (0xBF7D70A4, 0, 0xC12EF6D5), (0xBF7D70A4, 0, 0xC12EF6D8),
)


def cases(seed, count):
    """`count` seeded (sample, accumulator) rows as bit patterns: uint32 [count, 3] and [count, 4].
    First the table's full cross product, then the flush-boundary rows, the CAST_ROWS over a zero
    accumulator, then random bit patterns (half of them any uint32, half with exponents within the
    tonemap's interesting range).  The accumulator's w lane takes table and random values too: the
    blend computes it."""
    rng = np.random.default_rng(seed)
    rows = _table_rows(rng)
    s = np.array([r[0] for r in rows], np.uint32)
    a3 = np.array([r[1] for r in rows], np.uint32)
    t = np.array(TABLE_BITS, np.uint32)
    a = np.concatenate([a3, t[rng.integers(0, len(t), (len(rows), 1))]], axis=1)
    bs, ba = boundary_rows()
    cs = np.array(CAST_ROWS, np.uint32)
    s, a = np.concatenate([s, bs, cs]), np.concatenate([a, ba, np.zeros((len(cs), 4), np.uint32)])
    if count < len(s):
        raise ValueError(f"cases(): the table, boundary and cast rows alone are {len(s)}")
    n = count - len(s)
    rs = rng.integers(0, 2**32, (n, 3), dtype=np.uint64).astype(np.uint32)
    ra = rng.integers(0, 2**32, (n, 4), dtype=np.uint64).astype(np.uint32)
    # every other random row: exponents 2^-8 .. 2^8 (the tonemap's knee), non-negative, so that
    # RGB8 varies; the other half is any bit pattern at all
    mid = np.arange(n) % 2 == 1
    for r in (rs, ra):
        e = rng.integers(119, 136, r.shape, dtype=np.uint64).astype(np.uint32)
        r[mid] = (r[mid] & np.uint32(0x007FFFFF)) | (e[mid] << np.uint32(23))
    return np.concatenate([s, rs]), np.concatenate([a, ra])


N_TABLE = len(_table_rows(np.random.default_rng(0)))
N_BOUNDARY = len(boundary_rows()[0])


def rows_as_floats(bits):
    with np.errstate(invalid="ignore"):  # a signalling NaN's conversion raises the flag; the value stays a NaN
        return np.ascontiguousarray(bits, np.uint32).view(np.float32).astype(np.float64)


def reference(sample_bits, acc_bits, frame_index):
    """blend_ref + tonemap_ref over rows of bit patterns: (acc' bits [n,4], rgb8 [n])."""
    s, a = rows_as_floats(sample_bits), rows_as_floats(acc_bits)
    out = np.zeros((len(s), 4), np.float32)
    rgb = np.zeros(len(s), np.uint32)
    for i in range(len(s)):
        out[i] = blend_ref(s[i], frame_index, a[i])
        rgb[i] = tonemap_ref(out[i][:3])
    return out.view(np.uint32), rgb


def defined_rows(acc_bits):
    """cast_defined per row of blended accumulators (bit patterns [n, >=3])."""
    a = rows_as_floats(acc_bits)
    return np.array([cast_defined(r[:3]) for r in a], bool)


def compare(got_acc_bits, got_rgb, want_acc_bits, want_rgb):
    """The parity contract of the epilogue.  Accumulators: the NaN masks are equal and every other
    lane is bit-equal (a generated NaN is 0xffc00000 on x86 and 0x7fc00000 on gfx950).  RGB8
    (got_rgb None: not compared): equal on the rows where every channel's 255 * min(1, o), computed
    by the exact model from the wanted accumulator, is >= -2^63; below that the int64 cast is
    undefined in C for the oracle and the device alike.  Returns (failing row indices, share of
    rows left out of the RGB8 comparison)."""
    w = np.ascontiguousarray(want_acc_bits, np.uint32)
    w = w.reshape(len(w), -1)
    g = np.ascontiguousarray(got_acc_bits, np.uint32).reshape(w.shape)
    gn, wn = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = ((gn != wn) | (~wn & (g != w))).any(axis=1)
    defined = defined_rows(w)
    if got_rgb is not None:
        bad |= defined & (np.ascontiguousarray(got_rgb).view(np.uint32).reshape(-1) != np.asarray(want_rgb, np.uint32))
    return np.flatnonzero(bad).tolist(), float(1.0 - defined.mean())


# ------------------------------------------------------------------ packed tile layout
def slot_pixels(width, height, n_ranks):
    """include/vpx.h's packed layout, written out from its sentence: 16x16 tiles in row-major tile
    order, tile t in rank t % R's buffer as that rank's tile t // R, every rank's buffer
    ceil(tiles / R) tiles long; inside a tile entry i is pixel (8*((i>>6)&1) + (i&7),
    8*(i>>7) + ((i>>3)&7)).  Returns (L, pixel id y*W + x per slot of the R buffers back to back,
    -1 for the padding of partial tiles and of ranks with fewer tiles)."""
    tx, ty = (width + 15) // 16, (height + 15) // 16
    per_rank = -(-(tx * ty) // n_ranks)
    L = per_rank * 256
    out = np.full(n_ranks * L, -1, np.int64)
    for r in range(n_ranks):
        for j in range(per_rank):
            t = j * n_ranks + r
            if t >= tx * ty:
                continue
            for i in range(256):
                x = (t % tx) * 16 + 8 * ((i >> 6) & 1) + (i & 7)
                y = (t // tx) * 16 + 8 * (i >> 7) + ((i >> 3) & 7)
                if x < width and y < height:
                    out[r * L + j * 256 + i] = y * width + x
    return L, out
