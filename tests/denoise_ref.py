"""The plane-keyed a-trous filter (vpx_denoise_ids / vpx_denoise_host) restated in numpy.

Written from the filter's definition, not from csrc/vpx_denoise.hpp: float32 arrays, one
operation per numpy call (each rounds once, nearest-even), the taps in the defined order
(rows j = -2..2 outer, columns i = -2..2 inner), a tap that does not match never entering the
arithmetic (boolean indexing selects the matching pixels before anything is computed).

The device flushes subnormals and numpy does not, so the restatement asserts that the question
never arises: no nonzero finite intermediate has a magnitude below 2^-126.  Inputs are chosen
accordingly (colours in [2^-6, 2^6], sigma_l in [2^-4, 2^4]); NaN and infinity pass the check,
they are what the poisoning tests feed it.  A plain helper module, imported by
tests/test_denoise.py and tests/test_denoise_gpu.py.
"""
import numpy as np

F = np.float32
TINY = F(2.0) ** F(-126)
H1 = (F(0.375), F(0.25), F(0.0625))
LUM = (F(0.2126), F(0.7152), F(0.0722))


def _n(a):
    """`a`, after the assertion that nothing in it would have been flushed."""
    f = np.abs(a[np.isfinite(a)])
    assert not ((f != 0) & (f < TINY)).any(), "a subnormal intermediate: the input leaves the tested range"
    return a


def keys(ids):
    """ids: uint32 [H, W, 4].  Returns (a, b), uint32 [H, W] each; (0, 0) where the key is invalid."""
    ids = np.ascontiguousarray(ids).view(np.uint32)
    y, z, w = ids[..., 1], ids[..., 2], ids[..., 3]
    v, face = y & np.uint32(0xFFFF), y >> np.uint32(24)
    ok = (v >= 2) & (face >= 1) & (face <= 6)
    axis = (np.maximum(face, 1) - 1) >> 1
    coord = np.where(axis == 0, z & np.uint32(0xFFFF), np.where(axis == 1, z >> np.uint32(16), w))
    a = np.where(ok, y, 0).astype(np.uint32)
    b = np.where(ok, np.uint32(0x80000000) | coord, 0).astype(np.uint32)
    return a, b


def lum(c):
    """(c.x * 0.2126f + c.y * 0.7152f) + c.z * 0.0722f over [..., 3+]."""
    p0 = _n(np.multiply(c[..., 0], LUM[0], dtype=F))
    p1 = _n(np.multiply(c[..., 1], LUM[1], dtype=F))
    p2 = _n(np.multiply(c[..., 2], LUM[2], dtype=F))
    return _n(np.add(_n(np.add(p0, p1, dtype=F)), p2, dtype=F))


def one_pass(ka, kb, S, step, sigma_l):
    """One pass at `step` of image S (float32 [H, W, 4]).  Returns (D, taps): the image and the
    number of matching taps per pixel (0 where the key is invalid)."""
    Hh, Ww = ka.shape
    valid = kb != 0
    ys, xs = np.nonzero(valid)  # the pixels that are filtered, in row-major order
    acc = np.zeros((len(ys), 3), F)
    wsum = np.zeros(len(ys), F)
    taps = np.zeros(len(ys), np.int64)
    inv_sigma = F(1.0) / F(sigma_l) if sigma_l > 0 else None
    with np.errstate(all="ignore"):
        lq = lum(S[ys, xs]) if inv_sigma is not None else None
        for j in range(-2, 3):
            for i in range(-2, 3):
                rx, ry = xs + i * step, ys + j * step
                m = (rx >= 0) & (rx < Ww) & (ry >= 0) & (ry < Hh)
                m[m] = (ka[ry[m], rx[m]] == ka[ys[m], xs[m]]) & (kb[ry[m], rx[m]] == kb[ys[m], xs[m]])
                if not m.any():
                    continue
                c = S[ry[m], rx[m]]
                h = np.multiply(H1[abs(j)], H1[abs(i)], dtype=F)
                if inv_sigma is None:
                    w = np.full(int(m.sum()), h, F)
                else:
                    d = _n(np.multiply(_n(np.subtract(lum(c), lq[m], dtype=F)), inv_sigma, dtype=F))
                    w = _n(np.divide(h, _n(np.add(F(1.0), _n(np.multiply(d, d, dtype=F)), dtype=F)), dtype=F))
                for k in range(3):
                    acc[m, k] = _n(np.add(acc[m, k], _n(np.multiply(w, c[:, k], dtype=F)), dtype=F))
                wsum[m] = _n(np.add(wsum[m], w, dtype=F))
                taps[m] += 1
        D = S.copy()  # invalid keys keep all four channels; valid ones keep .w
        for k in range(3):
            D[ys, xs, k] = _n(np.divide(acc[:, k], wsum, dtype=F))
    count = np.zeros((Hh, Ww), np.int64)
    count[ys, xs] = taps
    return D, count


def run(ids, img, passes, sigma_l):
    """The results after 1 .. passes passes: ([out_1, ..., out_passes], pass 0's tap counts).
    ids: uint32 [H, W, 4]; img: float32 [H, W, 4]."""
    ka, kb = keys(ids)
    S = np.ascontiguousarray(img, F)
    outs, taps0 = [], None
    for p in range(passes):
        S, taps = one_pass(ka, kb, S, 1 << p, sigma_l)
        outs.append(S)
        if p == 0:
            taps0 = taps
    return outs, taps0
