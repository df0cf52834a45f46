"""The variance-guided a-trous filter (vpx_denoise_var / vpx_denoise_var_host) restated in numpy.

Written from the definition in include/vpx.h, not from csrc/vpx_denoise_var.hpp: float32 arrays, one
operation per numpy call (each rounds once, nearest-even), the taps in the defined order (rows j
outer, columns i inner), a tap that does not match never entering the arithmetic (boolean indexing
selects the matching pixels before anything is computed).  The key and the luminance are
denoise_ref's.

The device flushes subnormals and numpy does not, so every operation goes through denoise_ref._n:
no nonzero finite intermediate may lie below 2^-126.  The term to watch is (w * w) * var(r): with
colours in [2^-6, 2^6] a luminance difference is at most 2^6, so dd <= 2^6 / epsilon and
w >= 2^-8 / (1 + dd^2); a nonzero variance of such luminances is at least about 2^-37 (one ulp of
l^2 >= 2^-12, divided by a count) and loses at most 2^-6 per pass.  The tests therefore keep
colours in [2^-6, 2^6], sigma_v in [1, 16] and epsilon in [2^-6, 1]: w^2 * var >= 2^-48 * 2^-67,
above the limit, and _n checks it.  NaN and infinity pass _n; they are what the poisoning tests
feed it.  A plain helper module, imported by tests/test_denoise_var.py and
tests/test_denoise_var_gpu.py.
"""
import numpy as np

from denoise_ref import H1, _n, keys, lum

F = np.float32
G1 = (F(0.5), F(0.25))
ZERO, ONE = F(0.0), F(1.0)


def _matching(ka, kb, ys, xs, dy, dx):
    """The mask, over the pixels (ys, xs), of those whose tap (y + dy, x + dx) lies inside the image
    and carries their key; and the tap's coordinates under the mask."""
    Hh, Ww = ka.shape
    rx, ry = xs + dx, ys + dy
    m = (rx >= 0) & (rx < Ww) & (ry >= 0) & (ry < Hh)
    m[m] = (ka[ry[m], rx[m]] == ka[ys[m], xs[m]]) & (kb[ry[m], rx[m]] == kb[ys[m], xs[m]])
    return m, ry[m], rx[m]


def estimate(ka, kb, img, mom, min_history):
    """Step V.  Returns (var0 [H, W], temporal [H, W] bool: the pixels that took the temporal arm)."""
    Hh, Ww = ka.shape
    valid = kb != 0
    var0 = np.zeros((Hh, Ww), F)
    with np.errstate(all="ignore"):
        if mom is None:
            m1 = lum(img)
            m2 = _n(np.multiply(m1, m1, dtype=F))
            temporal = np.zeros((Hh, Ww), bool)
        else:
            m1, m2 = mom[..., 0], mom[..., 1]
            temporal = valid & (img[..., 3] >= F(min_history))  # a NaN fails
        ys, xs = np.nonzero(temporal)
        v = _n(np.subtract(m2[ys, xs], _n(np.multiply(m1[ys, xs], m1[ys, xs], dtype=F)), dtype=F))
        var0[ys, xs] = np.where(v > 0, v, ZERO)
        ys, xs = np.nonzero(valid & ~temporal)
        s1, s2, cnt = np.zeros(len(ys), F), np.zeros(len(ys), F), np.zeros(len(ys), F)
        for j in range(-2, 3):
            for i in range(-2, 3):
                m, ry, rx = _matching(ka, kb, ys, xs, j, i)
                s1[m] = _n(np.add(s1[m], m1[ry, rx], dtype=F))
                s2[m] = _n(np.add(s2[m], m2[ry, rx], dtype=F))
                cnt[m] = np.add(cnt[m], ONE, dtype=F)
        mean = _n(np.divide(s1, cnt, dtype=F))
        v = _n(np.subtract(_n(np.divide(s2, cnt, dtype=F)), _n(np.multiply(mean, mean, dtype=F)), dtype=F))
        var0[ys, xs] = np.where(v > 0, v, ZERO)
    return var0, temporal


def one_pass(ka, kb, S, var, step, sigma_v, epsilon):
    """One pass at `step` of colours S [H, W, 3+] and variance var [H, W].  Returns (D [H, W, 3], var')."""
    ys, xs = np.nonzero(kb != 0)
    n = len(ys)
    sigma_v, epsilon = F(sigma_v), F(epsilon)
    with np.errstate(all="ignore"):
        gs, gw = np.zeros(n, F), np.zeros(n, F)
        for j in range(-1, 2):
            for i in range(-1, 2):
                m, ry, rx = _matching(ka, kb, ys, xs, j, i)
                g = np.multiply(G1[abs(j)], G1[abs(i)], dtype=F)
                gs[m] = _n(np.add(gs[m], _n(np.multiply(g, var[ry, rx], dtype=F)), dtype=F))
                gw[m] = np.add(gw[m], g, dtype=F)
        gv = _n(np.divide(gs, gw, dtype=F))
        tol = _n(np.add(_n(np.multiply(sigma_v, _n(np.sqrt(gv, dtype=F)), dtype=F)), epsilon, dtype=F))
        inv = _n(np.divide(ONE, tol, dtype=F))
        lq = lum(S[ys, xs])
        acc, wsum, vacc = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F)
        for j in range(-2, 3):
            for i in range(-2, 3):
                m, ry, rx = _matching(ka, kb, ys, xs, j * step, i * step)
                if not m.any():
                    continue
                c = S[ry, rx]
                h = np.multiply(H1[abs(j)], H1[abs(i)], dtype=F)
                dd = _n(np.multiply(_n(np.subtract(lum(c), lq[m], dtype=F)), inv[m], dtype=F))
                w = _n(np.divide(h, _n(np.add(ONE, _n(np.multiply(dd, dd, dtype=F)), dtype=F)), dtype=F))
                for k in range(3):
                    acc[m, k] = _n(np.add(acc[m, k], _n(np.multiply(w, c[:, k], dtype=F)), dtype=F))
                wsum[m] = _n(np.add(wsum[m], w, dtype=F))
                ww = _n(np.multiply(w, w, dtype=F))
                vacc[m] = _n(np.add(vacc[m], _n(np.multiply(ww, var[ry, rx], dtype=F)), dtype=F))
        D = np.array(S[..., :3], F)  # invalid keys keep S and var
        V = var.copy()
        for k in range(3):
            D[ys, xs, k] = _n(np.divide(acc[:, k], wsum, dtype=F))
        V[ys, xs] = _n(np.divide(vacc, _n(np.multiply(wsum, wsum, dtype=F)), dtype=F))
    return D, V


def run(ids, img, mom, passes, sigma_v, epsilon, min_history):
    """The results after 1 .. passes passes: ([out_1, ..., out_passes], [var_0, ..., var_passes],
    temporal mask).  ids: uint32 [H, W, 4]; img: float32 [H, W, 4]; mom: float32 [H, W, 2] or None.
    out_k is what a call with passes = k returns: .w is img's."""
    ka, kb = keys(ids)
    img = np.ascontiguousarray(img, F)
    mom = None if mom is None else np.ascontiguousarray(mom, F)
    var, temporal = estimate(ka, kb, img, mom, min_history)
    S = img[..., :3]
    outs, variances = [], [var]
    for p in range(passes):
        S, var = one_pass(ka, kb, S, var, 1 << p, sigma_v, epsilon)
        out = img.copy()
        out[..., :3] = S
        outs.append(out)
        variances.append(var)
    return outs, variances, temporal
