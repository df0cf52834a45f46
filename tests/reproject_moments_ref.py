"""The moments payload of vpx_reproject_moments / vpx_reproject_moments_host restated in numpy.

Written from the definition in include/vpx.h, not from csrc/vpx_reproject.hpp: float32 scalars, one
rounded operation per call (test_kat_reproject's fadd / fmul ..., which assert that no subnormal
arises).  Which arm a pixel takes and which taps are usable is reproject_ids_ref's answer (its arm
and its usable-tap mask), so the two restatements cannot drift apart; the footprint's weights are
reproject_ids_ref.footprint's, from the hit point computed here as the definition states it.  A
tap that is not usable never enters the arithmetic.

Moments and colours in [2^-12, 2^12] keep every product above 2^-126 (a weight is at least 2^-24
where it is not zero: fx is a difference of floats below 2^15).  A plain helper module, imported by
tests/test_denoise_var.py and tests/test_reproject_moments_gpu.py.
"""
import numpy as np

import denoise_ref
import reproject_ids_ref as ids_ref
from test_kat_reproject import fadd, fdiv, fmul, fsub

F = np.float32
ONE = F(1.0)


def lum(c):
    return denoise_ref.lum(np.asarray(c, F)[None, :])[0]


def run(w, h, ids_cur, ids_prev, cur, hist_in, mom_in, cam, prev, max_history=32, nohist=(1, 0), cur_volumes=None,
        prev_volumes=None):
    """Arguments as reproject_ids_ref.run's, and mom_in: float32 [H, W, 2] or None.  Returns
    (hist_out, mom_out [H, W, 2], arm): hist_out and arm are reproject_ids_ref.run's."""
    hist_out, arm, mask = ids_ref.run(w, h, ids_cur, ids_prev, cur, hist_in, cam, prev, max_history, nohist, cur_volumes,
                                      prev_volumes)
    ids_cur = np.ascontiguousarray(ids_cur).view(np.uint32).reshape(h, w, 4)
    cur = np.ascontiguousarray(cur, F).reshape(h, w, 4)
    if hist_in is not None:
        hist_in = np.ascontiguousarray(hist_in, F).reshape(h, w, 4)
        mom_in = np.ascontiguousarray(mom_in, F).reshape(h, w, 2)
    mom_out = np.zeros((h, w, 2), F)
    cap = fsub(F(max_history), ONE)
    for y in range(h):
        for x in range(w):
            lq = lum(cur[y, x, :3])
            l2 = fmul(lq, lq)
            if arm[y, x] != ids_ref.HISTORY:
                mom_out[y, x] = (lq, l2)
                continue
            rec = ids_cur[y, x]
            ray = cam.primary_ray(x, y)
            P = fadd(ray.O, fmul(rec[0:1].view(F)[0], ray.D))
            if cur_volumes is not None and len(cur_volumes):
                v = (int(rec[1]) & 0xFFFF) - 2
                (cm, ci), (pm, pi) = cur_volumes[v], prev_volumes[v]
                if np.asarray(cm, F).tobytes() != np.asarray(pm, F).tobytes() or \
                        np.asarray(ci, F).tobytes() != np.asarray(pi, F).tobytes():
                    P = ids_ref.transform_position(ids_ref.transform_position(P, np.asarray(ci, F)), np.asarray(pm, F))
            tlx, tly, wts = ids_ref.footprint(prev, P, w, h)
            s1, s2, ws, nmin = F(0), F(0), F(0), None
            for k in range(4):
                if not mask[y, x] >> k & 1:
                    continue
                tx, ty = tlx + (k & 1), tly + (k >> 1)
                s1 = fadd(s1, fmul(wts[k], mom_in[ty, tx, 0]))
                s2 = fadd(s2, fmul(wts[k], mom_in[ty, tx, 1]))
                ws = fadd(ws, wts[k])
                hw = hist_in[ty, tx, 3]
                nmin = hw if nmin is None or hw < nmin else nmin
            a = fdiv(ONE, fadd(nmin if nmin < cap else cap, ONE))
            h1, h2 = fdiv(s1, ws), fdiv(s2, ws)
            mom_out[y, x] = (fadd(h1, fmul(fsub(lq, h1), a)), fadd(h2, fmul(fsub(l2, h2), a)))
    return hist_out, mom_out, arm
