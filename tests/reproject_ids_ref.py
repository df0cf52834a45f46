"""The plane-keyed reprojection (vpx_reproject_ids / vpx_reproject_ids_host) restated in numpy.

Written from the definition in include/vpx.h, not from csrc/vpx_reproject.hpp: float32 scalars, one
rounded operation per line.  The key is denoise_ref's; the ray (GetPrimaryRayNoDOF through
Ray::Ray) and PointToUV are test_kat_reproject.Camera's, the restatement that pins
vpx_camera_look_at / vpx_prev_camera_look_at and the static-camera path.  An unusable tap never
enters the arithmetic: it is skipped before anything of it is read into a sum.

Besides the image the restatement returns, per pixel, which arm of the definition was taken and
the mask of usable taps (bit k: tap k), so that the tests can assert what they cover.

The device flushes subnormals and numpy does not, so every operation asserts that the question
does not arise (test_kat_reproject's fadd / fmul ... and _n here).  A plain helper module,
imported by tests/test_reproject_ids.py and tests/test_reproject_ids_gpu.py.
"""
import numpy as np

import denoise_ref
from test_kat_reproject import fadd, fdiv, fdot, fmul, fsub

F = np.float32
ONE = F(1.0)

# the arms of the definition
INVALID_KEY, NOHIST_MATERIAL, NO_PREVIOUS, CAP_ONE, VOLUME_RANGE, OUTSIDE, NO_TAP, HISTORY = range(8)


def transform_position(p, m):
    """TransformPosition with rows 0-2 of the row-major 4x4 m: left-to-right sums."""
    out = []
    for r in range(3):
        a = fmul(m[4 * r], p[0])
        b = fmul(m[4 * r + 1], p[1])
        c = fmul(m[4 * r + 2], p[2])
        d = fmul(m[4 * r + 3], ONE)
        out.append(fadd(fadd(fadd(a, b), c), d))
    return np.array(out, F)


def footprint(prev, P, w, h):
    """None (no history), or (tlx, tly, the four weights)."""
    delta = fsub(P, prev.pos)
    ld, rd = fdot(prev.left_n, delta), fdot(prev.right_n, delta)
    td, bd = fdot(prev.top_n, delta), fdot(prev.bottom_n, delta)
    if not (ld > 0 and rd > 0 and td > 0 and bd > 0):
        return None
    u, v = prev.point_to_uv(P)
    assert u.view(np.uint32) == fdiv(ld, fadd(ld, rd)).view(np.uint32)
    px = fmul(u, F(w))
    py = fmul(v, F(h))
    if not (px >= 0 and px <= F(w) and py >= 0 and py <= F(h)):
        return None
    tlx, tly = int(px), int(py)
    fx = fsub(px, F(tlx))
    fy = fsub(py, F(tly))
    gx = fsub(ONE, fx)
    gy = fsub(ONE, fy)
    return tlx, tly, (fmul(gx, gy), fmul(fx, gy), fmul(gx, fy), fmul(fx, fy))


def run(w, h, ids_cur, ids_prev, cur, hist_in, cam, prev, max_history=32, nohist=(1, 0), cur_volumes=None,
        prev_volumes=None):
    """ids: uint32 [H, W, 4]; cur, hist_in: float32 [H, W, 4]; cam, prev: test_kat_reproject.Camera
    (the current and the previous one); volumes: None or sequences of (matrix, inv_matrix), 16
    float32 each.  Returns (hist_out [H, W, 4], arm [H, W], usable-tap mask [H, W])."""
    ids_cur = np.ascontiguousarray(ids_cur).view(np.uint32).reshape(h, w, 4)
    cur = np.ascontiguousarray(cur, F).reshape(h, w, 4)
    ka, kb = denoise_ref.keys(ids_cur)
    have_prev = ids_prev is not None and hist_in is not None
    if have_prev:
        ids_prev = np.ascontiguousarray(ids_prev).view(np.uint32).reshape(h, w, 4)
        hist_in = np.ascontiguousarray(hist_in, F).reshape(h, w, 4)
        pa, pb = denoise_ref.keys(ids_prev)
    out = cur.copy()
    out[..., 3] = ONE  # every arm but HISTORY
    arm = np.zeros((h, w), np.int64)
    mask = np.zeros((h, w), np.int64)
    cap = fsub(F(max_history), ONE)
    n_volumes = len(cur_volumes) if cur_volumes is not None else 0
    for y in range(h):
        for x in range(w):
            rec = ids_cur[y, x]
            if kb[y, x] == 0:
                arm[y, x] = INVALID_KEY
                continue
            if not have_prev:
                arm[y, x] = NO_PREVIOUS
                continue
            if not cap >= ONE:
                arm[y, x] = CAP_ONE
                continue
            mat = (int(rec[1]) >> 16) & 255
            if nohist[0] <= mat <= nohist[1]:
                arm[y, x] = NOHIST_MATERIAL
                continue
            ray = cam.primary_ray(x, y)
            t = rec[0:1].view(F)[0]
            P = fadd(ray.O, fmul(t, ray.D))
            if n_volumes:
                v = (int(rec[1]) & 0xFFFF) - 2
                if v >= n_volumes:
                    arm[y, x] = VOLUME_RANGE
                    continue
                (cm, ci), (pm, pi) = cur_volumes[v], prev_volumes[v]
                if np.asarray(cm, F).tobytes() != np.asarray(pm, F).tobytes() or \
                        np.asarray(ci, F).tobytes() != np.asarray(pi, F).tobytes():
                    P = transform_position(transform_position(P, np.asarray(ci, F)), np.asarray(pm, F))
            fp = footprint(prev, P, w, h)
            if fp is None:
                arm[y, x] = OUTSIDE
                continue
            tlx, tly, wts = fp
            hs = [F(0), F(0), F(0)]
            ws = F(0)
            nmin = None
            for k in range(4):
                tx, ty = tlx + (k & 1), tly + (k >> 1)
                if not (0 <= tx < w and 0 <= ty < h) or not wts[k] > 0:
                    continue
                if pa[ty, tx] != ka[y, x] or pb[ty, tx] != kb[y, x]:
                    continue
                hw = hist_in[ty, tx, 3]
                if not hw >= ONE:
                    continue
                mask[y, x] |= 1 << k
                for c in range(3):
                    hs[c] = fadd(hs[c], fmul(wts[k], hist_in[ty, tx, c]))
                ws = fadd(ws, wts[k])
                nmin = hw if nmin is None or hw < nmin else nmin
            if nmin is None:
                arm[y, x] = NO_TAP
                continue
            arm[y, x] = HISTORY
            n = fadd(nmin if nmin < cap else cap, ONE)
            a = fdiv(ONE, n)
            for c in range(3):
                hc = fdiv(hs[c], ws)
                out[y, x, c] = fadd(hc, fmul(fsub(cur[y, x, c], hc), a))
            out[y, x, 3] = n
    return out, arm, mask
