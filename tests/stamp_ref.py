"""Model stamps restated in numpy, independent of csrc/vpx_stamp.hpp's index formula.

The model is taken as the array [z, y, x] its bytes describe, transposed to the order of the
grid's axes, flipped along the mirrored ones and sliced for the clip; the per-cell rule is then
one boolean mask.  No model index is ever computed.
"""
import itertools

import numpy as np

from test_brush import bricks_empty

GRID_BYTES, CONSTANT = 1, 2

# every orientation as (axes, flips): axes[q] the model axis that feeds grid axis q
ORIENTATIONS = [(p, f) for p in itertools.permutations(range(3)) for f in itertools.product((False, True), repeat=3)]


def decode(orient):
    return tuple((orient >> (2 * q)) & 3 for q in range(3)), tuple(bool((orient >> (8 + q)) & 1) for q in range(3))


def oriented(size, voxels, orient):
    """The model as an array indexed [grid z, grid y, grid x] from the box's low corner."""
    sx, sy, sz = (int(s) for s in size)
    m = np.asarray(voxels, np.uint8).reshape(sz, sy, sx)
    axes, flips = decode(orient)
    perm = [0, 0, 0]
    for q in range(3):
        perm[2 - q] = 2 - axes[q]  # numpy's axis 2 - q is grid axis q
    t = m.transpose(perm)
    for q in range(3):
        if flips[q]:
            t = np.flip(t, axis=2 - q)
    return t


def numpy_stamp(g, models, st):
    """One stamp on the grid g [z, y, x], in place; returns the number of cells changed."""
    n = g.shape[0]
    size, voxels = models[st.model_id]
    t = oriented(size, voxels, int(st.orient))
    gs, ts = [], []
    for q in (2, 1, 0):  # numpy order: z, y, x
        o, e = int(st.origin[q]), t.shape[2 - q]
        lo, hi = max(o, 0), min(o + e, n)
        if lo >= hi:
            return 0
        gs.append(slice(lo, hi))
        ts.append(slice(lo - o, hi - o))
    v = t[tuple(ts)]
    c = g[tuple(gs)]
    solid = (v != 255) if st.flags & GRID_BYTES else (v != 0)
    w = np.full_like(v, st.value) if st.flags & CONSTANT else v
    m = solid & (c >= st.match_lo) & (c <= st.match_hi) & (c != w)
    c[m] = w[m]
    return int(m.sum())


def numpy_stamps(cells, n, models, stamps):
    """(cells after, changed, flipped) of the stamps applied in order to a copy of `cells`;
    models: a list of (size, voxels), indexed by model_id."""
    g = np.asarray(cells, np.uint8).reshape(n, n, n).copy()
    before = bricks_empty(g, n)
    changed = sum(numpy_stamp(g, models, st) for st in stamps)
    return g.reshape(-1), changed, int((before != bricks_empty(g, n)).sum())
