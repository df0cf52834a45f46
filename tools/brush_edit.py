"""Host wall time of one small world edit, ending in vpx_synchronize, on the C1 world (1024^3
tiled monu3) and on a 64^3 prop (monu2):

  dig1       one cell dug at a surface cell of the model (the top cell of a column)
  dig1_flip  one lone cell in open space dug again: the smallest edit that empties a brick
  sphere8    an r = 8 sphere dug at that surface cell
  stroke8    eight r = 3 spheres, 6 cells apart, dug in one call
  repaint    the r = 8 sphere repainted with the filter 0..254 (no brick flips)

  --mode brush      vpx_grid_brush (the region-local refresh)
  --mode write_box  the same cells written with vpx_grid_write_box, the box's bytes prepared
                    beforehand on the host.  Run this against a library built from the commit
                    before vpx_grid_brush (VPX_LIB=<that libvpx_hip.so> VPX_LIB_OLD=1) for the
                    baseline with the full rebuild; with the current library it times the same
                    refresh behind vpx_grid_write_box.

Every sample: the edit (timed), then the original bytes written back and a synchronise (not
timed).  Median with the 5th-95th percentile after warm-ups.  Needs a GPU.

  python tools/brush_edit.py --mode brush --world c1 [--edits 20] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as entry  # noqa: E402


def summary(ms):
    a = np.sort(np.array(ms))
    return {"median_ms": float(np.median(a)), "p5_ms": float(np.percentile(a, 5)), "p95_ms": float(np.percentile(a, 95)),
            "samples": len(a)}


def brush_box(b, n):
    """The brush's bounding box clipped to the grid: (lo, hi) inclusive."""
    if b.shape == 0:
        r = int(np.floor(np.sqrt(float(b.r2))))
        while r * r > b.r2:
            r -= 1
        while (r + 1) * (r + 1) <= b.r2:
            r += 1
        lo, hi = [c - r for c in b.center], [c + r for c in b.center]
    else:
        lo, hi = list(b.lo), list(b.hi)
    return [max(0, v) for v in lo], [min(n - 1, v) for v in hi]


def apply_in_box(box, origin, brushes):
    """The brushes on a read-back box [z, y, x] whose first cell is `origin` (numpy restatement)."""
    g = box.copy()
    dz, dy, dx = g.shape
    z, y, x = np.meshgrid(np.arange(dz) + origin[2], np.arange(dy) + origin[1], np.arange(dx) + origin[0], indexing="ij")
    for b in brushes:
        if b.shape == 0:
            m = (x - b.center[0]) ** 2 + (y - b.center[1]) ** 2 + (z - b.center[2]) ** 2 <= int(b.r2)
        else:
            m = (x >= b.lo[0]) & (x <= b.hi[0]) & (y >= b.lo[1]) & (y <= b.hi[1]) & (z >= b.lo[2]) & (z <= b.hi[2])
        m &= (g >= b.match_lo) & (g <= b.match_hi)
        g[m] = b.value
    return g


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["brush", "write_box"], default="brush")
    ap.add_argument("--world", choices=["c1", "prop"], default="c1")
    ap.add_argument("--edits", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated edit names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("brush_edit.py measures on a GPU; none is visible")
    pkg = entry.load_package()
    sc, abi = pkg.scene, pkg.abi
    ctx = pkg.context.Context(0)
    if args.world == "c1":
        n = 1024
        spec, _, _ = sc.tiled_grid("monu3", n)
        spec.upload(ctx.lib, ctx.h, 0)
    else:
        n = 64
        size, vox, _ = sc.load_model("monu2")
        ctx.lib.vpx_upload_grid(ctx.h, 0, sc.load_model_grid(size, vox, n).ctypes.data, n)
    ctx.synchronize()

    # a surface cell: the top solid cell of a column near the middle that has 24 empty cells above it
    surface = None
    for step in range(200):
        x, z = n // 2 + 3 * step, n // 2 + step
        if x >= n:
            break
        col = ctx.grid_read_box(0, (x, 0, z), (1, n, 1)).reshape(-1)
        solid = np.flatnonzero(col != 255)
        if len(solid) and solid[-1] + 24 < n and solid[-1] >= 2 and x + 6 < n and z + 6 < n:
            top = int(solid[-1])
            if (ctx.grid_read_box(0, (x - 5, top + 9, z - 5), (11, 11, 11)) == 255).all():  # open space above it
                surface = (x, top, z)
                break
    assert surface is not None, "no surface cell with open space above it found"
    sx, sy, sz = surface
    air = (sx, sy + 14, sz)
    ctx.grid_brush(0, [sc.box_brush(air, air, 3)]) if args.mode == "brush" else ctx.grid_write_box(0, np.full((1, 1, 1), 3, np.uint8), air)

    edits = {
        "dig1": [sc.box_brush(surface, surface, 255)],
        "dig1_flip": [sc.box_brush(air, air, 255)],
        "sphere8": [sc.sphere_brush(surface, 64, 255)],
        "stroke8": [sc.sphere_brush((min(n - 1, sx + 6 * k), sy, sz), 9, 255) for k in range(8)],
        "repaint": [sc.sphere_brush(surface, 64, 6, (0, 254))],
    }
    if args.only:
        edits = {k: v for k, v in edits.items() if k in args.only.split(",")}
    res = {"what": "host wall time per edit, ending in vpx_synchronize", "device": torch.cuda.get_device_name(0),
           "mode": args.mode, "library": os.environ.get("VPX_LIB", "in-tree"), "world": args.world, "n": n,
           "surface_cell": surface, "warmups": args.warmups, "edits": {}}
    for name, brushes in edits.items():
        los, his = zip(*[brush_box(b, n) for b in brushes])
        lo, hi = [min(v) for v in zip(*los)], [max(v) for v in zip(*his)]
        shape = (hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
        orig = ctx.grid_read_box(0, lo, shape)
        edited = apply_in_box(orig, lo, brushes)
        times, result = [], None
        for i in range(args.warmups + args.edits):
            ctx.synchronize()
            t0 = time.perf_counter()
            if args.mode == "brush":
                result = ctx.grid_brush(0, brushes)
            else:
                ctx.grid_write_box(0, edited, lo)
            ctx.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if i == 0:
                assert np.array_equal(ctx.grid_read_box(0, lo, shape), edited), name
            ctx.grid_write_box(0, orig, lo)  # back to the original world
            ctx.synchronize()
            if i >= args.warmups:
                times.append(dt)
        res["edits"][name] = dict(summary(times), brushes=len(brushes), cells_changed=int((orig != edited).sum()),
                                  box=list(shape[::-1]))
        if result is not None:
            res["edits"][name]["flipped"] = int(result.flipped)
            assert result.changed == int((orig != edited).sum()), name
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
