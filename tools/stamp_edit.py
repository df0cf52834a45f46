"""Host wall time of one model stamp, ending in vpx_synchronize:

  c1_empty     monu3 (Scene::LoadModel's orientation) into the C1 world (1024^3 tiled monu3) at an
               empty site, the gap beside a tile: bricks flip
  c1_onto      the same half a tile further, over existing geometry, filter 255..255: only the
               empty cells take a voxel
  prop64       monu2 with a quarter turn into a 64^3 grid that holds monu2 (a prop's grid)

  --mode stamp      vpx_grid_stamp of the resident model
  --mode write_box  the same cells through vpx_grid_write_box of the merged box, precomputed on the
                    host: the floor of the flow before vpx_grid_stamp (its merge is not timed).
                    Also timed with the vpx_grid_read_box that the merge needs in front.  Run this
                    against a library built from the commit before vpx_grid_stamp
                    (VPX_LIB=<that libvpx_hip.so> VPX_LIB_OLD=1) for the yardstick.
  --mode kernels    no timing: 256^3 stamps into 1024^3 and 256^3 captures, to be run under
                    rocprofv3 --kernel-trace --stats for stamp_k and capture_k

Every sample: the edit (timed), then the original bytes written back and a synchronise (not
timed).  Median with the 5th-95th percentile after warm-ups.  Both flows end in the same refresh.
Needs a GPU.

  python tools/stamp_edit.py --mode stamp [--edits 20] [--out profiles/x.json]
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


def merged_box(orig, model, st):
    """The stamp on the read-back box `orig` [z, y, x] whose first cell is the stamp's origin, in
    numpy (default byte convention, no CONSTANT): what the host of the old flow computes.  It
    needs no library call, so it also runs against a library from before vpx_grid_stamp."""
    (sx, sy, sz), vox = model
    t = np.asarray(vox, np.uint8).reshape(int(sz), int(sy), int(sx))
    axes = [(st.orient >> (2 * q)) & 3 for q in range(3)]
    t = t.transpose([2 - axes[2], 2 - axes[1], 2 - axes[0]])  # to [grid z, grid y, grid x]
    for q in range(3):
        if (st.orient >> (8 + q)) & 1:
            t = np.flip(t, axis=2 - q)
    dz, dy, dx = orig.shape
    t = t[:dz, :dy, :dx]
    out = orig.copy()
    m = (t != 0) & (out >= st.match_lo) & (out <= st.match_hi)
    out[m] = t[m]
    return out


def kernels(pkg):
    """The launches for a kernel trace: a 256^3 model, half of its voxels solid, stamped into an
    empty 1024^3 world, 5 times plain (model x along grid x: the model is read in rows) and 5 times
    with model z along grid x (stride 65536), each followed by the dig that undoes it; then 5
    captures of a 256^3 box of the C1 world with 16-byte rows and 5 of one a cell off."""
    sc = pkg.scene
    ctx = pkg.context.Context(0)
    spec, _, _ = sc.tiled_grid("monu3", 1024)
    spec.upload(ctx.lib, ctx.h, 0)
    spec.upload(ctx.lib, ctx.h, 1)
    ctx.grid_fill(0, 255)
    rng = np.random.default_rng(3)
    ctx.model_upload(0, (256, 256, 256), np.where(rng.random(256 ** 3) < 0.5, 7, 0).astype(np.uint8))
    origin = (384, 384, 384)
    for orient in (sc.orient(), sc.orient((2, 1, 0))):
        for _ in range(5):
            placed = ctx.grid_stamp(0, [sc.stamp(0, origin, orient)])
            dug = ctx.grid_stamp(0, [sc.stamp(0, origin, orient, pkg.abi.STAMP_CONSTANT, 255)])
            assert placed.changed == dug.changed > 0
    for x0 in (384, 385):
        for _ in range(5):
            ctx.model_capture(1, 1, (x0, 0, 384), (256, 256, 256))
    ctx.synchronize()
    ctx.close()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["stamp", "write_box", "kernels"], default="stamp")
    ap.add_argument("--edits", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated flow names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stamp_edit.py measures on a GPU; none is visible")
    pkg = entry.load_package()
    sc, abi = pkg.scene, pkg.abi
    if args.mode == "kernels":
        return kernels(pkg)
    res = {"what": "host wall time per edit, ending in vpx_synchronize", "device": torch.cuda.get_device_name(0),
           "mode": args.mode, "library": os.environ.get("VPX_LIB", "in-tree"), "warmups": args.warmups, "edits": {}}

    def flows():
        size, vox, _ = sc.load_model("monu3")
        spec, _, _ = sc.tiled_grid("monu3", 1024)
        (mx, my, mz), (px, py, pz) = spec.model_dims, spec.period
        tx, tz = 512 // px, 512 // pz
        c1 = lambda ctx: spec.upload(ctx.lib, ctx.h, 0)  # noqa: E731
        turned = abi.ORIENT_LOAD_MODEL
        yield "c1_empty", 1024, c1, (size, vox), sc.stamp(0, (tx * px + mx, spec.ground, tz * pz), turned), (mx, my, mz)
        yield "c1_onto", 1024, c1, (size, vox), sc.stamp(0, (tx * px + mx // 2, spec.ground, tz * pz), turned, match=(255, 255)), (mx, my, mz)
        size2, vox2, _ = sc.load_model("monu2")
        prop = lambda ctx: ctx.lib.vpx_upload_grid(ctx.h, 0, sc.load_model_grid(size2, vox2, 64).ctypes.data, 64)  # noqa: E731
        quarter = sc.orient((2, 1, 0), (True, False, False))
        ext = (min(64, int(size2[2])), min(64, int(size2[1])), min(64, int(size2[0])))
        yield "prop64", 64, prop, (size2, vox2), sc.stamp(0, (0, 0, 0), quarter), ext

    world = None
    ctx = None
    for name, n, upload, model, st, ext in flows():
        if args.only and name not in args.only.split(","):
            continue
        if world != n:
            if ctx is not None:
                ctx.close()
            ctx = pkg.context.Context(0)
            upload(ctx)
            ctx.synchronize()
            world = n
        if args.mode == "stamp":
            ctx.model_upload(0, *model)
        lo = [int(v) for v in st.origin]
        shape = (ext[2], ext[1], ext[0])
        orig = ctx.grid_read_box(0, lo, shape)
        if name == "c1_empty":
            assert (orig == 255).all(), "the site is not empty"
        edited = merged_box(orig, model, st)
        changed = int((orig != edited).sum())
        assert changed > 0, name
        rows = {"stamp": []} if args.mode == "stamp" else {"write_box": [], "read_box_write_box": []}
        result = None
        for row, times in rows.items():
            for i in range(args.warmups + args.edits):
                ctx.synchronize()
                t0 = time.perf_counter()
                if row == "stamp":
                    result = ctx.grid_stamp(0, [st])
                else:
                    if row == "read_box_write_box":
                        ctx.grid_read_box(0, lo, shape)
                    ctx.grid_write_box(0, edited, lo)
                ctx.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if i == 0:
                    assert np.array_equal(ctx.grid_read_box(0, lo, shape), edited), (name, row)
                ctx.grid_write_box(0, orig, lo)  # back to the original world
                ctx.synchronize()
                if i >= args.warmups:
                    times.append(dt)
        entry_ = {"n": n, "box": list(ext), "box_bytes": int(orig.size), "cells_changed": changed,
                  "rows": {row: summary(times) for row, times in rows.items()}}
        if result is not None:
            assert result.changed == changed, (name, result.changed, changed)
            entry_["flipped"] = int(result.flipped)
        res["edits"][name] = entry_
    if ctx is not None:
        ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
