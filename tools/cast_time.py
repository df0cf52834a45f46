"""Device time of the device ray batches (vpx_cast_nearest / vpx_cast_occluded), both forms, HIP
events on the context's stream:

  python tools/cast_time.py [--configs C1,C2,Z1] [--rays 4194304] [--repeats 12] [--warmups 3]
                            [--host-repeats 3] [--out profiles/cast_rays.json]

Per config (its world on one device) three batches, built on the device with a seeded generator:
  incoherent   origins uniform in the box of the volumes' bounds, directions uniform on the sphere
  pixels       the config's camera, one pixel-centre ray per pixel of its frame, row-major
  shuffled     the same rays in a seeded random order
Each repeat times, one after the other (interleaved, so every item sees the same clocks and the
same neighbours on the machine), per batch: vpx_cast_nearest with cells and without and
vpx_cast_occluded, each in the per-lane form and, where the batch visits one volume, in the pool
form; the pool with cells at a quarter and a half of the library's wave count as well.  Median
with the 5th-95th percentile after warm-ups.
Yardsticks, same run: (a) the per-lane form on the same batch; (b) the host entry
vpx_find_nearest_cells on the same rays from pageable host memory, its copies and its synchronise
included, by a host clock around the call; (c) for the pixel batch, vpx_render_ids of that view.
"pool_over_lane" gives median ratios, and "pool_wins_incoherent" whether the pool's p95 lies
below the per-lane form's p5 on the incoherent batch: the rule that decides what flags == 0 takes
(DESIGN.md section 4).  Needs a GPU.
"""
import argparse
import ctypes as C
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
            "min_ms": float(a[0]), "samples": len(a)}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C2,Z1")
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cast_time.py measures on a GPU; none is visible")
    pkg = entry.load_package()
    abi = pkg.abi
    dev = "cuda:0"
    stream = torch.cuda.Stream(device=0)
    res = {"what": "device time per call, HIP events on the context's stream, interleaved repeats; one run on one machine",
           "device": torch.cuda.get_device_name(0), "rays_incoherent": args.rays, "warmups": args.warmups, "configs": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for name in args.configs.split(","):
        desc = pkg.scene.CONFIGS[name]()
        ctx = pkg.context.Context(0)
        ctx.load_scene(desc)
        ctx.set_stream(stream.cuda_stream)
        nvol = len(desc.volumes)
        one_volume = nvol == 1
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for v in desc.volumes:
            b = (C.c_float * 6)()
            abi.check(ctx.lib, None, ctx.lib.vpx_volume_bounds(C.byref(v), b), "vpx_volume_bounds")
            lo, hi = np.minimum(lo, b[:3]), np.maximum(hi, b[3:])
        w, h = desc.width, desc.height
        gen = torch.Generator(device=dev).manual_seed(7)
        with torch.cuda.stream(stream):
            n = args.rays
            inc = torch.empty((n, 8), dtype=torch.float32, device=dev)
            inc[:, 0:3] = torch.rand((n, 3), generator=gen, device=dev) * torch.tensor(hi - lo, dtype=torch.float32, device=dev) \
                + torch.tensor(lo, dtype=torch.float32, device=dev)
            inc[:, 3:6] = torch.randn((n, 3), generator=gen, device=dev)
            inc[:, 6] = 1e34
            inc[:, 7] = 0.0
            cam = desc.camera
            tl, tr, bl, pos = (torch.tensor(list(x), dtype=torch.float32, device=dev)
                               for x in (cam.top_left, cam.top_right, cam.bottom_left, cam.cam_pos))
            u = (torch.arange(w, dtype=torch.float32, device=dev) / w).repeat(h)
            vv = (torch.arange(h, dtype=torch.float32, device=dev) / h).repeat_interleave(w)
            pix = torch.empty((w * h, 8), dtype=torch.float32, device=dev)
            pix[:, 0:3] = pos
            pix[:, 3:6] = tl + u[:, None] * (tr - tl) + vv[:, None] * (bl - tl) - pos
            pix[:, 6] = 1e34
            pix[:, 7] = 0.0
            shuf = pix[torch.randperm(w * h, generator=gen, device=dev)].contiguous()
            ids = torch.empty((h, w, 4), dtype=torch.int32, device=dev)
        stream.synchronize()
        batches = {"incoherent": inc, "pixels": pix, "shuffled": shuf}
        p = desc.frame_params(0)
        flt = ctx.ray_filter()  # every volume, the shapes: one volume visited only in a one-volume world
        # the library's wave count for the pool: what a call with max_waves = 0 launches
        props = torch.cuda.get_device_properties(0)
        choice = props.multi_processor_count * 4 * 5
        out = {k: (torch.empty((len(b), 8), dtype=torch.int32, device=dev), torch.empty((len(b), 8), dtype=torch.int32, device=dev),
                   torch.empty((len(b),), dtype=torch.uint8, device=dev)) for k, b in batches.items()}

        def cast(batch, kind, form, max_waves=0):
            rays, (hb, cb, ob) = batches[batch], out[batch]
            opt = abi.Cast(form, max_waves, (C.c_uint32 * 2)(0, 0))
            if kind == "occluded":
                rc = ctx.lib.vpx_cast_occluded(ctx.h, C.c_void_p(rays.data_ptr()), len(rays), C.byref(flt), C.byref(opt),
                                               C.c_void_p(ob.data_ptr()))
            else:
                rc = ctx.lib.vpx_cast_nearest(ctx.h, C.c_void_p(rays.data_ptr()), len(rays), C.byref(flt), C.byref(opt),
                                              C.c_void_p(hb.data_ptr()), C.c_void_p(cb.data_ptr()) if kind == "cells" else None)
            ctx._chk(rc, "vpx_cast_*")

        items = {}
        forms = [("lane", abi.CAST_PER_LANE)] + ([("pool", abi.CAST_POOL)] if one_volume else [])
        for b in batches:
            for kind in ("cells", "hits", "occluded"):
                for fname, form in forms:
                    items[f"{b}/{kind}/{fname}"] = (lambda b=b, kind=kind, form=form: cast(b, kind, form))
            if one_volume:
                for frac in (4, 2):
                    items[f"{b}/cells/pool/waves{choice // frac}"] = (
                        lambda b=b, frac=frac: cast(b, "cells", abi.CAST_POOL, choice // frac))
        items["render_ids"] = lambda: ctx._chk(ctx.lib.vpx_render_ids(ctx.h, C.byref(p), None, C.c_void_p(ids.data_ptr())),
                                               "vpx_render_ids")
        # both forms compute the same records
        if one_volume:
            for b in batches:
                got = {}
                for fname, form in forms:
                    cast(b, "cells", form)
                    cast(b, "occluded", form)
                    stream.synchronize()
                    got[fname] = [t.cpu().numpy().copy() for t in out[b]]
                assert all(np.array_equal(x, y) for x, y in zip(got["lane"], got["pool"])), f"{name}/{b}: the forms differ"
        times = {k: [] for k in items}
        for i in range(args.warmups + args.repeats):
            for k, fn in items.items():
                t = timed(fn)
                if i >= args.warmups:
                    times[k].append(t)
        # (b) the host entry on the same rays, pageable memory, copies and synchronise included
        host = {}
        for b in batches:
            hr = batches[b].cpu().numpy()
            rays = (abi.Ray * len(hr)).from_buffer_copy(hr.tobytes())
            hits, cells = (abi.Hit * len(hr))(), (abi.HitCell * len(hr))()
            ms = []
            for i in range(1 + args.host_repeats):
                t0 = time.perf_counter()
                ctx._chk(ctx.lib.vpx_find_nearest_cells(ctx.h, rays, len(hr), C.byref(flt), hits, cells), "vpx_find_nearest_cells")
                if i:
                    ms.append(1e3 * (time.perf_counter() - t0))
            host[b] = summary(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        cfg = {"width": w, "height": h, "volumes": nvol, "grid_n": desc.grids[0].n, "rays": {b: len(t) for b, t in batches.items()},
               "pool_waves_library_choice": choice if one_volume else None, "calls": {k: summary(v) for k, v in times.items()},
               "host_find_nearest_cells": host}
        if one_volume:
            cfg["pool_over_lane"] = {f"{b}/{kind}": med[f"{b}/{kind}/pool"] / med[f"{b}/{kind}/lane"]
                                     for b in batches for kind in ("cells", "hits", "occluded")}
            cfg["pool_wins_incoherent"] = {kind: cfg["calls"][f"incoherent/{kind}/pool"]["p95_ms"] <
                                           cfg["calls"][f"incoherent/{kind}/lane"]["p5_ms"] for kind in ("cells", "hits", "occluded")}
        cfg["pixels_cells_lane_over_render_ids"] = med["pixels/cells/lane"] / med["render_ids"]
        cfg["host_over_device_lane_cells"] = {b: host[b]["median_ms"] / med[f"{b}/cells/lane"] for b in batches}
        res["configs"][name] = cfg
        print(name, "done", file=sys.stderr, flush=True)
        ctx.close()
        del batches, out, inc, pix, shuf
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
