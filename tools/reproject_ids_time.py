"""Device time of the plane-keyed reprojection (vpx_reproject_ids) beside the frame it follows, HIP
events on the context's stream:

  python tools/reproject_ids_time.py [--config C1] [--repeats 30] [--warmups 5] [--out profiles/x.json]
                                     [--variant NAME=path/to/libvpx_hip.so ...] [--only frame]

The view is the config's, the previous camera a small step (--step, in world units) away from it.
Each repeat times, one after the other (interleaved, so all see the same clocks and the same
neighbours on the machine): the frame (vpx_render at the scene's depth; C1's is 0), the ID pass
(vpx_render_ids), a device-to-device copy, and the reprojection of the frame's samples from the
previous camera's ids and history: static world and moving volumes (every volume in the table, the
first one moved), each with rgb8 NULL and with the tonemap into the screen.  Median with the
5th-95th percentile after warm-ups.

Yardsticks, measured in the same run: (a) the copy moves the bytes the pass must move at the
least: per pixel two 16-byte records, the 16-byte sample and one 16-byte history pixel read, 16
(+4) bytes written, 80 bytes of traffic: a copy of 40 bytes per pixel (40 read, 40 written).  The
pass reads up to four history taps per pixel, neighbours share them through the caches.  (b) the
frame and the ID pass.
--variant times the same calls through another build of the library in the same run (e.g. one
compiled with -DVPX_REPROJECT_PREKEY=1, which runs k_plane_key over the previous ids first and
reads 8-byte keys per tap), the result checked bit for bit against the in-tree build's.
--only frame times the frame alone: with VPX_LIB=<the library of the commit before> VPX_LIB_OLD=1
that is the baseline which shows that the frame path has not moved.  Needs a GPU.
"""
import argparse
import ctypes as C
import json
import os
import sys

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
    ap.add_argument("--config", default="C1")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmups", type=int, default=5)
    ap.add_argument("--step", type=float, default=0.01)
    ap.add_argument("--variant", action="append", default=[], help="NAME=path of another libvpx_hip.so")
    ap.add_argument("--only", choices=("frame",), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reproject_ids_time.py measures on a GPU; none is visible")
    pkg = entry.load_package()
    abi = pkg.abi
    desc = pkg.scene.CONFIGS[args.config]()
    r = pkg.renderer.Renderer(desc, 0).Init()
    ctx, stream = r.ctx, r.stream
    w, h = desc.width, desc.height
    p = desc.frame_params(0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def frame():
        r.Update()

    def run(items):
        times = {k: [] for k in items}
        for i in range(args.warmups + args.repeats):
            for k, fn in items.items():
                t = timed(fn)
                if i >= args.warmups:
                    times[k].append(t)
        return times

    res = {"what": "device time per call, HIP events on the context's stream, interleaved repeats; one run on one machine",
           "device": torch.cuda.get_device_name(0), "config": args.config, "width": w, "height": h,
           "grid_n": desc.grids[0].n, "depth": int(p.max_bounces), "warmups": args.warmups,
           "library": os.path.basename(os.environ.get("VPX_LIB", "libvpx_hip.so"))}
    if args.only == "frame":
        res["calls"] = {k: summary(v) for k, v in run({"frame": frame}).items()}
    else:
        measure(args, pkg, abi, desc, r, ctx, stream, w, h, p, frame, run, res)
    r.ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def measure(args, pkg, abi, desc, r, ctx, stream, w, h, p, frame, run, res):
    import torch

    # the previous tick: the camera a step aside, its ids, and a history of length 1 (its samples)
    pos, tgt = tuple(desc._cam_pos), tuple(desc._cam_target)
    prev_pos = (pos[0] + args.step, pos[1] + 0.5 * args.step, pos[2] - args.step)
    prev_cam = pkg.scene.prev_camera(prev_pos, tgt, w, h)
    with torch.cuda.stream(stream):
        hist_in = torch.zeros_like(r.accumulator)
        out = torch.zeros_like(r.accumulator)
        copy_src = torch.zeros(40 * w * h, dtype=torch.uint8, device=r.device)
        copy_dst = torch.zeros_like(copy_src)
    r.LookAt(prev_pos, tgt)
    r.ResetAccumulator()
    r.Update()
    ids_prev = ctx.render_ids(p)
    ctx.reproject(p, ids_prev, None, r.accumulator, None, desc.camera, prev_cam, out=hist_in)
    r.LookAt(pos, tgt)
    r.ResetAccumulator()
    r.Update()
    ids_cur = ctx.render_ids(p)
    ctx.synchronize()
    cam = r.scene.camera
    cur_vols = [abi.Volume.from_buffer_copy(v) for v in desc.volumes]
    prev_vols = [abi.Volume.from_buffer_copy(v) for v in desc.volumes]
    prev_vols[0].matrix[3] += 0.5 * args.step   # the first volume came from a little to the left
    prev_vols[0].inv_matrix[3] -= 0.5 * args.step

    builds = {"shipped": (ctx.lib, ctx.h)}
    for v in args.variant:
        name, path = v.split("=", 1)
        lib = abi.load_library(path)
        hnd = C.c_void_p()
        abi.check(lib, None, lib.vpx_create(0, C.byref(hnd)), "vpx_create")
        abi.check(lib, hnd, lib.vpx_set_stream(hnd, C.c_void_p(stream.cuda_stream)), "vpx_set_stream")
        builds[name] = (lib, hnd)

    def id_pass():
        ctx._chk(ctx.lib.vpx_render_ids(ctx.h, C.byref(p), None, C.c_void_p(ids_cur.data_ptr())), "vpx_render_ids")

    def copy():
        with torch.cuda.stream(stream):
            copy_dst.copy_(copy_src)

    def reproject(build, moving, rgb):
        lib, hnd = builds[build]
        d, cv, pv = pkg.context.reproject_desc(cam, prev_cam, 32, (1, 0), cur_vols if moving else None,
                                               prev_vols if moving else None)
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        abi.check(lib, hnd, lib.vpx_reproject_ids(hnd, C.byref(p), ptr(ids_cur), ptr(ids_prev), ptr(r.accumulator), ptr(hist_in),
                                                  ptr(out), C.c_void_p(r.screen.data_ptr() if rgb else 0), C.byref(d), cv, pv),
                  "vpx_reproject_ids")

    # every build computes the same image
    same = {}
    for moving in (False, True):
        for b in builds:
            reproject(b, moving, False)
            stream.synchronize()
            same[b] = out.cpu().numpy().view(np.uint32).copy()
        for b in builds:
            assert np.array_equal(same[b], same["shipped"]), f"build {b} computes another image"
        if not moving:
            lengths = same["shipped"].view(np.float32).reshape(-1, 4)[:, 3]
            res["pixels_that_took_history"] = int((lengths > 1.0).sum())
    u = pkg.context.unpack_ids(ids_cur)
    res["pixels_with_a_valid_key"] = int(((u["vox_index"] >= 0) & (u["face"] >= 1) & (u["face"] <= 6)).sum())

    items = {"frame": frame, "render_ids": id_pass, "copy_40B_per_pixel": copy}
    for b in builds:
        for moving in (False, True):
            for rgb in (False, True):
                key = f"{b}/{'moving' if moving else 'static'}{'+rgb8' if rgb else ''}"
                items[key] = (lambda b=b, moving=moving, rgb=rgb: reproject(b, moving, rgb))
    times = run(items)
    med = {k: float(np.median(v)) for k, v in times.items()}
    res["variants"] = {v.split("=", 1)[0]: os.path.basename(v.split("=", 1)[1]) for v in args.variant}
    res["calls"] = {k: summary(v) for k, v in times.items()}
    res["over_copy"] = {k: med[k] / med["copy_40B_per_pixel"] for k in items if "/" in k}
    res["over_frame"] = {k: med[k] / med["frame"] for k in items if "/" in k}
    res["over_render_ids"] = {k: med[k] / med["render_ids"] for k in items if "/" in k}
    for b, (lib, hnd) in builds.items():
        if b != "shipped":
            lib.vpx_destroy(hnd)


if __name__ == "__main__":
    main()
