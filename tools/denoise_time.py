"""Device time of the plane-keyed denoise (vpx_denoise_ids) beside the frame it filters, HIP
events on the context's stream:

  python tools/denoise_time.py [--config C1] [--repeats 30] [--warmups 5] [--out profiles/x.json]
                               [--variant NAME=path/to/libvpx_hip.so ...]

Each repeat times, one after the other (interleaved, so all see the same clocks and the same
neighbours on the machine): the frame (vpx_render at the scene's depth; C1's is 0), the ID pass
(vpx_render_ids), a device-to-device copy, and the denoise of the frame's accumulator guided by
those ids with 1..5 passes at sigma_l 0 and 0.5 (rgb8 NULL), and with 1 and 5 passes with the
tonemap into the screen, as Renderer.Denoise calls it.  Median with the 5th-95th percentile after
warm-ups.

Yardsticks, measured in the same run: (a) the copy moves the bytes one pass must move at the
least, per pixel an 8-byte key and a 16-byte colour read and 16 bytes written, 40 bytes of
traffic: a copy of 20 bytes per pixel (20 read, 20 written); every pass is reported as a multiple
of it.  (b) the frame.
A call of k passes launches k_plane_key and k passes; "pass_ms" reports pass k >= 2 as the
difference of the medians of k and k - 1 passes (pass 1 comes with the key kernel).
--variant times the same calls through another build of the library in the same run (e.g. one
compiled with -DVPX_DENOISE_LDS=0, the plain form: every step gathers its 25 taps from global
memory), the result checked bit for bit against the in-tree build's.  Needs a GPU.
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
    ap.add_argument("--variant", action="append", default=[], help="NAME=path of another libvpx_hip.so")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("denoise_time.py measures on a GPU; none is visible")
    pkg = entry.load_package()
    abi = pkg.abi
    desc = pkg.scene.CONFIGS[args.config]()
    r = pkg.renderer.Renderer(desc, 0).Init()
    ctx, stream = r.ctx, r.stream
    w, h = desc.width, desc.height
    p = desc.frame_params(0)
    out = torch.zeros_like(r.accumulator)
    copy_src = torch.zeros(20 * w * h, dtype=torch.uint8, device=r.device)
    copy_dst = torch.zeros_like(copy_src)
    torch.cuda.synchronize()

    # the in-tree build, and the variants: a context each, on the same stream
    builds = {"shipped": (ctx.lib, ctx.h)}
    for v in args.variant:
        name, path = v.split("=", 1)
        lib = abi.load_library(path)
        hnd = C.c_void_p()
        abi.check(lib, None, lib.vpx_create(0, C.byref(hnd)), "vpx_create")
        abi.check(lib, hnd, lib.vpx_set_stream(hnd, C.c_void_p(stream.cuda_stream)), "vpx_set_stream")
        builds[name] = (lib, hnd)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def frame():
        r.Update()

    r.Update()
    ids = ctx.render_ids(p)
    ctx.synchronize()

    def id_pass():
        ctx._chk(ctx.lib.vpx_render_ids(ctx.h, p, None, ids.data_ptr()), "vpx_render_ids")

    def copy():
        with torch.cuda.stream(stream):
            copy_dst.copy_(copy_src)

    def denoise(build, passes, sigma_l, rgb):
        lib, hnd = builds[build]
        d = abi.Denoise(passes, sigma_l, 0, 0)
        abi.check(lib, hnd, lib.vpx_denoise_ids(hnd, C.byref(p), C.c_void_p(ids.data_ptr()),
                                                C.c_void_p(r.accumulator.data_ptr()), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(r.screen.data_ptr() if rgb else 0), C.byref(d)), "vpx_denoise_ids")

    # every build computes the same image
    same = {}
    for b in builds:
        denoise(b, 5, 0.5, False)
        stream.synchronize()
        same[b] = out.cpu().numpy().view(np.uint32).copy()
    for b in builds:
        assert np.array_equal(same[b], same["shipped"]), f"build {b} computes another image"

    items = {"frame": frame, "render_ids": id_pass, "copy_20B_per_pixel": copy}
    for b in builds:
        for s in (0.0, 0.5):
            for k in range(1, 6):
                items[f"{b}/sigma{s}/passes{k}"] = (lambda b=b, s=s, k=k: denoise(b, k, s, False))
            for k in (1, 5):
                items[f"{b}/sigma{s}/passes{k}+rgb8"] = (lambda b=b, s=s, k=k: denoise(b, k, s, True))
    times = {k: [] for k in items}
    for i in range(args.warmups + args.repeats):
        for k, fn in items.items():
            t = timed(fn)
            if i >= args.warmups:
                times[k].append(t)
    med = {k: float(np.median(v)) for k, v in times.items()}
    u = pkg.context.unpack_ids(ids)
    ka_valid = (u["vox_index"] >= 0) & (u["face"] >= 1) & (u["face"] <= 6)
    res = {"what": "device time per call, HIP events on the context's stream, interleaved repeats; one run on one machine",
           "device": torch.cuda.get_device_name(0), "config": args.config, "width": w, "height": h,
           "grid_n": desc.grids[0].n, "depth": int(p.max_bounces), "warmups": args.warmups,
           "pixels_with_a_valid_key": int(ka_valid.sum()), "variants": {v.split("=", 1)[0]: os.path.basename(v.split("=", 1)[1])
                                                                       for v in args.variant},
           "calls": {k: summary(v) for k, v in times.items()}, "pass_ms": {}, "pass_over_copy": {}, "denoise_over_frame": {}}
    for b in builds:
        for s in (0.0, 0.5):
            key = f"{b}/sigma{s}"
            ms = [med[f"{key}/passes1"]] + [med[f"{key}/passes{k}"] - med[f"{key}/passes{k - 1}"] for k in range(2, 6)]
            res["pass_ms"][key] = {"key+step1": ms[0], "step2": ms[1], "step4": ms[2], "step8": ms[3], "step16": ms[4]}
            res["pass_over_copy"][key] = {n: v / med["copy_20B_per_pixel"] for n, v in res["pass_ms"][key].items()}
            res["denoise_over_frame"][key] = {f"passes{k}+rgb8": med[f"{key}/passes{k}+rgb8"] / med["frame"] for k in (1, 5)}
    for b, (lib, hnd) in builds.items():
        if b != "shipped":
            lib.vpx_destroy(hnd)
    r.ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
