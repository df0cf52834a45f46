"""Device time of the variance-guided denoise (vpx_denoise_var, vpx_reproject_moments) beside the
calls it extends, HIP events on the context's stream:

  python tools/denoise_var_time.py [--repeats 20] [--warmups 3] [--sizes 1920x1080,3840x2160]
                                   [--out profiles/denoise_var.json]

One process, one bare context (no world, no camera: the calls read only their arguments).  The
inputs are synthetic: a plane facing the camera, cut into blocks of 97 x 61 pixels with seven keys
and a seventh of the blocks invalid, random colours, history lengths 1..32 and plausible moments;
the previous camera stands a little beside the current one, so the reprojection finds its taps.
Each repeat times, one after the other (interleaved, so all see the same clocks and the same
neighbours on the machine):
  vpx_denoise_var   passes 1..5 with moments, and 5 passes without (every valid pixel takes the
                    spatial arm), rgb8 NULL
  vpx_denoise_ids   passes 1..5 at sigma_l 0.5: the yardstick, the same taps and bytes per tap
  vpx_reproject_moments beside vpx_reproject_ids, rgb8 NULL
Median with the 5th-95th percentile after warm-ups; "spread" is (p95 - p5) / median of the
yardstick, the run-to-run noise a ratio has to exceed.  "pass_ms" reports pass k >= 2 as the
difference of the medians of k and k - 1 passes (pass 1 comes with the key kernel and, for
vpx_denoise_var, with k_var_estimate).  Needs a GPU.
"""
import argparse
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


def synthetic(pkg, w, h, pos, rng):
    """(camera, ids [H, W, 4] uint32) of the plane z = 4 seen from `pos` looking down +z."""
    cam = pkg.scene.look_at(pos, (pos[0], pos[1], pos[2] + 1.0), w, h)
    tl, tr, bl, o = (np.array(list(a), np.float64) for a in (cam.top_left, cam.top_right, cam.bottom_left, cam.cam_pos))
    u, v = np.meshgrid(np.arange(w) / w, np.arange(h) / h)
    d = tl + (tr - tl) * u[..., None] + (bl - tl) * v[..., None] - o
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    t = ((4.0 - o[2]) / d[..., 2]).astype(np.float32)
    hit = o + t[..., None].astype(np.float64) * d  # blocks fixed to the plane, not to the screen
    bx, by = np.floor(hit[..., 0] * w / 4.0 / 97.0).astype(np.int64), np.floor(hit[..., 1] * h / 4.0 / 61.0).astype(np.int64)
    block = (bx * 3 + by * 5) % 7
    ids = np.zeros((h, w, 4), np.uint32)
    ids[..., 0] = t.view(np.uint32)
    ids[..., 1] = np.where(block == 6, 255 << 16, 2 | 3 << 16 | 5 << 24).astype(np.uint32)  # a miss, or face 5: axis 2
    ids[..., 2] = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)
    ids[..., 3] = block.astype(np.uint32)
    return cam, ids


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("denoise_var_time.py measures on a GPU; none is visible")
    pkg = entry.load_package()
    ctx = pkg.context.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    res = {"what": "device time per call, HIP events on the context's stream, interleaved repeats; one run on one machine",
           "device": torch.cuda.get_device_name(0), "warmups": args.warmups, "sizes": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        rng = np.random.default_rng([w, h])
        pos, prev_pos = (0.0, 0.0, 0.0), (-0.02, 0.01, -0.01)
        cam, ids_cur = synthetic(pkg, w, h, pos, rng)
        _, ids_prev = synthetic(pkg, w, h, prev_pos, rng)
        prev = pkg.scene.prev_camera(prev_pos, (prev_pos[0], prev_pos[1], prev_pos[2] + 1.0), w, h)
        img = np.empty((h, w, 4), np.float32)
        img[..., :3] = np.exp2(rng.uniform(-4.0, 2.0, (h, w, 3)))
        img[..., 3] = rng.integers(1, 33, (h, w))
        lum = img[..., 0] * 0.2126 + img[..., 1] * 0.7152 + img[..., 2] * 0.0722
        mom = np.stack([lum, lum * lum + np.exp2(rng.uniform(-8.0, 0.0, (h, w)))], axis=2).astype(np.float32)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda()  # noqa: E731
        d_cur, d_prev, d_img, d_mom = dev(ids_cur), dev(ids_prev), dev(img), dev(mom)
        out, out2 = torch.zeros_like(d_img), torch.zeros_like(d_img)
        mom_out = torch.zeros_like(d_mom)
        p = pkg.abi.FrameParams()
        p.width, p.height = w, h
        torch.cuda.synchronize()

        var = lambda k, m: ctx.denoise_var(p, d_cur, d_img, m, out, k, 4.0, 2.0 ** -10, 4)  # noqa: E731
        items = {}
        for k in range(1, 6):
            items[f"denoise_var/passes{k}"] = (lambda k=k: var(k, d_mom))
            items[f"denoise_ids_sigma0.5/passes{k}"] = (lambda k=k: ctx.denoise(p, d_cur, d_img, out, k, 0.5))
        items["denoise_var_no_moments/passes5"] = lambda: var(5, None)
        items["reproject_ids"] = lambda: ctx.reproject(p, d_cur, d_prev, d_img, d_img, cam, prev, out=out2, nohist=(1, 0))
        items["reproject_moments"] = lambda: ctx.reproject_moments(p, d_cur, d_prev, d_img, d_img, d_mom, cam, prev, out=out2,
                                                                   mom_out=mom_out, nohist=(1, 0))
        times = {k: [] for k in items}
        for i in range(args.warmups + args.repeats):
            for k, fn in items.items():
                t = timed(fn)
                if i >= args.warmups:
                    times[k].append(t)
        took = int((out2.cpu().numpy().reshape(h, w, 4)[..., 3] > 1.0).sum())
        med = {k: float(np.median(v)) for k, v in times.items()}
        r = {"pixels": w * h, "pixels_with_a_valid_key": int(((ids_cur[..., 1] & 0xFFFF) >= 2).sum()),
             "pixels_that_took_history": took, "temporal_arm_pixels": int(((img[..., 3] >= 4) & ((ids_cur[..., 1] & 0xFFFF) >= 2)).sum()),
             "calls": {k: summary(v) for k, v in times.items()}, "pass_ms": {}}
        for key, first in (("denoise_var", "key+estimate+step1"), ("denoise_ids_sigma0.5", "key+step1")):
            ms = [med[f"{key}/passes1"]] + [med[f"{key}/passes{k}"] - med[f"{key}/passes{k - 1}"] for k in range(2, 6)]
            r["pass_ms"][key] = dict(zip((first, "step2", "step4", "step8", "step16"), ms))
        y = r["calls"]["denoise_ids_sigma0.5/passes5"]
        r["spread_of_the_yardstick"] = (y["p95_ms"] - y["p5_ms"]) / y["median_ms"]
        r["denoise_var_over_denoise_ids_5_passes"] = med["denoise_var/passes5"] / med["denoise_ids_sigma0.5/passes5"]
        r["no_moments_over_denoise_ids_5_passes"] = med["denoise_var_no_moments/passes5"] / med["denoise_ids_sigma0.5/passes5"]
        r["reproject_moments_over_reproject_ids"] = med["reproject_moments"] / med["reproject_ids"]
        res["sizes"][size] = r
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
