"""Device time of the ID pass (vpx_render_ids) beside the depth-0 frame (vpx_render) on one
scene, HIP events on the context's stream:

  python tools/ids_pass_time.py [--config C1] [--repeats 30] [--warmups 5] [--out profiles/x.json]

Each repeat times one ID pass, then one frame (interleaved, so both see the same clocks and the
same neighbours on the machine).  Median with the 5th-95th percentile after warm-ups.
--only render with VPX_LIB=<an earlier libvpx_hip.so> VPX_LIB_OLD=1 times the frame of that
library alone (the baseline of a commit that has no ID pass).  Needs a GPU.
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


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmups", type=int, default=5)
    ap.add_argument("--only", choices=["both", "render"], default="both")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ids_pass_time.py measures on a GPU; none is visible")
    pkg = entry.load_package()
    desc = pkg.scene.CONFIGS[args.config]()
    desc.max_bounces = 0
    r = pkg.renderer.Renderer(desc, 0).Init()
    ctx, stream = r.ctx, r.stream
    w, h = desc.width, desc.height
    ids = torch.empty((h, w, 4), dtype=torch.int32, device=r.device)
    torch.cuda.synchronize()
    p = desc.frame_params(0)
    p.max_bounces = 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def frame():
        r.Update()

    def id_pass():
        ctx._chk(ctx.lib.vpx_render_ids(ctx.h, p, None, ids.data_ptr()), "vpx_render_ids")

    t_ids, t_frame = [], []
    for i in range(args.warmups + args.repeats):
        a = timed(id_pass) if args.only == "both" else None
        b = timed(frame)
        if i >= args.warmups:
            t_frame.append(b)
            if a is not None:
                t_ids.append(a)
    res = {"what": "device time per launch, HIP events on the context's stream, interleaved repeats",
           "device": torch.cuda.get_device_name(0), "library": os.environ.get("VPX_LIB", "in-tree"), "config": args.config,
           "width": w, "height": h, "grid_n": desc.grids[0].n, "warmups": args.warmups,
           "render_depth0": summary(t_frame)}
    if t_ids:
        u = pkg.context.unpack_ids(ids)
        res["render_ids"] = summary(t_ids)
        res["ids_over_frame"] = res["render_ids"]["median_ms"] / res["render_depth0"]["median_ms"]
        res["pixels_hit"] = int((u["vox_index"] >= 0).sum())
    r.ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
