"""Host wall time of one prop edit (ModifyingProp::Update, src/Game/ModifyingProp.cpp:11-21),
ending in vpx_synchronize: monu2 in a 64^3 grid, indices cycling 16, 32, 48, 64.

  (a) the flow before vpx_grid_load_model: scene.load_model_partial on the host, vpx_grid_fill,
      vpx_grid_write_box of the slice's box (two level rebuilds);
  (b) one vpx_grid_load_model of the resident model (one level rebuild).
(a) is also timed with its slice precomputed: its library calls alone, without the numpy loop.

The two alternate in one process (warm-ups first), so drift hits both alike.  Also a full
LoadModel of teapot into 128^3: load_model_grid + vpx_upload_grid against vpx_grid_load_model.
At these sizes the time is launches and synchronisations, not bandwidth: the figures are
overhead-bound.  Needs a GPU.  Writes profiles/prop_edit.json.

  python tools/prop_edit.py [edits per flow, default 200] [out.json]
"""
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


def main():
    import torch

    if not torch.cuda.is_available():
        sys.exit("prop_edit.py measures on a GPU; none is visible")
    edits = max(200, int(sys.argv[1])) if len(sys.argv) > 1 else 200
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "prop_edit.json")
    pkg = entry.load_package()
    sc, abi = pkg.scene, pkg.abi
    ctx = pkg.context.Context(0)
    n = 64
    size, vox, _ = sc.load_model("monu2")
    ctx.model_upload(0, size, vox)
    ctx.grid_load_model(0, n, 0)  # grid 0 exists from here on
    indices = [16, 32, 48, 64]

    def old_flow(index):
        grid, box = sc.load_model_partial(size, vox, n, index, 16)
        ctx.grid_fill(0, abi.MAT_NONE)
        if box is not None:
            x0, y0, z0, x1, y1, z1 = box
            ctx.grid_write_box(0, grid.reshape(n, n, n)[z0:z1, y0:y1, x0:x1], (x0, y0, z0))
        ctx.synchronize()

    slices = {i: sc.load_model_partial(size, vox, n, i, 16) for i in indices}

    def old_flow_device_part(index):  # (a) without its host loop: what a host with a fast loop of its own pays
        grid, box = slices[index]
        ctx.grid_fill(0, abi.MAT_NONE)
        if box is not None:
            x0, y0, z0, x1, y1, z1 = box
            ctx.grid_write_box(0, grid.reshape(n, n, n)[z0:z1, y0:y1, x0:x1], (x0, y0, z0))
        ctx.synchronize()

    def new_flow(index):
        ctx.grid_load_model(0, n, 0, mode=abi.LOAD_PARTIAL, columns=index, thickness=16)
        ctx.synchronize()

    sums = {}
    times = {"old": [], "old_device": [], "new": []}
    for i in range(10 + edits):
        index = indices[i % 4]
        for name, fn in (("old", old_flow), ("old_device", old_flow_device_part), ("new", new_flow)):
            t0 = time.perf_counter()
            fn(index)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= 10:
                times[name].append(dt)
            sums.setdefault(name, {})[index] = ctx.grid_checksum(0)
    assert sums["old"] == sums["new"] == sums["old_device"], "the flows left different grids"

    # a whole LoadModel: teapot into 128^3
    tsize, tvox, _ = sc.load_model("teapot")
    ctx.model_upload(1, tsize, tvox)
    full = {"old": [], "new": []}
    for i in range(5 + 50):
        t0 = time.perf_counter()
        g = sc.load_model_grid(tsize, tvox, 128)
        ctx.lib.vpx_upload_grid(ctx.h, 1, g.ctypes.data, 128)
        ctx.synchronize()
        t1 = time.perf_counter()
        ctx.grid_load_model(1, 128, 1)
        ctx.synchronize()
        t2 = time.perf_counter()
        if i >= 5:
            full["old"].append((t1 - t0) * 1e3)
            full["new"].append((t2 - t1) * 1e3)
    res = {
        "what": "host wall time per edit, ending in vpx_synchronize; overhead-bound (launches and syncs, not bandwidth)",
        "device": torch.cuda.get_device_name(0),
        "prop_edit_monu2_64": {
            "host_loop_fill_write_box": dict(summary(times["old"]), level_rebuilds_per_edit=2),
            "fill_write_box_of_a_precomputed_slice": dict(summary(times["old_device"]), level_rebuilds_per_edit=2),
            "grid_load_model": dict(summary(times["new"]), level_rebuilds_per_edit=1),
            "warmups": 10, "indices": indices, "grids_equal": True},
        "load_model_teapot_128": {"load_model_grid_upload_grid": dict(summary(full["old"]), level_rebuilds_per_edit=1),
                                  "grid_load_model": dict(summary(full["new"]), level_rebuilds_per_edit=1),
                                  "warmups": 5},
    }
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
