"""Host wall time of one noise world (Scene::GenerateSomeNoise / GenerateSomeSmoke), ending in
vpx_synchronize, at n = 256 and 512:

  (a) what a host had to do before vpx_grid_generate_noise: the generator on the CPU
      (vpx_noise_generate_host, one thread) and vpx_upload_grid of its n^3 bytes;
  (b) one vpx_grid_generate_noise.
Both end with the level rebuild, and both leave the same grid (checked by checksum).  The two
alternate in one process after a warm-up of each.

With --trace DIR the tool also starts one child under `rocprofv3 --kernel-trace --stats`, a run
of its own, that generates a 1024^3 noise world and a 1024^3 smoke volume, and reads the
generator kernels' time and the level rebuild's (build_l1_k .. build_wide_k, df_plane_k) from
that trace.  Needs a GPU.  Writes profiles/noise_gen_time.json.

  python tools/noise_gen_time.py [--reps 3] [--trace DIR] [--out out.json]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as entry  # noqa: E402

GEN_KERNELS = ("smoke_gen_k", "noise_mark_k", "noise_scan_k", "noise_draw_k")
LEVEL_KERNELS = ("build_l1_k", "build_up_k", "df_plane_k", "build_planes_k", "build_axis_k", "build_wide_k")
SEED = 0x12345678


def summary(ms):
    a = np.array(ms)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "samples": len(a)}


def traced_child(n):
    """The work of the traced run: one noise world and one smoke volume of n^3."""
    pkg = entry.load_package()
    ctx = pkg.context.Context(0)
    for mode, f in ((pkg.abi.GEN_NOISE, 0.03), (pkg.abi.GEN_SMOKE, 0.167)):
        res = ctx.grid_generate_noise(0, n, mode, f, SEED)
        ctx.synchronize()
        print(json.dumps({"n": n, "mode": mode, "draws": res.draws, "checksum": str(ctx.grid_checksum(0))}), flush=True)
    ctx.close()


def read_trace(directory):
    """Kernel name -> (calls, total ms) from the trace's kernel_stats csv."""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for k in GEN_KERNELS + LEVEL_KERNELS:
                    if name.startswith(k) or (k + "(") in name:
                        calls, ms = out.get(k, (0, 0.0))
                        out[k] = (calls + int(row["Calls"]), ms + float(row["TotalDurationNs"]) * 1e-6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", default=None, help="directory for the rocprofv3 run of the 1024^3 calls")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "noise_gen_time.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("noise_gen_time.py measures on a GPU; none is visible")
    if a.child:
        return traced_child(a.child)
    pkg = entry.load_package()
    sc, abi = pkg.scene, pkg.abi
    ctx = pkg.context.Context(0)
    res = {"what": "host wall time per world, ending in vpx_synchronize, level rebuild included",
           "device": torch.cuda.get_device_name(0), "seed": SEED, "sizes": {}}
    for n in (256, 512):
        for name, gen, mode, f in (("noise", sc.generate_some_noise, abi.GEN_NOISE, 0.03),
                                   ("smoke", sc.generate_some_smoke, abi.GEN_SMOKE, 0.167)):
            times = {"host_generate": [], "upload_grid": [], "device_call": []}
            for i in range(1 + a.reps):
                t0 = time.perf_counter()
                cells, hres = gen(n, f, SEED)
                t1 = time.perf_counter()
                ctx.lib.vpx_upload_grid(ctx.h, 0, cells.ctypes.data, n)
                ctx.synchronize()
                t2 = time.perf_counter()
                want = ctx.grid_checksum(0)
                t3 = time.perf_counter()
                dres = ctx.grid_generate_noise(0, n, mode, f, SEED)
                ctx.synchronize()
                t4 = time.perf_counter()
                assert ctx.grid_checksum(0) == want and bytes(dres) == bytes(hres), "the two flows left different grids"
                if i:  # the first round warms both up
                    times["host_generate"].append((t1 - t0) * 1e3)
                    times["upload_grid"].append((t2 - t1) * 1e3)
                    times["device_call"].append((t4 - t3) * 1e3)
            res["sizes"][f"{name}_{n}"] = {"frequency": f, "draws": int(dres.draws),
                                           "filled_cells": int((cells != abi.MAT_NONE).sum()),
                                           **{k: summary(v) for k, v in times.items()}}
            print(name, n, res["sizes"][f"{name}_{n}"], flush=True)
    ctx.close()
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.trace, "--",
               sys.executable, os.path.abspath(__file__), "--child", "1024"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        rows = read_trace(a.trace) if p.returncode == 0 else {}
        res["trace_1024"] = {
            "what": "rocprofv3 --kernel-trace --stats of one noise and one smoke call at 1024^3 (two level rebuilds)",
            "returncode": p.returncode, "child": [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")],
            "kernels": {k: {"calls": c, "total_ms": ms} for k, (c, ms) in sorted(rows.items())},
            "generators_ms": sum(ms for k, (_, ms) in rows.items() if k in GEN_KERNELS),
            "level_rebuild_ms_two_calls": sum(ms for k, (_, ms) in rows.items() if k in LEVEL_KERNELS)}
        if p.returncode:
            res["trace_1024"]["stderr"] = p.stderr[-2000:]
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
