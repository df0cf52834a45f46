"""Wave-cost model of the primary walk: per-ray (steps, skips) from the CPU walker on whole
16x16 tiles, then the cost of 64-lane waves (max over lanes) without and with compacting
the unfinished rays of a tile after a budget.  Then the wave cost of the primary walks and of the
shadow walks toward the first point light, for the walkers' three box kinds (cubes, axis boxes,
wide boxes), lanes in the kernel's 8x8-per-wave order and each tile's shadow rays compacted.
Usage: [TILES=400] python tools/wavecost.py [C1]"""
import ctypes as C, os, subprocess, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as g
so = "/tmp/walkstats.so"
subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I",
                f"{REPO}/raytracer-voxpopuli_amd/csrc", f"{REPO}/tools/native/walkstats.cpp", "-o", so], check=True)
lib = C.CDLL(so)
V = C.c_void_p
pkg, orc = g.load_package(), g.load_oracle()
cfg = sys.argv[1] if len(sys.argv) > 1 else "C1"
d = pkg.scene.CONFIGS[cfg]()
o = orc.Oracle(pkg.abi, d)
cells = o.cells[0]; n = d.grids[0].n
nb = [(n + 3) // 4]; nb.append((nb[0] + 3) // 4); nb.append((nb[1] + 3) // 4)
l1, l2 = np.zeros(nb[1] ** 3 * 64, np.uint64), np.zeros(nb[2] ** 3 * 64, np.uint64)
lib.build_masks.argtypes = [V, C.c_uint32, V, V]
lib.build_masks(cells.ctypes.data, n, l1.ctypes.data, l2.ctypes.data)
W, H = d.width, d.height
rng = np.random.default_rng(1)
T = int(os.environ.get("TILES", "200"))
tx, ty = rng.integers(0, W // 16, T), rng.integers(0, H // 16, T)
xs = (tx[:, None] * 16 + np.arange(256)[None, :] % 16).reshape(-1)
ys = (ty[:, None] * 16 + np.arange(256)[None, :] // 16).reshape(-1)
cam = d.camera
f = lambda a: np.array(a[:], np.float32)
tl, tr, bl, cp = f(cam.top_left), f(cam.top_right), f(cam.bottom_left), f(cam.cam_pos)
u = (xs.astype(np.float32) * np.float32(1.0 / W))[:, None]; v = (ys.astype(np.float32) * np.float32(1.0 / H))[:, None]
P = (tl + (tr - tl) * u) + (bl - tl) * v
D = P - cp; D = D / np.sqrt((D * D).sum(1, keepdims=True))
with np.errstate(divide="ignore"):
    rD = (np.float32(1) / D).astype(np.float32)
t0 = np.max(np.minimum((0 - cp) * rD, (1 - cp) * rD), 1); t1 = np.min(np.maximum((0 - cp) * rD, (1 - cp) * rD), 1)
ok = (t1 >= t0) & (t0 > 0)
ds = (D < 0).astype(np.float32)
pos = (cp + D * (t0[:, None] + np.float32(5e-5))) * np.float32(n)
P0 = np.clip(pos.astype(np.int64), 0, n - 1)
step = (1 - 2 * ds).astype(np.int32)
cell = np.float32(1.0 / n)
tdel = (cell * step.astype(np.float32)) * rD
tmax = ((np.ceil(pos) - ds) * cell - cp) * rD
st = np.ascontiguousarray(np.concatenate([t0[:, None], tmax, tdel], 1).astype(np.float32))
si = np.ascontiguousarray(np.concatenate([P0, step], 1).astype(np.int32))
per = np.zeros((len(st), 2), np.uint32)
out = np.zeros(8, np.uint64)
lib.walk_sim.argtypes = [V, V, V, C.c_uint32, V, V, V, C.c_uint32, V, V, V]
bnd = np.full(len(st), 1e34, np.float32)
MODE = int(os.environ.get("MODE", "0"))  # walkstats box experiments (1: anisotropic slabs)
if MODE:
    nbk = nb[0]
    bocc = np.ascontiguousarray((np.pad(cells.reshape(n, n, n), [(0, nbk * 4 - n)] * 3, constant_values=255)
                                .reshape(nbk, 4, nbk, 4, nbk, 4) != 255).any(axis=(1, 3, 5)).astype(np.uint8))
    lib.build_slabs.argtypes = [V, C.c_uint32]
    lib.build_slabs(bocc.ctypes.data, nbk)
    lib.set_mode.argtypes = [C.c_int]
    lib.set_mode(MODE)
lib.walk_sim(cells.ctypes.data, l1.ctypes.data, l2.ctypes.data, n, st.ctypes.data, si.ctypes.data, bnd.ctypes.data,
             len(st), out.ctypes.data, None, per.ctypes.data)
SKIP = float(os.environ.get("SKIPCOST", "5.8"))
cost = (per[:, 0] + per[:, 1] + 1) + SKIP * per[:, 1]
cost = np.where(ok, cost, 0).reshape(T, 256)
okt = ok.reshape(T, 256)
def waves(c):  # c: costs of the rays to walk, in order -> sum over 64-lane waves of the max
    return sum(c[i:i + 64].max() for i in range(0, len(c), 64)) if len(c) else 0
base = sum(waves(cost[t][okt[t]]) for t in range(T))
ideal = cost.sum() / 64
print(f"{cfg}: {okt.sum()} walking rays in {T} tiles; mean cost {cost[okt].mean():.1f}, p99 {np.percentile(cost[okt], 99):.0f}")
print(f"  no compaction: {base:.0f}   perfect packing bound: {ideal:.0f} ({base / ideal:.2f}x)")
for B in (20, 40, 60, 80, 120):
    tot = 0
    for t in range(T):
        c = cost[t][okt[t]]
        nw = (len(c) + 63) // 64
        first = sum(min(B, c[i:i + 64].max()) for i in range(0, len(c), 64))
        rem = c[c > B] - B
        tot += first + waves(rem)
    print(f"  compact after {B:4d}: {tot:.0f} ({tot / base:.2f} of no compaction)")
# Ordering the tile's walking rays by their cost before dealing them to waves (e.g. sorted
# by the previous frame's per-pixel walk cost): sum over waves of the max.
srt = sum(waves(np.sort(cost[t][okt[t]])) for t in range(T))
print(f"  sorted by cost within the tile: {srt:.0f} ({srt / base:.2f} of pixel order)")
for q in (4, 8, 16):  # coarse buckets of the cost (what a counting sort on a quantised cost gives)
    tot = 0
    for t in range(T):
        c = cost[t][okt[t]]
        key = np.minimum((c * q / max(c.max() if len(c) else 1, 1)).astype(int), q - 1)
        tot += waves(c[np.argsort(key, kind="stable")])
    print(f"  {q} cost buckets: {tot:.0f} ({tot / base:.2f})")

# ---- the box kinds: primary + shadow wave cost (DESIGN.md section 4's model tables)
lib.build_axis.argtypes = [V, V, C.c_uint32]
lib.build_axis(l1.ctypes.data, l2.ctypes.data, n)
lib.set_mode.argtypes = lib.set_axis.argtypes = lib.set_wide.argtypes = [C.c_int]
lib.set_mode(0)
lane = np.arange(256)
w8 = lane // 64
perm = ((w8 // 2) * 8 + (lane % 64) // 8) * 16 + (w8 % 2) * 8 + lane % 8  # pixel (row-major in the tile) of lane i
light = np.float32(d.points[0].position[:]) if len(d.points) else np.float32([0.5, 1.5, 0.5])
def run(st_, si_, bnd_):
    per_, out_, th_ = np.zeros((len(st_), 2), np.uint32), np.zeros(8, np.uint64), np.zeros(len(st_), np.float32)
    lib.walk_sim(cells.ctypes.data, l1.ctypes.data, l2.ctypes.data, n, np.ascontiguousarray(st_).ctypes.data,
                 np.ascontiguousarray(si_).ctypes.data, np.ascontiguousarray(bnd_, np.float32).ctypes.data, len(st_),
                 out_.ctypes.data, th_.ctypes.data, per_.ctypes.data)
    return per_, out_, th_
lib.set_gate.argtypes = [C.c_int, C.c_int]
lib.set_full.argtypes = lib.set_more.argtypes = [C.c_int]
lib.adv_out.argtypes = [V]
def adv():  # landing skips by the events they advanced (bins 0, 1, 2, 3-4, 5-8, ... 513+), then reset
    h = np.zeros(12, np.uint64); lib.adv_out(h.ctypes.data); return [int(x) for x in h]
# The box kinds, then (round 10) on the wide boxes the maturity gate for G in {1, 2, 3} and N in
# {4, 8, 16}, the lean tier with 3 to 6 segments, both, and the whole-box tier that bounds what
# any number of segments can reach (GATES="" skips these).
# Round 12: the plain-step prefix (the walkers' pre bit) on the wide boxes, alone, under the gates
# G1 N4, G1 N8 and G2 N4, and with a third segment.
rows = [("cubes", 0, 0, 0, 0, 0, 0, 0), ("axis boxes", 2, 0, 0, 0, 0, 0, 0), ("wide boxes", 2, 1, 0, 0, 0, 0, 0)]
if os.environ.get("GATES", "1"):
    rows += [(f"gate G{G} N{4 << f}", 2, 1, G, f, 0, 0, 0) for G in (1, 2, 3) for f in (0, 1, 2)]
    rows += [(f"{2 + m} segments", 2, 1, 0, 0, 0, m, 0) for m in (1, 2, 3, 4)]
    rows += [(f"{2 + m} seg., G{G} N{4 << f}", 2, 1, G, f, 0, m, 0) for m in (1, 2, 3) for G, f in ((1, 0), (1, 1), (2, 0))]
    rows += [("whole boxes", 2, 1, 0, 0, 1, 0, 0), ("whole, G1 N4", 2, 1, 1, 0, 1, 0, 0)]
    rows += [("plain step", 2, 1, 0, 0, 0, 0, 1)]
    rows += [(f"plain step, G{G} N{4 << f}", 2, 1, G, f, 0, 0, 1) for G, f in ((1, 0), (1, 1), (2, 0))]
    rows += [("plain step, 3 seg.", 2, 1, 0, 0, 0, 1, 1)]
if os.environ.get("ROWS"):  # a subset by name, separated by ';' (its first row sets the baseline)
    rows = [r for r in rows if r[0] in os.environ["ROWS"].split(";")]
lib.set_pre.argtypes = [C.c_int]
first = None
for name, axis, wide, G, f, full, more, pre in rows:
    lib.set_axis(axis); lib.set_wide(wide); lib.set_gate(G, f); lib.set_full(full); lib.set_more(more); lib.set_pre(pre)
    per, out, th = run(st, si, bnd)
    padv = adv()
    hit = ok & (th > 0)
    cp_ = np.where(ok, per[:, 0] + per[:, 1] + 1 + SKIP * per[:, 1], 0).reshape(T, 256)[:, perm]
    okp = ok.reshape(T, 256)[:, perm]
    prim = sum(waves(cp_[t][okp[t]]) for t in range(T))
    # shadow rays from every hit toward the light (no facing test), DDA state as the primary's
    org = ((cp + D * th[:, None]) - D * np.float32(2e-4)).astype(np.float32)
    dl = light - org
    dist = np.sqrt((dl * dl).sum(1)).astype(np.float32)
    sd = (dl / dist[:, None]).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        srD = (np.float32(1) / sd).astype(np.float32)
    sds = (sd < 0).astype(np.float32)
    spos = (org + sd * np.float32(5e-5)) * np.float32(n)
    sP0 = np.clip(np.nan_to_num(spos).astype(np.int64), 0, n - 1)
    sstep = (1 - 2 * sds).astype(np.int32)
    sst = np.concatenate([np.zeros((len(org), 1), np.float32), ((np.ceil(spos) - sds) * cell - org) * srD,
                          (cell * sstep.astype(np.float32)) * srD], 1).astype(np.float32)
    ssi = np.concatenate([sP0, sstep], 1).astype(np.int32)
    sper, sout, _ = run(sst[hit], ssi[hit], dist[hit])
    sadv = adv()
    cs_ = np.zeros(len(st)); cs_[hit] = sper[:, 0] + sper[:, 1] + 1 + SKIP * sper[:, 1]
    cs_ = cs_.reshape(T, 256)[:, perm]; hp = hit.reshape(T, 256)[:, perm]
    shad = sum(waves(cs_[t][hp[t]]) for t in range(T))
    tot = prim + shad
    if first is None: first, first_p, first_s = tot, prim, shad
    print(f"  {name:10s}: primary skips/ray {per[ok, 1].mean():.2f} (max {per[ok, 1].max()}) steps {per[ok, 0].mean():.2f}, "
          f"shadow skips/ray {sper[:, 1].mean():.2f} (max {sper[:, 1].max()}) steps {sper[:, 0].mean():.2f}; mean cost "
          f"{cp_[okp].mean():.1f} / {cs_[hp].mean():.1f}; wave cost {prim:.0f} + {shad:.0f} = {tot:.0f} ({tot / first - 1:+.1%}); "
          f"hits {int(hit.sum())} occluded {int(sout[3])} sum of hit t bits {int(out[5])}; end cells {int(out[4])} / {int(sout[4])}, "
          f"shadow t bits {int(sout[5])}, cells {int(out[0])} / {int(sout[0])}")
    print(f"      wave cost primary {prim / first_p - 1:+.1%} shadow {shad / first_s - 1:+.1%} vs cubes; events per landing skip "
          f"(0, 1, 2, -4, -8, ... 513+): primary {padv} shadow {sadv}")
