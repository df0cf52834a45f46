"""Scratch accesses per kernel of a device listing, and how many of them sit inside a loop.

  hipcc <the build's flags> --cuda-device-only -S -o k.s csrc/vpx_kernels.hip
  python tools/loop_scratch.py k.s [substring of the kernel name, default k_frame0]

A block of the listing that belongs to a loop carries the compiler's comment "in Loop: Header=BBn_m
Depth=d" (the header itself "Loop Header: Depth=d"); a scratch access in such a block runs once per
iteration at least.  Per kernel: all scratch accesses, those inside any loop, and per loop header
the count with the loop's depth and size in instructions (the walk loops are the large ones).
"""
import collections
import re
import sys

from mark_counts import kernels


def main():
    want = sys.argv[2] if len(sys.argv) > 2 else "k_frame0"
    print(f"{'instr':>6} {'scr':>4} {'loop':>5}  kernel: header(depth, instructions in the loop)=accesses")
    for name, body in kernels(sys.argv[1]).items():
        if want not in name:
            continue
        loop, n, total = None, 0, 0
        size, hits, depth = collections.Counter(), collections.Counter(), {}
        for line in body:
            t = line.strip()
            m = re.match(r"(?:\.L(BB\d+_\d+):|; %bb\.\d+:)", t)
            if m:
                h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", t)
                own = re.search(r"Loop Header: Depth=(\d+)", t)
                if own and m.group(1):
                    loop = m.group(1)
                    depth[loop] = int(own.group(1))
                elif h:
                    loop = h.group(1)
                    depth[loop] = int(h.group(2))
                else:
                    loop = None
                continue
            if not t or t[0] in ";." or t.endswith(":"):
                continue
            n += 1
            if loop:
                size[loop] += 1
            if t.startswith("scratch_"):
                total += 1
                if loop:
                    hits[loop] += 1
        rows = " ".join(f"{h}({depth[h]}, {size[h]})={c}" for h, c in hits.items())
        print(f"{n:>6} {total:>4} {sum(hits.values()):>5}  {name}: {rows}")


if __name__ == "__main__":
    main()
