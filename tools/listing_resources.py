"""Per-kernel LDS / register / spill table from the metadata of a device listing.

  hipcc <the build's flags> --cuda-device-only -S -o k.s csrc/vpx_kernels.hip
  python tools/listing_resources.py k.s [substring of the kernel name, default k_frame0]

The columns are the code object's own fields (.group_segment_fixed_size, .sgpr_count,
.sgpr_spill_count, .vgpr_count, .vgpr_spill_count, .private_segment_fixed_size): what the loader
allocates, where tools/regs.py prints the compiler's remarks (its occupancy column divides the LDS
by the static bytes alone: it knows neither the allocation granule nor a launch's dynamic bytes).
"""
import re
import subprocess
import sys


def main():
    txt = open(sys.argv[1]).read()
    want = sys.argv[2] if len(sys.argv) > 2 else "k_frame0"
    rows = []
    for m in re.finditer(r"  - \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)", txt, re.S):
        get = lambda k: (re.search(r"\.%s:\s*(\S+)" % k, m.group(0)) or [None, "?"])[1]
        rows.append([get(k) for k in ("name", "group_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count",
                                      "vgpr_spill_count", "private_segment_fixed_size")])
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    print(f"{'LDS':>6} {'SGPR':>5} {'sSpl':>5} {'VGPR':>5} {'vSpl':>5} {'scr':>5}  kernel")
    for r, n in zip(rows, names):
        n = re.sub(r"\(.*", "", n).replace("void vpx::", "")
        if want in n:
            print(f"{r[1]:>6} {r[2]:>5} {r[3]:>5} {r[4]:>5} {r[5]:>5} {r[6]:>5}  {n}")


if __name__ == "__main__":
    main()
