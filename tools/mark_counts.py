"""Static instruction counts between the "; MARK" lines of a kernel in an -DVPX_ASM_MARKS listing.

  hipcc <the build's flags> --cuda-device-only -S -DVPX_ASM_MARKS -o marks.s csrc/vpx_kernels.hip
  python tools/mark_counts.py marks.s 'k_frame0<true, 1, true, 2>' [...]

Counts follow the listing's order (the compiler's block layout), so code the compiler moved across
a mark is counted where it landed.  A mark inside a loop the compiler unrolled appears once per copy:
sections of the same name are summed.
"""
import collections
import re
import subprocess
import sys


def kernels(path):
    """{demangled name: body lines} of the listing's kernels."""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(line)
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"\(.*", "", d).replace("void vpx::", ""): out[n] for n, d in zip(names, dem)}


def count(body):
    sec, rows = "(before the first mark)", collections.OrderedDict()
    for line in body:
        t = line.strip()
        m = re.match(r"; MARK (.*)", t)
        if m:
            sec = m.group(1)
            continue
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        op = t.split()[0]
        r = rows.setdefault(sec, collections.Counter())
        r["all"] += 1
        r["valu"] += op.startswith("v_") and not op.startswith(("v_readlane", "v_writelane", "v_readfirstlane"))
        r["lane"] += op.startswith(("v_readlane", "v_writelane"))
        r["salu"] += op.startswith("s_") and not op.startswith(("s_load", "s_buffer_load", "s_waitcnt", "s_nop"))
        r["div"] += op.startswith("v_div_fixup")
        r["f64"] += op.endswith("_f64")
        r["scratch"] += op.startswith("scratch_")
    return rows


def main():
    ks = kernels(sys.argv[1])
    for want in sys.argv[2:]:
        body = ks[want]
        rows = count(body)
        print(f"== {want}")
        print(f"{'all':>6} {'VALU':>6} {'SALU':>6} {'lane':>5} {'div':>4} {'f64':>4} {'scr':>4}  section")
        tot = collections.Counter()
        for sec, r in rows.items():
            tot.update(r)
            print(f"{r['all']:>6} {r['valu']:>6} {r['salu']:>6} {r['lane']:>5} {r['div']:>4} {r['f64']:>4} {r['scratch']:>4}  {sec}")
        print(f"{tot['all']:>6} {tot['valu']:>6} {tot['salu']:>6} {tot['lane']:>5} {tot['div']:>4} {tot['f64']:>4} {tot['scratch']:>4}  total")


if __name__ == "__main__":
    main()
