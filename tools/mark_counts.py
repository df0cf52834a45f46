"""Static instruction counts between the "; MARK" lines of a kernel in an -DVPX_ASM_MARKS listing.

  hipcc <the build's flags> --cuda-device-only -S -DVPX_ASM_MARKS -o marks.s csrc/vpx_kernels.hip
  python tools/mark_counts.py marks.s 'k_frame0<true, 1, true, 2>' [...]

Counts follow the listing's order (the compiler's block layout), so code the compiler moved across
a mark is counted where it landed.  A mark inside a loop the compiler unrolled appears once per copy:
sections of the same name are summed.  cmp / cnd / mov: v_cmp*, v_cndmask* and v_mov* (all VALU);
carry: v_addc* / v_subb*; nop: s_nop instructions, wait: the wait states they idle (s_nop N: N + 1).
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
        r["cmp"] += op.startswith("v_cmp")
        r["cnd"] += op.startswith("v_cndmask")
        r["mov"] += op.startswith("v_mov")
        r["carry"] += op.startswith(("v_addc", "v_subb"))
        if op == "s_nop":  # s_nop N idles N + 1 wait states
            r["nop"] += 1
            r["wait"] += int(t.split()[1], 0) + 1
    return rows


def main():
    ks = kernels(sys.argv[1])
    for want in sys.argv[2:]:
        body = ks[want]
        rows = count(body)
        print(f"== {want}")
        cols = [("all", 6, "all"), ("VALU", 6, "valu"), ("SALU", 6, "salu"), ("lane", 5, "lane"), ("div", 4, "div"),
                ("f64", 4, "f64"), ("scr", 4, "scratch"), ("cmp", 5, "cmp"), ("cnd", 5, "cnd"), ("mov", 5, "mov"),
                ("carry", 6, "carry"), ("nop", 4, "nop"), ("wait", 5, "wait")]
        print(" ".join(f"{h:>{w}}" for h, w, _ in cols) + "  section")
        tot = collections.Counter()
        for sec, r in list(rows.items()) + [("total", tot)]:
            if r is not tot:
                tot.update(r)
            print(" ".join(f"{r[k]:>{w}}" for _, w, k in cols) + f"  {sec}")


if __name__ == "__main__":
    main()
