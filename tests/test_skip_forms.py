"""The walkers' rewritten instruction forms (csrc/vpx_skip.hpp), on the CPU.

tests/native/skip_forms_test.cpp keeps verbatim restatements of the helpers that were rewritten
(df_box_axis with dom_axis / sec_axis / wid_dfw, seg_params_nb) and compares the new forms
(box_sel / df_box_sel, the clamp as a median, the range test as one compare) with them bit for
bit: every tdelta triple out of ordinary, pairwise and triply equal, infinite, NaN, denormal and
huge values; every octant x dominant axis x second axis with cells at 0, 1, 3, 4, n - 4 and
n - 1 for n = 8, 64 and 1024 (boxes clipped at both faces) and bytes 1, 2 and 255; heads at,
below and above their tdelta over every exponent and every shift around the clamp's ends, exact
ties and refused values; the step body's forms (the cell's bit, the moved test, the class table,
the mask bit) and step1 against the reference's branches on heads full of ties, zeros, infinities
and NaNs.  Then 20 000 seeded rays per world of skip_walk_test.cpp (n = 64 and
128, three densities, axis-aligned rays with +-0 components among them) walk with the packed
selectors on and off under the gates the walk kinds use, against the cell-by-cell march: hit,
end cell, t, the three tmax and the cell count.  A second build runs the same under ASan + UBSan
as a stand-alone program.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "raytracer-voxpopuli_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


@pytest.mark.parametrize("sanitize", [False, True])
def test_skip_forms_native(tmp_path, sanitize):
    exe = tmp_path / "skip_forms_test"
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(HERE, "native", "skip_forms_test.cpp"),
           "-o", str(exe)]
    subprocess.run(cmd + (SAN if sanitize else []), check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = r.stdout
    assert all(k in out for k in ("selectors and boxes:", "seg_params:", "step forms:", "step1:", "walks: rays=")), out
    assert out.count("bad=0") == 5, out
    rays = int(out.split("walks: rays=")[1].split()[0])
    hits = int(out.split("hits=")[1].split()[0])
    assert rays >= 6 * 10000 and hits >= rays // 4, out  # most seeded rays reach the cube; many end in a hit
