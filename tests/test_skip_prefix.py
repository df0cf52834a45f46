"""The lean skip tier's plain-step prefix (csrc/vpx_skip.hpp skip_box_lean's PRE, walk_skip's
kGatePre), on the CPU.

tests/native/skip_prefix_test.cpp checks both lean forms with the bit against each other and against
the general skip_box on random boxes with one, two or three immature axes (h < d, h in d's binade, h
one ulp below a power of two, a tdelta that makes the plain step a tie), and walk_skip with the bit,
alone, under every gate G in {1, 2, 3} x N in {4, 8, 16} and with further segments, against the
cell-by-cell march on 64^3 and 128^3 street worlds: hit, cell count, end cell, t bits and heads.  Rays
start inside at t = 0, on a cell face, with tied components and parallel to an axis, and from outside.
It prints, per ray class, how many skips advanced an axis that the tier without the bit clips to zero
events, and fails when a t = 0 class has none; and it checks, by a checksum recorded from the header
before the bit, that with the bit off every box and walk comes out as it did.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "raytracer-voxpopuli_amd", "csrc")


def test_plain_step_prefix_cpu(tmp_path):
    exe = tmp_path / "skip_prefix_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(HERE, "native", "skip_prefix_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "box bad=0" in r.stdout and "ray bad=0" in r.stdout, r.stdout
    assert "spread missing" not in r.stdout and "took the plain step" not in r.stdout, r.stdout
    assert "results differ" not in r.stdout, r.stdout
