"""The host paths of csrc/vpx_denoise_var.hpp and of csrc/vpx_reproject.hpp's moments payload under
AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
(tests/native/denoise_var_host_test.cpp, its own main) built with g++ and run as a child process.
Host code only; no GPU, nothing loaded into this interpreter."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "raytracer-voxpopuli_amd", "csrc")


def test_denoise_var_host_paths_are_clean_under_sanitizers(tmp_path):
    exe = tmp_path / "denoise_var_host_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "native", "denoise_var_host_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "denoise_var host: calls=120 reproject_moments host: calls=48 took_history=yes bad=0" in r.stdout, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
