"""The block layout and the strided copy of the camera stage's host code (sr_livo_amd/csrc/srl_carve.h) compiled as plain C++ and run on
the CPU, in the manner of tests/test_consensus_math.py: tests/carve_main.cpp, a stand-alone program with its own main, is built twice
with the host compiler -- plain, and with -fsanitize=address,undefined -- and run directly.  The program checks itself (its header
comment lists what); here its verdict and its case counts are asserted: 5^3 count triples for each of the element sizes 1, 4, 8 and 12,
and 3 x 3 x 3 images.  No device call, and nothing of Python in the instrumented process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_carve_and_pack_rows(build, tmp_path):
    out = str(tmp_path / build)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", out, os.path.join(ROOT, "tests", "carve_main.cpp")]
    if build == "sanitized":
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr and "No such file" in b.stderr):
        pytest.skip("the sanitizer runtimes of g++ are not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines()[-1] == "carve: 500 layouts, 27 packed images, 0 failures", r.stdout[-2000:]
