"""The host side of srl_pc2_decode that reads the caller's bytes (sr_livo_amd/csrc/srl_pc2_layout.cpp: the layout validation and
srl_pc2_yaw_angles) under AddressSanitizer and UBSan: tests/pc2_layout_san_main.cpp, a stand-alone program with its own main, is compiled
together with that translation unit with -fsanitize=address,undefined and run.  It walks a RoboSense layout with the double at offset 18
and row-padded layouts over heap blocks of exactly the message's size: no device call, no Python in the instrumented process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_layout_validation_and_yaw_angles_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "pc2_layout_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "pc2_layout_san_main.cpp"), os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_pc2_layout.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr and "No such file" in b.stderr):
        pytest.skip("the sanitizer runtimes of g++ are not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1"))
    assert r.returncode == 0 and "pc2 layout: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
