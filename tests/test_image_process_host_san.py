"""The host mirror's imageProcessing::process (sr_livo_amd/csrc/host/imageProcessing.cpp) under AddressSanitizer and UBSan, in the
manner of tests/test_track_host_san.py: tests/image_process_san_main.cpp, a stand-alone program with its own main, is compiled together
with the mirror's translation units with -fsanitize=address,undefined and run.  It drives process over whole sequences of frames with
stub steps -- a first frame that fails and is offered again, both point gates, a selection of thousands, an empty one -- and checks that
nothing of the first data is done twice.  No device call, no Python in the instrumented process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_process_mirror_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "image_process_host_san")
    host = os.path.join(ROOT, "sr_livo_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "image_process_san_main.cpp"), os.path.join(host, "imageProcessing.cpp"),
           os.path.join(host, "opticalFlowTracker.cpp"), os.path.join(host, "lkpyramid.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr and "No such file" in b.stderr):
        pytest.skip("the sanitizer runtimes of g++ are not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1"))
    assert r.returncode == 0 and "image process host mirror: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
