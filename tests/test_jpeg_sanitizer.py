"""The host half of the JPEG decode (sr_livo_amd/csrc/srl_jpeg_scan.cpp: the marker walk and the Huffman decode, the code that reads the
caller's bytes) under AddressSanitizer and UBSan, in the manner of tests/test_pc2_sanitizer.py: tests/jpeg_scan_san_main.cpp, a stand-alone
program with its own main, is compiled together with that translation unit with -fsanitize=address,undefined and run.  It decodes embedded
streams out of heap blocks of exactly their size, then every truncation of them and single-byte corruptions of every header and table
byte: no device call, no Python in the instrumented process, nothing preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_parse_and_entropy_decode_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "jpeg_scan_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "jpeg_scan_san_main.cpp"), os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_jpeg_scan.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr and "No such file" in b.stderr):
        pytest.skip("the sanitizer runtimes of g++ are not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1"))
    assert r.returncode == 0 and "jpeg scan: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_the_embedded_streams_are_the_fixtures():
    """the program's data file holds streams of tests/golden/golden_jpeg.npz and the hash of the checker's decode of each"""
    import re

    import jpeg_cases as jc
    import jpeg_checker as ck
    golden = jc.load_golden()
    text = open(os.path.join(ROOT, "tests", "jpeg_scan_san_streams.inc")).read()
    found = re.findall(r"// (\S+): (\d+) bytes\nstatic const unsigned char stream_(\d+)\[\] = \{([^}]*)\};\nstatic const unsigned long long stream_\d+_hash = 0x([0-9a-f]+)ull;", text)
    assert len(found) >= 4
    for name, n, _, body, want in found:
        data = bytes(int(v) for v in body.replace("\n", "").split(",") if v.strip())
        assert data == golden[name][0] and len(data) == int(n), name
        coef, qt = ck.entropy_decode(data)
        h = 0xcbf29ce484222325
        for x in coef.astype("<i2").tobytes() + qt.astype("<u2").tobytes():
            h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        assert h == int(want, 16), name
