"""Build-time guard for the kernels of srl_jpeg.hip (CPU-only: hipcc cross-compiles gfx950), in the manner of
tests/test_image_resize_resources.py; it reads the compiler's resource remarks and nothing else.

Recorded (VGPRs / scratch bytes per lane / LDS bytes per block / waves per SIMD):
  k_jpeg_idct<false>  32-bit registers   32 / 0 /  9216 / 8
  k_jpeg_idct<true>   64-bit registers   47 / 0 / 18432 / 8
  k_jpeg_color                           25 / 0 /     0 / 8
Asserted: the three exist; none uses scratch (a lane's eight values and its twelve output bytes are registers, no per-lane array is
indexed at run time); the IDCT's LDS is exactly 32 blocks x 8 rows x 9 words of its register width, the colour kernel takes none."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_the_jpeg_kernels_use_no_scratch_and_the_lds_they_declare(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_jpeg.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "k.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen = {}
    for b in re.split(r"remark: Function Name: ", out)[1:]:
        m = re.search(r"(k_jpeg_idctILb[01]E|k_jpeg_color)", b.split()[0])
        if not m:
            continue
        vg = int(re.search(r"VGPRs: (\d+)", b).group(1))
        sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        seen[m.group(1)] = (vg, sc, lds)
    print("VGPRs / scratch / LDS:", seen)
    assert set(seen) == {"k_jpeg_idctILb0E", "k_jpeg_idctILb1E", "k_jpeg_color"}, out[-2000:]
    assert seen["k_jpeg_idctILb0E"][1:] == (0, 32 * 72 * 4) and seen["k_jpeg_idctILb1E"][1:] == (0, 32 * 72 * 8) and seen["k_jpeg_color"][1:] == (0, 0), seen
    assert all(v[0] <= 64 for v in seen.values()), seen     # eight waves per SIMD
