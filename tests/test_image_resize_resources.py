"""Build-time guard for the resize kernel of srl_image_prep.hip (CPU-only: hipcc cross-compiles gfx950), beside
tests/test_image_prep_resources.py, which holds the three kernels behind it; it reads the compiler's resource remarks and nothing else.

Recorded (VGPRs / scratch bytes per lane / LDS bytes per block):
  k_resize_bgr<true>   the 2 x 2 box mean        30 / 0 / 0
  k_resize_bgr<false>  the general rule          46 / 0 / 0
Asserted: both instantiations exist, neither uses scratch (the twelve output bytes of a lane's four pixels are registers, no per-lane
array is indexed at run time) and neither takes LDS (it declares none)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_the_resize_kernel_uses_neither_scratch_nor_lds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_image_prep.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "k.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen = {}
    for b in re.split(r"remark: Function Name: ", out)[1:]:
        m = re.search(r"k_resize_bgrILb([01])E", b.split()[0])
        if not m:
            continue
        vg = int(re.search(r"VGPRs: (\d+)", b).group(1))
        sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        seen[int(m.group(1))] = (vg, sc, lds)
    assert set(seen) == {0, 1}, out[-2000:]
    print("VGPRs / scratch / LDS:", seen)
    assert seen[0][1:] == (0, 0) and seen[1][1:] == (0, 0), seen
