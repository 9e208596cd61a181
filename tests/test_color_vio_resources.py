"""Build-time guard for the camera ESIKF's measurement pass (CPU-only: hipcc cross-compiles gfx950), in the manner of
tests/test_color_select_resources.py: the one kernel of srl_color_vio.hip uses no scratch -- a point's 24 doubles and the 78 sums go
through LDS, not through 78 live accumulators per lane -- and stays within the register budget of four waves per SIMD (128 VGPRs;
recorded at 93) and within 64 KiB of LDS (recorded at 53 848 bytes: 256 x 25 doubles of rows, 4 x 80 doubles of wave sums, the counters
and the ticket's flag)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_vio_kernel_has_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_color_vio.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "k.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen = {}
    for b in re.split(r"remark: Function Name: ", out)[1:]:
        name = b.split()[0]
        vg = int(re.search(r"VGPRs: (\d+)", b).group(1))
        sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        seen[name] = (vg, sc, lds)
    print("VGPRs / scratch / LDS:", seen)
    assert len(seen) == 1 and "k_vio_rows" in next(iter(seen)), out[-2000:]
    for k, (vg, sc, lds) in seen.items():
        assert sc == 0, (k, sc)
        assert vg <= 128, (k, vg)
        assert 256 * 25 * 8 <= lds <= 65536, (k, lds)
