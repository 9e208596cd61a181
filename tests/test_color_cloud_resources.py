"""Build-time guard for the kernels of the cloud export (CPU-only: hipcc cross-compiles gfx950), in the manner of
tests/test_color_select_resources.py: no kernel of srl_color_cloud.hip uses scratch; the flag kernel, in both of its forms (one element
per thread, and eight), keeps the register budget of eight waves per SIMD (64 VGPRs) and holds LDS only for its counter rows (sixteen
waves x two counters, and the ticket's flag); the scan kernels with the record sink keep the scan's own LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_cloud_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_color_cloud.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "k.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    flags, scans = {}, {}
    for b in re.split(r"remark: Function Name: ", out)[1:]:
        name = b.split()[0]
        vg = int(re.search(r"VGPRs: (\d+)", b).group(1))
        sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        if "k_cloud_flags" in name:
            flags[name] = (vg, sc, lds)
        elif "k_scan_small" in name or "k_scan_tile_sums" in name:      # (the header of the scan also brings kernels this file never launches)
            scans[name] = (vg, sc, lds)
    print("VGPRs / scratch / LDS:", flags, {n[:70]: v for n, v in scans.items()})
    assert len(flags) == 2, out[-2000:]                                     # <1024, 1> and <1024, 8>
    assert sum(1 for n in scans if "CloudRecordSink" in n) == 1            # the scan with the record sink; the sums and their scan are the shared ones
    for k, (vg, sc, lds) in {**flags, **scans}.items():
        assert sc == 0, (k, sc)
    for vg, sc, lds in flags.values():
        assert vg <= 64, vg
        assert lds <= 16 * 2 * 4 + 4, lds                                  # the counter rows and the ticket's flag
    assert all(lds <= 128 for _, _, lds in scans.values())
