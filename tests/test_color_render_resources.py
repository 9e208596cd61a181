"""Build-time guard for the render kernels (CPU-only: hipcc cross-compiles gfx950), in the manner of tests/test_kernel_resources.py:
k_render_mark, k_render_points and the gather of srl_color_registered_rgb use no scratch; k_render_points keeps the register budget of
eight waves per SIMD (64 VGPRs; recorded at 56) and no LDS beyond its counter reduction."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_render_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_color_render.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "k.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen = {}
    for b in re.split(r"remark: Function Name: ", out)[1:]:
        name = b.split()[0]
        vg = int(re.search(r"VGPRs: (\d+)", b).group(1))
        sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        for k in ("k_render_mark", "k_render_points", "k_render_reg_gather"):
            if k in name:
                seen[k] = (vg, sc, lds)
    assert set(seen) == {"k_render_mark", "k_render_points", "k_render_reg_gather"}, out[-2000:]
    print("VGPRs / scratch / LDS:", seen)
    for k, (vg, sc, lds) in seen.items():
        assert sc == 0, (k, sc)
        assert vg <= 64, (k, vg)
    assert seen["k_render_mark"][2] == 0 and seen["k_render_reg_gather"][2] == 0
    assert seen["k_render_points"][2] <= 128          # four waves x six counters, and the ticket's flag
