"""Build-time guard for the optical flow (CPU-only: hipcc cross-compiles gfx950), in the manner of tests/test_color_vio_resources.py:
every kernel of srl_flow.hip uses no scratch; the track kernel stays within 128 VGPRs and within 64 KiB of LDS.  Recorded: k_flow_level0
13 VGPRs, k_flow_down 44, k_flow_scharr 14, k_flow_track 52 VGPRs and 3 648 bytes of LDS (four windows of 441 int16 and 16 floats of
chain results), all without scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_flow_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_flow.hip")
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
    assert len(seen) == 4 and all(any(k in n for n in seen) for k in ("k_flow_level0", "k_flow_down", "k_flow_scharr", "k_flow_track")), out[-2000:]
    for k, (vg, sc, lds) in seen.items():
        assert sc == 0, (k, sc)
        assert vg <= 128, (k, vg)
        if "k_flow_track" in k:
            assert 4 * 441 * 2 <= lds <= 65536, (k, lds)
        else:
            assert lds == 0, (k, lds)
