"""Build-time guard for the kernels of srl_image_prep.hip (CPU-only: hipcc cross-compiles gfx950), in the manner of
tests/test_consensus_resources.py; it reads the compiler's resource remarks and nothing else.

Recorded (VGPRs / scratch bytes per lane / LDS bytes per block):
  k_prep_pixel   57 / 0 / 0        (four pixels per lane: the twelve output bytes and the packed words are registers)
  k_prep_tiles   21 / 0 / 4096     (= four waves x 256 bins x 4 bytes; the clip, the redistribution and the scan run in registers
                                    and through the wave shuffles, which take no LDS allocation)
  k_prep_apply   53 / 0 / 0
Asserted: no kernel uses scratch (so no per-lane array is indexed at run time), the per-tile kernel's LDS is exactly its histograms,
and the per-pixel kernels use no LDS at all (they declare none)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES_PER_BLOCK = 4                 # k_prep_tiles: one wave per (plane, tile)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_no_scratch_and_the_tile_kernel_holds_only_its_histograms(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_image_prep.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "k.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen = {}
    for b in re.split(r"remark: Function Name: ", out)[1:]:
        m = re.search(r"(k_prep_[a-z]+)", b.split()[0])
        if not m:
            continue
        vg = int(re.search(r"VGPRs: (\d+)", b).group(1))
        sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        seen[m.group(1)] = (vg, sc, lds)
    assert set(seen) == {"k_prep_pixel", "k_prep_tiles", "k_prep_apply"}, out[-2000:]
    print("VGPRs / scratch / LDS:", seen)
    assert seen["k_prep_tiles"][1:] == (0, WAVES_PER_BLOCK * 256 * 4), seen
    assert seen["k_prep_pixel"][1:] == (0, 0), seen
    assert seen["k_prep_apply"][1:] == (0, 0), seen
