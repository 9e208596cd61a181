"""Build-time guard for the selection kernels (CPU-only: hipcc cross-compiles gfx950), in the manner of tests/test_color_render_resources.py:
no kernel of srl_color_select.hip uses scratch; the per-candidate kernels (k_select_tails, k_select_lookup, k_select_cells, k_select_file)
keep the register budget of eight waves per SIMD (64 VGPRs; recorded at 6 / 11 / 26 / 8) and hold no LDS beyond the counter reduction of
k_select_cells; the shared scan kernels keep theirs."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_CANDIDATE = ("k_select_tails", "k_select_lookup", "k_select_cells", "k_select_file")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_select_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_color_select.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "k.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen, scans = {}, {}
    for b in re.split(r"remark: Function Name: ", out)[1:]:
        name = b.split()[0]
        vg = int(re.search(r"VGPRs: (\d+)", b).group(1))
        sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        for k in PER_CANDIDATE:
            if k in name:
                seen[k] = (vg, sc, lds)
        if "k_scan_small" in name or "k_scan_tile_sums" in name:
            scans[name] = (vg, sc, lds)
    assert set(seen) == set(PER_CANDIDATE), out[-2000:]
    assert sum(1 for n in scans if "Select" in n) == 4                  # the compaction and the holder scan, each with its tile sums
    print("VGPRs / scratch / LDS:", seen, {n[:60]: v for n, v in scans.items() if "Select" in n})
    for k, (vg, sc, lds) in {**seen, **scans}.items():
        assert sc == 0, (k, sc)
    for k, (vg, sc, lds) in seen.items():
        assert vg <= 64, (k, vg)
    assert all(seen[k][2] == 0 for k in ("k_select_tails", "k_select_lookup", "k_select_file"))
    assert seen["k_select_cells"][2] <= 128             # four waves x four counters, and the ticket's flag
    assert all(lds <= 128 for _, _, lds in scans.values())
