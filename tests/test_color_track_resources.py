"""Build-time guard for the kernels of the tracker's point-set update (CPU-only: hipcc cross-compiles gfx950), in the manner of
tests/test_color_select_resources.py: no kernel of srl_color_track.hip uses scratch; the per-point kernels (k_track_file, k_track_old,
k_track_cand, k_track_count) keep the register budget of eight waves per SIMD (64 VGPRs; recorded at 10 / 38 / 20 / 44) and hold no LDS
beyond the counter reduction of k_track_old (100 bytes: four waves x six counters, and the ticket's flag) and k_track_count (116 bytes:
four waves x seven counters); the shared scan kernels keep theirs (24 VGPRs, 128 bytes; their tile sums 17 VGPRs, 64 bytes)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_POINT = ("k_track_file", "k_track_old", "k_track_cand", "k_track_count")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_track_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_color_track.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "k.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen, scans = {}, {}
    for b in re.split(r"remark: Function Name: ", out)[1:]:
        name = b.split()[0]
        vg = int(re.search(r"VGPRs: (\d+)", b).group(1))
        sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        for k in PER_POINT:
            if k in name:
                seen[k] = (vg, sc, lds)
        if "k_scan_small" in name or "k_scan_tile_sums" in name:
            scans[name] = (vg, sc, lds)
    assert set(seen) == set(PER_POINT), out[-2000:]
    assert sum(1 for n in scans if "Track" in n) == 4                   # the kept points' scan and the winners' scan, each with its tile sums
    print("VGPRs / scratch / LDS:", seen, {n[:70]: v for n, v in scans.items() if "Track" in n})
    for k, (vg, sc, lds) in {**seen, **scans}.items():
        assert sc == 0, (k, sc)
    for k, (vg, sc, lds) in seen.items():
        assert vg <= 64, (k, vg)
    assert seen["k_track_file"][2] == 0 and seen["k_track_cand"][2] == 0
    assert seen["k_track_old"][2] <= 4 * 6 * 4 + 4 and seen["k_track_count"][2] <= 4 * 7 * 4 + 4      # the totals reduction alone
    assert all(lds <= 128 for _, _, lds in scans.values())
