"""Build-time guard for the kernels of srl_consensus.hip (CPU-only: hipcc cross-compiles gfx950), in the manner of
tests/test_color_track_resources.py; it reads the compiler's resource remarks and nothing else.

Recorded (VGPRs / scratch bytes per lane / LDS bytes per block), fundamental then PnP:
  k_cons_prep    38 / 0 / 8208      19 / 0 / 16        (the four-value block sum of Hartley's normalisation; the wave counts alone)
  k_cons_hyp     92 / 0 / 41472    122 / 0 / 0         (64 lanes x 81 doubles of lane-interleaved 7 x 9 systems; P3P keeps its roots in
                                                         fixed slots and writes each accepted pose straight to its global slot, so
                                                         nothing is indexed at run time in a per-lane array)
  k_cons_score   64 / 0 / 16384     66 / 0 / 20480     (= the staged chunk: 1024 points x 4 or 5 floats)
  k_cons_pick    46 / 0 / 3088      40 / 0 / 3088      (three 256-entry reduction arrays and four wave counts)
Asserted: the scoring and pick kernels use no scratch, the scoring kernels' LDS is exactly the staged chunk of points, the pick
kernels' LDS is their reduction arrays.  The solver kernels are only recorded (neither uses scratch as compiled now)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1024                        # CONS_CHUNK of srl_consensus.hip
FLOATS = {0: 4, 1: 5}               # per staged point: (x1, y1, x2, y2) / (X, Y, Z, u, v)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_scoring_and_pick_kernels_have_no_scratch_and_stage_one_chunk(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_consensus.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / "k.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen = {}
    for b in re.split(r"remark: Function Name: ", out)[1:]:
        name = b.split()[0]
        m = re.search(r"(k_cons_[a-z]+)ILi([01])E", name)
        if not m:
            continue
        vg = int(re.search(r"VGPRs: (\d+)", b).group(1))
        sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        seen[(m.group(1), int(m.group(2)))] = (vg, sc, lds)
    assert set(seen) == {(k, m) for k in ("k_cons_prep", "k_cons_hyp", "k_cons_score", "k_cons_pick") for m in (0, 1)}, out[-2000:]
    print("VGPRs / scratch / LDS:", seen)
    for model in (0, 1):
        vg, sc, lds = seen[("k_cons_score", model)]
        assert sc == 0 and lds == CHUNK * FLOATS[model] * 4, (model, vg, sc, lds)
        vg, sc, lds = seen[("k_cons_pick", model)]
        assert sc == 0 and lds == 3 * 256 * 4 + 4 * 4, (model, vg, sc, lds)
        assert seen[("k_cons_prep", model)][1] == 0
