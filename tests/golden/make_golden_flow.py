"""Writes tests/golden/golden_flow.npz: what the reference's own LKOpticalFlowKernel::trackImage (src/lkpyramid.cpp compiled where it
lies against tests/stub_opencv_lk, driven by tests/flow_ref_reader.cpp) produces on the scenes of tests/flow_checker.py -- per scene the
level count L, per call a CRC-32 of every padded level and derivative, and for the tracking calls next_xy as raw float bits and the
status.  Results only; the images are generated, not stored.  The reference tree must be present.  Run from the repository root:
python tests/golden/make_golden_flow.py"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import flow_reader as fr  # noqa: E402

if __name__ == "__main__":
    out = os.path.join(HERE, "golden_flow.npz")
    with tempfile.TemporaryDirectory() as tmp:
        pack = fr.golden_pack(fr.build(os.path.join(tmp, "reader")))
    np.savez_compressed(out, **pack)
    print(out, os.path.getsize(out), "bytes")
