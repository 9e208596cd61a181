"""Writes tests/golden/golden_color_vio.npz: what the sequential restatement of tests/vio_checker.py computes for the measurement loops
of vioEsikf and vioPhotometric on the scenes of the tests -- both image sizes, both modes, the four estimate_* combinations -- as the
tracked lists, the outcomes, the in-order sums and a CRC-32 of the rows; and the per-iteration states and final covariances of vioEsikf
then vioPhotometric as tests/vio_ref_reader.cpp runs them (the reference's own pieces, the explicit K on the stand-in Eigen), for which
oracle/_ref and the reference tree must be present.  Data only; the layout is vio_checker.golden_pack's and golden_pack_reader's.  Run from
the repository root: python tests/golden/make_golden_color_vio.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import tempfile  # noqa: E402

import vio_checker as vc  # noqa: E402
import vio_reader as vr  # noqa: E402

if __name__ == "__main__":
    out = os.path.join(HERE, "golden_color_vio.npz")
    with tempfile.TemporaryDirectory() as tmp:
        reader = vc.golden_pack_reader(vr.build(os.path.join(tmp, "reader")))
    np.savez_compressed(out, **vc.golden_pack(), **reader)
    print(out, os.path.getsize(out), "bytes")
