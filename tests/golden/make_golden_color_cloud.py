"""Writes tests/golden/golden_color_cloud.npz: the coloured cloud the sequential restatement of tests/cloud_export_checker.py builds on the
render scene for three calls (cloud_export_checker.GOLDEN_CALLS: an early render ascending at one view, the last render as saveColorPoints
walks it at three views, and the observation-time cut) -- records, registered indices and totals.  Data only; the layout is
cloud_export_checker.golden_pack's.  Run from the repository root: python tests/golden/make_golden_color_cloud.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cloud_export_checker as ck  # noqa: E402

if __name__ == "__main__":
    out = os.path.join(HERE, "golden_color_cloud.npz")
    np.savez_compressed(out, **ck.golden_pack())
    print(out, os.path.getsize(out), "bytes")
