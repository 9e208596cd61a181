"""Writes tests/golden/golden_color_track.npz: what the sequential restatement of tests/track_checker.py makes of the tracker's point set
over the fixed sequence of calls on the scene of the tests (track_checker.cases) -- per call the records, both outcome arrays and the
totals.  Data only; the layout is track_checker.golden_pack's.  Run from the repository root: python tests/golden/make_golden_color_track.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import track_checker as tk  # noqa: E402

if __name__ == "__main__":
    out = os.path.join(HERE, "golden_color_track.npz")
    np.savez_compressed(out, **tk.golden_pack())
    print(out, os.path.getsize(out), "bytes")
