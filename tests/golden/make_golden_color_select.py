"""Writes tests/golden/golden_color_select.npz: what the sequential restatement of tests/select_checker.py selects for projection on the
scenes of the tests -- the list-mode sequence over render_checker's poses (every parameter set, both margins, both image sizes), the
all-points calls on the map of three and of four insertions, and the two thin shells -- as totals and records.  Data only; the layout is
select_checker.golden_pack's.  Run from the repository root: python tests/golden/make_golden_color_select.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import select_checker as sk  # noqa: E402

if __name__ == "__main__":
    out = os.path.join(HERE, "golden_color_select.npz")
    np.savez_compressed(out, **sk.golden_pack())
    print(out, os.path.getsize(out), "bytes")
