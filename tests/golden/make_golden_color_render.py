"""Writes tests/golden/golden_color_render.npz: the per-point colour state (rgb, N_rgb, cov_rgb, observe_distance, last_observe_time) after
every render of the sequence of tests/render_checker.py (option set 0, both image sizes, six poses and times), in the order
srl_color_map_download_rgb gives it, and the totals of every render -- as the sequential restatement computes them.  Data only; the
layout is render_checker.golden_pack's.  Run from the repository root: python tests/golden/make_golden_color_render.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import render_checker as rc  # noqa: E402

if __name__ == "__main__":
    _, totals, map_states, _ = rc.scene_sequence()
    out = os.path.join(HERE, "golden_color_render.npz")
    np.savez_compressed(out, **rc.golden_pack(totals, map_states))
    print(out, os.path.getsize(out), "bytes")
