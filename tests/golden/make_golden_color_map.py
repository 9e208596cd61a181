"""Writes tests/golden/golden_color_map.npz: what the colour half of addPointsToMap (lioOptimization.cpp:448-554) decides on the scene of
tests/color_checker.py (three batches, by recipe: seeds 9100 + j) for the four option sets -- per batch the outcome bytes, the visited
list and, per stored point, its batch index, point_index, slot and voxel key; per option set the final sizes.  Indices, flags and int16
keys only: the positions are the FP32 roundings of the inputs.  Recorded from the sequential restatement, which
tests/test_color_checker_reference.py holds against the reference's own translation units together with this file.

    python tests/golden/make_golden_color_map.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import color_checker as cc  # noqa: E402


def record():
    out = {}
    for o, opt in enumerate(cc.OPTION_SETS):
        chk = cc.ColorChecker(*opt)
        t = 1.0
        for j in range(3):
            outcome, stored, visited = chk.insert(cc.scene_batch(j), t)
            t += 1.0 + j
            assert np.abs(visited).max() < 32768 and stored["slot"].max() < 256
            out[f"o{o}_b{j}_outcome"] = outcome
            out[f"o{o}_b{j}_visited"] = visited.astype(np.int16)
            out[f"o{o}_b{j}_batch_index"] = stored["batch_index"]
            out[f"o{o}_b{j}_point_index"] = stored["point_index"]
            out[f"o{o}_b{j}_slot"] = stored["slot"].astype(np.uint8)
            out[f"o{o}_b{j}_keys"] = np.stack([stored["kx"], stored["ky"], stored["kz"]], 1)
        out[f"o{o}_sizes"] = np.array(chk.sizes(), dtype=np.int64)
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "golden_color_map.npz")
    np.savez_compressed(path, **record())
    print(path, os.path.getsize(path), "bytes")
