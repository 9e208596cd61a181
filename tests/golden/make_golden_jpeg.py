"""Writes tests/golden/golden_jpeg.npz: JPEG streams from Pillow's encoder and the pixels Pillow's decoder (libjpeg-turbo, its defaults)
gives for them, for the cases tests/jpeg_cases.py names.  Needs Pillow; the tests that read the file do not.
    python tests/golden/make_golden_jpeg.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpeg_cases as jc      # noqa: E402


def main():
    by_name = {c[0]: c for c in jc.grid()}
    out = {}
    for name in jc.golden_names():
        data = jc.make(by_name[name])
        out["jpeg_" + name] = np.frombuffer(data, np.uint8)
        out["bgr_" + name] = jc.pillow_decode(data)
    np.savez_compressed(jc.GOLDEN, **out)
    print(f"{len(out) // 2} cases, {os.path.getsize(jc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
