"""Writes tests/golden/golden_undistort_edges.npz and its further parts (_part2, _part3, ...: every file stays below the size limit of a
committed file): for every scene of tests/undistort_checker.py the inputs, the branch every point takes and the exact imu_point and
raw_point of the mpmath model as a double hi + lo pair.  Data only, made from the checker's scenes and its model; the layout is
undistort_checker.golden_pack's, the bytes depend on the arrays alone.  Run from the repository root:
python tests/golden/make_golden_undistort.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import undistort_checker as uc  # noqa: E402

if __name__ == "__main__":
    for old in uc.golden_paths():
        os.remove(old)
    for k, part in enumerate(uc.golden_pack(), 1):
        out = os.path.join(HERE, uc.GOLDEN_STEM + (".npz" if k == 1 else "_part%d.npz" % k))
        uc.save_npz_reproducibly(out, part)
        print(out, os.path.getsize(out), "bytes")
