"""The CPU oracle against the reference's own translation units on every scene of tests/undistort_checker.py, bit for bit:
distortFrameByConstant, distortFrameByImu and transformAllImuPoint of src/utility.cpp compiled where they lie
(oracle/_ref/libref_path.so through oracle/pyref.py).  With this, what the device tests compare with bit for bit IS the reference, and
the oracle's error against the exact model (ORACLE_WORST) is the reference's own.  Skipped where the library is absent."""
import numpy as np
import pytest

import undistort_checker as uc
from oracle import pyoracle as po
from oracle import pyref as pr

pytestmark = pytest.mark.skipif(not pr.available(), reason="needs oracle/_ref/libref_path.so (the reference's translation units)")


def same_bits_or_both_nan(a, b):
    au, bu = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
    return bool(((au == bu) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("mode", [uc.MC_CONSTANT_VELOCITY, uc.MC_IMU])
def test_the_oracle_equals_the_reference_on_every_scene(oracle_backend, mode):
    """every scene in both modes, not only in its own"""
    R_il, t_il, scenes = uc.golden_load()
    nan_points = 0
    for sc in scenes:
        args = (sc["raw"], sc["rel"], sc["states"], sc["tfb"], mode, R_il, t_il)
        imu_o, _ = po.distort_frame(*args, imu_point_in=sc["sentinel"], backend=oracle_backend)
        imu_r = pr.distort_frame(*args, imu_point_in=sc["sentinel"])
        assert same_bits_or_both_nan(imu_o, imu_r), sc["name"]
        raw_o = po.transform_all_imu_point(imu_o, sc["states"], R_il, t_il, backend=oracle_backend)
        raw_r = pr.transform_all_imu_point(imu_r, sc["states"], R_il, t_il)
        assert same_bits_or_both_nan(raw_o, raw_r), sc["name"]
        nan_points += int(np.isnan(imu_o).any(axis=1).sum())
    assert nan_points == (2 if mode == uc.MC_CONSTANT_VELOCITY else 0)         # the NaN times of scenes i and s


def test_the_sentinel_through_transform_all_imu_point(oracle_backend):
    """MC_NONE: buildFrame calls neither distortFrame function; transformAllImuPoint runs on what imu_point held"""
    R_il, t_il, scenes = uc.golden_load()
    for sc in scenes:
        if sc["mode"] == uc.MC_NONE:
            assert np.array_equal(po.transform_all_imu_point(sc["sentinel"], sc["states"], R_il, t_il, backend=oracle_backend),
                                  pr.transform_all_imu_point(sc["sentinel"], sc["states"], R_il, t_il)), sc["name"]
