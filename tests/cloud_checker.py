"""What a map insertion stored, read off the oracle: the checker of srl_map_insert_report / srl_frame_commit_report.

The outcome of point i is NOT restated here: the batch goes into an oracle map ONE point at a time (oracle Map.add_points, pinned bitwise
to the reference's own addPointToMap, tests/test_cloud_checker_reference.py) and the outcome is what changed -- nothing stored: 0; stored
and the voxel count unchanged: 1 (appended to a voxel that existed, lioOptimization.cpp:428-429: the only place addPointToPcl is called
from); stored and one voxel more: 2 (the voxel's creator, :437-441, which the reference does not publish).  The cloud follows from the
outcomes in NumPy: the FP32 positions of the points with outcome 1 in batch order and intensity = 50 * (z - ref_z) in FP64, rounded once
(addPointToPcl, :1346-1355)."""
import numpy as np


def classify(m, xyz, voxel_size=1.0, cap=20, min_dist=0.15, min_num_points=0, only=None):
    """outcome byte per point of xyz (n x 3, FP64) inserted into the map-like object m (add_points / num_voxels) in batch order.
    only: the batch indices to insert and classify (ascending; the others keep 0 and are NOT inserted -- sound when they fall into other
    voxels, which addPointToMap treats independently)."""
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    out = np.zeros(len(xyz), np.uint8)
    voxels = m.num_voxels()
    for i in (range(len(xyz)) if only is None else only):
        stored = m.add_points(xyz[i:i + 1], voxel_size, cap, min_dist, min_num_points)
        now = m.num_voxels()
        assert stored in (0, 1) and now - voxels in (0, 1) and (stored or now == voxels), (i, stored, voxels, now)
        out[i] = 0 if stored == 0 else (1 if now == voxels else 2)
        voxels = now
    return out


def cloud_of(outcome, xyz, ref_z):
    """(m, 4) float32 rows x, y, z, intensity of the points with outcome 1, in batch order"""
    f = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3).astype(np.float32)[np.asarray(outcome) == 1]
    intensity = (50.0 * (f[:, 2].astype(np.float64) - np.float64(ref_z))).astype(np.float32)
    return np.column_stack([f, intensity]).astype(np.float32).reshape(-1, 4)


def voxel_keys(xyz, voxel_size=1.0):
    """int16 voxel key per point: short(float(p) / voxel_size) per axis (lioOptimization.cpp:403-405; C truncation towards zero)"""
    f = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3).astype(np.float32).astype(np.float64)
    return np.trunc(f / np.float64(voxel_size)).astype(np.int64).astype(np.int16)


def bits(a):
    """bit pattern view for bit-for-bit comparisons of float32 arrays (NaN-safe, -0.0 != +0.0)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
