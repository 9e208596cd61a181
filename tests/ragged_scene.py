"""A map with RAGGED voxel occupancy, for the options the saturated maps of sr_livo_amd/synth.py cannot exercise.

synth.map_candidates() is built to saturate: almost every voxel of the map it gives holds 18..20 points, so
`threshold_voxel_occupancy` (searchNeighbors skips a voxel with fewer resident points, optimize.cpp:389) selects the same voxels at 1,
5 and 12.  Here the same candidates are thinned with a keep probability that varies smoothly over the footprint (period ~20 m: several
lobes on the smallest map), so the counts spread evenly over 1..20 and every threshold between 2 and 20 changes which voxels a keypoint
sees -- its neighbours, its candidate count P_k, whether it has a plane at all.

A plain helper module (no fixtures, no arithmetic of the hot path).  The preconditions the GPU tests rest on -- the histogram, the share
of keypoints a threshold changes, every status present, no NaN planarity, eigen gaps -- are asserted from the oracle alone in
tests/test_ragged_scene.py.
"""
import numpy as np

from sr_livo_amd import synth

INT_MAX = 2**31 - 1

# (map seed, target points, keypoints): the small scene rides on the seeds of conftest.small_scene, the large one on C1's size
SMALL = (777, 30_000, 2048)
LARGE = (4242, 100_000, 4096)

# icpOptions of odometryOptions::defaultRobustOutdoorLowInertia (parameters.cpp:51-68) that differ from the defaults the suite runs with
LOW_INERTIA = dict(threshold_voxel_occupancy=5, size_voxel_map=0.8, weight_alpha=0.8, weight_neighborhood=0.2, max_num_residuals=600)


def ragged_candidates(seed, target_points):
    """synth.map_candidates thinned by a smooth keep probability in [0.02, 1].  Returns (points in insertion order, half extent L)."""
    pts, L = synth.map_candidates(seed, target_points)
    rng = np.random.default_rng(seed + 99)
    ph = 0.5 * (1.0 + np.sin(0.35 * pts[:, 0]) * np.cos(0.27 * pts[:, 1]))
    keep = rng.uniform(0.0, 1.0, len(pts)) < 0.02 + 0.98 * ph**2
    return pts[keep], L


def ragged_scene(oracle_lib, backend, seed, target_points, n_keypoints, voxel_size=1.0):
    """The oracle's map of the thinned candidates (the sequential addPointsToMap at `voxel_size`) and a livox sweep over it."""
    pts, L = ragged_candidates(seed, target_points)
    m = oracle_lib.Map(backend)
    m.add_points(pts, voxel_size=voxel_size)
    sweep = synth.make_sweep(seed + 1, n_keypoints, L)
    keys, counts, xyz = m.export()
    return dict(map=m, keys=keys, counts=counts, xyz=xyz, sweep=sweep, L=L, candidates=pts, voxel_size=voxel_size)


def occupancy_histogram(counts, cap=20):
    """share of the voxels that hold c points, c = 0..cap"""
    return np.bincount(np.asarray(counts), minlength=cap + 1)[: cap + 1] / max(len(counts), 1)


def candidate_counts(keys, counts, world, size, nb, thr):
    """P_k by a plain count, independent of the device and of the oracle: the resident points of the (2 nb + 1)^3 voxels around
    key = static_cast<short>(p / size) (truncation toward zero, optimize.cpp:372-374) that hold at least `thr` points (:389)."""
    table = {(int(k[0]), int(k[1]), int(k[2])): int(c) for k, c in zip(keys, counts)}
    home = np.trunc(np.asarray(world, np.float64) / size).astype(np.int64).astype(np.int16)
    off = range(-nb, nb + 1)
    out = np.zeros(len(home), np.int32)
    for i, (kx, ky, kz) in enumerate(home.tolist()):
        tot = 0
        for dx in off:
            for dy in off:
                for dz in off:
                    c = table.get((kx + dx, ky + dy, kz + dz), 0)
                    if c >= thr and c > 0:
                        tot += c
        out[i] = tot
    return out


def oracle_reference(o):
    """pyoracle's build_plane_residuals result under the key names check_pass_against (tests/test_gpu_parity.py) reads"""
    ref = {f"x_one_{k}": v for k, v in o.items() if isinstance(v, np.ndarray)}
    ref.update(x_one_num_ties=o["neq"].num_ties, x_one_num_residuals=o["neq"].num_residuals, x_one_success=o["neq"].success,
               x_one_loss=o["neq"].loss_sum)
    return ref
