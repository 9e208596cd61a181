"""Scenes of tests/test_gpu_sharded_stream.py: sweeps, pose sequences, budgets and map edits for sharded contexts.

A plain helper module (no fixtures, no device, no arithmetic of the hot path).  What the GPU tests rest on -- where every budget is
spent, that every shard keeps accepted keypoints, that an insertion and a prune change neighbourhoods in every shard -- is proved from
the oracle alone in tests/test_shard_scene.py; the numbers the GPU tests need from that proof (accepted keypoints per rank at the first
pose) are the constants ACCEPTED below, which that test recomputes.

Sizes are the smallest at which the paths differ: three ranks make every range ragged; 7 001 keypoints give shards of 2 333 / 2 334 /
2 334 (sixteen-wave workgroups, fused when no taps and no cut), 3 001 give four-wave unfused passes; two ranks over 4 095 keypoints put
one rank on either side of the 2 048-keypoint line (2 047 / 2 048), 4 096 put both above it; 1 ... 4 keypoints over three ranks leave
ranks empty."""
import numpy as np

from sr_livo_amd import synth

INT_MAX = 2**31 - 1
K = 20
CAP = 20

MAP_SEED = 5101
MAP_POINTS = 60_000
G = 3
N_LARGE = 7001            # sixteen-wave shards
N_SMALL = 3001            # four-wave shards
N_OTHER = 6998            # uploaded over N_LARGE: every range moves
N_SPLIT = (4095, 4096)    # two ranks: 2 047 | 2 048 and 2 048 | 2 048
N_TINY = (1, 2, 3, 4)     # three ranks, some of them empty
LIFT = {N_LARGE: 37 + 2400, N_SMALL: 37 + 1067}     # keypoints lifted out of the map's reach: the `-1` budget's stop keypoint lives in rank 1
SWEEP_SEED = 5200

# accepted keypoints (status 2) of rank 0, 1, 2 at the first pose of poses(): proved in tests/test_shard_scene.py
ACCEPTED = {N_LARGE: (2121, 2122, 2122), N_SMALL: (909, 909, 910)}


def shard_range(n, nranks, rank):
    """srl_shard_range, restated"""
    b = rank * n // nranks
    return b, (rank + 1) * n // nranks - b


def ranges(n, nranks=G):
    return [shard_range(n, nranks, r) for r in range(nranks)]


def map_points():
    """(candidates in insertion order, half extent)"""
    return synth.map_candidates(MAP_SEED, MAP_POINTS)


def sweep(n, L, seed=None):
    """a livox sweep over the map; every eleventh keypoint is moved out of the map's reach (no neighbours: status 0), so that accepted
    counts differ from keypoint counts and a budget's keypoint is not simply its index"""
    sw = dict(synth.make_sweep((SWEEP_SEED + n) if seed is None else seed, n, L))
    raw = sw["raw"].copy()
    raw[5::11] = raw[5::11] + np.array([0.0, 0.0, 900.0])
    sw["raw"] = raw
    return sw


def poses(sw, count=5, seed=1, jump=3):
    """_poses of tests/test_gpu_bound_culling.py: consecutive ESIKF iterations moving towards the ground truth, one far jump in between"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count - (1 if jump is not None else 0)):
        a = 0.7 ** k
        q = synth.quat_mul(sw["q_gt"], synth.quat_from_rotvec(a * rng.normal(0, 0.004, 3)))
        t = sw["t_gt"] + a * (sw["t_pred"] - sw["t_gt"]) + rng.normal(0, 1e-4, 3)
        out.append((q, t))
    if jump is not None:
        out.insert(jump, (synth.quat_mul(sw["q_gt"], synth.quat_from_rotvec([0.0, 0.0, 0.3])), sw["t_gt"] + np.array([1.5, -0.7, 0.2])))
    return out


def lifted(raw):
    """the sweep with its first LIFT[n] keypoints out of the map's reach (test_class_default_max_num_residuals_stops_at_the_first_...)"""
    out = raw.copy()
    count = LIFT[len(raw)]
    out[:count] = out[:count] + np.array([0.0, 0.0, 900.0])
    return out


def budgets(n):
    """(name, max_num_residuals, lifted sweep?) of every budget regime, from the accepted counts at the first pose"""
    a = ACCEPTED[n]
    return [("inside rank 0", 600, False),
            ("rank 0's last accepted", a[0], False),
            ("rank 1's first accepted", a[0] + 1, False),
            ("inside rank 2", a[0] + a[1] + 5, False),
            ("all accepted", sum(a), False),
            ("first plane", -1, False),
            ("first plane in rank 1", -1, True),
            ("no cut", INT_MAX, False)]


def spent_at(status, max_res):
    """index of the keypoint at which the sequential loop stops (optimize.cpp:107), or None when it runs to the end: the max_res-th
    accepted keypoint; max_res <= 0: the first keypoint with a plane (status 1 or 2)"""
    status = np.asarray(status)
    hits = np.flatnonzero(status == 2) if max_res > 0 else np.flatnonzero((status == 1) | (status == 2))
    want = max_res if max_res > 0 else 1
    return int(hits[want - 1]) if len(hits) >= want else None


def owner(index, n, nranks=G):
    for r, (b, c) in enumerate(ranges(n, nranks)):
        if b <= index < b + c:
            return r
    return None


# ------------------------------------------------------------------------------------------------ map edits
def insert_points(sw, pose):
    """the construction of test_a_map_change_or_another_sweep_voids_the_bounds: every seventh keypoint at `pose`, 2 cm above itself
    (its K-th neighbour moves closer) and in a voxel beside it (a voxel that was empty or sparse fills up)"""
    q, t = pose
    R = synth.quat_to_rot(np.asarray(q) / np.linalg.norm(q))
    world = sw["raw"][::7] @ R.T + t
    return np.concatenate([world + np.array([0.0, 0.0, 0.02]), world + np.array([1.2, 0.0, 0.6])])


PRUNE_DISTANCE = 14.0


def prune_args(sw):
    """(location, distance) of the prune: everything farther than PRUNE_DISTANCE from the sensor goes"""
    return np.asarray(sw["t_gt"], np.float64).copy(), PRUNE_DISTANCE


def prune_keep(xyz, location, distance):
    """keep flag per voxel (creation order) of removePointsFarFromLocation (lioOptimization.cpp:556-572), restated: a voxel goes iff its
    first stored point (FP32) lies farther than distance from location, in FP64 with the sum ((dx dx + dy dy) + dz dz)"""
    d = xyz[:, 0, :].astype(np.float64) - np.asarray(location, np.float64)
    return ~(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > np.float64(distance) * np.float64(distance))


def reinsert_points(cands):
    """candidates of the original map: those whose voxel the prune erased re-create it, the others meet their own copies"""
    return cands[::2]


def search_batch(sw, pose, count=257):
    """a fixed batch of world points for srl_search_neighbors: keypoints at `pose`, and a few far outside the map"""
    q, t = pose
    R = synth.quat_to_rot(np.asarray(q) / np.linalg.norm(q))
    world = sw["raw"][:: max(len(sw["raw"]) // count, 1)][:count] @ R.T + t
    return np.concatenate([world, world[:5] + np.array([0.0, 0.0, 500.0])])


def kth_distance(ids, point_world, map_xyz):
    """distance of every keypoint's farthest listed neighbour (NaN without a full row)"""
    flat = np.asarray(map_xyz, np.float64).reshape(-1, 3)
    out = np.full(len(ids), np.nan)
    full = ids.min(axis=1) >= 0
    d = flat[ids[full]] - point_world[full][:, None, :]
    out[full] = np.sqrt((d * d).sum(-1)).max(-1)
    return out
