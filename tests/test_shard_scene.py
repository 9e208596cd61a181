"""What tests/test_gpu_sharded_stream.py rests on, proved from the oracle alone (no device): where every budget of
shard_scene.budgets() is spent, that every shard keeps accepted keypoints, and that the map edits change neighbourhoods in every shard
-- so that a stale neighbourhood bound on any rank would give other neighbours than a fresh search."""
import numpy as np
import pytest

import shard_scene as sc


@pytest.fixture(scope="module")
def world(oracle_lib, oracle_backend):
    cands, L = sc.map_points()
    m = oracle_lib.Map(oracle_backend)
    m.add_points(cands)
    return dict(map=m, cands=cands, L=L, po=oracle_lib, backend=oracle_backend)


def _pass(world, m, raw, pose, sw, max_res=sc.INT_MAX, **kw):
    po = world["po"]
    return m.build_plane_residuals(po.default_opts(max_num_residuals=max_res, **kw), raw, pose[0], pose[1], sw["t_last"])


def _accepted(status, n, nranks):
    return [int((status[b:b + c] == 2).sum()) for b, c in sc.ranges(n, nranks)]


def test_shard_range_is_the_librarys():
    import sr_livo_amd as srl
    for n in (0, 1, 2, 3, 4, 4095, 4096, sc.N_SMALL, sc.N_OTHER, sc.N_LARGE):
        for nranks in (1, 2, 3, 8):
            for rank in range(nranks):
                assert sc.shard_range(n, nranks, rank) == tuple(srl.shard_range(n, nranks, rank))
    assert [c for _, c in sc.ranges(sc.N_LARGE)] == [2333, 2334, 2334]
    assert [c for _, c in sc.ranges(4095, 2)] == [2047, 2048] and [c for _, c in sc.ranges(4096, 2)] == [2048, 2048]
    assert [[c for _, c in sc.ranges(n)] for n in sc.N_TINY] == [[0, 0, 1], [0, 1, 1], [1, 1, 1], [1, 1, 2]]
    assert [b for b, _ in sc.ranges(sc.N_LARGE)] != [b for b, _ in sc.ranges(sc.N_OTHER)]      # every range moves


@pytest.mark.parametrize("n,nranks", [(sc.N_LARGE, 3), (sc.N_SMALL, 3), (sc.N_OTHER, 3), (4095, 2), (4096, 2)])
def test_every_shard_holds_accepted_keypoints_at_every_pose(world, n, nranks):
    sw = sc.sweep(n, world["L"])
    kinds = set()
    for i, pose in enumerate(sc.poses(sw)):
        o = _pass(world, world["map"], sw["raw"], pose, sw)
        assert o["neq"].nan_error == 0
        acc = _accepted(o["status"], n, nranks)
        assert min(acc) >= 2, (i, acc)
        kinds |= set(np.unique(o["status"]).tolist())
        if i == 0 and n in sc.ACCEPTED:
            assert tuple(acc) == sc.ACCEPTED[n]
    assert {0, 2} <= kinds                       # keypoints without neighbours lie between the accepted ones: a count is not an index


@pytest.mark.parametrize("n", [sc.N_LARGE, sc.N_SMALL])
def test_the_budgets_land_where_the_gpu_test_says(world, n):
    sw = sc.sweep(n, world["L"])
    pose = sc.poses(sw)[0]
    full = _pass(world, world["map"], sw["raw"], pose, sw)["status"]
    a = sc.ACCEPTED[n]
    rng = sc.ranges(n)
    acc_idx = np.flatnonzero(full == 2)
    landed = {}
    for name, max_res, lift in sc.budgets(n):
        raw = sc.lifted(sw["raw"]) if lift else sw["raw"]
        o = _pass(world, world["map"], raw, pose, sw, max_res=max_res)
        stop = sc.spent_at(_pass(world, world["map"], raw, pose, sw)["status"], max_res)
        assert (o["neq"].num_visited - 1) == (stop if stop is not None else n - 1), name          # the model of the cut is the oracle's
        landed[name] = stop
    b0, c0 = rng[0]
    b1, c1 = rng[1]
    b2, c2 = rng[2]
    assert b0 <= landed["inside rank 0"] < acc_idx[a[0] - 1]                                      # 600: inside rank 0, not at its end
    assert landed["rank 0's last accepted"] == acc_idx[a[0] - 1] < b0 + c0                       # A_0: rank 0's last accepted keypoint
    assert landed["rank 1's first accepted"] == acc_idx[a[0]] >= b1                              # A_0 + 1: rank 1's first accepted
    assert b2 <= landed["inside rank 2"] < b2 + c2 and landed["inside rank 2"] == acc_idx[a[0] + a[1] + 4]
    assert landed["all accepted"] == acc_idx[-1] and sum(a) == len(acc_idx) <= n                 # can trigger (max <= n), never binds
    assert sc.owner(landed["first plane"], n) == 0
    assert landed["first plane in rank 1"] == sc.LIFT[n] and sc.owner(sc.LIFT[n], n) == 1
    assert landed["no cut"] is None
    assert all(a[r] < rng[r][1] for r in range(3))                                               # counts are not indices


def test_the_sums_of_init_mode_and_of_an_occupancy_threshold_have_support_in_every_shard(world):
    """init mode (frame_id 5: neighbourhood 2, threshold 1) on the synthetic map, threshold_voxel_occupancy = 5 on the ragged one"""
    import ragged_scene as rs
    po = world["po"]
    n = sc.N_SMALL
    sw = sc.sweep(n, world["L"])
    for pose in sc.poses(sw):
        o = world["map"].build_plane_residuals(po.default_opts(max_num_residuals=sc.INT_MAX), sw["raw"], pose[0], pose[1], sw["t_last"], frame_id=5)
        assert min(_accepted(o["status"], n, 3)) >= 2
    pts, L = rs.ragged_candidates(sc.MAP_SEED, sc.MAP_POINTS)
    assert L == world["L"]
    m = po.Map(world["backend"])
    m.add_points(pts)
    changed = 0
    for pose in sc.poses(sw):
        o5 = _pass(world, m, sw["raw"], pose, sw, threshold_voxel_occupancy=5)
        o1 = _pass(world, m, sw["raw"], pose, sw)
        assert min(_accepted(o5["status"], n, 3)) >= 2 and o5["neq"].nan_error == 0
        changed += int((o5["ids"] != o1["ids"]).any(1).sum())
    assert changed > 100                                                 # the threshold selects other voxels on this map


def test_the_map_edits_change_neighbourhoods_in_every_shard(world):
    po = world["po"]
    n = sc.N_LARGE
    sw = sc.sweep(n, world["L"])
    ps = sc.poses(sw)
    pose = ps[1]
    m = po.Map(world["backend"])
    m.add_points(world["cands"])
    _, _, x0 = m.export()
    pre = _pass(world, m, sw["raw"], pose, sw)
    # ---- the insertion
    assert m.add_points(sc.insert_points(sw, pose)) > 0
    k1, c1, x1 = m.export()
    post = _pass(world, m, sw["raw"], pose, sw)
    d0 = sc.kth_distance(pre["ids"], pre["point_world"], x0)
    d1 = sc.kth_distance(post["ids"], post["point_world"], x1)
    for b, c in sc.ranges(n):
        closer = d1[b:b + c] < d0[b:b + c]
        assert closer.sum() >= 1                                         # a K-th neighbour moved closer: the old bound is too wide, not wrong
        assert (post["ids"][b:b + c] != pre["ids"][b:b + c]).any(1).sum() >= 1       # post-edit ids differ from pre-edit ids (the control)
    # ---- the prune
    loc, dist = sc.prune_args(sw)
    keep = sc.prune_keep(x1, loc, dist)
    assert 0 < (~keep).sum() < len(keep)
    erased = np.zeros(len(keep) + 1, bool)
    erased[:-1] = ~keep
    vox = np.where(post["ids"] >= 0, post["ids"] // sc.CAP, len(keep))
    lost = erased[vox].any(1)
    m2 = po.Map(world["backend"])
    m2.import_(k1[keep], c1[keep], x1[keep])
    pruned = _pass(world, m2, sw["raw"], pose, sw)
    for b, c in sc.ranges(n):
        assert lost[b:b + c].sum() >= 1                                  # a keypoint of the shard had a neighbour in an erased voxel
        assert (pruned["status"][b:b + c] == 2).sum() >= 2
        # ... and the survivors are renumbered: a stale id would name another point
        assert (pruned["ids"][b:b + c] != post["ids"][b:b + c]).any(1).sum() >= 1
    # ---- the insertion that re-creates erased keys
    v0 = m2.num_voxels()
    assert m2.add_points(sc.reinsert_points(world["cands"])) > 0 and m2.num_voxels() > v0
    k3, _, _ = m2.export()
    old = {tuple(k) for k in k1[~keep].tolist()}
    assert any(tuple(k) in old for k in k3[v0:].tolist())                # erased keys come back, as new voxels at the end
    again = _pass(world, m2, sw["raw"], pose, sw)
    for b, c in sc.ranges(n):
        assert (again["ids"][b:b + c] != pruned["ids"][b:b + c]).any(1).sum() >= 1
