"""removePointsFarFromLocation (lioOptimization.cpp:556-572) on the device map: srl_map_remove_far.

The checker is a NumPy restatement of the rule on maps in creation order (oracle Map.export()): a voxel is erased iff its FIRST stored
point p0 (slot 0, FP32) satisfies ((dx dx + dy dy) + dz dz) > distance * distance with d = (double) p0 - location, in FP64.  The
survivors keep their creation order; the oracle's map after a prune is Map.import_() of the survivors, in that order.  Every comparison
of maps is bit for bit (keys, counts, xyz, order); passes on a pruned map must equal the oracle's passes on the imported survivors."""
import numpy as np
import pytest

import sr_livo_amd as srl
from sr_livo_amd import capi, synth
from test_gpu_bound_culling_sparse import _box_d2

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
K = 20
TIGHT = 1e-9          # test_gpu_parity.TIGHT: same algorithm in FP64, summation order only


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ------------------------------------------------------------------------------------------------ the rule, restated
def _sq(xyz, location):
    p0 = xyz[:, 0, :].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p0 - np.asarray(location, np.float64)
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def prune_keep(xyz, location, distance):
    """keep flag per voxel (creation order) of lioOptimization.cpp:556-572"""
    r = np.float64(distance)
    with np.errstate(invalid="ignore", over="ignore"):
        return ~(_sq(xyz, location) > r * r)


def _apply(k, c, x, location, distance):
    keep = prune_keep(x, location, distance)
    return (k[keep], c[keep], x[keep]), int((~keep).sum()), int(c[~keep].sum())


def _omap(po, backend, k, c, x):
    m = po.Map(backend)
    if len(c):
        m.import_(k, c, x)
    return m


def _check_map(ctx, k, c, x):
    kd, cd, xd = ctx.map_download()
    assert np.array_equal(kd, k) and np.array_equal(cd, c) and np.array_equal(xd, x)
    assert ctx.map_size() == (int(c.sum()), len(c))


def _prune_and_check(ctx, m, loc, dist):
    """prune the device map and the model; returns the model's map after the prune and the number of voxels removed"""
    m2, nv, npnt = _apply(*m, loc, dist)
    assert ctx.map_remove_far(loc, dist) == (nv, npnt)
    _check_map(ctx, *m2)
    return m2, nv


def _pass(ctx, raw, q, t, t_last, opts, frame_id=100):
    ctx.set_taps(1)
    neq, rc = ctx.build_residuals(capi.make_frame(q, t, t_last, frame_id=frame_id), opts)
    ids, status, ncand = ctx.fetch_neighbors(K=K)
    ctx.set_taps(0)
    return dict(neq=neq, rc=rc, ids=ids.copy(), status=status.copy(), ncand=ncand.copy())


def _check_vs_oracle(g, o):
    nv = o["neq"].num_visited
    assert g["neq"].last_visited == nv - 1
    bad = np.flatnonzero((g["ids"][:nv] != o["ids"][:nv]).any(1))
    assert bad.size == 0, ("ids", bad[:8])
    assert np.array_equal(g["status"][:nv], o["status"][:nv])
    assert int(g["ncand"][:nv].sum()) == o["neq"].sum_candidates
    assert g["neq"].num_residuals == o["neq"].num_residuals and g["neq"].success == o["neq"].success
    assert _rel(np.array(g["neq"].HtH).reshape(6, 6), o["HtH"]) < TIGHT and _rel(np.array(g["neq"].Hth), o["Hth"]) < TIGHT


def _same_pass(a, b):
    assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["status"], b["status"]) and np.array_equal(a["ncand"], b["ncand"])
    an, bn = a["neq"], b["neq"]
    assert (an.num_residuals, an.sum_candidates, an.last_visited, an.success) == (bn.num_residuals, bn.sum_candidates, bn.last_visited, bn.success)
    assert np.array_equal(np.array(an.HtH), np.array(bn.HtH)) and np.array_equal(np.array(an.Hth), np.array(bn.Hth)) and an.loss_sum == bn.loss_sum


@pytest.fixture(scope="module")
def scene(oracle_lib, oracle_backend):
    """a ~100k-point map as the device and the oracle build it, and a 4096-keypoint sweep over it"""
    pts, L = synth.map_candidates(931, 100_000)
    m = oracle_lib.Map(oracle_backend)
    m.add_points(pts)
    sweep = synth.make_sweep(932, 4096, L)
    world = synth.quat_to_rot(sweep["q_pred"]) @ sweep["raw"].T
    world = world.T + sweep["t_pred"]
    return dict(pts=pts, L=L, map=m.export(), sweep=sweep, world=world)


def _ctx_with(scene):
    ctx = srl.Context(0)
    ctx.map_insert(scene["pts"])
    return ctx


# ------------------------------------------------------------------------------------------------ 1. synthetic maps
@pytest.mark.parametrize("seed,n", [(941, 100_000), (942, 1_000_000)])
def test_prune_matches_the_model_on_synthetic_maps(oracle_lib, oracle_backend, seed, n):
    pts, L = synth.map_candidates(seed, n)
    om = oracle_lib.Map(oracle_backend)
    om.add_points(pts)
    m = om.export()
    ctx = srl.Context(0)
    try:
        ctx.map_insert(pts)
        _check_map(ctx, *m)
        p0 = m[2][:, 0].astype(np.float64)
        centre = p0.mean(0)
        d = np.sqrt(((p0 - centre) ** 2).sum(1))
        loc_half = centre + np.array([0.3, -0.7, 0.1]) * L * 0.1
        d_half = float(np.median(np.sqrt(((p0 - loc_half) ** 2).sum(1))))
        V0 = len(m[1])
        m, nv = _prune_and_check(ctx, m, centre, float(d.max()) * 1.01)          # nothing
        assert nv == 0 and len(m[1]) == V0
        m, nv = _prune_and_check(ctx, m, loc_half, d_half)                         # about half
        assert 0.3 * V0 < nv < 0.7 * V0
        m, nv = _prune_and_check(ctx, m, loc_half, 0.75 * d_half)                  # some more, on a renumbered map
        assert nv > 0 and len(m[1]) > 0
        m, nv = _prune_and_check(ctx, m, centre + 10 * L, 1.0)                     # everything
        assert nv > 0 and len(m[1]) == 0
        assert ctx.map_remove_far(centre, 0.0) == (0, 0)                           # an empty map
    finally:
        ctx.close()


@pytest.mark.parametrize("V", [200_000, 1_100_000])
def test_prune_of_maps_beyond_one_scan_launch(V):
    """more voxels than one launch of the scan covers (131 072: two launches; 1 M: the tile sums scanned themselves)"""
    rng = np.random.default_rng(V)
    side = int(np.ceil(V ** (1 / 3))) + 1
    cells = rng.permutation(side ** 3)[:V]
    keys = np.stack([cells % side, (cells // side) % side, cells // (side * side)], 1).astype(np.int16) - side // 2
    counts = rng.integers(1, 21, V).astype(np.int32)
    xyz = np.zeros((V, 20, 3), np.float32)
    base = keys.astype(np.float32) + np.where(keys >= 0, 0.5, -0.5).astype(np.float32)
    xyz[:] = base[:, None, :] + (rng.random((V, 20, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.8)
    xyz[np.arange(20)[None, :] >= counts[:, None]] = 0.0
    ctx = srl.Context(0)
    try:
        ctx.map_upload(keys, counts, xyz)
        m = (keys, counts, xyz)
        m, nv = _prune_and_check(ctx, m, [3.0, -2.0, 1.0], 0.8 * side / 2)
        assert 0 < nv < V
        m, nv = _prune_and_check(ctx, m, [-5.0, 4.0, 0.0], 0.5 * side / 2)
        assert nv > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the decision boundary
TRIPLES = [(3, 4, 0), (0, 3, 4), (4, 0, 3), (2, 3, 6), (6, 2, 3), (3, 6, 2), (1, 4, 8), (8, 1, 4), (4, 4, 7), (7, 4, 4)]     # 5, 7, 9


def _tie_scene(loc):
    """voxels whose first point lies EXACTLY at distance 5 s, 7 s or 9 s (s = 1/4, 1, 4) from loc (every sign), plus a voxel whose first
    point IS loc, voxels whose first point is inside while later points are outside, and the reverse.  Keys by truncation (voxel size 1);
    a candidate whose cell is taken already is dropped."""
    loc = np.asarray(loc, np.float64)
    cells, order = {}, []

    def add(points):
        p = np.asarray(points, np.float32)
        key = tuple(int(np.trunc(float(v))) for v in p[0])
        if key in cells or any(tuple(int(np.trunc(float(v))) for v in q) != key for q in p):
            return False
        cells[key] = p; order.append(key)
        return True

    add([loc])
    signs = [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    for s in (0.25, 1.0, 4.0):
        for tr in TRIPLES:
            for sg in signs:
                u = np.array(tr, np.float64) * np.array(sg) * s
                p0 = loc + u
                e = u / np.linalg.norm(u)
                # first point on the sphere, a later one 0.05 outside or inside (whichever stays in the cell)
                if not add([p0, p0 + 0.05 * e, p0 - 0.05 * e]):
                    add([p0])
    # first point inside by 1e-3, later points outside -- and the reverse -- at every tie radius
    for r in (1.25, 5.0, 20.0, 1.75, 7.0, 28.0, 2.25, 9.0, 36.0):
        for e in (np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0), np.array([-2.0, 1.0, -2.0]) / 3.0, np.array([0.0, -0.6, 0.8])):
            add([loc + (r - 1e-3) * e, loc + (r + 0.3) * e])
            add([loc + (r + 1e-3) * e, loc + (r - 0.3) * e])
    V = len(order)
    keys = np.array(order, np.int16)
    counts = np.array([len(cells[k]) for k in order], np.int32)
    xyz = np.zeros((V, 20, 3), np.float32)
    for v, k in enumerate(order):
        xyz[v, : counts[v]] = cells[k]
    return keys, counts, xyz


@pytest.mark.parametrize("loc", [(0.0, 0.0, 0.0), (-37.5, 12.25, -3.0), (0.5, -0.75, 0.25)])
def test_prune_decides_exact_ties_like_the_reference(loc):
    k, c, x = _tie_scene(loc)
    sq = _sq(x, loc)
    # exact ties really are in the scene (a radius whose tie cells the others took is left out: at most one of the nine)
    radii = [r for r in (1.25, 5.0, 20.0, 1.75, 7.0, 28.0, 2.25, 9.0, 36.0) if int(np.count_nonzero(sq == r * r)) >= 4]
    assert len(radii) >= 8, radii
    assert int(np.count_nonzero(sq == 0.0)) == 1
    assert np.any(k < 0) and np.any(x[:, 0] < 0) and np.any((x[:, 0] > -1) & (x[:, 0] < 1) & (x[:, 0] != 0))
    ctx = srl.Context(0)
    try:
        cases = []
        for r in radii:
            below, above = float(np.nextafter(r, 0.0)), float(np.nextafter(r, np.inf))
            cases += [(loc, r), (loc, below), (loc, above), (loc, -r), (loc, -below)]
        cases += [(loc, 0.0), (loc, -0.0), (loc, np.inf), (loc, -np.inf), (loc, np.nan), ((np.nan, loc[1], loc[2]), 5.0),
                  ((loc[0], loc[1], np.nan), 0.0)]
        removed = {}
        for cl, d in cases:
            ctx.map_upload(k, c, x)
            _, nv = _prune_and_check(ctx, (k, c, x), cl, d)
            removed[(cl is loc, d if d == d else "nan")] = nv
        for r in radii:
            below = float(np.nextafter(r, 0.0))
            assert removed[(True, below)] - removed[(True, r)] == int(np.count_nonzero(sq == r * r))    # the ties, and only they, go below r
            assert removed[(True, -r)] == removed[(True, r)]
        assert removed[(True, 0.0)] == len(c) - 1                                    # all but the voxel whose first point IS the location
        assert removed[(True, np.inf)] == removed[(True, -np.inf)] == removed[(True, "nan")] == 0
        assert removed[(False, 5.0)] == removed[(False, 0.0)] == 0                   # a NaN location erases nothing
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 3. search after a prune
def test_passes_on_a_pruned_map_equal_the_oracle_on_the_survivors(scene, oracle_lib, oracle_backend):
    sw = scene["sweep"]
    loc = sw["t_pred"] + np.array([2.0, -1.0, 0.5])
    dist = float(np.median(np.linalg.norm(scene["world"] - loc, axis=1)))
    ctx = _ctx_with(scene)
    up = srl.Context(0)
    try:
        ctx.sweep_upload(sw["raw"])
        om_full = _omap(oracle_lib, oracle_backend, *scene["map"])
        m, nv = _prune_and_check(ctx, scene["map"], loc, dist)
        assert nv > 0
        om = _omap(oracle_lib, oracle_backend, *m)
        up.map_upload(*m)
        up.sweep_upload(sw["raw"])
        for max_res, frame_id in ((INT_MAX, 100), (600, 100), (INT_MAX, 5)):
            opts = srl.default_opts(max_num_residuals=max_res)
            oo = oracle_lib.opts_from_product(opts)
            o = om.build_plane_residuals(oo, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"], frame_id=frame_id)
            g = _pass(ctx, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"], opts, frame_id)
            _check_vs_oracle(g, o)
            _same_pass(g, _pass(up, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"], opts, frame_id))     # = the survivors uploaded
            if max_res == INT_MAX and frame_id == 100:
                of = om_full.build_plane_residuals(oo, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"], frame_id=frame_id)
                lost = (of["ids"] != o["ids"]).any(1)
                assert int(lost.sum()) >= 50                                        # neighbourhoods that lost voxels to the prune
    finally:
        ctx.close()
        up.close()


# ------------------------------------------------------------------------------------------------ 4. insert after a prune
def test_insert_after_a_prune_recreates_erased_keys_at_the_end_and_grows(scene, oracle_lib, oracle_backend):
    pts = scene["pts"]
    ctx = _ctx_with(scene)
    try:
        p0 = scene["map"][2][:, 0].astype(np.float64)
        loc = p0.mean(0)
        m, nv = _prune_and_check(ctx, scene["map"], loc, float(np.median(np.linalg.norm(p0 - loc, axis=1))))
        erased_keys = set(map(tuple, scene["map"][0].tolist())) - set(map(tuple, m[0].tolist()))
        rng = np.random.default_rng(7)
        # (a) points of the erased voxels (their keys come back as NEW voxels, behind the survivors) and of surviving ones
        batch = pts[rng.choice(len(pts), 20_000, replace=False)] + rng.normal(0, 0.05, (20_000, 3))
        # (b) then enough new voxels to grow the slabs and the table: a far-away block, one point per 1 m voxel
        far = np.stack(np.meshgrid(np.arange(60), np.arange(60), np.arange(80), indexing="ij"), -1).reshape(-1, 3) + np.array([2000.5, 2000.5, 2000.5])
        om = _omap(oracle_lib, oracle_backend, *m)
        for b in (batch, far):
            before = om.size()
            om.add_points(b)
            assert ctx.map_insert(b) == om.size() - before
            _check_map(ctx, *om.export())
        k, _, _ = om.export()
        tail = set(map(tuple, k[len(m[1]):].tolist()))
        assert len(tail & erased_keys) > 100                                            # re-created at the end
        assert len(k) > 2 * len(scene["map"][1])
        m2, nv = _prune_and_check(ctx, om.export(), loc, 1e3)                           # the far block goes again
        assert nv == len(far)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. neighbourhood bounds
def _stale_bound_culls(keys_new, xyz_old, raw, pose_prev, ids_prev, pose, ids_new):
    """per keypoint: oracle neighbours of the pass on the pruned map at `pose` that lie in voxels beyond the radius the PREVIOUS pass's
    bounds (K-th neighbour on the map before the prune) plus the movement would allow -- what stale bounds would have culled"""
    def world(q, t):
        return raw @ synth.quat_to_rot(np.asarray(q) / np.linalg.norm(q)).T + np.asarray(t)
    flat_old = xyz_old.reshape(-1, 3).astype(np.float64)
    p_prev, p = world(*pose_prev), world(*pose)
    full = ids_prev.min(1) >= 0
    tau = np.full(len(raw), np.inf)
    tau[full] = ((flat_old[ids_prev[full, K - 1]] - p_prev[full]) ** 2).sum(1)
    qf = p.astype(np.float32).astype(np.float64)
    r = np.sqrt(tau) * 1.000001 + np.linalg.norm(qf - p_prev.astype(np.float32).astype(np.float64), axis=1) * 1.000001 + (1e-3 + 1e-6 * np.abs(qf).sum(1))
    vk = keys_new[np.maximum(ids_new, 0) // K]
    return ((_box_d2(vk, qf, 1.0) > (r * r * 1.00001)[:, None]) & (ids_new >= 0)).sum(1)


def test_bounds_of_the_pass_before_a_prune_are_not_used_after_it(scene, oracle_lib, oracle_backend):
    sw = scene["sweep"]
    loc = sw["t_pred"] + np.array([1.0, 2.0, 0.0])
    dist = float(np.median(np.linalg.norm(scene["world"] - loc, axis=1)))
    q = sw["q_pred"]
    pose1, pose2 = (q, sw["t_pred"]), (q, sw["t_pred"] + np.array([0.04, -0.03, 0.01]))
    opts = srl.default_opts(max_num_residuals=INT_MAX)
    runs = {}
    for culling in (1, 0):
        ctx = _ctx_with(scene)
        try:
            ctx.set_bound_culling(culling)
            ctx.sweep_upload(sw["raw"])
            p1 = _pass(ctx, sw["raw"], *pose1, sw["t_last"], opts)
            m, nv = _prune_and_check(ctx, scene["map"], loc, dist)
            p2 = _pass(ctx, sw["raw"], *pose2, sw["t_last"], opts)
            runs[culling] = (p1, p2, m)
        finally:
            ctx.close()
    _same_pass(runs[1][0], runs[0][0])
    _same_pass(runs[1][1], runs[0][1])
    p1, p2, m = runs[1]
    om = _omap(oracle_lib, oracle_backend, *m)
    o2 = om.build_plane_residuals(oracle_lib.opts_from_product(opts), sw["raw"], *pose2, sw["t_last"], frame_id=100)
    _check_vs_oracle(p2, o2)
    culled = _stale_bound_culls(m[0], scene["map"][2], sw["raw"], pose1, p1["ids"], pose2, o2["ids"])
    assert int(np.count_nonzero(culled)) > 0                                             # the stale bounds would have lost true neighbours


# ------------------------------------------------------------------------------------------------ 6. armed launches
class _EskfAdapter:
    def __init__(self, lio): self.lio = lio
    def set_noise(self, *a): self.lio.eskf_set_noise(*a)
    def scale_init_cov(self): self.lio.eskf_scale_init_cov()
    def init_imu(self, a, g): self.lio.eskf_init_imu(a, g)
    def predict(self, dt, a, g): self.lio.eskf_predict(dt, a, g)
    def get_state(self): return self.lio.eskf_get_state()
    def set_state(self, s): self.lio.eskf_set_state(s)


def test_a_prune_cancels_the_armed_launch_and_the_next_solve_equals_an_unarmed_one(scene):
    sw = scene["sweep"]
    lio = srl.Lio(0)
    try:
        lio.add_points_to_map(scene["pts"])
        prior_state = synth.eskf_prior(_EskfAdapter(lio), sw["q_pred"], sw["t_pred"], sw["vel"]).copy()
        prior_cov = lio.eskf_get_cov().copy()
        state0 = np.concatenate([sw["q_pred"], sw["t_pred"], sw["vel"], np.zeros(6)])
        lio.resident_sweep(sw["raw"])
        solve = lio.bound_solver(srl.default_opts(max_num_residuals=INT_MAX), prior_state, prior_cov, state0, sw["t_last"], 100, len(sw["raw"]))
        lio.ctx.set_armed_launch(2)
        solve(); solve()
        s0 = lio.ctx.arm_stats()
        loc = sw["t_pred"] + np.array([2.0, -1.0, 0.5])
        lio.remove_points_far_from_location(loc, float(np.median(np.linalg.norm(scene["world"] - loc, axis=1))))
        s1 = lio.ctx.arm_stats()
        # the launch left waiting behind the last pass (if any) is cancelled by the prune, not left to expire: nothing waits after it
        assert s1["expired"] == s0["expired"] and s1["armed"] == s0["armed"]
        assert s1["cancelled"] - s0["cancelled"] == s0["armed"] - s0["fired"] - s0["cancelled"]
        assert s1["armed"] == s1["fired"] + s1["cancelled"]
        rc, _, _ = solve(); got = solve.state.copy()
        assert rc == 0
        solve()
        assert np.array_equal(solve.state, got)
        lio.ctx.set_armed_launch(0)
        solve()
        assert np.array_equal(solve.state, got)
    finally:
        lio.close()


# ------------------------------------------------------------------------------------------------ 7. deferred commit
def test_a_prune_right_behind_a_deferred_commit_sees_the_settled_map(scene, oracle_lib, oracle_backend):
    sw = scene["sweep"]
    ctx = _ctx_with(scene)
    try:
        ctx.frame_upload(sw["raw"])
        world, added = ctx.frame_commit(sw["q_pred"], sw["t_pred"], want_world=True, want_added=False)
        assert added is None
        om = _omap(oracle_lib, oracle_backend, *scene["map"])
        om.add_points(world)
        loc = sw["t_pred"]
        m = om.export()
        _prune_and_check(ctx, m, loc, float(np.median(np.linalg.norm(m[2][:, 0].astype(np.float64) - loc, axis=1))))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 8. the replay driver, pruning
MAX_DISTANCE = 15.0


@pytest.mark.parametrize("mc", [capi.MC_CONSTANT_VELOCITY, capi.MC_IMU])
def test_replay_with_pruning_matches_the_reference_loop(oracle_lib, oracle_backend, mc):
    """test_gpu_parity.test_replay_driver_matches_reference_loop with the reference's commented-out call (lioOptimization.cpp:1032)
    restored: removePointsFarFromLocation(voxel_map, p_state->translation, max_distance) right after addPointsToMap, on both sides"""
    from replay_reference import OracleReplay

    class PruningReplay(OracleReplay):
        def __init__(self, *a, max_distance, **kw):
            super().__init__(*a, **kw)
            self.max_distance = max_distance
            self.pruned = []

        def process(self, ms, imu_states):
            info = super().process(ms, imu_states)
            if info["success"]:
                k, c, x = self.m.export()
                loc = info["state"][4:7].copy()
                keep = prune_keep(x, loc, self.max_distance)
                self.pruned.append(dict(xyz=x, loc=loc, removed=int((~keep).sum())))
                self.m = _omap(self.po, self.backend, k[keep], c[keep], x[keep])
            return info

    pts, L = synth.map_candidates(555, 60_000)
    meas, gt, _ = synth.make_sequence(31, 7, 24_000, L)
    oo = dict(init_voxel_size=0.2, init_sample_voxel_size=1.0, init_num_frames=6, num_for_initialization=10, voxel_size=0.2,
              sample_voxel_size=1.5, max_num_points_in_voxel=20, min_distance_points=0.1, motion_compensation=mc, initialization=0,
              point_time_enable=1, acc_cov=0.1, gyr_cov=0.1, b_acc_cov=1e-4, b_gyr_cov=1e-4)
    icp_p = srl.default_opts(max_num_residuals=600)
    ref = PruningReplay(oracle_lib, oracle_backend, oo, oracle_lib.opts_from_product(icp_p), max_distance=MAX_DISTANCE)
    lio = srl.Lio(0)
    try:
        lio.set_initial_flag(False)
        lio.set_odometry_options(icp=icp_p, **oo)
        processed = 0
        margins = []
        for i, ms in enumerate(meas):
            want = ref.run_measurement(ms)
            got = lio.run_measurement(ms["time_frame"], ms["imu_t"], ms["imu_acc"], ms["imu_gyr"], ms["pts_raw"], ms["pts_timestamp"],
                                      ms["time_sweep_begin"], ms["time_sweep_offset"])
            assert got["rc"] == 0
            assert got["processed"] == (want is not None) and got["initialized"] == ref.initial_flag
            assert got["index_frame"] == ref.index_frame
            if want is None:
                continue
            processed += 1
            assert got["success"] and want["success"]
            assert got["frame_points"] == want["frame_points"] and got["keypoints"] == want["keypoints"]
            assert got["iters"] == want["iters"] and got["num_residuals"] == want["num_residuals"]
            assert got["points_added"] == want["points_added"]
            assert _rel(got["state"], want["state"]) < 1e-9
            f = lio.last_frame(); fo = ref.frames[-1]
            assert _rel(f["raw_point"], fo["raw"]) < 1e-11 and _rel(f["imu_point"], fo["imu_point"]) < 1e-11
            assert _rel(f["point"], fo["point"]) < 1e-9
            assert _rel(lio.eskf_get_cov(), ref.e.get_cov()) < 1e-8
            # the insertion's decision boundaries, as in test_replay_driver_matches_reference_loop: (a) voxel seams, (b) FP32 rounding
            pd, ph = np.asarray(f["point"], np.float64), np.asarray(fo["point"], np.float64)
            delta = float(np.max(np.abs(pd - ph)))
            seam = float(np.min(np.abs(ph - np.round(ph))))
            f32 = ph.astype(np.float32)
            up = np.nextafter(f32, np.float32(np.inf)).astype(np.float64); dn = np.nextafter(f32, np.float32(-np.inf)).astype(np.float64)
            mid = np.minimum(np.abs(ph - 0.5 * (f32.astype(np.float64) + up)), np.abs(ph - 0.5 * (f32.astype(np.float64) + dn)))
            flips = int(np.count_nonzero(pd.astype(np.float32) != f32))
            assert seam > 100.0 * delta, (delta, seam)
            assert flips <= 3 and (flips == 0 or float(np.min(mid)) <= delta)
            # (c) the prune's sphere: no first point lies closer to it than the device / host location difference plus one FP32 ulp of a
            # stored first point (a counted flip) could move it -- the two sides erase the same voxels
            pr = ref.pruned[-1]
            loc_delta = float(np.max(np.abs(got["state"][4:7] - pr["loc"])))
            ulp = float(np.max(np.spacing(np.abs(pr["xyz"][:, 0]).astype(np.float32)))) if len(pr["xyz"]) else 0.0
            margin = float(np.min(np.abs(np.sqrt(_sq(pr["xyz"], pr["loc"])) - MAX_DISTANCE))) if len(pr["xyz"]) else np.inf
            assert margin > 100.0 * np.sqrt(3.0) * (loc_delta + ulp), (margin, loc_delta, ulp)
            margins.append((pr["removed"], margin, flips))
            lio.remove_points_far_from_location(got["state"][4:7], MAX_DISTANCE)
            assert lio.map_size() == ref.m.size()
        assert processed == ref.index_frame - 1 and processed >= 9
        print("voxels removed, distance of the nearest first point to the sphere, FP32 flips per frame:", margins)
        assert sum(1 for r_, _, _ in margins[1:] if r_ > 0) >= 2                             # the fixture prunes after the map exists
        total_flips = sum(m_[2] for m_ in margins)
        kg, cg, xg = lio.ctx.map_download(); ko, co, xo = ref.m.export()
        assert np.array_equal(kg, ko) and np.array_equal(cg, co)
        differ = xg != xo
        assert int(np.count_nonzero(differ)) <= total_flips
        if differ.any():
            assert np.all(np.abs(xg[differ].astype(np.float64) - xo[differ].astype(np.float64)) <= np.spacing(np.abs(xo[differ]))), "more than one FP32 ulp"
    finally:
        lio.set_initial_flag(False)
        lio.close()


# ------------------------------------------------------------------------------------------------ 9. empty cases
def test_empty_cases(scene, oracle_lib, oracle_backend):
    sw = scene["sweep"]
    ctx = srl.Context(0)
    lio = srl.Lio(0)
    try:
        assert ctx.map_remove_far([0.0, 0.0, 0.0], 1.0) == (0, 0)                            # no map yet
        assert ctx.map_size() == (0, 0)
        lio.remove_points_far_from_location([0.0, 0.0, 0.0], 1.0)
        assert lio.map_size() == 0
        ctx.map_insert(scene["pts"])
        m = scene["map"]
        assert ctx.map_remove_far(sw["t_pred"], -1.0) == (len(m[1]), int(m[1].sum()))       # everything
        assert ctx.map_size() == (0, 0)
        ctx.sweep_upload(sw["raw"])
        opts = srl.default_opts(max_num_residuals=INT_MAX)
        g = _pass(ctx, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"], opts)
        o = oracle_lib.Map(oracle_backend).build_plane_residuals(oracle_lib.opts_from_product(opts), sw["raw"], sw["q_pred"], sw["t_pred"],
                                                                   sw["t_last"], frame_id=100)
        assert g["neq"].success == 0 and o["neq"].success == 0
        _check_vs_oracle(g, o)
        assert ctx.map_remove_far(sw["t_pred"], 0.0) == (0, 0)                               # an emptied map
        ctx.map_insert(scene["pts"])                                                          # = a fresh build
        _check_map(ctx, *m)
    finally:
        ctx.close()
        lio.close()
