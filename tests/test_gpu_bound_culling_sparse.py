"""Neighbourhood bounds on SPARSE maps, where the K-th neighbour of a keypoint lies about one voxel edge away or further.

A pass that starts from the previous pass's bounds (SrlAssocArgs::bound_in) skips the voxels further from the keypoint than
r = sqrt(tau) + |p_w - p_w_prev| + slack.  That is exact only while the previous pass's K neighbours are still candidates: searchNeighbors
(optimize.cpp:365-426) visits the (2 NB + 1)^3 voxels around the keypoint's CURRENT voxel, so a keypoint that crosses a voxel face can
lose its old neighbours with the layer it leaves, and its true K nearest inside the new region may lie beyond r.  Every test here builds
scenes where exactly that happens, proves it with a NumPy model of the plain rule (_plain_rule_drops), and asserts that every pass
equals the oracle at that pose (ids, status, candidate counts exactly; normal equations to the parity tolerance) and equals the same
passes without the bounds bit for bit:
  a. crafted r = 1 crossings: every axis, both directions, negative coordinates, the truncation seam at 0 (key 0 spans (-1, 1)),
     voxel sizes 0.5 / 1 / 1.5, finite and unlimited residual budgets; per launch a PAIR of keypoints (the pair path) and a single
     one (the odd keypoint), one of the pair keeping some but fewer than K candidates under the plain rule;
  b. the same in init mode (r = 2, frame_id < init_num_frames), the neighbours two layers away;
  c. randomised sparse maps (small clusters in one voxel of eight), 16k keypoints, pose steps of 0.05 ... 0.6 m;
  d. full ESIKF solves on a thinned map: states and covariances with and without the bounds bit for bit, and the oracle's."""
import numpy as np
import pytest

import sr_livo_amd as srl
from sr_livo_amd import capi, synth
from test_gpu_eigen_stress import _voxelise

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
K = 20
TIGHT = 1e-9          # test_gpu_parity.TIGHT: same algorithm in FP64, summation order only
T_LAST = np.array([0.0, 0.0, 30.0])


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ------------------------------------------------------------------------------------------------ the plain rule, restated
def _box_d2(keys, q, size):
    """squared distance of FP32 queries q (n, 3) to the boxes of voxel keys (n, ..., 3), the truncation-toward-zero boxes of
    probe_finish: v > 0: [v, v + 1), v < 0: (v - 1, v], v = 0: (-1, 1), times the voxel size"""
    v = keys.astype(np.int64)
    lo = np.where(v > 0, v, v - 1) * size
    hi = np.where(v < 0, v, v + 1) * size
    qq = q.reshape(q.shape[:1] + (1,) * (v.ndim - 2) + (3,))
    d = np.maximum(np.maximum(lo - qq, qq - hi), 0.0)
    return (d * d).sum(-1)


def _world(raw, q, t):
    return raw @ synth.quat_to_rot(np.asarray(q) / np.linalg.norm(q)).T + np.asarray(t)


def _plain_rule_drops(keys, xyz, size, raw, pose_prev, ids_prev, pose, ids):
    """Per keypoint: how many of the oracle's neighbours `ids` at `pose` lie in voxels that the plain rule -- the squared cull radius of
    the previous pass's K-th neighbour distance plus the movement, no condition on the region -- would let this pass skip (-1 where the
    previous pass had fewer than K neighbours: no bound)."""
    flat = xyz.reshape(-1, 3).astype(np.float64)
    p_prev = _world(raw, *pose_prev)
    p = _world(raw, *pose)
    full_prev = ids_prev.min(1) >= 0
    tau = np.full(len(raw), np.inf)
    tau[full_prev] = ((flat[ids_prev[full_prev, K - 1]] - p_prev[full_prev]) ** 2).sum(1)
    qf = p.astype(np.float32).astype(np.float64)
    bf = p_prev.astype(np.float32).astype(np.float64)
    mag = np.abs(qf).sum(1)
    r = np.sqrt(tau) * 1.000001 + np.linalg.norm(qf - bf, axis=1) * 1.000001 + (1e-3 + 1e-6 * mag)
    r2 = r * r * 1.00001
    vk = keys[np.maximum(ids, 0) // K]                                  # (n, K, 3): the voxel of every neighbour
    drop = (_box_d2(vk, qf, size) > r2[:, None]) & (ids >= 0)
    return np.where(full_prev, drop.sum(1), -1)


# ------------------------------------------------------------------------------------------------ passes: device and oracle
def _oracle_passes(oracle_lib, oracle_backend, keys, counts, xyz, raw, poses, opts, frame_id):
    m = oracle_lib.Map(oracle_backend)
    m.import_(keys, counts, xyz)
    oo = oracle_lib.opts_from_product(opts)
    return [m.build_plane_residuals(oo, raw, q, t, T_LAST, frame_id=frame_id) for q, t in poses]


def _device_passes(ctx, raw, poses, opts, frame_id, culling, armed):
    ctx.set_armed_launch(armed)
    ctx.set_bound_culling(culling)
    ctx.sweep_upload(raw)                 # a new sweep: no bounds from earlier runs
    ctx.set_taps(1)
    out = []
    for q, t in poses:
        neq, rc = ctx.build_residuals(capi.make_frame(q, t, T_LAST, frame_id=frame_id), opts)
        ids, status, ncand = ctx.fetch_neighbors(K=K)
        out.append(dict(neq=neq, ids=ids.copy(), status=status.copy(), ncand=ncand.copy()))
    ctx.set_taps(0)
    ctx.set_armed_launch(1)
    return out


def _check_passes(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses, opts, frame_id=100):
    """every pass against the oracle; bounds on (plain and armed launches) against bounds off, bit for bit.  Returns the oracle's passes."""
    ctx.map_upload(keys, counts, xyz)
    orc = _oracle_passes(oracle_lib, oracle_backend, keys, counts, xyz, raw, poses, opts, frame_id)
    ref = _device_passes(ctx, raw, poses, opts, frame_id, 0, 0)
    for k, (g, o) in enumerate(zip(ref, orc)):
        nv = o["neq"].num_visited                   # a finite budget: the reference's loop stops at the residual that fills it
        assert g["neq"].last_visited == nv - 1, ("last_visited", k)
        bad = np.flatnonzero((g["ids"][:nv] != o["ids"][:nv]).any(1))
        assert bad.size == 0, ("ids", k, bad[:8])
        assert np.array_equal(g["status"][:nv], o["status"][:nv]), ("status", k)
        # P_k of the keypoints the reference visited; the device's total counts every keypoint of the pass (finite budgets: all of them)
        assert int(g["ncand"][:nv].sum()) == o["neq"].sum_candidates and int(g["ncand"].sum()) == g["neq"].sum_candidates, ("sum_candidates", k)
        assert g["neq"].num_residuals == o["neq"].num_residuals, ("num_residuals", k)
        assert _rel(np.array(g["neq"].HtH).reshape(6, 6), o["HtH"]) < TIGHT and _rel(np.array(g["neq"].Hth), o["Hth"]) < TIGHT, k
    for armed in (0, 2):
        got = _device_passes(ctx, raw, poses, opts, frame_id, 1, armed)
        for k, (g, r, o) in enumerate(zip(got, ref, orc)):
            what = (armed, k)
            # the oracle first: a pass that skipped a voxel holding one of the K nearest shows here by name
            nv = o["neq"].num_visited
            lost = np.flatnonzero((g["ids"][:nv] != o["ids"][:nv]).any(1))
            assert lost.size == 0, ("ids differ from the oracle", what, lost[:8], g["ncand"][lost[:8]])
            assert np.array_equal(g["status"][:nv], o["status"][:nv]), what
            assert np.array_equal(g["ids"], r["ids"]) and np.array_equal(g["status"], r["status"]) and np.array_equal(g["ncand"], r["ncand"]), what
            gn, rn = g["neq"], r["neq"]
            assert gn.num_residuals == rn.num_residuals and gn.sum_candidates == rn.sum_candidates and gn.last_visited == rn.last_visited, what
            assert np.array_equal(np.array(gn.HtH), np.array(rn.HtH)) and np.array_equal(np.array(gn.Hth), np.array(rn.Hth)), what
            assert gn.loss_sum == rn.loss_sum, what
    return orc


@pytest.fixture(scope="module")
def ctx():
    c = srl.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ a. / b. crafted crossings
def _centre(v):
    return v + 0.5 if v > 0 else (v - 0.5 if v < 0 else 0.0)


def _crossing_cell(rng, F, NB, y0, z0, partial):
    """One keypoint in voxel units (canonical frame: it crosses the face x = F from key F into key F - 1, y / z keys y0 / z0).
    Pass 1 probes the x layers F - NB ... F + NB and finds its K nearest on a plane in layer F + NB (distance NB - 0.01; five more
    points there a little further keep P_k > K).  Pass 2 probes F - 1 - NB ... F + NB - 1: the plane's layer is gone, the new layer
    holds 20 points in the voxel (F - 1 - NB, y0 + NB, z0 + NB), whose box lies ~0.2 (r = 1) / ~0.8 (r = 2) voxel edges beyond the
    plain rule's radius.  partial: eight more points in the keypoint's pass-2 voxel, among the K nearest of both passes -- the plain
    rule then keeps eight candidates of P_k = 28."""
    kp = np.array([F + 0.03, y0 + 0.5, z0 + 0.5])
    D = F + NB
    u = rng.uniform(-0.15, 0.15, (20, 2))
    near = np.column_stack([D + 0.02 + 0.03 * (u[:, 0] + 0.15) + 0.02 * (u[:, 1] + 0.15) + rng.uniform(0, 0.004, 20), y0 + 0.5 + u[:, 0], z0 + 0.5 + u[:, 1]])
    extra = np.column_stack([D + 0.02 + rng.uniform(0, 0.004, 5), y0 + 0.5 + rng.uniform(-0.1, 0.1, 5), z0 + 1.1 + rng.uniform(-0.05, 0.05, 5)])
    v = F - 1 - NB
    w = rng.uniform(-0.3, 0.3, (20, 2))
    far = np.column_stack([_centre(v) + 0.1 * w[:, 0] - 0.05 * w[:, 1] + rng.uniform(-0.004, 0.004, 20), y0 + NB + 0.5 + w[:, 0], z0 + NB + 0.5 + w[:, 1]])
    parts = [near, extra, far]
    if partial:
        parts.append(np.column_stack([np.full(8, F - 0.5) + rng.uniform(-0.2, 0.2, 8), y0 + 0.5 + rng.uniform(-0.3, 0.3, 8), z0 + 0.5 + rng.uniform(-0.3, 0.3, 8)]))
    return kp, np.concatenate(parts)


def _crossing_scene(seed, F, NB, away, axis, sign, size):
    """three crafted keypoints (a pair and the odd one; the pair's second keeps some candidates), their map, and the pass poses.
    Canonical frame -> world: away = mirror x about the face (the keypoint leaves the origin instead of approaching it), then the
    canonical x axis goes to `axis` (cyclic), everything times `sign` (truncation is odd: -x has key -key(x), so the voxel structure is
    the same on the negative side) and times the voxel size."""
    rng = np.random.default_rng(seed)
    kps, pts = [], []
    for i, partial in enumerate((False, True, False)):
        kp, P = _crossing_cell(rng, F, NB, 10 + 8 * i, 10 + 3 * i, partial)
        kps.append(kp); pts.append(P)
    kps, pts = np.array(kps), np.concatenate(pts)
    step = np.array([-0.06, 0.0, 0.0])
    if away:
        kps[:, 0] = 2 * F - kps[:, 0]; pts[:, 0] = 2 * F - pts[:, 0]; step = -step
    perm = [(0 - axis) % 3, (1 - axis) % 3, (2 - axis) % 3]              # world axis a takes canonical axis perm[a]
    M = np.eye(3)[perm] * sign * size
    kps, pts, step = kps @ M.T, pts @ M.T, M @ step
    keys, counts, xyz = _voxelise(pts.astype(np.float32), size=size)
    q = np.array([1.0, 0, 0, 0])
    # there, across, stay, back, across again
    poses = [(q, np.zeros(3)), (q, step), (q, step), (q, np.zeros(3)), (q, step)]
    return keys, counts, xyz, kps, poses


def _prove_crossing(keys, xyz, size, raw, poses, orc):
    """the plain rule drops oracle neighbours of all three keypoints on both crossings (passes 2 and 5); the pair's second keeps some"""
    for k in (1, 4):
        drops = _plain_rule_drops(keys, xyz, size, raw, poses[k - 1], orc[k - 1]["ids"], poses[k], orc[k]["ids"])
        assert np.all(drops > 0), (k, drops)
        assert drops[0] == K and drops[2] == K and 0 < drops[1] < K, (k, drops)
        assert np.all(orc[k]["neq"].sum_candidates > K)
    # P_k > K on the first pass too: the neighbours are the K nearest of more candidates
    assert orc[0]["neq"].sum_candidates >= 3 * 25


_CROSSINGS = [(12, away, axis, sign) for axis in range(3) for away in (False, True) for sign in (1, -1)] + \
             [(1, False, axis, sign) for axis in range(3) for sign in (1, -1)]          # the seam: key 1 -> key 0, i.e. [1, 2) -> (-1, 1)


@pytest.mark.parametrize("F,away,axis,sign", _CROSSINGS)
def test_crafted_crossings_r1(ctx, oracle_lib, oracle_backend, F, away, axis, sign):
    keys, counts, xyz, raw, poses = _crossing_scene(100 + axis, F, 1, away, axis, sign, 1.0)
    opts = srl.default_opts(max_num_residuals=INT_MAX)
    orc = _check_passes(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses, opts)
    _prove_crossing(keys, xyz, 1.0, raw, poses, orc)


@pytest.mark.parametrize("size", [0.5, 1.0, 1.5])
@pytest.mark.parametrize("max_res", [INT_MAX, 600])
@pytest.mark.parametrize("F,away,sign", [(12, False, 1), (12, True, -1), (1, False, -1)])
def test_crafted_crossings_r1_sizes_and_budgets(ctx, oracle_lib, oracle_backend, F, away, sign, size, max_res):
    keys, counts, xyz, raw, poses = _crossing_scene(200, F, 1, away, 1, sign, size)
    opts = srl.default_opts(max_num_residuals=max_res, size_voxel_map=size)
    orc = _check_passes(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses, opts)
    _prove_crossing(keys, xyz, size, raw, poses, orc)


@pytest.mark.parametrize("F,away,axis,sign", [(12, False, 0, 1), (12, True, 1, -1), (12, False, 2, -1), (1, False, 0, 1), (1, False, 2, -1)])
def test_crafted_crossings_init_mode_r2(ctx, oracle_lib, oracle_backend, F, away, axis, sign):
    keys, counts, xyz, raw, poses = _crossing_scene(300 + axis, F, 2, away, axis, sign, 1.0)
    opts = srl.default_opts(max_num_residuals=INT_MAX)
    assert 5 < opts.init_num_frames
    orc = _check_passes(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses, opts, frame_id=5)
    _prove_crossing(keys, xyz, 1.0, raw, poses, orc)


# ------------------------------------------------------------------------------------------------ c. randomised sparse maps
def _clustered_sparse_map(seed, occupancy=0.12, lo=5, hi=20):
    """24 x 24 x 6 voxels of 1 m, each occupied with probability `occupancy` by lo ... hi points in a cluster of random size and place.
    (test_gpu_band_bisection's map -- one to three points in EVERY voxel -- is sparse but uniform: a keypoint's K nearest inside the region
    it moves to are no further than those it had, and the plain rule happens to hold for all of its keypoints.  Empty voxels between small
    clusters are what makes the K-th neighbour of the new region lie beyond sqrt(tau) + movement.)"""
    rng = np.random.default_rng(seed)
    pts = []
    for ix in range(-12, 12):
        for iy in range(-12, 12):
            for iz in range(-3, 3):
                if rng.uniform() < occupancy:
                    n = int(rng.integers(lo, hi + 1)); c = rng.uniform(0.1, 0.9, 3); s = rng.uniform(0.05, 0.4)
                    pts.append(np.array([ix, iy, iz]) + np.clip(c + rng.uniform(-s, s, (n, 3)), 0.01, 0.99))
    return _voxelise(np.concatenate(pts).astype(np.float32))


def _random_poses(seed, count):
    """a walk with steps of 0.05 ... 0.6 m in random directions and a few mrad of rotation per step"""
    rng = np.random.default_rng(seed)
    q, t = np.array([1.0, 0, 0, 0]), np.zeros(3)
    out = [(q, t)]
    for _ in range(count - 1):
        d = rng.normal(size=3); d *= rng.uniform(0.05, 0.6) / np.linalg.norm(d)
        q = synth.quat_mul(q, synth.quat_from_rotvec(rng.normal(0, 0.003, 3))); t = t + d
        out.append((q, t))
    return out


@pytest.mark.parametrize("max_res", [INT_MAX, 600])
def test_random_sparse_maps_many_crossings(ctx, oracle_lib, oracle_backend, max_res):
    keys, counts, xyz = _clustered_sparse_map(81)
    rng = np.random.default_rng(82)
    raw = rng.uniform([-9, -9, -2], [9, 9, 2], size=(16_384, 3))
    poses = _random_poses(83, 6)
    opts = srl.default_opts(max_num_residuals=max_res)
    orc = _check_passes(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses, opts)
    # the regime, counted: keypoints of which the plain rule would drop at least one neighbour, per pass 2 ... 6
    # (of the keypoints the reference visits: ~900 of them under the budget of 600 residuals)
    hit = [int((_plain_rule_drops(keys, xyz, 1.0, raw, poses[k - 1], orc[k - 1]["ids"], poses[k], orc[k]["ids"])[:orc[k]["neq"].num_visited] > 0).sum())
           for k in range(1, len(poses))]
    print("keypoints in the regime per pass:", hit)
    lo, total = (20, 150) if max_res == INT_MAX else (1, 8)
    assert min(hit) >= lo and sum(hit) >= total, hit


# ------------------------------------------------------------------------------------------------ d. full solves
def _thinned_map(seed, map_pts, per_voxel):
    """synth's scene, at most `per_voxel` points per 1 m voxel (first come): the K-th neighbour ~1 ... 2 m away"""
    pts, L = synth.map_candidates(seed, map_pts)
    keys, counts, xyz = _voxelise(pts.astype(np.float32), cap=K)
    counts = np.minimum(counts, per_voxel)
    for i, c in enumerate(counts):
        xyz[i, c:] = 0.0
    return keys, counts, xyz, L


def _prior(oracle_lib, oracle_backend, sw):
    e = oracle_lib.Eskf(oracle_backend)
    synth.eskf_prior(e, sw["q_pred"], sw["t_pred"], sw["vel"])
    return e.get_state().copy(), e.get_cov().copy()


def test_full_solves_on_a_thinned_map(oracle_lib, oracle_backend):
    seed = 20250304 + 11
    keys, counts, xyz, L = _thinned_map(seed, 100_000, 3)
    sweeps = [synth.make_sweep(seed + 1000 + j, 4096, L) for j in range(2)]
    priors = [_prior(oracle_lib, oracle_backend, sw) for sw in sweeps]
    opts = srl.default_opts(max_num_residuals=INT_MAX)
    out = {}
    for mode in (0, 1):
        lio = srl.Lio(0)
        try:
            lio.ctx.set_bound_culling(mode)
            lio.ctx.map_upload(keys, counts, xyz)
            res = []
            for sw, (ps, pc) in zip(sweeps, priors):
                lio.eskf_set_state(ps); lio.eskf_set_cov(pc)
                st = np.concatenate([sw["q_pred"], sw["t_pred"], sw["vel"], np.zeros(6)])
                g = lio.update_iekf(opts, sw["raw"], st, sw["t_last"])
                assert g["rc"] == 0 and g["iters"] >= 2
                res.append((g["iters"], g["num_residuals"], g["state"].copy(), lio.eskf_get_cov().copy()))
            out[mode] = res
        finally:
            lio.close()
    for a, b in zip(out[0], out[1]):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    # the oracle: the same solves; and the pose of every ESIKF iteration (solves cut after j iterations), passed through the plain rule
    m = oracle_lib.Map(oracle_backend)
    m.import_(keys, counts, xyz)
    hit = 0
    for sw, (ps, pc), (iters, nres, state, cov) in zip(sweeps, priors, out[1]):
        st = np.concatenate([sw["q_pred"], sw["t_pred"], sw["vel"], np.zeros(6)])

        def solve(n_iter):
            e = oracle_lib.Eskf(oracle_backend)
            e.set_state(ps); e.set_cov(pc)
            u = oracle_lib.update_iekf(m, e, oracle_lib.opts_from_product(srl.default_opts(max_num_residuals=INT_MAX, num_iters_icp=n_iter)), sw["raw"], st, sw["t_last"])
            return u, e
        u, e = solve(opts.num_iters_icp)
        assert u["rc"] == iters and u["num_residuals"] == nres
        assert _rel(state, u["state"]) < 1e-9 and _rel(cov, e.get_cov()) < 1e-9
        poses = [(sw["q_pred"], sw["t_pred"])] + [(s[0:4], s[4:7]) for s in (solve(j)[0]["state"] for j in range(1, iters))]
        oo = oracle_lib.opts_from_product(opts)
        ids = [m.build_plane_residuals(oo, sw["raw"], q, t, sw["t_last"])["ids"] for q, t in poses]
        for k in range(1, len(poses)):
            hit += int((_plain_rule_drops(keys, xyz, 1.0, sw["raw"], poses[k - 1], ids[k - 1], poses[k], ids[k]) > 0).sum())
    print("iterations' keypoints in the regime:", hit)
    assert hit >= 5, hit
