"""The option envelope of buildPlaneResiduals on the device: `threshold_voxel_occupancy` and `voxel_neighborhood` (optimize.cpp:21-23,
:389), on the ragged-occupancy scene (tests/ragged_scene.py) where they change what a keypoint sees.

The device reads the threshold in three places -- probe_finish (the paired r = 1 fast path), probe_voxels (the general selection path, every
two-layer pass, the init fast path) and the search kernel's call of probe_voxels -- and it is part of two signatures on the host: the one
that voids the neighbourhood bounds of the previous pass and the one that decides whether an armed launch may be fired.  Every saturated
map of the suite gives the same answer at thresholds 1, 5 and 12, so none of these was pinned; here each one is, against the live oracle
(tests/test_ragged_scene.py holds the oracle to the reference's own translation units on the same scene and asserts the scene's
preconditions), against a golden of the reference, and against a plain NumPy count of the candidates.

Bars as in tests/test_gpu_parity.py: neighbour ids, status, counts and the per-keypoint candidate count exact; residual fields and normal
equations to TIGHT = 1e-9; solved state 1e-9 and covariance 1e-8 (tests/test_gpu_fuzz.py).  No keypoint is masked and no case skipped.
"""
import os

import numpy as np
import pytest

import ragged_scene as rs
import sr_livo_amd as srl
from sr_livo_amd import capi, synth

from test_gpu_bound_culling import _poses, _same
from test_gpu_parity import INT_MAX, TIGHT, check_pass_against, check_pass_against_reference_tu, gpu_pass, rel, state16

pytestmark = pytest.mark.gpu

SCENES = {"small": rs.SMALL, "large": rs.LARGE}
ALWAYS = 2          # srl_set_armed_launch(ctx, 2): a launch armed behind every eligible pass


@pytest.fixture(scope="module")
def scenes(oracle_lib, oracle_backend):
    """(name, voxel size) -> the oracle's ragged map, its export and the sweep; built on first use"""
    cache = {}

    def get(name, voxel_size=1.0):
        if (name, voxel_size) not in cache:
            cache[name, voxel_size] = rs.ragged_scene(oracle_lib, oracle_backend, *SCENES[name], voxel_size=voxel_size)
        return cache[name, voxel_size]
    return get


@pytest.fixture(scope="module")
def ctxs(scenes):
    """(name, voxel size) -> ONE device context per map for the whole module: the cases below change options under it as a caller would"""
    cache = {}

    def get(name, voxel_size=1.0):
        if (name, voxel_size) not in cache:
            sc = scenes(name, voxel_size)
            ctx = srl.Context(0)
            ctx.map_upload(sc["keys"], sc["counts"], sc["xyz"])
            cache[name, voxel_size] = ctx
        return cache[name, voxel_size]
    yield get
    for ctx in cache.values():
        ctx.close()


_oracle_cache = {}


def oracle_pass(oracle_lib, sc, raw, q, t, t_last, frame_id=100, **kw):
    """the oracle's pass, remembered: the selection paths and launch shapes of one case share it"""
    key = (id(sc), len(raw), tuple(np.asarray(q).tolist()), tuple(np.asarray(t).tolist()), frame_id, tuple(sorted(kw.items())))
    if key not in _oracle_cache:
        o = sc["map"].build_plane_residuals(oracle_lib.default_opts(**kw), raw, q, t, t_last, frame_id=frame_id)
        assert o["neq"].nan_error == 0 and o["neq"].num_ties == 0              # (scene preconditions: tests/test_ragged_scene.py)
        _oracle_cache[key] = o
    return _oracle_cache[key]


_count_cache = {}


def numpy_counts(sc, o, size, nb, thr):
    """P_k of every keypoint by ragged_scene.candidate_counts (a dict of the exported map, truncated keys, a plain sum)"""
    key = (id(sc), id(o), size, nb, thr)
    if key not in _count_cache:
        _count_cache[key] = rs.candidate_counts(sc["keys"], sc["counts"], o["point_world"], size, nb, thr)
    return _count_cache[key]


def effective(kw, frame_id):
    """(layers, threshold) the pass must use: the options, or 2 / 1 in the init mode (optimize.cpp:21-23)"""
    if frame_id < kw.get("init_num_frames", 20):
        return 2, 1
    return kw.get("voxel_neighborhood", 1), kw.get("threshold_voxel_occupancy", 1)


def check_against_oracle(g, o, sc, kw, frame_id=100):
    check_pass_against(g, rs.oracle_reference(o), "x")
    assert g["neq"].last_visited == o["neq"].num_visited - 1
    visited = o["status"] != 3
    if visited.all():                                                           # no cut binds: the sum is over every keypoint
        assert g["neq"].sum_candidates == o["neq"].sum_candidates
    nb, thr = effective(kw, frame_id)
    want = numpy_counts(sc, o, kw.get("size_voxel_map", 1.0), nb, thr)
    assert np.array_equal(g["ncand"][visited], want[visited]), "per-keypoint candidate count"
    assert int(want[visited].sum()) == o["neq"].sum_candidates or not visited.all()


# ----------------------------------------------------------------------------- (a) one pass against the oracle
def _case(thr, nb, mode=0, K=20, mn=20, max_res=INT_MAX, n=2048, size=1.0, frame_id=100, **extra):
    kw = dict(threshold_voxel_occupancy=thr, voxel_neighborhood=nb, max_number_neighbors=K, min_number_neighbors=mn, max_num_residuals=max_res, **extra)
    if size != 1.0:
        kw["size_voxel_map"] = size
    ident = f"thr{thr}-nb{nb}-mode{mode}-K{K}.{mn}-max{'inf' if max_res == INT_MAX else max_res}-n{n}-size{size}" + ("-weights" if extra else "")
    return pytest.param(kw, mode, n, size, id=ident)


def _pass_cases():
    cases = []
    # every (threshold > 1, layers) through every selection path and both launch shapes: n < 2048 runs four-wave workgroups, n >= 2048
    # sixteen-wave ones (plan_pass)
    for thr in (2, 5, 12, 20, 21):
        for nb in (1, 2):
            for mode in (0, 1, 2, 5):
                for n in (1500, 2048):
                    cases.append(_case(thr, nb, mode=mode, n=n))
    # thresholds that must behave as 1
    cases += [_case(thr, nb) for thr in (0, -3, 1) for nb in (1, 2)]
    for thr, nb in ((5, 1), (12, 2), (20, 1), (5, 2)):
        cases += [_case(thr, nb, K=5, mn=5), _case(thr, nb, K=32, mn=20), _case(thr, nb, K=5, mn=5, mode=2), _case(thr, nb, K=32, mn=20, mode=1)]
        cases += [_case(thr, nb, max_res=m) for m in (600, 37, -1)]
        cases += [_case(thr, nb, n=n) for n in (1, 63, 65, 4096)]
        cases += [_case(thr, nb, size=0.8), _case(thr, nb, size=0.8, n=4096)]
    cases += [_case(thr, nb, n=4096, mode=mode) for thr in (2, 12, 20, 21) for nb in (1, 2) for mode in (0, 2)]
    cases += [_case(5, 1, max_res=600, size=0.8, n=n, weight_alpha=0.8, weight_neighborhood=0.2) for n in (2048, 4096)]      # rs.LOW_INERTIA
    return cases


@pytest.mark.parametrize("kw,mode,n,size", _pass_cases())
def test_one_pass_matches_the_oracle_on_the_ragged_scene(oracle_lib, scenes, ctxs, kw, mode, n, size):
    name = "large" if n > 2048 else "small"
    sc = scenes(name, size); sw = sc["sweep"]
    raw = sw["raw"][:n]
    g = gpu_pass(ctxs(name, size), raw, sw["q_pred"], sw["t_pred"], sw["t_last"], select_mode=mode, **kw)
    o = oracle_pass(oracle_lib, sc, raw, sw["q_pred"], sw["t_pred"], sw["t_last"], **kw)
    check_against_oracle(g, o, sc, kw)
    if kw["threshold_voxel_occupancy"] == 21:
        assert g["neq"].num_residuals == 0 and g["neq"].success == 0 and np.all(g["ncand"] == 0) and np.all(g["ids"] == -1)


# ----------------------------------------------------------------------------- (b) the init mode ignores both options
def _bitwise_same_pass(a, b):
    """two device passes, bit for bit, in everything a pass defines: ids / counts of visited keypoints, fields of those with a plane"""
    assert np.array_equal(a["status"], b["status"])
    visited, has_plane, acc = a["status"] != 3, (a["status"] == 1) | (a["status"] == 2), a["status"] == 2
    for k in ("ids", "ncand"):
        assert np.array_equal(a[k][visited], b[k][visited]), k
    for k in ("normal", "a2D", "weight", "norm_offset", "distance"):
        assert np.array_equal(a[k][has_plane], b[k][has_plane]), k
    assert np.array_equal(a["jacobian"][acc], b["jacobian"][acc])
    _same((a["neq"], None), (b["neq"], None), "normal equations")


@pytest.mark.parametrize("init_num_frames", [20, 40, 0])
def test_init_mode_ignores_threshold_and_neighbourhood(oracle_lib, scenes, ctxs, init_num_frames):
    """frame_id < init_num_frames: two layers, threshold 1, whatever the options say.  The pass with (12, 1) equals the pass with (1, 2) bit
    for bit and the oracle; one frame later the options hold.  init_num_frames = 40 is the robust driving profile's value."""
    sc = scenes("small"); sw = sc["sweep"]; ctx = ctxs("small")
    base = dict(max_num_residuals=INT_MAX, init_num_frames=init_num_frames)
    a_kw = dict(base, threshold_voxel_occupancy=12, voxel_neighborhood=1)
    b_kw = dict(base, threshold_voxel_occupancy=1, voxel_neighborhood=2)
    pose = (sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"])
    frames = sorted({5 if init_num_frames > 5 else init_num_frames - 1, init_num_frames - 1})
    for frame_id in frames:
        a = gpu_pass(ctx, *pose, frame_id=frame_id, **a_kw)
        b = gpu_pass(ctx, *pose, frame_id=frame_id, **b_kw)
        _bitwise_same_pass(a, b)
        check_against_oracle(a, oracle_pass(oracle_lib, sc, *pose, frame_id=frame_id, **a_kw), sc, a_kw, frame_id)
    first = gpu_pass(ctx, *pose, frame_id=init_num_frames, **a_kw)              # the first frame the options apply to
    check_against_oracle(first, oracle_pass(oracle_lib, sc, *pose, frame_id=init_num_frames, **a_kw), sc, a_kw, init_num_frames)
    assert np.any(first["ids"] != a["ids"]) and not np.array_equal(first["ncand"], a["ncand"])


# ----------------------------------------------------------------------------- (c) the reference's own translation units
@pytest.fixture(scope="module")
def gragged():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_ref_tu_ragged.npz"), allow_pickle=False))


@pytest.mark.parametrize("prefix,which,kw", [("t5n1", "map", dict(threshold_voxel_occupancy=5, voxel_neighborhood=1, max_num_residuals=INT_MAX)),
                                             ("t12n2", "map", dict(threshold_voxel_occupancy=12, voxel_neighborhood=2, max_num_residuals=INT_MAX)),
                                             ("lowinertia", "map08", rs.LOW_INERTIA)])
def test_one_pass_matches_the_ragged_reference_golden(gragged, prefix, which, kw):
    """golden_ref_tu_ragged.npz: lioOptimization::buildPlaneResiduals of the reference, compiled in place, on the small ragged scene"""
    g = gragged
    ctx = srl.Context(0)
    try:
        ctx.map_upload(g[f"{which}_keys"], g[f"{which}_counts"], g[f"{which}_xyz"])
        p = gpu_pass(ctx, g["raw"], g["q_pred"], g["t_pred"], g["t_last"], **kw)
    finally:
        ctx.close()
    check_pass_against_reference_tu(p, g, prefix, g["raw"])
    assert p["neq"].num_residuals >= 500


# ----------------------------------------------------------------------------- (d) neighbourhood bounds under a threshold
def _run_poses(ctx, sw, poses, opts, taps):
    out = []
    ctx.set_taps(taps)
    for q, t in poses:
        neq, _ = ctx.build_residuals(capi.make_frame(q, t, sw["t_last"]), opts)
        rec = dict(neq=neq, ids=None)
        if taps:
            ids, status, ncand = ctx.fetch_neighbors(K=opts.max_number_neighbors)
            rec.update(ids=ids, status=status, ncand=ncand, **ctx.fetch_residuals())
        out.append(rec)
    ctx.set_taps(False)
    return out


@pytest.mark.parametrize("thr,nb", [(5, 1), (12, 2), (20, 1)])
def test_bounds_under_a_threshold_change_no_bit(oracle_lib, scenes, thr, nb):
    """Five consecutive poses of one sweep (one of them a jump) with the bounds of the previous pass on and off, taps on and off, armed
    launches off and always: bit for bit the same, the first and the last pass equal to the oracle, and P_k still the count over EVERY
    qualifying voxel -- a culled voxel stays in P_k, a voxel below the threshold never enters it."""
    sc = scenes("large"); sw = sc["sweep"]
    kw = dict(threshold_voxel_occupancy=thr, voxel_neighborhood=nb, max_num_residuals=INT_MAX)
    opts = srl.default_opts(**kw)
    poses = _poses(sw, 4, 7, jump=3)
    assert len(poses) == 5
    ctx = srl.Context(0)
    try:
        ctx.map_upload(sc["keys"], sc["counts"], sc["xyz"])
        runs = {}
        for cull in (0, 1):
            for taps in (True, False):
                for armed in (0, ALWAYS):
                    ctx.set_armed_launch(armed)
                    ctx.set_bound_culling(cull)
                    ctx.sweep_upload(sw["raw"])
                    runs[cull, taps, armed] = _run_poses(ctx, sw, poses, opts, taps)
        ctx.disarm()
        ref = runs[0, True, 0]
        for key, got in runs.items():
            for k, (g, r) in enumerate(zip(got, ref)):
                _same((g["neq"], g["ids"]), (r["neq"], r["ids"] if g["ids"] is not None else None), (key, k))
                if g["ids"] is not None:
                    _bitwise_same_pass(g, r)
        for k in (0, len(poses) - 1):
            q, t = poses[k]
            o = oracle_pass(oracle_lib, sc, sw["raw"], q, t, sw["t_last"], **kw)
            for key in ((1, True, 0), (1, True, ALWAYS), (0, True, 0)):
                check_against_oracle(runs[key][k], o, sc, kw)
            assert rel(np.array(runs[1, False, ALWAYS][k]["neq"].HtH).reshape(6, 6), o["HtH"]) < TIGHT
    finally:
        ctx.close()


# ----------------------------------------------------------------------------- (e) options changing under a live context
# (threshold, layers, frame_id) per pass: threshold 1 -> 5 -> 5 -> 1 -> 12, layers 1 -> 2 -> 1, frame 5 -> 100 -> 5 -> 100, and back
OPTION_WALK = [(1, 1, 5),        # init mode: two layers, threshold 1 -- bounds and an armed launch are left behind with those
               (5, 2, 100),      # same layers as the init pass ran with, ANOTHER threshold: only the threshold tells the two passes apart
               (5, 2, 100),      # nothing changes: the armed launch is fired, the bounds are used
               (5, 1, 100),      # layers 2 -> 1
               (1, 1, 100),      # threshold 5 -> 1
               (12, 1, 100),     # threshold 1 -> 12 under the same layers: bounds written at threshold 1 are too tight for 12
               (12, 1, 100),
               (12, 2, 5),       # back into the init mode
               (12, 2, 100),     # out of it: two layers as before, threshold 1 -> 12
               (12, 2, 100)]


def test_options_changing_under_a_live_context(oracle_lib, scenes):
    """One context, one sweep uploaded once, bounds on, a launch armed behind every pass; the options change from pass to pass.  Every
    pass equals the same pass on a fresh context without bounds and without armed launches, bit for bit, and the oracle.  A launch armed
    under other options is cancelled, never fired (srl_get_arm_stats)."""
    sc = scenes("large"); sw = sc["sweep"]
    poses = _poses(sw, len(OPTION_WALK), 11)
    kws = [dict(threshold_voxel_occupancy=thr, voxel_neighborhood=nb, max_num_residuals=INT_MAX) for thr, nb, _ in OPTION_WALK]
    optss = [srl.default_opts(**kw) for kw in kws]
    frames = [capi.make_frame(q, t, sw["t_last"], frame_id=fid) for (q, t), (_, _, fid) in zip(poses, OPTION_WALK)]
    live = srl.Context(0)
    try:
        live.map_upload(sc["keys"], sc["counts"], sc["xyz"])
        live.set_bound_culling(1)
        live.set_armed_launch(ALWAYS)
        live.set_arm_linger(host_linger_us=1e5, kernel_linger_us=2e5)          # an interpreter sits between two passes here, not a C loop
        live.sweep_upload(sw["raw"])
        stats = [live.arm_stats()]
        got = []
        for frame, opts in zip(frames, optss):                                 # back to back: nothing but the pass between two passes
            got.append(live.build_residuals(frame, opts)[0])
            stats.append(live.arm_stats())
        live.disarm()
    finally:
        live.close()
    thr_only_cancel = fired_same = 0
    for step, (kw, (thr, nb, frame_id), (q, t)) in enumerate(zip(kws, OPTION_WALK, poses)):
        fresh = srl.Context(0)
        try:
            fresh.map_upload(sc["keys"], sc["counts"], sc["xyz"])
            fresh.set_bound_culling(0)
            fresh.set_armed_launch(0)
            fresh.sweep_upload(sw["raw"])
            want, _ = fresh.build_residuals(frames[step], optss[step])
        finally:
            fresh.close()
        _same((got[step], None), (want, None), (step, thr, nb, frame_id))
        o = oracle_pass(oracle_lib, sc, sw["raw"], q, t, sw["t_last"], frame_id=frame_id, **kw)
        assert got[step].num_residuals == o["neq"].num_residuals and got[step].sum_candidates == o["neq"].sum_candidates, step
        assert rel(np.array(got[step].HtH).reshape(6, 6), o["HtH"]) < TIGHT and rel(np.array(got[step].Hth), o["Hth"]) < TIGHT, step
        if step == 0:
            continue
        before, after = stats[step], stats[step + 1]                           # around this pass
        had_armed = stats[step]["armed"] - stats[step - 1]["armed"] == 1      # the previous pass left a launch behind
        eff, prev_eff = effective(kw, frame_id), effective(kws[step - 1], OPTION_WALK[step - 1][2])
        if eff != prev_eff:
            assert after["fired"] == before["fired"], (step, "a launch armed under other options was fired")
            if had_armed:
                assert after["cancelled"] == before["cancelled"] + 1, step
                thr_only_cancel += int(eff[0] == prev_eff[0])
        elif had_armed:
            assert after["fired"] == before["fired"] + 1 and after["cancelled"] == before["cancelled"], step
            fired_same += 1
    assert stats[-1]["expired"] == 0
    assert thr_only_cancel >= 2 and fired_same >= 2                           # the mechanism was live: launches were armed, fired and cancelled


# ----------------------------------------------------------------------------- (f) fused and armed passes: full solves
def _prior(oracle_lib, oracle_backend, sw):
    e = oracle_lib.Eskf(oracle_backend)
    synth.eskf_prior(e, sw["q_pred"], sw["t_pred"], sw["vel"])
    return e, e.get_state().copy(), e.get_cov().copy()


@pytest.mark.parametrize("kw", [dict(threshold_voxel_occupancy=5, voxel_neighborhood=1, max_num_residuals=INT_MAX),
                                dict(threshold_voxel_occupancy=5, voxel_neighborhood=2, max_num_residuals=INT_MAX),
                                dict(threshold_voxel_occupancy=12, voxel_neighborhood=1, max_num_residuals=INT_MAX), rs.LOW_INERTIA],
                         ids=["thr5-nb1", "thr5-nb2", "thr12-nb1", "low_inertia"])
@pytest.mark.parametrize("tight", [False, True], ids=["converges", "all-iterations"])
def test_full_solve_under_a_threshold_matches_the_oracle(oracle_lib, oracle_backend, scenes, kw, tight):
    """Lio.update_iekf without taps on the 4096-keypoint scene: sixteen-wave workgroups, the fused final reduction, a launch armed behind
    every pass, bounds from pass to pass -- against the oracle's updateIEKF.  With the shipped convergence thresholds the solve ends after
    two passes; with thresholds it cannot meet it runs all num_iters_icp + 1 of them."""
    if tight:
        kw = dict(kw, threshold_orientation_norm=1e-7, threshold_translation_norm=1e-7)
    sc = scenes("large", kw.get("size_voxel_map", 1.0)); sw = sc["sweep"]
    lio = srl.Lio(0)
    try:
        lio.ctx.map_upload(sc["keys"], sc["counts"], sc["xyz"])
        lio.ctx.set_armed_launch(ALWAYS)
        e, s0, P0 = _prior(oracle_lib, oracle_backend, sw)
        lio.eskf_set_state(s0); lio.eskf_set_cov(P0)
        opts = srl.default_opts(**kw)
        before = lio.ctx.arm_stats()
        r = lio.update_iekf(opts, sw["raw"], state16(sw), sw["t_last"])
        after = lio.ctx.arm_stats()
        u = oracle_lib.update_iekf(sc["map"], e, oracle_lib.opts_from_product(opts), sw["raw"], state16(sw), sw["t_last"])
        assert r["rc"] == 0 and r["iters"] == u["rc"] and u["rc"] >= (6 if tight else 2) and r["num_residuals"] == u["num_residuals"] > 0
        assert rel(r["state"], u["state"]) < 1e-9
        assert rel(lio.eskf_get_state(), e.get_state()) < 1e-9 and rel(lio.eskf_get_cov(), e.get_cov()) < 1e-8
        if kw["max_num_residuals"] == INT_MAX:
            assert after["fired"] > before["fired"]                            # the armed launches ran: the solve was not a series of plain ones
        lio.ctx.disarm()
    finally:
        lio.close()


def test_a_threshold_nothing_meets_fails_the_solve_and_leaves_the_context_usable(oracle_lib, oracle_backend, scenes):
    """threshold 21 on a map of at most 20 points per voxel: no neighbour, no residual -- SRL_ERR_NOT_ENOUGH_RESIDUALS, like the oracle (rc < 0),
    the pose untouched; the default solve right after it on the same handle equals the oracle's"""
    sc = scenes("large"); sw = sc["sweep"]
    lio = srl.Lio(0)
    try:
        lio.ctx.map_upload(sc["keys"], sc["counts"], sc["xyz"])
        lio.ctx.set_armed_launch(ALWAYS)
        e, s0, P0 = _prior(oracle_lib, oracle_backend, sw)
        for nb in (1, 2):
            lio.eskf_set_state(s0); lio.eskf_set_cov(P0); e.set_state(s0); e.set_cov(P0)
            opts = srl.default_opts(threshold_voxel_occupancy=21, voxel_neighborhood=nb, max_num_residuals=INT_MAX)
            r = lio.update_iekf(opts, sw["raw"], state16(sw), sw["t_last"])
            u = oracle_lib.update_iekf(sc["map"], e, oracle_lib.opts_from_product(opts), sw["raw"], state16(sw), sw["t_last"])
            assert r["rc"] == capi.SRL_ERR_NOT_ENOUGH_RESIDUALS and u["rc"] < 0
            assert r["num_residuals"] == u["num_residuals"] == 0
            assert np.array_equal(r["state"], state16(sw)) and np.array_equal(u["state"], state16(sw))
        lio.eskf_set_state(s0); lio.eskf_set_cov(P0); e.set_state(s0); e.set_cov(P0)
        opts = srl.default_opts(max_num_residuals=INT_MAX)
        r = lio.update_iekf(opts, sw["raw"], state16(sw), sw["t_last"])
        u = oracle_lib.update_iekf(sc["map"], e, oracle_lib.opts_from_product(opts), sw["raw"], state16(sw), sw["t_last"])
        assert r["rc"] == 0 and r["iters"] == u["rc"] >= 2 and r["num_residuals"] == u["num_residuals"]
        assert rel(r["state"], u["state"]) < 1e-9 and rel(lio.eskf_get_cov(), e.get_cov()) < 1e-8
        lio.ctx.disarm()
    finally:
        lio.close()


# ----------------------------------------------------------------------------- (g) searchNeighbors
def _search_points(sc):
    """300 world points: keypoints of the sweep, points in empty space, and points next to the sparsest voxels (whose neighbourhoods hold
    fewer than K qualifying points at the higher thresholds)"""
    sw = sc["sweep"]
    world = sw["raw"][:200] @ synth.quat_to_rot(sw["q_pred"] / np.linalg.norm(sw["q_pred"])).T + sw["t_pred"]
    rng = np.random.default_rng(5)
    L = sc["L"]
    empty = np.column_stack([rng.uniform(-L, L, 40), rng.uniform(-L, L, 40), rng.uniform(8.0, 30.0, 40)])      # above every wall
    sparse = np.flatnonzero(sc["counts"] <= 3)[:60]
    near = sc["xyz"][sparse, 0].astype(np.float64) + rng.normal(0, 0.05, (len(sparse), 3))
    q = np.concatenate([world, empty, near])
    assert len(q) == 300
    return q


@pytest.mark.parametrize("K", [5, 20, 32])
@pytest.mark.parametrize("nb", [1, 2])
def test_search_neighbors_under_a_threshold(scenes, ctxs, nb, K):
    """srl_search_neighbors and, through Lio.search_neighbors, the host mirror's searchNeighbors: num_found, ids and coordinates exact
    against the oracle for thresholds 0, 1, 5, 20 and 21"""
    sc = scenes("small"); ctx = ctxs("small")
    q = _search_points(sc)
    lio = srl.Lio(0)
    try:
        lio.ctx.map_upload(sc["keys"], sc["counts"], sc["xyz"])
        none = short = 0                                                        # counted below threshold 21, where nothing is found anyway
        for thr in (0, 1, 5, 20, 21):
            ids, xyz, nf = ctx.search_neighbors(q, nb=nb, K=K, thr=thr)
            for i in range(len(q)):
                r = sc["map"].search_neighbors(q[i], nb=nb, K=K, thr=thr)
                assert nf[i] == r["n"], (thr, i)
                assert np.array_equal(ids[i, : r["n"]], r["ids"]), (thr, i)
                assert np.all(ids[i, r["n"]:] == -1)
                assert np.array_equal(xyz[i, : r["n"]].astype(np.float64), r["xyz"])
                assert np.all(sc["counts"][r["ids"] // 20] >= thr)
                none += int(r["n"] == 0 and thr < 21); short += int(0 < r["n"] < K)
                if i % 6 == 0:                                                  # the class surface, one point per call
                    pts, vox = lio.search_neighbors(q[i], nb=nb, K=K, thr=thr)
                    assert np.array_equal(pts, r["xyz"]) and np.array_equal(vox, sc["keys"][r["ids"] // 20]), (thr, i)
            if thr == 21:
                assert np.all(nf == 0)
        assert none >= 160 and (short > 0 or K == 5)                           # the 40 points in empty space at four thresholds; short lists
    finally:
        lio.close()


# ----------------------------------------------------------------------------- (h) the envelope's edges fail loudly
def test_unsupported_neighbourhoods_are_refused_by_name_and_launch_nothing(oracle_lib, scenes):
    sc = scenes("small"); sw = sc["sweep"]
    ctx = srl.Context(0)
    try:
        ctx.map_upload(sc["keys"], sc["counts"], sc["xyz"])
        ctx.set_armed_launch(ALWAYS)
        ctx.sweep_upload(sw["raw"])
        frame = capi.make_frame(sw["q_pred"], sw["t_pred"], sw["t_last"])
        good_kw = dict(threshold_voxel_occupancy=5, voxel_neighborhood=2, max_num_residuals=INT_MAX)
        o = oracle_pass(oracle_lib, sc, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"], **good_kw)
        ctx.set_profiling(1)                                                    # Timing.calls counts the association launches
        ctx.build_residuals(frame, srl.default_opts(**good_kw))
        for nb in (0, 3, -1):
            calls, stats = ctx.timing().calls, ctx.arm_stats()
            with pytest.raises(srl.SrlError) as err:
                ctx.build_residuals(frame, srl.default_opts(voxel_neighborhood=nb, max_num_residuals=INT_MAX))
            assert err.value.status == capi.SRL_ERR_UNSUPPORTED and "voxel_neighborhood" in str(err.value)
            assert ctx.timing().calls == calls and ctx.arm_stats()["armed"] == stats["armed"]
            # ... and the next valid pass on the same context is right
            g = gpu_pass(ctx, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"], **good_kw)
            check_against_oracle(g, o, sc, good_kw)
        q = _search_points(sc)
        for nb in (0, 3):
            with pytest.raises(srl.SrlError) as err:
                ctx.search_neighbors(q, nb=nb, K=20, thr=5)               # (refused before the device is touched: srl_search_neighbors)
            assert err.value.status == capi.SRL_ERR_UNSUPPORTED and "nb_voxels_visited" in str(err.value)
            ids, _, nf = ctx.search_neighbors(q[:50], nb=1, K=20, thr=5)
            for i in range(50):
                r = sc["map"].search_neighbors(q[i], nb=1, K=20, thr=5)
                assert nf[i] == r["n"] and np.array_equal(ids[i, : r["n"]], r["ids"])
        ctx.set_profiling(0)
        # in the init mode the option is not read (optimize.cpp:21-23): an unsupported value is not an error there
        g = gpu_pass(ctx, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"], frame_id=5, voxel_neighborhood=3, max_num_residuals=INT_MAX)
        kw5 = dict(voxel_neighborhood=3, max_num_residuals=INT_MAX)
        check_against_oracle(g, oracle_pass(oracle_lib, sc, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"], frame_id=5, **kw5), sc, kw5, 5)
    finally:
        ctx.close()
