"""Passes of the r = 1 fast path with the neighbour records (srl_debug_set_neighbour_records 1, the default: a keypoint's 27 voxel
lookups come from its home voxel's record, srl_kernels.hip: record_resolve) against the same passes on the table lookups (0), bit for
bit -- neighbour ids (the parity tap), status, candidate counts (P_k), the sums, num_fallback, the bounds a pass leaves and the solved
state -- and, wherever the CPU can check it, against the oracle:
  1. a dense scene, 1 999 keypoints (an odd tail pair), a first pass and passes from bounds, budgets INT_MAX and 600, an occupancy threshold
     above some voxels' counts, init mode (r = 2: never reads a record);
  2. keypoints whose home voxel is not in the map -- alone in a pair, as both of a pair, as the unpaired last keypoint of an odd tile --
     and a keypoint in a voxel without any occupied neighbour: the pair asks the table and stays on the fast path;
  3. a solve (srl_lio_update_iekf);
  4. an armed stream across a map insertion between two sweeps;
  5. a two-shard context."""
import numpy as np
import pytest

import shard_harness as sh
import sr_livo_amd as srl
from sr_livo_amd import capi, synth
from test_gpu_bound_culling import _poses, _same
from test_gpu_eigen_stress import _voxelise

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
K = 20
Q0 = np.array([1.0, 0.0, 0.0, 0.0])


def _passes(ctx, raw, poses, records, t_last, opts=None, armed=0, frame_id=100, taps=True, bounds_every_pass=True):
    """the passes of one sweep from a fresh upload; per pass the record, the taps and the bounds it left (reading the bounds cancels a
    waiting launch: an armed stream reads them behind its last pass only)"""
    opts = opts or srl.default_opts(max_num_residuals=INT_MAX)
    ctx.set_armed_launch(armed)
    ctx.set_neighbour_records(records)
    ctx.sweep_upload(raw)
    ctx.set_taps(1 if taps else 0)
    out = []
    for q, t in poses:
        neq, rc = ctx.build_residuals(capi.make_frame(q, t, t_last, frame_id=frame_id), opts)
        ids, status, ncand = (a.copy() for a in ctx.fetch_neighbors(K=K)) if taps else (None, None, None)
        last = len(out) == len(poses) - 1
        out.append(dict(neq=neq, ids=ids, status=status, ncand=ncand, bounds=ctx.bounds_download() if bounds_every_pass or last else None))
    ctx.set_taps(0)
    ctx.set_armed_launch(1)
    ctx.set_neighbour_records(1)
    return out


def _equal(got, ref, what):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        _same((g["neq"], g["ids"]), (r["neq"], r["ids"]), (what, k))
        assert g["neq"].num_fallback == r["neq"].num_fallback, (what, k, g["neq"].num_fallback, r["neq"].num_fallback)
        if g["ids"] is not None:
            assert np.array_equal(g["status"], r["status"]) and np.array_equal(g["ncand"], r["ncand"]), (what, k)
        assert g["bounds"].tobytes() == r["bounds"].tobytes() and len(g["bounds"]) > 0, (what, k, "bounds")


def _against_oracle(got, orc, what):
    for k, (g, o) in enumerate(zip(got, orc)):
        bad = np.flatnonzero((g["ids"] != o["ids"]).any(1))
        assert bad.size == 0, (what, "ids differ from the oracle", k, bad[:8])
        assert np.array_equal(g["status"], o["status"]), (what, k)
        assert g["neq"].sum_candidates == o["neq"].sum_candidates and g["neq"].num_residuals == o["neq"].num_residuals, (what, k)


def _workgroups(ctx):
    """workgroups of the last pass's association launch (srl_debug_block_times reports the count)"""
    import ctypes as C
    out = np.zeros((2048, 3))
    nb = C.c_int()
    ctx._chk(ctx.lib.srl_debug_block_times(ctx.h, out.ctypes.data_as(C.c_void_p), 2048, C.byref(nb)), "srl_debug_block_times")
    return nb.value


# ------------------------------------------------------------------------------------------------ 1. the dense scene
@pytest.fixture(scope="module")
def dense(oracle_lib, oracle_backend):
    cands, L = synth.map_candidates(7301, 40_000)
    c = srl.Context(0)
    c.map_insert(cands)
    sw = synth.make_sweep(7302, 1_999, L)
    m = oracle_lib.Map(oracle_backend)
    m.import_(*c.map_download())
    yield dict(ctx=c, L=L, sw=sw, omap=m, cands=cands)
    c.close()


@pytest.mark.parametrize("max_res,thr", [(INT_MAX, 1), (600, 1), (INT_MAX, 6)])
def test_dense_passes_agree_and_equal_the_oracle(dense, oracle_lib, max_res, thr):
    c, sw = dense["ctx"], dense["sw"]
    poses = _poses(sw, 3, 1)                                               # a first pass and two from bounds
    opts = srl.default_opts(max_num_residuals=max_res, threshold_voxel_occupancy=thr)
    if thr > 1:
        _, counts, _ = c.map_download()
        assert 0 < (counts < thr).mean() < 0.9, "the threshold lies above some voxels' counts"
    ref = _passes(c, sw["raw"], poses, 0, sw["t_last"], opts)
    got = _passes(c, sw["raw"], poses, 1, sw["t_last"], opts)
    _equal(got, ref, ("dense", max_res, thr))
    if max_res == INT_MAX:      # (with a budget the device's taps cover the whole sweep, the oracle's loop stops at the budget)
        orc = [dense["omap"].build_plane_residuals(oracle_lib.opts_from_product(opts), sw["raw"], q, t, sw["t_last"], frame_id=100) for q, t in poses]
        _against_oracle(got, orc, ("dense", max_res, thr))
    no_taps = [_passes(c, sw["raw"], poses, r, sw["t_last"], opts, taps=False) for r in (0, 1)]
    _equal(no_taps[1], no_taps[0], ("dense, no taps", max_res, thr))


def test_init_mode_is_untouched(dense):
    c, sw = dense["ctx"], dense["sw"]
    poses = _poses(sw, 2, 5)
    _equal(_passes(c, sw["raw"], poses, 1, sw["t_last"], frame_id=5), _passes(c, sw["raw"], poses, 0, sw["t_last"], frame_id=5), "init mode")


# ------------------------------------------------------------------------------------------------ 2. home voxels the map does not have
def _block(rng, lo):
    """2 x 2 x 2 full voxels from `lo`"""
    return np.concatenate([lo + np.array([i, j, k]) + rng.uniform(0.02, 0.98, (20, 3)) for i in range(2) for j in range(2) for k in range(2)])


def _absent_home_scene(seed, groups):
    """per group a block of eight full voxels at (8 g + 2, 2, 2) .. and keypoints `inside` it (home voxel present) or just `outside` its
    +x face (home voxel empty, nine of its 27 neighbours occupied), in the order of `pattern`; one lone voxel far away with seven points and
    a keypoint in it (no occupied neighbour, fewer than K candidates).  The last keypoint is an `outside` one and the count is odd."""
    rng = np.random.default_rng(seed)
    pts, kps, absent = [], [], []
    pattern = "ioooiioi"          # pairs: (present, absent) (absent, absent) (present, present) (absent, present)
    for g in range(groups):
        lo = np.array([8.0 * g + 2.0, 2.0, 2.0])
        pts.append(_block(rng, lo))
        for ch in pattern:
            inside = lo + rng.uniform(0.2, 1.8, 3)
            outside = lo + np.array([2.0 + rng.uniform(0.05, 0.4), rng.uniform(0.3, 1.7), rng.uniform(0.3, 1.7)])
            kps.append(inside if ch == "i" else outside)
            absent.append(ch == "o")
    lone = np.array([2.5, 40.5, 2.5])
    pts.append(lone + rng.uniform(-0.4, 0.4, (7, 3)))
    kps += [lone + 0.05, lone - 0.07]; absent += [False, False]
    lo = np.array([8.0 * (groups - 1) + 2.0, 2.0, 2.0])
    kps.append(lo + np.array([2.2, 1.0, 1.0])); absent.append(True)
    assert len(kps) % 2 == 1
    return np.concatenate(pts).astype(np.float32), np.array(kps), np.array(absent)


@pytest.mark.parametrize("max_res", [INT_MAX, 600])
def test_keypoints_without_a_home_voxel_stay_on_the_fast_path(oracle_lib, oracle_backend, max_res):
    pts, raw, absent = _absent_home_scene(7311, groups=9)                   # 75 keypoints: five tiles of 16 (pinned below), the last one of 11
    keys, counts, xyz = _voxelise(pts)
    have = {tuple(k) for k in keys.tolist()}
    home = [tuple(int(np.trunc(c)) for c in p) for p in raw]
    assert [h not in have for h in home] == absent.tolist() and absent.sum() > 30
    poses = [(Q0, np.zeros(3)), (Q0, np.array([0.01, -0.01, 0.012])), (Q0, np.array([0.012, -0.01, 0.012]))]
    opts = srl.default_opts(max_num_residuals=max_res)
    c = srl.Context(0)
    try:
        c.map_upload(keys, counts, xyz)
        c.set_launch_shape(4, 4)                                            # workgroups of 4 waves x 4 keypoints: the tiles the scene is built for
        t_last = np.zeros(3)
        ref = _passes(c, raw, poses, 0, t_last, opts)
        got = _passes(c, raw, poses, 1, t_last, opts)
        assert _workgroups(c) == 5 and len(raw) - 4 * 16 == 11 and absent[-1], "the last tile is odd and ends on a keypoint without a home voxel"
    finally:
        c.close()
    _equal(got, ref, ("absent homes", max_res))
    if max_res == INT_MAX:
        m = oracle_lib.Map(oracle_backend)
        m.import_(keys, counts, xyz)
        orc = [m.build_plane_residuals(oracle_lib.opts_from_product(opts), raw, q, t, t_last, frame_id=100) for q, t in poses]
        _against_oracle(got, orc, ("absent homes", max_res))
    # the scene does what it is meant to: the keypoints outside a block find that block's face (nine voxels at most), the lone voxel's find 7
    assert np.all(got[0]["ncand"][absent] > 0) and np.all(got[0]["ncand"][-3:-1] == 7)
    assert all(g["neq"].num_fallback == 0 for g in got), [g["neq"].num_fallback for g in got]


# ------------------------------------------------------------------------------------------------ 3. a solve
def test_solved_state_is_the_same(dense, oracle_lib, oracle_backend):
    """0 against 1 bit for bit, and both against the oracle's updateIEKF within the 1e-9 the smoke run grants that comparison"""
    sw = dense["sw"]
    st = np.concatenate([sw["q_pred"], sw["t_pred"], sw["vel"], np.zeros(6)])
    opts = srl.default_opts(max_num_residuals=INT_MAX)
    eo = oracle_lib.Eskf(oracle_backend)
    synth.eskf_prior(eo, sw["q_pred"], sw["t_pred"], sw["vel"])
    prior_state, prior_cov = eo.get_state().copy(), eo.get_cov().copy()
    o = oracle_lib.update_iekf(dense["omap"], eo, oracle_lib.opts_from_product(opts), sw["raw"], st, sw["t_last"], log_iters=8)
    out = []
    for records in (0, 1):
        lio = srl.Lio(0)
        try:
            lio.ctx.set_neighbour_records(records)
            lio.add_points_to_map(dense["cands"])
            lio.eskf_set_state(prior_state)
            lio.eskf_set_cov(prior_cov)
            out.append(lio.update_iekf(opts, sw["raw"], st, sw["t_last"], log_iters=8))
        finally:
            lio.close()
    a, b = out
    assert a["rc"] == b["rc"] == 0 and a["iters"] == b["iters"] >= 2 and a["num_residuals"] == b["num_residuals"]
    assert np.asarray(a["state"]).tobytes() == np.asarray(b["state"]).tobytes()
    assert b["iters"] == o["rc"], (b["iters"], o["rc"])
    err = float(np.max(np.abs(b["state"] - o["state"])) / np.max(np.abs(o["state"])))
    assert err < 1e-9, err


# ------------------------------------------------------------------------------------------------ 4. armed launches across a map edit
def test_armed_stream_across_a_map_insertion(dense, oracle_lib, oracle_backend):
    """sixteen-wave workgroups (fused final reduction: what an armed launch needs), no taps; sweep 1, an insertion into the map, sweep 2.
    The insertion cancels the launch armed behind sweep 1's last pass and brings the records up to date for sweep 2."""
    sw1 = dense["sw"]
    sw2 = synth.make_sweep(7303, 1_999, dense["L"])
    extra = synth.map_candidates(7304, 4_000)[0]
    out, stats = [], []
    for records in (0, 1):
        c = srl.Context(0)
        try:
            c.set_launch_shape(8, 16)
            c.set_arm_linger(host_linger_us=1e5, kernel_linger_us=2e5)     # an interpreter sits between two passes here, not a C loop
            c.map_insert(dense["cands"])
            res = _passes(c, sw1["raw"], _poses(sw1, 3, 1), records, sw1["t_last"], armed=2, taps=False, bounds_every_pass=False)
            c.map_insert(extra)
            res += _passes(c, sw2["raw"], _poses(sw2, 3, 2), records, sw2["t_last"], armed=2, taps=False, bounds_every_pass=False)
            res += _passes(c, sw2["raw"], _poses(sw2, 2, 3), records, sw2["t_last"], armed=0, taps=True)
            out.append(res); stats.append(c.arm_stats())
            map_after = c.map_download()
        finally:
            c.close()
    for k, (g, r) in enumerate(zip(out[1], out[0])):
        _same((g["neq"], g["ids"]), (r["neq"], r["ids"]), ("armed", k))
        assert g["neq"].num_fallback == r["neq"].num_fallback, ("armed", k)
        assert (g["bounds"] is None) == (r["bounds"] is None) and (g["bounds"] is None or g["bounds"].tobytes() == r["bounds"].tobytes()), ("armed", k)
    # the armed passes carry no taps (a tap read-back cancels a waiting launch): the CPU checks the two tapped passes behind them, on the
    # map as the insertion left it
    m = oracle_lib.Map(oracle_backend)
    m.import_(*map_after)
    oo = oracle_lib.default_opts(max_num_residuals=INT_MAX)
    orc = [m.build_plane_residuals(oo, sw2["raw"], q, t, sw2["t_last"], frame_id=100) for q, t in _poses(sw2, 2, 3)]
    _against_oracle(out[1][-2:], orc, "armed, behind the insertion")
    print("arm statistics, records off / on:", stats)
    assert all(s["fired"] >= 2 for s in stats), stats


# ------------------------------------------------------------------------------------------------ 5. two shards
class _Rank(sh.ContextRank):
    def __init__(self, rank, G, coll, map_arrays, records):
        super().__init__(rank, G, coll, map_arrays)
        self.ctx.set_neighbour_records(records)

    def do_map_records(self):
        return self.ctx.neighbour_records_download()


def test_two_shards_each_with_its_own_records(dense, oracle_lib):
    sw = dense["sw"]
    map_arrays = dense["ctx"].map_download()
    poses = _poses(sw, 3, 1)
    extra = synth.map_candidates(7305, 3_000)[0]
    script = [("upload", sw["raw"])]
    for max_res in (INT_MAX, 600):
        script += [("pass", q, t, sw["t_last"], dict(max_num_residuals=max_res), True, 100) for q, t in poses]
    script += [("map_insert", extra), ("map_records",)]
    script += [("pass", q, t, sw["t_last"], dict(max_num_residuals=INT_MAX), True, 100) for q, t in poses[:2]]
    runs = []
    for records in (0, 1):
        results, errors = sh.run(2, lambda rank, coll: _Rank(rank, 2, coll, map_arrays, records), script)
        err = sh.first_error(errors)
        assert err is None, (records, repr(err), errors)
        runs.append(results)
    off, on = runs
    for r in range(2):
        for i, s in enumerate(script):
            if s[0] == "pass":
                assert on[r][i]["rc"] == off[r][i]["rc"] and sh.records_equal(on[r][i]["neq"], off[r][i]["neq"]), (r, i)
                assert sh.taps_equal(on[r][i], off[r][i]), (r, i)
                assert sh.records_equal(on[r][i]["neq"], on[0][i]["neq"]), (r, i)
    # the passes without a budget in front of the insertion against the oracle over the whole sweep: the ranks' ranges, in rank order
    oo = oracle_lib.default_opts(max_num_residuals=INT_MAX)
    for i, (q, t) in enumerate(poses, start=1):
        o = dense["omap"].build_plane_residuals(oo, sw["raw"], q, t, sw["t_last"], frame_id=100)
        ids = np.concatenate([on[0][i]["ids"], on[1][i]["ids"]])
        status = np.concatenate([on[0][i]["status"], on[1][i]["status"]])
        assert np.array_equal(ids, o["ids"]) and np.array_equal(status, o["status"]), ("shards against the oracle", i)
        assert on[0][i]["neq"]["sum_candidates"] == o["neq"].sum_candidates, i
    i_rec = script.index(("map_records",))
    assert sh.same_bytes(on[0][i_rec], on[1][i_rec]) and sh.same_bytes(on[0][i_rec], off[0][i_rec]), "the replicated map: the same records on every rank"
