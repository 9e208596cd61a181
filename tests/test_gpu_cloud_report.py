"""What a map insertion stored (cloud_world: addPointToMap -> addPointToPcl, lioOptimization.cpp:428-429, 1346-1355) on the device:
srl_map_insert_report / srl_frame_commit_report and the mirror's points_world.

Every comparison is bit for bit.  The expected outcome of every point comes from tests/cloud_checker.py (the batch inserted one point at a
time into an oracle map; tied to the reference's own addPointToMap by tests/test_cloud_checker_reference.py), the expected cloud follows
from it in NumPy.  Every case also runs the PLAIN call on a second context and asserts the same map (keys, counts, xyz, order) and the
same num_added."""
import numpy as np
import pytest

import cloud_checker as cc
import sr_livo_amd as srl
from sr_livo_amd import capi, synth

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
SRL_ERR_UNSUPPORTED = -4      # include/srlivo_hip.h: srl_status
ROW = np.dtype([("x", "<u4"), ("y", "<u4"), ("z", "<u4")])
KW = dict(voxel_size=0.5, cap=20, min_dist=0.1)


def _omap(po, backend, m=None):
    om = po.Map(backend)
    if m is not None and len(m[1]):
        om.import_(*m)
    return om


def _same_map(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(cc.bits(a[2]), cc.bits(b[2]))


def _invariants(outcome, cloud, added, before, after, m_after):
    """what must hold over ALL points whatever the batch: the counts against the map's growth, and every record's position among the
    stored points of slots >= 1 (a creator sits in slot 0 and is not published)"""
    dv, dp = after[1] - before[1], after[0] - before[0]
    assert int((outcome == 2).sum()) == dv
    assert int((outcome == 1).sum()) == dp - dv == len(cloud)
    assert int((outcome != 0).sum()) == added == dp
    assert cloud.dtype == np.float32 and cloud.shape == (dp - dv, 4)
    if len(cloud):
        k, c, x = m_after
        live = np.arange(x.shape[1])[None, :] < c[:, None]
        live[:, 0] = False
        stored = np.ascontiguousarray(cc.bits(x)[live]).view(ROW).ravel()
        assert np.isin(np.ascontiguousarray(cc.bits(cloud[:, :3])).view(ROW).ravel(), stored).all()


def _report_vs_checker(rep, plain, om, batch, ref_z, kw, call=None, only=None):
    """one report insertion on `rep` against the plain insertion on `plain` and the checker on the oracle map `om` (all three hold the
    same map on entry and on return).  call: the report call to make instead of rep.map_insert_report.  Returns (outcome, cloud)."""
    before = rep.map_size()
    outcome, cloud, added = call() if call else rep.map_insert_report(batch, ref_z=ref_z, **kw)
    assert plain.map_insert(batch, **kw) == added
    m_r, m_p = rep.map_download(), plain.map_download()
    _same_map(m_r, m_p)
    assert rep.map_size() == plain.map_size()
    _invariants(outcome, cloud, added, before, rep.map_size(), m_r)
    want = cc.classify(om, batch, only=only, **kw)
    assert np.array_equal(outcome, want), np.flatnonzero(outcome != want)[:8]
    assert np.array_equal(cc.bits(cloud), cc.bits(cc.cloud_of(want, batch, ref_z)))
    _same_map(m_r, om.export())
    return outcome, cloud


def _world(sw):
    return sw["raw"] @ synth.quat_to_rot(sw["q_pred"]).T + sw["t_pred"]


@pytest.fixture(scope="module")
def room():
    """candidate points of one room, shuffled: [0, 40 000) is the base map of the cases that need one, the rest feeds the batches"""
    pts, L = synth.map_candidates(6101, 1_048_577)
    rng = np.random.default_rng(6102)
    pts = pts[rng.permutation(len(pts))]
    assert len(pts) >= 40_000 + 1_048_577
    return dict(base=pts[:40_000].copy(), rest=pts[40_000:], L=L)


def _pair(room=None, kw=KW):
    rep, plain = srl.Context(0), srl.Context(0)
    if room is not None:
        rep.map_insert(room["base"], **kw)
        plain.map_insert(room["base"], **kw)
    return rep, plain


# ------------------------------------------------------------------------------------------------ 1. consecutive sweeps, growing map
@pytest.mark.parametrize("min_num_points", [0, 3])
def test_five_sweeps_into_a_growing_map(room, oracle_lib, oracle_backend, min_num_points):
    kw = dict(voxel_size=1.0, cap=20, min_dist=0.1, min_num_points=3) if min_num_points else dict(voxel_size=0.15, cap=20, min_dist=0.04, min_num_points=0)
    # min_num_points 3 never opens a voxel (lioOptimization.cpp:437): that run appends to a dense map that exists; 0 starts from nothing
    rep, plain = _pair()
    try:
        if min_num_points:
            dense = np.ascontiguousarray(room["rest"][-400_000:])
            rep.map_insert(dense, **dict(kw, min_num_points=0)); plain.map_insert(dense, **dict(kw, min_num_points=0))
        om = _omap(oracle_lib, oracle_backend, rep.map_download() if min_num_points else None)
        seen = set()
        grew = []
        for s in range(5):
            sw = synth.make_sweep(6110 + s, 24_000, room["L"])
            batch = _world(sw)
            outcome, _ = _report_vs_checker(rep, plain, om, batch, float(sw["t_pred"][2]), kw)
            seen |= set(np.unique(outcome).tolist())
            grew.append(rep.map_size())
        assert seen == ({0, 1} if min_num_points else {0, 1, 2})
        assert grew[-1][0] > grew[0][0]
        if not min_num_points:
            # a frame-sized insertion reserves slabs for (voxels + n) * 1.5 up front: the first call leaves room for 36 000, so the later
            # ones grow slabs and table again once the map holds more than 12 000 voxels
            assert all(b[1] > a[1] for a, b in zip(grew, grew[1:])) and grew[2][1] > 12_000
    finally:
        rep.close(); plain.close()


# ------------------------------------------------------------------------------------------------ 2. every branch, by construction
def test_a_batch_built_to_hit_every_branch(oracle_lib, oracle_backend):
    kw = dict(voxel_size=1.0, cap=20, min_dist=0.25, min_num_points=0)
    ref_z = 1234.56789
    rng = np.random.default_rng(6120)
    rep, plain = _pair()
    try:
        om = _omap(oracle_lib, oracle_backend)
        # (a) the empty map: one creator per voxel and, later in the batch, points too close to them -- outcomes 0 and 2 only, no cloud
        creators = np.array([[x + 0.5, y + 0.5, 0.5] for x in range(1, 13) for y in range(1, 13)])
        close = creators[::3] + np.array([0.1, 0.0, 0.05])
        outcome, cloud = _report_vs_checker(rep, plain, om, np.concatenate([creators, close]), ref_z, kw)
        assert set(np.unique(outcome).tolist()) == {0, 2} and len(cloud) == 0
        assert (outcome[: len(creators)] == 2).all() and (outcome[len(creators):] == 0).all()
        # (b) everything else in one batch; `tag` remembers where each group went after the shuffle of the groups' interleaving
        g = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(4), indexing="ij"), -1).reshape(-1, 3) * 0.3 + np.array([10.05, 10.05, 10.05])
        fill = g[rng.permutation(len(g))]                                                 # 36 points 0.3 apart in ONE new voxel: 20 fit
        near = np.array([[30.5, 30.5, 30.5], [30.6, 30.5, 30.5], [31.5, 30.5, 30.5], [31.5, 30.62, 30.5]])     # pairs 0.1 / 0.12 apart
        exact = np.array([[5.25, 5.5, 5.5], [5.5, 5.5, 5.5]])                             # FP64 squared distance == 0.25^2: `>` rejects
        chain = np.array([[20.1, 20.1, 20.1], [20.5, 20.1, 20.1], [20.9, 20.1, 20.1]])    # a creator and two appenders
        faces = np.array([[-0.3, 20.5, 0.5], [0.3, 20.5, 0.5], [-0.9, 20.5, 0.5], [-1.2, 20.5, 0.5], [-1.7, -20.4, 0.4], [-0.99, -20.9, -0.2],
                          [0.7, -20.1, -0.6]])                                            # short() truncates towards zero: -0.3 and 0.3 share voxel 0
        into_a = creators[1::2] + np.array([0.3, 0.3, 0.3])                               # appended to voxels of (a)
        groups = dict(fill=fill, near=near, exact=exact, chain=chain, faces=faces, into_a=into_a)
        batch = np.concatenate(list(groups.values()))
        tag = np.concatenate([np.full(len(v), i) for i, v in enumerate(groups.values())])
        # interleave the groups (a stable merge of random ranks keeps every group's own order)
        rank = np.concatenate([np.sort(rng.random(len(v))) for v in groups.values()])
        order = np.argsort(rank, kind="stable")
        batch, tag = batch[order], tag[order]
        outcome, cloud = _report_vs_checker(rep, plain, om, batch, ref_z, kw)
        names = list(groups)
        o = {n: outcome[tag == i] for i, n in enumerate(names)}
        assert o["fill"].tolist() == [2] + [1] * 19 + [0] * 16                           # the tail was never visited
        assert o["near"].tolist() == [2, 0, 2, 0]
        assert o["exact"].tolist() == [2, 0]
        assert o["chain"].tolist() == [2, 1, 1]
        assert o["faces"].tolist() == [2, 1, 1, 2, 2, 2, 1]                              # -0.3, 0.3, -0.9 share key 0; so do -0.99 / 0.7, -20.9 / -20.1, -0.2 / -0.6
        assert (o["into_a"] == 1).all()
        exactly = cloud[:, 3].astype(np.float64) != 50.0 * (cloud[:, 2].astype(np.float64) - ref_z)
        assert exactly.any()                                                              # the intensity's one rounding is visible
        # (c) min_num_points 3 on that map: voxels with fewer residents refuse, absent voxels are never looked at, fuller ones append
        kw3 = dict(kw, min_num_points=3)
        absent = np.array([[40.5, 40.5, 40.5], [41.5, 40.5, 40.5], [40.5, 40.5, 40.5]])
        thin = np.array([[30.9, 30.9, 30.9], [5.9, 5.9, 5.9]])                            # voxels with one stored point
        full = np.array([[10.5, 10.5, 10.95], [10.95, 10.95, 10.95]])                     # the voxel filled above
        fat = np.array([[20.1, 20.5, 20.1], [20.1, 20.9, 20.5]])                          # the chain's voxel: 3 stored
        batch3 = np.concatenate([absent, thin, full, fat])[[0, 3, 5, 7, 1, 4, 6, 8, 2]]
        outcome3, _ = _report_vs_checker(rep, plain, om, batch3, -ref_z, kw3)
        assert outcome3.tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0]
    finally:
        rep.close(); plain.close()


# ------------------------------------------------------------------------------------------------ 3. both sides of every path switch
SIZES = [1, 63, 64, 65, 131_072, 131_073, 262_144, 1_048_576, 1_048_577]
SAMPLED_FROM = 1_048_576      # from here on the one-at-a-time loop runs over the points of 2 000 voxels


@pytest.mark.parametrize("n", SIZES)
def test_sizes_on_both_sides_of_every_path_switch(room, oracle_lib, oracle_backend, n):
    kw = dict(KW, min_num_points=0)
    batch = np.ascontiguousarray(room["rest"][:n])
    ref_z = 0.625
    rep, plain = _pair(room)
    try:
        m_before = rep.map_download()
        om = _omap(oracle_lib, oracle_backend, m_before)
        if n < SAMPLED_FROM:
            outcome, _ = _report_vs_checker(rep, plain, om, batch, ref_z, kw)
            if n >= 131_072:
                assert set(np.unique(outcome).tolist()) == {0, 1, 2}
            return
        # voxels are independent of each other in addPointToMap: all points of 2 000 voxels, in batch order, on a map that holds what
        # the device map held before the call; and the WHOLE map after the call against the oracle's whole-batch insertion
        before = rep.map_size()
        outcome, cloud, added = rep.map_insert_report(batch, ref_z=ref_z, **kw)
        assert plain.map_insert(batch, **kw) == added
        m_r = rep.map_download()
        _same_map(m_r, plain.map_download())
        _invariants(outcome, cloud, added, before, rep.map_size(), m_r)
        keys = cc.voxel_keys(batch, kw["voxel_size"]).astype(np.int64)
        packed = (keys[:, 0] + 32768) << 32 | (keys[:, 1] + 32768) << 16 | (keys[:, 2] + 32768)
        uniq = np.unique(packed)
        drawn = np.random.default_rng(6130).choice(uniq, 2000, replace=False)
        only = np.flatnonzero(np.isin(packed, drawn))
        want = cc.classify(om, batch, only=only, **kw)
        assert np.array_equal(outcome[only], want[only])
        assert {0, 1, 2} <= set(np.unique(want[only]).tolist())
        where = np.cumsum(outcome == 1) - 1                                               # record index of every appended point
        sel = only[want[only] == 1]
        assert np.array_equal(cc.bits(cloud[where[sel]]), cc.bits(cc.cloud_of(want, batch, ref_z)))
        whole = _omap(oracle_lib, oracle_backend, m_before)
        assert whole.add_points(batch, **kw) == added
        _same_map(m_r, whole.export())
    finally:
        rep.close(); plain.close()


# ------------------------------------------------------------------------------------------------ 4. the frame commit
def _pose():
    q = synth.quat_from_rotvec([0.11, -0.23, 0.71])
    t = np.array([1.37, -2.11, 0.83])
    R_il = synth.quat_to_rot(synth.quat_from_rotvec([0.02, 0.01, -0.03]))
    t_il = np.array([0.04, -0.02, 0.11])
    return q, t, R_il, t_il


def test_frame_commit_report_equals_the_plain_commit_and_the_checker(room, oracle_lib, oracle_backend):
    kw = dict(KW, min_num_points=0)
    sw = synth.make_sweep(6140, 24_000, room["L"])
    q, t, R_il, t_il = _pose()
    rep, plain = _pair(room)
    try:
        om = _omap(oracle_lib, oracle_backend, rep.map_download())
        before = rep.map_size()
        rep.frame_upload(sw["raw"]); plain.frame_upload(sw["raw"])
        outcome, cloud, added, world = rep.frame_commit_report(q, t, R_il=R_il, t_il=t_il, want_world=True, **kw)
        world_p, added_p = plain.frame_commit(q, t, R_il=R_il, t_il=t_il, **kw)
        assert np.array_equal(world.view(np.uint64), world_p.view(np.uint64)) and added == added_p
        m_r = rep.map_download()
        _same_map(m_r, plain.map_download())
        _invariants(outcome, cloud, added, before, rep.map_size(), m_r)
        want = cc.classify(om, world, **kw)
        assert np.array_equal(outcome, want)
        assert np.array_equal(cc.bits(cloud), cc.bits(cc.cloud_of(want, world, t[2])))
        assert set(np.unique(outcome).tolist()) == {0, 1, 2}
        _same_map(m_r, om.export())
        # without any output but the counts (every pointer optional)
        rep.frame_upload(sw["raw"] * 0.97); plain.frame_upload(sw["raw"] * 0.97)
        nc, na = capi.C.c_int(-1), capi.C.c_int(-1)
        d = capi._dptr
        rc = rep.lib.srl_frame_commit_report(rep.h, d(capi._f64(q)), d(capi._f64(t)), d(capi._f64(R_il).ravel()), d(capi._f64(t_il)), kw["voxel_size"], 20,
                                             kw["min_dist"], 0, None, None, None, capi.C.byref(nc), capi.C.byref(na))
        assert rc == capi.SRL_OK
        _, added_p = plain.frame_commit(q, t, R_il=R_il, t_il=t_il, **kw)
        assert na.value == added_p and 0 < nc.value <= na.value
        _same_map(rep.map_download(), plain.map_download())
    finally:
        rep.close(); plain.close()


def test_refusals_on_a_live_context(room):
    rep = srl.Context(0)
    try:
        pts = np.ascontiguousarray(room["rest"][:100])
        o, c, a = rep.map_insert_report(pts[:0], **KW)                                    # n == 0: SRL_OK, counts 0, no map needed
        assert len(o) == 0 and len(c) == 0 and a == 0
        rep.map_insert(room["base"][:5000], **KW)
        before = rep.map_download()
        nc, na = capi.C.c_int(7), capi.C.c_int(7)
        rc = rep.lib.srl_map_insert_report(rep.h, capi._ptr(pts), 100, 0.5, 19, 0.1, 0, 0.0, None, None, capi.C.byref(nc), capi.C.byref(na))
        assert rc == SRL_ERR_UNSUPPORTED and (nc.value, na.value) == (0, 0)               # cap != 20
        _same_map(before, rep.map_download())
    finally:
        rep.close()


# ------------------------------------------------------------------------------------------------ 5. behind a deferred commit / an armed launch
def test_report_calls_behind_a_deferred_commit(room, oracle_lib, oracle_backend):
    kw = dict(KW, min_num_points=0)
    sw1, sw2 = synth.make_sweep(6150, 24_000, room["L"]), synth.make_sweep(6151, 24_000, room["L"])
    batch = np.ascontiguousarray(room["rest"][:30_000])
    q, t, R_il, t_il = _pose()
    rep, plain = _pair(room)
    try:
        om = _omap(oracle_lib, oracle_backend, rep.map_download())
        # (a) srl_map_insert_report while the previous frame's commit is only enqueued
        rep.frame_upload(sw1["raw"]); plain.frame_upload(sw1["raw"])
        world, none = rep.frame_commit(q, t, R_il=R_il, t_il=t_il, want_added=False, **kw)
        assert none is None
        # (no map_size() here: reading the size would settle the commit)
        outcome, cloud, added = rep.map_insert_report(batch, ref_z=0.5, **kw)
        world_p, _ = plain.frame_commit(q, t, R_il=R_il, t_il=t_il, **kw)                 # the synchronous sequence
        assert np.array_equal(world.view(np.uint64), world_p.view(np.uint64))
        assert plain.map_insert(batch, **kw) == added
        om.add_points(world, **kw)
        want = cc.classify(om, batch, **kw)
        assert np.array_equal(outcome, want) and np.array_equal(cc.bits(cloud), cc.bits(cc.cloud_of(want, batch, 0.5)))
        _same_map(rep.map_download(), plain.map_download())
        _same_map(rep.map_download(), om.export())
        # (b) srl_frame_commit_report behind a deferred commit
        rep.frame_upload(sw1["raw"] * 0.99); plain.frame_upload(sw1["raw"] * 0.99)
        w1, _ = rep.frame_commit(q, t, R_il=R_il, t_il=t_il, want_added=False, **kw)
        rep.frame_upload(sw2["raw"])
        outcome, cloud, added, w2 = rep.frame_commit_report(q, t, R_il=R_il, t_il=t_il, want_world=True, **kw)
        plain.frame_commit(q, t, R_il=R_il, t_il=t_il, **kw)
        plain.frame_upload(sw2["raw"])
        w2_p, added_p = plain.frame_commit(q, t, R_il=R_il, t_il=t_il, **kw)
        assert np.array_equal(w2.view(np.uint64), w2_p.view(np.uint64)) and added == added_p
        om.add_points(w1, **kw)
        want = cc.classify(om, w2, **kw)
        assert np.array_equal(outcome, want) and np.array_equal(cc.bits(cloud), cc.bits(cc.cloud_of(want, w2, t[2])))
        _same_map(rep.map_download(), plain.map_download())
        _same_map(rep.map_download(), om.export())
    finally:
        rep.close(); plain.close()


class _EskfAdapter:
    def __init__(self, lio): self.lio = lio
    def set_noise(self, *a): self.lio.eskf_set_noise(*a)
    def scale_init_cov(self): self.lio.eskf_scale_init_cov()
    def init_imu(self, a, g): self.lio.eskf_init_imu(a, g)
    def predict(self, dt, a, g): self.lio.eskf_predict(dt, a, g)
    def get_state(self): return self.lio.eskf_get_state()
    def set_state(self, s): self.lio.eskf_set_state(s)


def test_a_report_call_cancels_an_armed_launch_and_equals_the_synchronous_sequence(oracle_lib, oracle_backend):
    pts, L = synth.map_candidates(6160, 100_000)
    sw = synth.make_sweep(6161, 4096, L)
    batch = _world(synth.make_sweep(6162, 24_000, L))
    kw = dict(voxel_size=1.0, cap=20, min_dist=0.15, min_num_points=0)                    # the mirror's add_points_to_map defaults
    lio, plain = srl.Lio(0), srl.Context(0)
    try:
        lio.add_points_to_map(pts)
        plain.map_insert(pts, **kw)
        om = _omap(oracle_lib, oracle_backend, plain.map_download())
        prior_state = synth.eskf_prior(_EskfAdapter(lio), sw["q_pred"], sw["t_pred"], sw["vel"]).copy()
        prior_cov = lio.eskf_get_cov().copy()
        state0 = np.concatenate([sw["q_pred"], sw["t_pred"], sw["vel"], np.zeros(6)])
        lio.resident_sweep(sw["raw"])
        solve = lio.bound_solver(srl.default_opts(max_num_residuals=INT_MAX), prior_state, prior_cov, state0, sw["t_last"], 100, len(sw["raw"]))
        lio.ctx.set_armed_launch(2)
        solve(); solve()
        s0 = lio.ctx.arm_stats()
        outcome, cloud, added = lio.ctx.map_insert_report(batch, ref_z=-3.25, **kw)
        s1 = lio.ctx.arm_stats()
        assert s1["expired"] == s0["expired"] and s1["armed"] == s0["armed"]
        assert s1["cancelled"] - s0["cancelled"] == s0["armed"] - s0["fired"] - s0["cancelled"]      # cancelled by the call, not left to expire
        assert s1["armed"] == s1["fired"] + s1["cancelled"]
        assert plain.map_insert(batch, **kw) == added
        want = cc.classify(om, batch, **kw)
        assert np.array_equal(outcome, want) and np.array_equal(cc.bits(cloud), cc.bits(cc.cloud_of(want, batch, -3.25)))
        _same_map(lio.ctx.map_download(), plain.map_download())
        _same_map(lio.ctx.map_download(), om.export())
        rc, _, _ = solve()                                                                 # the next solve runs on the grown map
        assert rc == 0
    finally:
        lio.close(); plain.close()


# ------------------------------------------------------------------------------------------------ 6. nothing of the previous frame leaks
def test_the_previous_frames_outcomes_do_not_leak(room, oracle_lib, oracle_backend):
    kw = dict(voxel_size=2.0, cap=20, min_dist=0.1, min_num_points=0)                     # coarse voxels: many of them fill
    rep, plain = _pair()
    try:
        om = _omap(oracle_lib, oracle_backend)
        big = np.ascontiguousarray(room["rest"][:200_000])
        outcome, _ = _report_vs_checker(rep, plain, om, big, 0.0, kw)
        assert (outcome[:2000] != 0).mean() > 0.5                                         # the head of the array is full of 1s and 2s
        # the small batch is made of points that are never visited: voxels that do not exist under min_num_points 3, and the tails of
        # voxels that are full -- their bytes are whatever the kernel in front of the replay left there
        kw3 = dict(kw, min_num_points=3)
        k, c, x = rep.map_download()
        fullv = np.flatnonzero(c == 20)[:40]
        assert len(fullv) == 40
        tails = np.repeat((k[fullv].astype(np.float64) + np.where(k[fullv] >= 0, 0.5, -0.5)) * kw["voxel_size"], 8, axis=0)
        tails = tails + np.random.default_rng(6170).uniform(-0.2, 0.2, tails.shape) * kw["voxel_size"]
        absent = np.random.default_rng(6171).uniform(500.0, 520.0, (700, 3))
        small = np.concatenate([absent[:350], tails, absent[350:]])
        outcome, cloud = _report_vs_checker(rep, plain, om, small, 0.0, kw3)
        assert not outcome.any() and len(cloud) == 0
        # ... and a small ordinary batch behind it
        _report_vs_checker(rep, plain, om, np.ascontiguousarray(room["rest"][200_000:201_000]), 0.0, kw)
    finally:
        rep.close(); plain.close()


# ------------------------------------------------------------------------------------------------ 7. the mirror
def _replay(meas, oo, icp_p, collect, then):
    """the sequence through a fresh Lio (one at a time: the replay's initialisation flag is per process); per processed frame the
    state, the covariance, the counts and the cloud; then(lio, last result) runs on the live object before it is closed"""
    lio = srl.Lio(0)
    frames = []
    try:
        lio.set_initial_flag(False)
        lio.set_odometry_options(icp=icp_p, **oo)
        assert len(lio.points_world()) == 0
        lio.set_collect_points_world(collect)
        got = None
        for ms in meas:
            before = lio.ctx.map_size()
            r = lio.run_measurement(ms["time_frame"], ms["imu_t"], ms["imu_acc"], ms["imu_gyr"], ms["pts_raw"], ms["pts_timestamp"],
                                    ms["time_sweep_begin"], ms["time_sweep_offset"])
            assert r["rc"] == 0
            if not r["processed"]:
                frames.append(None)
                continue
            got = r
            frames.append(dict(state=np.array(r["state"], np.float64), cov=lio.eskf_get_cov().copy(), added=r["points_added"], iters=r["iters"],
                               before=before, after=lio.ctx.map_size(), cloud=lio.points_world()))
        return frames, then(lio, got)
    finally:
        lio.set_initial_flag(False)
        lio.close()


def test_the_mirror_collects_points_world_without_changing_the_replay(oracle_lib, oracle_backend):
    pts, L = synth.map_candidates(555, 60_000)
    meas, _, _ = synth.make_sequence(31, 7, 12_000, L)
    oo = dict(init_voxel_size=0.2, init_sample_voxel_size=1.0, init_num_frames=6, num_for_initialization=10, voxel_size=0.2,
              sample_voxel_size=1.5, max_num_points_in_voxel=20, min_distance_points=0.1, motion_compensation=capi.MC_CONSTANT_VELOCITY,
              initialization=0, point_time_enable=1, acc_cov=0.1, gyr_cov=0.1, b_acc_cov=1e-4, b_gyr_cov=1e-4)
    icp_p = srl.default_opts(max_num_residuals=600)
    kw = dict(voxel_size=0.2, cap=20, min_dist=0.1, min_num_points=0)
    raw = np.ascontiguousarray(meas[-1]["pts_raw"][:10_000])

    def then(lio, last):
        """commit_frame on a given state and add_points_to_map on the replay's final map"""
        out = dict(map0=lio.ctx.map_download())
        state = np.asarray(last["state"], np.float64).copy()
        state[4:7] += np.array([0.05, -0.03, 0.02])
        lio.ctx.frame_upload(raw)
        world, added = lio.commit_frame(state, **kw)
        out.update(state=state, world=world, added=added, cloud1=lio.points_world(), map1=lio.ctx.map_download())
        batch = world[:3000] + 0.07
        lio.add_points_to_map(batch, **kw)
        out.update(batch=batch, cloud2=lio.points_world(), map2=lio.ctx.map_download())
        lio.set_collect_points_world(False)
        lio.add_points_to_map(batch + 0.07, **kw)
        out.update(cloud3=lio.points_world())
        return out

    f_off, t_off = _replay(meas, oo, icp_p, False, then)
    f_on, t_on = _replay(meas, oo, icp_p, True, then)
    assert [f is None for f in f_on] == [f is None for f in f_off]
    published = []
    for a, b in zip(f_on, f_off):
        if a is None:
            continue
        assert np.array_equal(a["state"], b["state"]) and np.array_equal(a["cov"], b["cov"])
        assert (a["added"], a["iters"], a["before"], a["after"]) == (b["added"], b["iters"], b["before"], b["after"])
        assert len(a["cloud"]) == (a["after"][0] - a["before"][0]) - (a["after"][1] - a["before"][1])
        assert len(b["cloud"]) == 0
        # the records are points of the frame, and the intensity's reference is the frame's own translation.z()
        cloud = a["cloud"]
        assert np.array_equal(cc.bits(cloud[:, 3]), cc.bits((50.0 * (cloud[:, 2].astype(np.float64) - a["state"][6])).astype(np.float32)))
        published.append(len(cloud))
    assert len(published) >= 8 and sum(1 for m in published if m > 0) >= 6, published
    for k in ("map0", "map1", "map2"):
        _same_map(t_on[k], t_off[k])
    assert np.array_equal(t_on["world"].view(np.uint64), t_off["world"].view(np.uint64)) and t_on["added"] == t_off["added"]
    assert len(t_off["cloud1"]) == 0 and len(t_off["cloud2"]) == 0
    # commit_frame on a given state: the records against the checker on an oracle map holding what the device map held just before
    om = _omap(oracle_lib, oracle_backend, t_on["map0"])
    want = cc.classify(om, t_on["world"], **kw)
    assert int((want != 0).sum()) == t_on["added"] and (want == 1).any()
    assert np.array_equal(cc.bits(t_on["cloud1"]), cc.bits(cc.cloud_of(want, t_on["world"], t_on["state"][6])))
    _same_map(t_on["map1"], om.export())
    # add_points_to_map: the C handle builds the frame on a default state, translation 0
    want = cc.classify(om, t_on["batch"], **kw)
    assert (want == 1).any()
    assert np.array_equal(cc.bits(t_on["cloud2"]), cc.bits(cc.cloud_of(want, t_on["batch"], 0.0)))
    _same_map(t_on["map2"], om.export())
    assert len(t_on["cloud3"]) == 0                                                       # cleared at the start, not filled while off
