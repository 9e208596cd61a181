"""The measurement passes of the camera ESIKF on the device (srl_color_map_vio_rows: the per-point loops of imageProcessing::vioEsikf,
imageProcessing.cpp:308-349, and vioPhotometric, :463-518) against the sequential restatement of tests/vio_checker.py and the records of
tests/golden/golden_color_vio.npz.

Rows and outcomes are compared bit for bit.  A sum is compared with the checker's in-order sum within n_used * 2^-52 * sum |terms|, the
bound of reordering a sum of n_used doubles, the absolute sum taken from the checker; the device's order (64 points of a wave in list
order, the four waves, the workgroups in index order) IS the list's order up to 64 points, so there the sums are equal.  Counts are exact."""
import ctypes as C
import os

import numpy as np
import pytest

import color_checker as cc
import render_checker as rk
import vio_checker as vc
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRL_ERR_BAD_ARG, SRL_ERR_NO_MAP, SRL_ERR_NO_SWEEP = -3, -5, -6         # include/srlivo_hip.h: srl_status
SHAPES = (0, 1, 9, 10, 63, 64, 65, 255, 256, 257, 513, 1025)


def _cam(c):
    return capi.ColorCamera((C.c_double * 4)(*c.q), (C.c_double * 3)(*c.t), c.fx, c.fy, c.cx, c.cy, c.fov_margin)


def _args(sc, mode, ext=1, intr=1):
    return capi.ColorVioArgs(_cam(sc.camera), sc.time_td, (C.c_double * 9)(*sc.R), mode, ext, intr)


def _ctx():
    o = rk.OPT
    ctx = srl.Context(0)
    ctx.color_map_create(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
    return ctx


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_color_vio.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def device():
    """a device map holding render_checker's scene after its render sequence"""
    ctx = _ctx()
    visited = [ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)[2] for j in range(3)]
    for k in range(len(rk.RENDERS)):
        cam, which, obs_time, voxels = rk.render_call(k, visited)
        ctx.color_image_upload(rk.scene_image(which))
        ctx.color_map_render(_cam(cam), voxels, obs_time)
    assert rk.state_bytes(ctx.color_map_download_rgb()) == rk.state_bytes(rk.scene_sequence()[0].map_state())
    assert ctx.color_map_size()[0] == vc.scene(0).num_points
    yield ctx
    ctx.close()


def _upload(ctx, which):
    ctx.color_image_upload(rk.scene_image(which))


def _sums_vector(sums):
    """the 78 sums in the checker's order from the call's record; the record itself is full and symmetric, zero where it must be"""
    H, r, acc = sums.as_arrays()
    assert np.array_equal(H, H.T)
    return np.concatenate([[H[a, b] for a, b in vc.PAIRS], r, [acc]])


def _check(got, want, what, exact_sums=False):
    sums, rows, outcome = got
    assert outcome.tobytes() == want.outcome.tobytes(), (what, np.flatnonzero(outcome != want.outcome)[:8])
    assert rows.tobytes() == want.rows.tobytes(), (what, np.argwhere(rows.view(np.uint64) != want.rows.view(np.uint64))[:8])
    assert sums.counts() == want.counts, (what, sums.counts(), want.counts)
    dev = _sums_vector(sums)
    err = np.abs(dev - want.sums)
    assert (err <= want.bound()).all(), (what, np.flatnonzero(err > want.bound()), err.max())
    if exact_sums:
        assert np.array_equal(dev, want.sums), what
    return dev


# ------------------------------------------------------------------------------------------------ 1., 2. rows, outcomes, sums
@pytest.mark.parametrize("which", range(len(vc.SCENE_RENDERS)))
def test_rows_outcomes_and_sums_equal_the_restatement_and_the_golden(device, golden, which):
    sc = vc.scene(which)
    _upload(device, which)
    assert np.array_equal(golden["configs"], np.array(vc.CONFIGS)) and golden["s%d_points" % which].tobytes() == sc.points.tobytes()
    for c, ((mode, ext, intr), want) in enumerate(zip(vc.CONFIGS, vc.scene_results(which))):
        got = device.color_map_vio_rows(_args(sc, mode, ext, intr), sc.points)
        dev = _check(got, want, (which, mode, ext, intr))
        name = "s%d_c%d" % (which, c)
        assert vc.golden_check(golden, name, got[1], got[2]) is None, name
        err = np.abs(dev - golden[name + "_sums"])
        assert (err <= want.bound()).all(), name
        H, r, _ = got[0].as_arrays()
        if mode == vc.PHOTOMETRIC:
            assert not H[6:, :].any() and not H[:, 6:].any() and not r[6:].any()
        assert got[0].used >= 10 and H[0, 0] > 0 if mode == vc.REPROJECTION else got[0].acc_residual > 0


# ------------------------------------------------------------------------------------------------ 3. determinism
def test_two_calls_give_the_same_bytes_with_and_without_rows_or_outcomes(device):
    sc = vc.scene(1)
    _upload(device, 1)
    for mode in (vc.REPROJECTION, vc.PHOTOMETRIC):
        base = vc.scene_results(1)[vc.CONFIGS.index((mode, 1, 1))]
        index = vc.cut_or_cycle(len(sc.points), 1025)                      # five workgroups: the ticket and the rows take part
        pts = sc.points[index]
        first = device.color_map_vio_rows(_args(sc, mode), pts)
        ref = bytes(first[0])
        assert first[0].used == base.take(index).counts[vc.USED] > 64
        for with_rows, with_outcome in ((True, True), (False, False), (True, False), (False, True), (True, True)):
            again = device.color_map_vio_rows(_args(sc, mode), pts, with_rows, with_outcome)
            assert bytes(again[0]) == ref, (mode, with_rows, with_outcome)
            assert again[1] is None or again[1].tobytes() == first[1].tobytes()
            assert again[2] is None or again[2].tobytes() == first[2].tobytes()


# ------------------------------------------------------------------------------------------------ 4. wave and workgroup edges
@pytest.mark.parametrize("mode", (vc.REPROJECTION, vc.PHOTOMETRIC))
def test_list_lengths_at_wave_and_workgroup_edges(device, mode):
    sc = vc.scene(1)
    _upload(device, 1)
    base = vc.scene_results(1)[vc.CONFIGS.index((mode, 1, 1))]
    for n in SHAPES:
        index = vc.cut_or_cycle(len(sc.points), n)
        want = base.take(index)
        got = device.color_map_vio_rows(_args(sc, mode), sc.points[index])
        if n == 0:
            assert got[0].counts() == (0,) * 5 and not any(got[0].HtH[:]) and not any(got[0].Htr[:]) and got[0].acc_residual == 0.0
            continue
        _check(got, want, (mode, n), exact_sums=n <= 64)
        assert n < 10 or got[0].used > 0


# ------------------------------------------------------------------------------------------------ 5. outcome classes
def test_every_outcome_class_and_the_footprints_edges(device):
    sc = vc.scene(1)
    _upload(device, 1)
    edges, designed = vc.edge_list(sc)
    pts = np.concatenate([edges, sc.points])
    assert -1 in pts["pool"] and sc.num_points in pts["pool"]
    want = vc.vio_rows(sc, vc.PHOTOMETRIC, points=pts)
    assert tuple(want.outcome[:len(edges)]) == designed and all(c > 0 for c in want.counts)      # from the checker alone
    _check(device.color_map_vio_rows(_args(sc, vc.PHOTOMETRIC), pts), want, "classes")
    # in reprojection mode the views and the image are not asked
    want = vc.vio_rows(sc, vc.REPROJECTION, points=pts)
    assert want.counts[vc.FEW_VIEWS] == 0 and want.counts[vc.OUTSIDE] == 0 and want.counts[vc.BEHIND] > 0 and want.counts[vc.UNKNOWN] == 2
    _check(device.color_map_vio_rows(_args(sc, vc.REPROJECTION), pts), want, "classes, reprojection")


def test_on_a_map_never_rendered_every_point_has_too_few_views():
    sc = vc.scene(0)
    ctx = _ctx()
    try:
        for j in range(3):
            ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)
        pts = sc.points[(sc.points["pool"] >= 0) & (sc.points["pool"] < sc.num_points)]
        want = vc.vio_rows(sc, vc.REPROJECTION, points=pts)
        _check(ctx.color_map_vio_rows(_args(sc, vc.REPROJECTION), pts), want, "reprojection needs neither image nor state")
        ctx.color_image_upload(rk.scene_image(0))
        sums, rows, outcome = ctx.color_map_vio_rows(_args(sc, vc.PHOTOMETRIC), pts)
        assert (outcome == vc.FEW_VIEWS).all() and sums.counts() == (0, len(pts), 0, 0, 0) and not rows.any()
        assert not any(sums.HtH[:]) and not any(sums.Htr[:]) and sums.acc_residual == 0.0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 6. the mirror on the device
def _lio_with_scene():
    lio = srl.Lio(0)
    o = rk.OPT
    lio.ctx.color_map_create(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
    visited = [lio.ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)[2] for j in range(3)]
    for k in range(len(rk.RENDERS)):
        cam, which, obs_time, voxels = rk.render_call(k, visited)
        lio.ctx.color_image_upload(rk.scene_image(which))
        lio.ctx.color_map_render(_cam(cam), voxels, obs_time)
    return lio


def test_the_mirrors_updates_through_the_handles_against_the_golden(golden):
    """vioEsikf then vioPhotometric with the device's measurement pass, against the states and covariances recorded from the literal
    update; the tolerance is the one measured and recorded in tests/test_host_vio_mirror.py"""
    import test_host_vio_mirror as hm
    lio = _lio_with_scene()
    try:
        for which in range(len(vc.SCENE_RENDERS)):
            lio.ctx.color_image_upload(rk.scene_image(which))
            got = hm.run_sequence(lio, which)
            for name, g in zip(("esikf", "photometric"), got):
                w_states, w_cov = golden["s%d_%s_states" % (which, name)], golden["s%d_%s_cov" % (which, name)]
                accepted, used = (int(v) for v in golden["s%d_%s_used" % (which, name)])
                assert g[0] == bool(accepted) and len(g[1]) == len(w_states) >= 1 and g[3] == used >= 10, (which, name, len(g[1]), g[3])
                d = vc.difference(g[1], g[2], w_states, w_cov)
                print("scene %d %s on the device: largest difference %.3e" % (which, name, d))
                assert d <= hm.TOLERANCE, (which, name, d)
        # fewer than ten tracked points: nothing is done, nothing launched
        sc = vc.scene(0)
        for (ok, states, cov, used) in hm.run_sequence(lio, 0, sc.points[:9]):
            assert not ok and len(states) == 0 and np.array_equal(cov, vc.initial_cov())
        # twelve tracked points of which nine are used: the gate breaks the loop, the covariance update runs on zeros
        nine = sc.points[vc.scene_results(0)[0].outcome == vc.USED][:9]
        unknown = np.zeros(3, vc.POINT_DTYPE); unknown["pool"] = -1
        a, b = hm.run_sequence(lio, 0, np.concatenate([nine, unknown]))
        assert a[0] and len(a[1]) == 0 and a[3] == 9 and np.array_equal(a[2], vc.initial_cov())
        assert b[0] and len(b[1]) == 0 and b[3] < 10 and np.array_equal(b[2], vc.initial_cov())
        assert np.array_equal(lio.vio_get_camera_state(), vc.initial_state(0).vector())
    finally:
        lio.close()


# ------------------------------------------------------------------------------------------------ 7. status codes
def test_status_codes():
    sc = vc.scene(0)
    ctx = srl.Context(0)
    try:
        lib = ctx.lib
        pts = np.ascontiguousarray(sc.points[:4])

        def call(args=None, points=pts, n=4, with_args=True, with_sums=True):
            sums = capi.ColorVioSums()
            sums.used, sums.HtH[0] = 7, 7.0
            a = _args(sc, vc.REPROJECTION) if args is None else args
            rc = lib.srl_color_map_vio_rows(ctx.h, C.byref(a) if with_args else None, capi._ptr(points), n, C.byref(sums) if with_sums else None, None, None)
            assert rc == capi.SRL_OK or (sums.counts() == (0,) * 5 and sums.HtH[0] == 0.0) or not with_sums
            return rc
        assert call() == SRL_ERR_NO_MAP
        ctx.color_map_create()
        ctx.color_map_insert(cc.scene_batch(0)[:500], 1.0, 0.0)
        assert call() == capi.SRL_OK and call(n=0) == capi.SRL_OK and call(points=None, n=0) == capi.SRL_OK
        assert call(n=-1) == SRL_ERR_BAD_ARG and call(points=None) == SRL_ERR_BAD_ARG
        assert call(with_args=False) == SRL_ERR_BAD_ARG and call(with_sums=False) == SRL_ERR_BAD_ARG
        big = np.zeros(capi.SRL_COLOR_VIO_MAX_POINTS + 1, capi.COLOR_VIO_POINT_DTYPE)
        assert call(points=big, n=len(big)) == SRL_ERR_BAD_ARG and call(points=big, n=len(big) - 1) == capi.SRL_OK
        for mode in (-1, 2):
            assert call(args=_args(sc, mode)) == SRL_ERR_BAD_ARG
        bad = _args(sc, vc.REPROJECTION); bad.time_td = float("nan")
        assert call(args=bad) == SRL_ERR_BAD_ARG
        bad = _args(sc, vc.REPROJECTION); bad.R_imu_camera[4] = float("inf")
        assert call(args=bad) == SRL_ERR_BAD_ARG
        bad = _args(sc, vc.REPROJECTION); bad.cam.fx = float("nan")
        assert call(args=bad) == SRL_ERR_BAD_ARG
        bad = _args(sc, vc.REPROJECTION); bad.cam.t_world_camera[2] = float("inf")
        assert call(args=bad) == SRL_ERR_BAD_ARG
        ok = _args(sc, vc.REPROJECTION); ok.cam.fov_margin = float("nan")   # ignored
        assert call(args=ok) == capi.SRL_OK
        assert call(args=_args(sc, vc.PHOTOMETRIC)) == SRL_ERR_NO_SWEEP
        ctx.color_image_upload(rk.scene_image(0))
        assert call(args=_args(sc, vc.PHOTOMETRIC)) == capi.SRL_OK
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])       # more than one rank: what the render returns
        assert call() == capi.SRL_ERR_UNSUPPORTED
        ctx.comm_set_host_callbacks(1, 0, None, None)
        assert call() == capi.SRL_OK
    finally:
        ctx.close()
