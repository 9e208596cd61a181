"""imageProcessing::process of the host mirror (csrc/host/imageProcessing.cpp; srl_lio_image_process of include/srlivo_host.h) without a
device: every step that leaves the mirror is replaced by a recording stand-in (srl_lio_image_set_steps) on a host-only handle, and the
records pin the order of the reference's statements (src/imageProcessing.cpp:89-164), its gates, the first-data branch and the
arguments each step is handed.  The stand-ins are trivial on purpose: the flow moves every point by (2, 1), both consensus steps keep
what they are told to keep, the measurement pass returns empty sums, the track-update keeps every tracked point."""
import ctypes as C

import numpy as np
import pytest

import sr_livo_amd as srl
from sr_livo_amd import capi

SRL_OK, SRL_ERR_NO_DEVICE, SRL_ERR_BAD_ARG, SRL_ERR_UNSUPPORTED = 0, -1, -3, -4
FX, FY, CX, CY = 95.0, 97.0, 52.5, 36.5
DIST = [0.1, -0.02, 0.001, -0.002, 0.003]
SEL = capi.COLOR_SELECTED_DTYPE
TRK = capi.COLOR_TRACK_POINT_DTYPE


def _view(address, count, dtype):
    dtype = np.dtype(dtype)
    if not count or not address:
        return np.zeros(0, dtype)
    return np.frombuffer((C.c_char * (count * dtype.itemsize)).from_address(address), dtype=dtype)


class Recorder:
    """the ten stand-ins; log: (name, details) in call order"""

    def __init__(self, n_selected=40, fundamental_keeps=None, fail=None):
        self.log, self.n_selected, self.fundamental_keeps, self.fail = [], n_selected, fundamental_keeps, fail or {}
        s = self.steps = capi.ImageProcessSteps()
        s.prep_create = capi.IMAGE_PREP_CREATE_STEP_FN(self.prep_create)
        s.prepare = capi.IMAGE_PREPARE_STEP_FN(self.prepare)
        s.consensus_setup = capi.IMAGE_CONSENSUS_SETUP_STEP_FN(self.consensus_setup)
        s.select = capi.IMAGE_SELECT_STEP_FN(self.select)
        s.flow = capi.OFT_FLOW_PROVIDER_FN(self.flow)
        s.fundamental = capi.OFT_FUNDAMENTAL_PROVIDER_FN(self.fundamental)
        s.pnp = capi.OFT_PNP_PROVIDER_FN(self.pnp)
        s.rows = capi.VIO_ROWS_PROVIDER_FN(self.rows)
        s.render = capi.IMAGE_RENDER_STEP_FN(self.render)
        s.track_update = capi.OFT_UPDATE_PROVIDER_FN(self.track_update)

    def _rc(self, name, **details):
        self.log.append((name, details))
        return self.fail.get(name, SRL_OK)

    def names(self, collapse=True):
        out = []
        for name, _ in self.log:
            if not (collapse and out and out[-1] == name):
                out.append(name)
        return out

    def of(self, name):
        return [d for n, d in self.log if n == name]

    def prep_create(self, o, user):
        o = o.contents
        return self._rc("prep_create", size=(o.rows, o.cols), k=(o.fx, o.fy, o.cx, o.cy), dist=list(o.dist), clips=(o.clip_gray, o.clip_color), tiles=o.tiles)

    def prepare(self, raw, rows, cols, stride, resized, user):
        return self._rc("prepare", raw=raw, size=(rows, cols), stride=stride, resized=resized)

    def consensus_setup(self, k, user):
        return self._rc("consensus_setup", k=tuple(k[i] for i in range(4)))

    def select(self, cam, rows, cols, o, refresh, out, capacity, n, user):
        cam, o = cam.contents, o.contents
        rc = self._rc("select", size=(rows, cols), minimum_dis=o.minimum_dis, skip_step=o.skip_step, use_all=o.use_all_points,
                      depths=(o.minimum_depth, o.maximum_depth), refresh=refresh, margin=cam.fov_margin, k=(cam.fx, cam.fy, cam.cx, cam.cy))
        n[0] = self.n_selected
        if capacity < self.n_selected:
            return SRL_ERR_BAD_ARG
        rec = _view(out, capacity, SEL)[:self.n_selected]
        k = np.arange(self.n_selected)
        rec["index"], rec["pool"], rec["point_index"] = k, 3 * k + 1, k
        rec["x"], rec["y"], rec["z"] = 0.1 * k, 0.2 * k, 5.0
        rec["u"], rec["v"] = 12.0 + 2.0 * (k % 40), 14.0 + 9.0 * (k // 40)
        return rc

    def flow(self, gray, rows, cols, stride, prev, n, nxt, status, user):
        rc = self._rc("flow", gray=gray, size=(rows, cols), n=n)
        _view(nxt, 2 * n, "<f4")[:] = _view(prev, 2 * n, "<f4") + np.tile(np.float32([2.0, 1.0]), n)
        _view(status, n, np.uint8)[:] = 1
        return rc

    def fundamental(self, last, cur, n, status, user):
        st = _view(status, n, np.uint8)
        st[:] = 1
        if self.fundamental_keeps is not None:
            st[self.fundamental_keeps:] = 0
        return self._rc("fundamental", n=n)

    def pnp(self, xyz, uv, n, inliers, n_inliers, user):
        _view(inliers, n, "<i4")[:] = np.arange(n)
        n_inliers[0] = n
        return self._rc("pnp", n=n)

    def rows(self, args, points, n, sums, user):
        a = args.contents
        C.memset(sums, 0, C.sizeof(capi.ColorVioSums))
        sums.contents.used = n
        return self._rc("rows", mode=a.mode, n=n, k=(a.cam.fx, a.cam.fy, a.cam.cx, a.cam.cy))

    def render(self, cam, obs_time, totals, user):
        cam = cam.contents
        totals.contents.listed = 7
        return self._rc("render", obs_time=obs_time, margin=cam.fov_margin, k=(cam.fx, cam.fy, cam.cx, cam.cy))

    def track_update(self, cam, rows, cols, tracked, n, cand, nc, opts, out, cap, tot, user):
        o, t = opts.contents, tot.contents
        _view(out, cap, TRK)[:n] = _view(tracked, n, TRK)
        t.tracked_in, t.kept, t.candidates = n, n, nc
        return self._rc("track_update", size=(rows, cols), n=n, candidates=nc, mini_distance=o.mini_distance, maximum=o.maximum_tracked_points,
                        margin=cam.contents.fov_margin)


def _camera_state():
    s = np.zeros(31)
    s[1:10] = np.eye(3).ravel()                          # R_imu_camera
    s[13:17] = FX, FY, CX, CY
    s[17] = 1.0                                          # q_world_camera
    s[24] = 1.0                                          # rotation
    return s


def _lio(rec, **opts):
    lio = srl.Lio(-1)                                    # host-only: no device anywhere in this file
    lio.vio_set_options(2, True, True, np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]]), np.eye(3), np.zeros(3))
    lio.vio_set_camera_state(_camera_state())
    base = dict(image_width=106, image_height=74, dist=DIST)
    base.update(opts)
    lio.image_set_options(**base)
    if rec is not None:
        lio.image_set_steps(rec.steps)
    return lio


def _frame(rows=74, cols=106):
    stride = 3 * cols + 13
    buf = np.full(rows * stride, 0xA5, np.uint8)
    return np.lib.stride_tricks.as_strided(buf, shape=(rows, cols, 3), strides=(stride, 3, 1))


FIRST = ["prep_create", "consensus_setup", "prepare", "select", "flow", "fundamental", "pnp", "rows", "render", "select", "track_update"]
LATER = ["prepare", "flow", "fundamental", "pnp", "rows", "render", "select", "track_update"]


def test_the_first_frame_runs_the_references_order_and_the_second_skips_select_and_init():
    rec = Recorder()
    lio = _lio(rec)
    try:
        assert lio.image_time_last_process() == -1e5
        img = _frame()
        r = lio.image_process(img, 10.0, 7)
        assert rec.names() == FIRST, rec.names()
        # init's flow call (the tracker's first image: only stored) and trackImage's, both on the prepared image: no gray, its size
        flows = rec.of("flow")
        assert len(flows) == 2 and all(f["gray"] is None and f["size"] == (74, 106) and f["n"] == 40 for f in flows)
        assert (r.first_data, r.prepared_rows, r.prepared_cols, r.image_scale_factor) == (1, 74, 106, 1.0)
        assert (r.tracked_after_flow, r.tracked_after_pnp, r.pnp_accepted) == (40, 40, 1)
        assert (r.esikf_accepted, r.photometric_accepted, r.refreshed_candidates) == (1, 1, 40)
        assert r.render.listed == 7 and r.track.kept == 40 and r.track.candidates == 40
        # the plain prepare at ratio 1.0, on the caller's buffer as it is
        p, = rec.of("prepare")
        assert p == dict(raw=img.ctypes.data, size=(74, 106), stride=3 * 106 + 13, resized=0)
        # the scaled intrinsics (scale 1.0: unchanged), the coefficients and the reference's defaults reach the preparer and the consensus setup
        pc, = rec.of("prep_create")
        assert pc == dict(size=(74, 106), k=(FX, FY, CX, CY), dist=DIST, clips=(3.0, 1.0), tiles=0)
        assert rec.of("consensus_setup") == [dict(k=(FX, FY, CX, CY))]
        # the two selections: window / scale with skip 1 on the frame's camera, then the refresh's (10.0, 1) with a margin of -0.4
        first, refresh = rec.of("select")
        assert (first["minimum_dis"], first["skip_step"], first["use_all"], first["refresh"], first["margin"]) == (40.0, 1, 0, 0, 0.005)
        assert (refresh["minimum_dis"], refresh["skip_step"], refresh["use_all"], refresh["refresh"], refresh["margin"]) == (10.0, 1, 0, 1, -0.4)
        assert first["depths"] == refresh["depths"] == (0.1, 200.0) and first["size"] == refresh["size"] == (74, 106)
        # vioEsikf's passes come first, vioPhotometric's after them
        modes = [d["mode"] for d in rec.of("rows")]
        assert modes == sorted(modes) and set(modes) == {srl.SRL_VIO_REPROJECTION, srl.SRL_VIO_PHOTOMETRIC}
        assert srl.SRL_VIO_REPROJECTION < srl.SRL_VIO_PHOTOMETRIC
        assert rec.of("render") == [dict(obs_time=10.0, margin=0.005, k=(FX, FY, CX, CY))]
        tu, = rec.of("track_update")
        assert tu == dict(size=(74, 106), n=40, candidates=40, mini_distance=40.0, maximum=300, margin=0.005)
        assert lio.image_time_last_process() == 10.0
        oft = lio.image_oft()
        assert oft.sizes()[:2] == (40, 40) and oft.times() == (10.0, 10.0)
        assert len(lio.image_candidates()) == 40

        rec.log.clear()
        r = lio.image_process(img, 10.1, 8)
        assert rec.names() == LATER, rec.names()
        assert r.first_data == 0 and rec.of("select")[0]["refresh"] == 1 and len(rec.of("flow")) == 1
        assert rec.of("render")[0]["obs_time"] == 10.1 and lio.image_time_last_process() == 10.1
        # the flow's (2, 1) per frame is in the pose map: the point selected at (12, 14) has been tracked twice
        cur = oft.pose_map(1)
        assert cur["pool"][0] == 1 and (cur["u"][0], cur["v"][0]) == (16.0, 16.0)

        # refreshPointsForProjection returns at once on a frame_id it has refreshed for
        rec.log.clear()
        lio.image_process(img, 10.2, 8)
        assert rec.names() == [n for n in LATER if n != "select"], rec.names()
    finally:
        lio.close()


def test_pnp_not_accepted_skips_both_updates_but_not_render_refresh_and_top_up():
    rec = Recorder(fundamental_keeps=5)                  # five points survive the flow: below the gate of ten
    lio = _lio(rec)
    try:
        r = lio.image_process(_frame(), 10.0, 1)
        assert rec.names() == ["prep_create", "consensus_setup", "prepare", "select", "flow", "fundamental", "render", "select", "track_update"], rec.names()
        assert (r.tracked_after_flow, r.tracked_after_pnp, r.pnp_accepted) == (5, 5, 0)
        assert (r.esikf_accepted, r.esikf_iterations, r.photometric_accepted, r.photometric_iterations) == (0, 0, 0, 0)
        # the top-up works on map_rgb_points_in_last_image_pose, which only an accepted PnP rewrites: still the forty of init
        assert r.render.listed == 7 and rec.of("track_update")[0]["n"] == 40 and lio.image_time_last_process() == 10.0
    finally:
        lio.close()


def test_fewer_than_thirty_points_only_move_the_time():
    rec = Recorder(n_selected=29)
    lio = _lio(rec)
    try:
        r = lio.image_process(_frame(), 10.0, 1)
        # init's flow call stores the first image; trackImage returns before its own (opticalFlowTracker.cpp:126-131)
        assert rec.names() == ["prep_create", "consensus_setup", "prepare", "select", "flow", "render", "select", "track_update"], rec.names()
        assert len(rec.of("flow")) == 1 and (r.tracked_after_flow, r.pnp_accepted) == (0, 0)
    finally:
        lio.close()


@pytest.mark.parametrize("ratio,resized", [(1.0, 0), (1.0 + 5e-7, 0), (0.5, 1), (2.0, 1)])
def test_the_ratio_chooses_the_prepare_and_scales_what_the_steps_are_handed(ratio, resized):
    rec = Recorder()
    width, height = 100, 70                              # the configured size; the frame that arrives is 74 x 106
    lio = _lio(rec, image_width=width, image_height=height, image_resize_ratio=ratio, track_windows_size=36.0, maximum_tracked_points=123,
               tracker_minimum_depth=0.3, tracker_maximum_depth=55.0)
    try:
        r = lio.image_process(_frame(), 10.0, 1)
        scale = width * ratio / 106                      # :93
        assert r.image_scale_factor == scale
        size = (int(height / scale), int(width / scale))
        assert (r.prepared_rows, r.prepared_cols) == size
        k = (FX / scale, FY / scale, CX / scale, CY / scale)
        assert rec.of("prep_create")[0]["size"] == size and rec.of("prep_create")[0]["k"] == k and rec.of("consensus_setup")[0]["k"] == k
        # the raw frame goes in at its own size; the flow runs on the prepared one
        assert rec.of("prepare")[0]["resized"] == resized and rec.of("prepare")[0]["size"] == (74, 106)
        assert all(f["size"] == size for f in rec.of("flow"))
        first, refresh = rec.of("select")
        assert first["minimum_dis"] == 36.0 / scale and refresh["minimum_dis"] == 10.0
        assert first["depths"] == refresh["depths"] == (0.3, 55.0)
        # image_rows / image_cols of the projection tests stay the raw frame's (lioOptimization.cpp:1080-1081)
        assert first["size"] == refresh["size"] == rec.of("track_update")[0]["size"] == (74, 106)
        tu = rec.of("track_update")[0]
        assert tu["mini_distance"] == 36.0 / scale and tu["maximum"] == 123
        # the camera state is the caller's: process does not rescale it
        assert rec.of("render")[0]["k"][0] == pytest.approx(FX, abs=1e-6)
        # a second frame divides nothing again
        rec.log.clear()
        r = lio.image_process(_frame(), 10.1, 2)
        assert r.image_scale_factor == scale and (r.prepared_rows, r.prepared_cols) == size and rec.of("prepare")[0]["resized"] == resized
    finally:
        lio.close()


@pytest.mark.parametrize("step", FIRST[:3] + ["flow", "fundamental", "pnp", "rows", "render", "track_update"])
def test_a_failing_step_returns_its_status_and_no_later_step_is_called(step):
    rec = Recorder(fail={step: SRL_ERR_UNSUPPORTED})
    lio = _lio(rec)
    try:
        rc, r = lio.image_process(_frame(), 10.0, 1, ok=(SRL_ERR_UNSUPPORTED,))
        assert rc == SRL_ERR_UNSUPPORTED
        names = rec.names()
        assert names == FIRST[:FIRST.index(step) + 1], names
        assert len(rec.of(step)) == 1
        assert lio.image_time_last_process() == -1e5     # the frame did not finish
        # the record holds what the frame reached
        assert r.first_data == 1 and r.refreshed_candidates == (40 if step == "track_update" else 0)
        assert r.render.listed == (7 if step in ("render", "track_update") else 0)
    finally:
        lio.close()


def test_a_failing_selection_ends_the_frame_at_either_place():
    for which, want in ((0, FIRST[:4]), (1, FIRST[:10])):
        rec = Recorder()
        lio = _lio(rec)
        try:
            calls = []
            inner = rec.select

            def select(*a, calls=calls, inner=inner, which=which):
                calls.append(1)
                rc = inner(*a)
                return SRL_ERR_UNSUPPORTED if len(calls) == which + 1 else rc
            rec.steps.select = keep = capi.IMAGE_SELECT_STEP_FN(select)
            lio.image_set_steps(rec.steps)
            rc, _ = lio.image_process(_frame(), 10.0, 1, ok=(SRL_ERR_UNSUPPORTED,))
            assert rc == SRL_ERR_UNSUPPORTED and rec.names() == want, (which, rec.names())
            del keep
        finally:
            lio.close()


def test_a_selection_larger_than_the_first_buffer_is_asked_again():
    rec = Recorder(n_selected=5000)
    lio = _lio(rec, maximum_tracked_points=6000)
    try:
        r = lio.image_process(_frame(), 10.0, 1)
        assert len(rec.of("select")) == 4 and r.refreshed_candidates == 5000 and len(lio.image_candidates()) == 5000
    finally:
        lio.close()


def test_a_host_only_handle_without_every_stand_in_has_no_device():
    lio = _lio(None)
    try:
        rc, r = lio.image_process(_frame(), 10.0, 1, ok=(SRL_ERR_NO_DEVICE,))
        assert rc == SRL_ERR_NO_DEVICE and bytes(r) == bytes(C.sizeof(r))
        rec = Recorder()
        rec.steps.render = capi.IMAGE_RENDER_STEP_FN()   # one step left at its default
        lio.image_set_steps(rec.steps)
        rc, _ = lio.image_process(_frame(), 10.0, 1, ok=(SRL_ERR_NO_DEVICE,))
        assert rc == SRL_ERR_NO_DEVICE and rec.log == []
        lio.image_set_steps(None)
        rc, _ = lio.image_process(_frame(), 10.0, 1, ok=(SRL_ERR_NO_DEVICE,))
        assert rc == SRL_ERR_NO_DEVICE
    finally:
        lio.close()


@pytest.mark.parametrize("step", ["prep_create", "consensus_setup", "prepare", "select", "flow"])
def test_a_frame_that_failed_in_its_first_data_is_offered_again_and_nothing_is_done_twice(step):
    """frame 1 fails at `step`; the same frame offered again succeeds: the preparer is created once, the consensus setup runs once, the
    intrinsics are divided by the scale once (the scale is not 1 here, so a second division would show in every K)"""
    rec = Recorder(fail={step: SRL_ERR_UNSUPPORTED})
    width, height, ratio = 100, 70, 0.5
    lio = _lio(rec, image_width=width, image_height=height, image_resize_ratio=ratio)
    try:
        lio.set_color_times(time_last_process=3.5)       # the caller's value: a frame that does not finish must leave it
        rc, r = lio.image_process(_frame(), 10.0, 1, ok=(SRL_ERR_UNSUPPORTED,))
        assert rc == SRL_ERR_UNSUPPORTED and r.first_data == 1 and lio.image_time_last_process() == 3.5
        rec.fail.clear()
        r = lio.image_process(_frame(), 10.0, 1)
        scale = width * ratio / 106
        k = (FX / scale, FY / scale, CX / scale, CY / scale)
        size = (int(height / scale), int(width / scale))
        assert r.first_data == 1 and (r.prepared_rows, r.prepared_cols, r.image_scale_factor) == size + (scale,)
        created, setups = rec.of("prep_create"), rec.of("consensus_setup")
        # (a step that failed was called twice: once refused, once for good -- never again behind a success)
        assert len(created) == (2 if step == "prep_create" else 1) and all(c["k"] == k and c["size"] == size for c in created)
        assert len(setups) == (2 if step == "consensus_setup" else 1) and all(s["k"] == k for s in setups)
        assert [d["minimum_dis"] for d in rec.of("select") if not d["refresh"]][-1] == 40.0 / scale
        assert (r.tracked_after_flow, r.pnp_accepted, r.refreshed_candidates) == (40, 1, 40) and lio.image_time_last_process() == 10.0
        # the whole of the reference's order came behind the retry, and the frame after it is an ordinary later frame
        tail = rec.names()[-(len(FIRST) - FIRST.index("prepare")):]
        assert tail == FIRST[FIRST.index("prepare"):], rec.names()
        rec.log.clear()
        r = lio.image_process(_frame(), 10.1, 2)
        assert rec.names() == LATER and r.first_data == 0 and r.image_scale_factor == scale
    finally:
        lio.close()
