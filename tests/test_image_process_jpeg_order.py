"""srl_lio_image_process_jpeg of the host mirror (include/srlivo_host.h: lioOptimization::compressedImageHandler followed by
imageProcessing::process) without a device, in the manner of tests/test_image_process_order.py, whose recording stand-ins are used here:
the JPEG step and every other step are replaced on a host-only handle.  The frame runs srl_lio_image_process's statements in their
order with the prepare step replaced by the JPEG step; rows and cols -- image_scale_factor, the preparer's size, every projection test --
come from the stream's header; a failing JPEG step ends the frame."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases as jc
import sr_livo_amd as srl
import test_image_process_order as base
from sr_livo_amd import capi

SRL_OK, SRL_ERR_NO_DEVICE, SRL_ERR_BAD_ARG, SRL_ERR_UNSUPPORTED = 0, -1, -3, -4
GOLDEN = jc.load_golden()
STREAM = np.frombuffer(GOLDEN["37x43_420_r1"][0], np.uint8)      # 43 rows x 37 columns
FIRST = [("jpeg" if n == "prepare" else n) for n in base.FIRST]
LATER = [("jpeg" if n == "prepare" else n) for n in base.LATER]


class Recorder(base.Recorder):
    """the selection inside the stream's 37 x 43 pixels (the tracker drops points that leave the image), a few (2, 1) steps of room"""

    def select(self, cam, rows, cols, o, refresh, out, capacity, n, user):
        rc = super().select(cam, rows, cols, o, refresh, out, capacity, n, user)
        if capacity >= self.n_selected:
            rec = base._view(out, capacity, base.SEL)[:self.n_selected]
            k = np.arange(self.n_selected)
            rec["u"], rec["v"] = 4.0 + 3.0 * (k % 8), 4.0 + 5.0 * (k // 8)
        return rc


def _lio(rec, **opts):
    """test_image_process_order's handle with the JPEG step recorded in the same log"""
    opts.setdefault("image_width", 37)
    opts.setdefault("image_height", 43)
    lio = base._lio(rec, **opts)

    def step(address, n, user):
        rec.log.append(("jpeg", dict(address=address, n=n)))
        return rec.fail.get("jpeg", SRL_OK)
    lio.image_set_jpeg_step(step)
    return lio


def test_the_frame_runs_image_process_order_with_the_jpeg_step_in_the_prepares_place():
    rec = Recorder()
    lio = _lio(rec)
    try:
        r = lio.image_process_jpeg(STREAM, 10.0, 7)
        assert rec.names() == FIRST, rec.names()
        assert rec.of("prepare") == [] and rec.of("jpeg") == [dict(address=STREAM.ctypes.data, n=STREAM.size)]      # the caller's bytes as they are
        assert (r.first_data, r.prepared_rows, r.prepared_cols, r.image_scale_factor) == (1, 43, 37, 1.0)
        assert (r.tracked_after_flow, r.pnp_accepted, r.refreshed_candidates, r.render.listed) == (40, 1, 40, 7)
        # the size every projection test is handed is the one srl_jpeg_parse read
        first, refresh = rec.of("select")
        assert first["size"] == refresh["size"] == rec.of("track_update")[0]["size"] == (43, 37)
        assert all(f["gray"] is None and f["size"] == (43, 37) for f in rec.of("flow"))
        assert lio.image_time_last_process() == 10.0
        rec.log.clear()
        r = lio.image_process_jpeg(STREAM, 10.1, 8)
        assert rec.names() == LATER and r.first_data == 0 and lio.image_time_last_process() == 10.1
        # a raw frame on the same handle takes the table's prepare step, a compressed one the JPEG step again
        rec.log.clear()
        lio.image_process(base._frame(43, 37), 10.2, 9)
        assert rec.names() == base.LATER and rec.of("jpeg") == []
        rec.log.clear()
        lio.image_process_jpeg(GOLDEN["37x43_420_r1"][0], 10.3, 10)      # bytes as well as arrays
        assert rec.names() == LATER
    finally:
        lio.close()


@pytest.mark.parametrize("width,height,ratio", [(74, 86, 1.0), (37, 43, 0.5), (100, 70, 2.0)])
def test_the_intrinsics_are_scaled_from_the_parsed_size(width, height, ratio):
    rec = Recorder()
    lio = _lio(rec, image_width=width, image_height=height, image_resize_ratio=ratio, track_windows_size=36.0)
    try:
        r = lio.image_process_jpeg(STREAM, 10.0, 1)
        scale = width * ratio / 37                          # :93, on the stream's 37 columns
        assert r.image_scale_factor == scale
        size = (int(height / scale), int(width / scale))
        assert (r.prepared_rows, r.prepared_cols) == size and rec.of("prep_create")[0]["size"] == size
        k = (base.FX / scale, base.FY / scale, base.CX / scale, base.CY / scale)
        assert rec.of("prep_create")[0]["k"] == k and rec.of("consensus_setup")[0]["k"] == k
        assert all(f["size"] == size for f in rec.of("flow"))
        first, refresh = rec.of("select")
        assert first["minimum_dis"] == 36.0 / scale and first["size"] == refresh["size"] == (43, 37)
        assert len(rec.of("jpeg")) == 1 and rec.of("prepare") == []      # whatever the ratio: the JPEG step resizes by itself
    finally:
        lio.close()


def test_a_failing_jpeg_step_ends_the_frame():
    rec = Recorder(fail={"jpeg": SRL_ERR_UNSUPPORTED})
    lio = _lio(rec)
    try:
        rc, r = lio.image_process_jpeg(STREAM, 10.0, 1, ok=(SRL_ERR_UNSUPPORTED,))
        assert rc == SRL_ERR_UNSUPPORTED and rec.names() == FIRST[:FIRST.index("jpeg") + 1]
        assert r.first_data == 1 and r.refreshed_candidates == 0 and lio.image_time_last_process() == -1e5
        rec.fail.clear()
        r = lio.image_process_jpeg(STREAM, 10.0, 1)        # offered again: nothing of the first data is done twice
        assert len(rec.of("prep_create")) == 1 and len(rec.of("consensus_setup")) == 1 and r.first_data == 1
        assert rec.names()[-(len(FIRST) - FIRST.index("jpeg")):] == FIRST[FIRST.index("jpeg"):]
    finally:
        lio.close()


def test_streams_the_parser_refuses_never_reach_a_step():
    rec = Recorder()
    lio = _lio(rec)
    try:
        progressive = bytearray(STREAM.tobytes())
        progressive[progressive.index(b"\xFF\xC0") + 1] = 0xC2
        for data, status in ((bytes(progressive), SRL_ERR_UNSUPPORTED), (STREAM.tobytes()[:40], SRL_ERR_BAD_ARG), (b"\x00" * 64, SRL_ERR_BAD_ARG)):
            rc, r = lio.image_process_jpeg(data, 10.0, 1, ok=(status,))
            assert rc == status and rec.log == [] and bytes(r) == bytes(C.sizeof(r))
        res = capi.ImageProcessResult()
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        assert lio.lib.srl_lio_image_process_jpeg(lio.h, None, 10, 10.0, 1, C.byref(res)) == SRL_ERR_BAD_ARG and bytes(res) == bytes(C.sizeof(res))
        assert lio.lib.srl_lio_image_process_jpeg(lio.h, capi._ptr(STREAM), 1, 10.0, 1, None) == SRL_ERR_BAD_ARG
        assert lio.lib.srl_lio_image_process_jpeg(None, capi._ptr(STREAM), STREAM.size, 10.0, 1, None) == SRL_ERR_BAD_ARG
        assert lio.lib.srl_lio_image_set_jpeg_step(None, capi.IMAGE_JPEG_STEP_FN(), None) == SRL_ERR_BAD_ARG
        # the same in front of a measurement
        assert lio.lib.srl_lio_run_measurement_image_jpeg(lio.h, 0.0, None, None, None, 0, None, None, 0, 0.0, 0.0, capi._ptr(STREAM), 40, None, res) == SRL_ERR_BAD_ARG
        assert rec.log == []
    finally:
        lio.close()


def test_a_host_only_handle_with_the_jpeg_step_at_its_default_has_no_device():
    rec = Recorder()
    lio = base._lio(rec, image_width=37, image_height=43)  # every member of the table replaced, the JPEG step not
    try:
        rc, r = lio.image_process_jpeg(STREAM, 10.0, 1, ok=(SRL_ERR_NO_DEVICE,))
        assert rc == SRL_ERR_NO_DEVICE and rec.log == [] and bytes(r) == bytes(C.sizeof(r))
        lio.image_process(base._frame(43, 37), 10.0, 1)   # raw frames do not need it
        assert rec.names() == base.FIRST
        # the step is no member of the table: it survives a new table, and NULL puts the default (no device here) back
        lio.image_set_jpeg_step(lambda address, n, user: rec._rc("jpeg", n=n))
        lio.image_set_steps(rec.steps)
        rec.log.clear()
        lio.image_process_jpeg(STREAM, 10.1, 2)
        assert rec.names() == LATER
        lio.image_set_jpeg_step(None)
        rc, _ = lio.image_process_jpeg(STREAM, 10.2, 3, ok=(SRL_ERR_NO_DEVICE,))
        assert rc == SRL_ERR_NO_DEVICE
        # options never set
        other = srl.Lio(-1)
        try:
            rc = other.lib.srl_lio_image_process_jpeg(other.h, capi._ptr(STREAM), STREAM.size, 10.0, 1, None)
            assert rc == SRL_ERR_BAD_ARG
        finally:
            other.close()
    finally:
        lio.close()


def test_the_step_table_keeps_its_layout():
    assert [f for f, _ in capi.ImageProcessSteps._fields_] == ["user", "prep_create", "prepare", "consensus_setup", "select", "flow", "fundamental", "pnp",
                                                               "rows", "render", "track_update"]
