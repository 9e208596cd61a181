"""The ABI of the point side (srl_livox_decode, the point queue, srl_frame_undistort_cut and the mirror's entry points): struct sizes against
ctypes and the checker's record, the exported symbols, and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np

import livox_cases as lc
import livox_checker as lk
import sr_livo_amd as srl
from sr_livo_amd import capi

NEW_SYMBOLS = ("srl_time_unit_scale", "srl_livox_decode", "srl_points_info", "srl_points_clear", "srl_points_cut", "srl_frame_undistort_cut",
               "srl_frame_point_times", "srl_points_queue_download", "srl_points_cut_download", "srl_debug_points_fallbacks",
               "srl_lio_set_lidar_options", "srl_lio_feed_livox", "srl_lio_points_info", "srl_lio_run_measurement_queued")


def _header(name):
    return open(os.path.join(capi.INCLUDE_DIR, name)).read()


def test_record_and_struct_sizes():
    assert capi.LIVOX_POINT_DTYPE.itemsize == 20 == lk.POINT_DTYPE.itemsize == lc.POINT_DTYPE.itemsize
    assert capi.LIVOX_POINT_DTYPE == lk.POINT_DTYPE == lc.POINT_DTYPE
    assert [capi.LIVOX_POINT_DTYPE.fields[f][1] for f in ("offset_time", "x", "y", "z", "reflectivity", "tag", "line")] == [0, 4, 8, 12, 16, 17, 18]
    assert C.sizeof(capi.LivoxOpts) == 32 and C.sizeof(capi.LivoxReport) == 40 and C.sizeof(capi.PointsCutReport) == 16
    assert (capi.LivoxOpts.time_unit_scale.offset, capi.LivoxOpts.blind.offset, capi.LivoxOpts.point_filter_num.offset) == (8, 16, 24)
    assert (capi.LivoxReport.last_end_time.offset, capi.LivoxReport.last_timestamp.offset) == (16, 32)
    assert capi.PointsCutReport.front_timestamp.offset == 8
    # the header says the same (the library's own static_asserts hold it at build time)
    text = _header("srlivo_hip.h")
    assert re.search(r"typedef struct srl_livox_point \{ uint32_t offset_time; float x, y, z; uint8_t reflectivity, tag, line, pad; \}", text)


def test_every_new_symbol_is_declared_and_exported():
    declared = srl.declared_symbols()
    lib = srl.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert "srl_points_queue_download" not in re.sub(r"/\*.*?\*/", "", _header("srlivo_hip.h"), flags=re.S)      # read-backs: the debug header


def test_refusals_that_need_no_device():
    lib = srl.load_library()
    o = srl.livox_opts()
    r = capi.LivoxReport()
    pts = lc.make_message(8, 1)
    p = pts.ctypes.data_as(C.c_void_p)
    assert lib.srl_livox_decode(None, p, 8, 1.0, C.byref(o), C.byref(r)) == capi.SRL_ERR_BAD_ARG
    assert (r.valid, r.picked, r.appended) == (0, 0, 0) and np.isnan(r.last_end_time) and np.isnan(r.first_timestamp)
    cr = capi.PointsCutReport()
    assert lib.srl_points_cut(None, 1.0, C.byref(cr)) == capi.SRL_ERR_BAD_ARG and cr.count == 0 and np.isnan(cr.front_timestamp)
    assert lib.srl_points_info(None, None, None, None) == capi.SRL_ERR_BAD_ARG
    assert lib.srl_points_clear(None) == capi.SRL_ERR_BAD_ARG
    n = C.c_int(7)
    assert lib.srl_frame_undistort_cut(None, 0.0, 0.1, 1, None, 0, 0, None, None, C.byref(n)) == capi.SRL_ERR_BAD_ARG and n.value == 0
    assert lib.srl_frame_point_times(None, None, 0, None, None, None) == capi.SRL_ERR_BAD_ARG
    assert lib.srl_points_queue_download(None, None, None, None, 0, C.byref(n)) == capi.SRL_ERR_BAD_ARG
    assert lib.srl_points_cut_download(None, None, None, None, 0, C.byref(n)) == capi.SRL_ERR_BAD_ARG
    assert lib.srl_debug_points_fallbacks(None, None) == capi.SRL_ERR_BAD_ARG
    assert lib.srl_lio_set_lidar_options(None, C.byref(o)) == capi.SRL_ERR_BAD_ARG
    assert lib.srl_lio_feed_livox(None, p, 8, 1.0, C.byref(r)) == capi.SRL_ERR_BAD_ARG
    assert lib.srl_lio_points_info(None, None, None, None, None, None) == capi.SRL_ERR_BAD_ARG
    out = capi.ReplayResult()
    assert lib.srl_lio_run_measurement_queued(None, 0.0, None, None, None, 0, 0.0, 0.0, 0.1, C.byref(out)) == capi.SRL_ERR_BAD_ARG


def test_the_time_unit_helper_is_pure():
    assert [srl.time_unit_scale(u) for u in (0, 1, 2, 3)] == [float(np.float32(v)) for v in (1.e3, 1.0, 1.e-3, 1.e-6)]
