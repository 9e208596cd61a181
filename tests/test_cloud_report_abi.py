"""srl_map_insert_report / srl_frame_commit_report / srl_lio_points_world (cloud_world: addPointToPcl, lioOptimization.cpp:1346-1355) on
a box without a GPU: the entry points are declared and exported, NULL arguments are refused before anything touches a device with the
counts written as 0, the record is 16 bytes on both sides, and a host-only handle has no points_world and no host-side insert."""
import ctypes as C
import os
import re

import numpy as np

import sr_livo_amd as srl
from sr_livo_amd import capi

SRL_ERR_BAD_ARG = -3          # include/srlivo_hip.h: srl_status
NEW = ("srl_map_insert_report", "srl_frame_commit_report", "srl_lio_set_collect_points_world", "srl_lio_points_world")


def test_report_entry_points_are_declared_and_exported():
    lib = srl.load_library()
    for name in NEW:
        assert name in srl.declared_symbols()
        assert hasattr(lib, name)


def test_cloud_point_is_sixteen_bytes_on_both_sides():
    assert C.sizeof(capi.CloudPoint) == 16 and capi.CLOUD_POINT_DTYPE.itemsize == 16
    assert [f[0] for f in capi.CloudPoint._fields_] == ["x", "y", "z", "intensity"] == list(capi.CLOUD_POINT_DTYPE.names)
    text = open(os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h")).read()
    assert re.search(r"typedef struct srl_cloud_point \{ float x, y, z, intensity; \} srl_cloud_point;", text)
    # (the C side: four floats as declared, and a static_assert on 16 bytes where the kernels write the record as one float4)
    scratch = open(os.path.join(os.path.dirname(capi.INCLUDE_DIR), "sr_livo_amd", "csrc", "srl_frame_scratch.h")).read()
    assert "static_assert(sizeof(srl_cloud_point) == 16" in scratch
    # the limit on n is the header's and is not below the frame pipeline's 1 M
    limit = int(re.search(r"#define SRL_MAP_INSERT_REPORT_MAX_POINTS (\d+)", text).group(1))
    assert limit >= 1_048_576


def test_null_arguments_are_refused_without_a_device_and_zero_the_counts():
    lib = srl.load_library()
    pts = np.zeros((4, 3))
    dummy = (C.c_char * 64)()
    ctx = C.cast(dummy, C.c_void_p)
    outcome = np.full(4, 9, np.uint8)
    cloud = np.full((4, 4), 9.0, np.float32)
    nc, na = C.c_int(7), C.c_int(7)
    args = (1.0, 20, 0.1, 0, 0.0, capi._ptr(outcome), capi._ptr(cloud), C.byref(nc), C.byref(na))
    assert lib.srl_map_insert_report(None, capi._ptr(pts), 4, *args) == SRL_ERR_BAD_ARG
    assert (nc.value, na.value) == (0, 0)
    nc.value = na.value = 7
    assert lib.srl_map_insert_report(ctx, None, 4, *args) == SRL_ERR_BAD_ARG          # refused before the context is looked at
    assert (nc.value, na.value) == (0, 0)
    assert lib.srl_map_insert_report(ctx, capi._ptr(pts), -1, *args) == SRL_ERR_BAD_ARG
    assert lib.srl_map_insert_report(None, None, 0, 1.0, 20, 0.1, 0, 0.0, None, None, None, None) == SRL_ERR_BAD_ARG
    assert (outcome == 9).all() and (cloud == 9.0).all()
    q = np.array([1.0, 0.0, 0.0, 0.0]); t = np.zeros(3); R = np.eye(3).ravel(); ti = np.zeros(3)
    d = capi._dptr
    tail = (1.0, 20, 0.1, 0, None, capi._ptr(outcome), capi._ptr(cloud), C.byref(nc), C.byref(na))
    for bad in ((None, d(q), d(t), d(R), d(ti)), (ctx, None, d(t), d(R), d(ti)), (ctx, d(q), None, d(R), d(ti)),
                (ctx, d(q), d(t), None, d(ti)), (ctx, d(q), d(t), d(R), None)):
        nc.value = na.value = 7
        assert lib.srl_frame_commit_report(*bad, *tail) == SRL_ERR_BAD_ARG
        assert (nc.value, na.value) == (0, 0)
    assert (outcome == 9).all() and (cloud == 9.0).all()
    n = C.c_int(7)
    assert lib.srl_lio_points_world(None, None, 0, C.byref(n)) == SRL_ERR_BAD_ARG and n.value == 0
    assert lib.srl_lio_set_collect_points_world(None, 1) == SRL_ERR_BAD_ARG


def test_host_only_handle_has_no_points_world_and_no_host_side_insert():
    lib = srl.load_library()
    h = C.c_void_p()
    assert lib.srl_lio_create(-1, C.byref(h)) == capi.SRL_OK        # host-only object: no device map behind it
    try:
        assert lib.srl_lio_set_collect_points_world(h, 1) == capi.SRL_OK
        pts = np.array([[0.1, 0.1, 0.1], [0.4, 0.1, 0.1]])
        assert lib.srl_lio_add_points_to_map(h, capi._ptr(pts), 2, 1.0, 20, 0.1, 0) != capi.SRL_OK     # an error, never a host-side insert
        n = C.c_int(7)
        rec = (capi.CloudPoint * 2)()
        assert lib.srl_lio_points_world(h, C.cast(rec, C.c_void_p), 2, C.byref(n)) != capi.SRL_OK
        assert n.value == 0
        assert lib.srl_lio_points_world(h, None, 0, None) == SRL_ERR_BAD_ARG
    finally:
        lib.srl_lio_destroy(h)
