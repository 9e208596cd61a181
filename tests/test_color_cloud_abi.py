"""srl_color_map_export_cloud and the host handle's srl_lio_color_cloud / srl_lio_color_topic_sizes (the loops of pubColorPoints,
threadPubColorPoints and saveColorPoints, lioOptimization.cpp:1210-1426) on a box without a GPU: the entry points are declared and
exported, the records have one layout on both sides (16 bytes the point, 16 the options, 32 the four int64 totals), the defaults are
the reference's, the refusals that can be reached without a context zero the totals and leave the output alone, and a host-only handle
has the topic schedule but no cloud.  (The refusals that need a context are decided before a device is touched too; a context exists
only on a device: tests/test_gpu_color_cloud.py.)"""
import ctypes as C
import math
import os
import re

import numpy as np

import cloud_export_checker as ck
import sr_livo_amd as srl
from sr_livo_amd import capi

SRL_ERR_BAD_ARG = -3          # include/srlivo_hip.h: srl_status
NEW = ("srl_color_map_export_cloud", "srl_color_cloud_opts_default", "srl_lio_color_cloud", "srl_lio_color_cloud_view", "srl_lio_color_topic_sizes",
       "srl_lio_color_topic_state")
CSRC = os.path.join(os.path.dirname(capi.INCLUDE_DIR), "sr_livo_amd", "csrc")


def test_cloud_entry_points_are_declared_and_exported():
    lib = srl.load_library()
    for name in NEW:
        assert name in srl.declared_symbols()
        assert hasattr(lib, name)
    hip = open(os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h")).read()
    host = open(os.path.join(capi.INCLUDE_DIR, "srlivo_host.h")).read()
    assert "int srl_color_map_export_cloud(srl_ctx *ctx, int64_t first, int64_t count, const srl_color_cloud_opts *opts," in hip
    assert re.search(r"\bint srl_lio_color_cloud\(srl_lio \*lio, int which, int minimum_views,", host)
    assert re.search(r"\bint srl_lio_color_topic_sizes\(srl_lio \*lio, int64_t published,", host)
    # the header says that the layout is meant as PCL's and that nothing here confirms it, and what happens to a range beyond one scan
    assert "the stand-in pcl::PointXYZRGB of oracle/ref_shim is not PCL" in hip
    assert re.search(r"more than 2\^27 points.*\n.*REFUSED with SRL_ERR_UNSUPPORTED", hip)
    # the calls this one stands beside did not change
    assert "int srl_color_registered_download(srl_ctx *ctx, int64_t first, int count, srl_color_stored *out);" in hip
    assert "int srl_color_registered_rgb(srl_ctx *ctx, int64_t first, int count, int16_t *rgb, int16_t *n_rgb, float *cov_rgb, double *observe_distance," in hip


def _fields(header, struct):
    m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return tuple(re.findall(r"\b([a-z_]+)\s*[,;]", body))


def test_records_have_one_layout_on_both_sides():
    hip = open(os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h")).read()
    assert capi.COLOR_CLOUD_DTYPE.itemsize == 16 and C.sizeof(capi.ColorCloudOpts) == 16 and C.sizeof(capi.ColorCloudTotals) == 32
    assert _fields(hip, "srl_color_cloud_point") == capi.COLOR_CLOUD_DTYPE.names == ck.CLOUD_DTYPE.names == ("x", "y", "z", "b", "g", "r", "a")
    assert capi.COLOR_CLOUD_DTYPE == ck.CLOUD_DTYPE
    assert [capi.COLOR_CLOUD_DTYPE.fields[f][1] for f in ("x", "y", "z", "b", "g", "r", "a")] == [0, 4, 8, 12, 13, 14, 15]      # b, g, r, a from the low byte
    assert _fields(hip, "srl_color_cloud_opts") == tuple(f for f, _ in capi.ColorCloudOpts._fields_)
    assert _fields(hip, "srl_color_cloud_totals") == tuple(f for f, _ in capi.ColorCloudTotals._fields_) == ck.TOTALS
    src = open(os.path.join(CSRC, "srl_color_cloud.hip")).read()
    assert "static_assert(sizeof(srl_color_cloud_point) == 16" in src
    # the map's layouts are as they were: the export owns no persistent bytes
    layout = open(os.path.join(CSRC, "srl_color_map.h")).read()
    assert "struct SrlColorPoint { float x, y, z; int voxel; int slot; int reg; };" in layout
    assert "struct SrlColorState { double observe_distance; double last_observe_time; float cov_rgb[3]; short rgb[3]; short n_rgb; };" in layout
    assert "hipMalloc" not in src


def test_the_defaults_are_the_references():
    o = capi.default_color_cloud_opts()
    assert (o.minimum_views, o.reverse) == (1, 0) and o.since == -math.inf
    srl.load_library().srl_color_cloud_opts_default(None)                  # a NULL is ignored
    header = open(os.path.join(CSRC, "host", "lioOptimization.h")).read()
    assert "int number_of_points_per_topic = 1000;" in header and "int sleep_time_after_pub = 10;" in header
    assert ":1398" in header                                               # the loop that never reaches index 0 is cited where it is mirrored


def test_refusals_without_a_context_zero_the_totals_and_leave_the_output():
    lib = srl.load_library()
    o = capi.default_color_cloud_opts()
    out = np.full(4, 9, np.uint8).repeat(16).view(capi.COLOR_CLOUD_DTYPE)
    idx = np.full(4, 9, np.int32)
    before = out.tobytes()
    tot = capi.ColorCloudTotals(7, 7, 7, 7)
    assert lib.srl_color_map_export_cloud(None, 0, -1, C.byref(o), capi._ptr(out), capi._ptr(idx), 4, C.byref(tot)) == SRL_ERR_BAD_ARG
    assert tot.as_tuple() == (0,) * 4 and out.tobytes() == before and (idx == 9).all()
    assert lib.srl_color_map_export_cloud(None, 0, 0, None, None, None, 0, None) == SRL_ERR_BAD_ARG
    n = C.c_int64(5)
    tot = capi.ColorCloudTotals(7, 7, 7, 7)
    assert lib.srl_lio_color_cloud(None, 0, 1, capi._ptr(out), capi._ptr(idx), 4, C.byref(n), C.byref(tot)) == SRL_ERR_BAD_ARG
    assert n.value == 0 and tot.as_tuple() == (0,) * 4 and out.tobytes() == before
    m = C.c_int(5)
    assert lib.srl_lio_color_topic_sizes(None, 10, None, 0, C.byref(m)) == SRL_ERR_BAD_ARG and m.value == 0


def test_host_only_handle_has_the_schedule_and_no_cloud():
    lib = srl.load_library()
    h = C.c_void_p()
    assert lib.srl_lio_create(-1, C.byref(h)) == capi.SRL_OK        # host-only object: no device behind it
    try:
        out = np.zeros(4, capi.COLOR_CLOUD_DTYPE)
        n = C.c_int64(5)
        tot = capi.ColorCloudTotals(7, 7, 7, 7)
        for which in (0, 1):
            assert lib.srl_lio_color_cloud(h, which, 1, capi._ptr(out), None, 4, C.byref(n), C.byref(tot)) == capi.SRL_ERR_NO_DEVICE      # never a host loop
            assert n.value == 0 and tot.as_tuple() == (0,) * 4
        pts, ids = C.c_void_p(5), C.c_void_p(5)
        assert lib.srl_lio_color_cloud_view(h, 0, 1, 1, C.byref(pts), C.byref(ids), C.byref(n), C.byref(tot)) == capi.SRL_ERR_NO_DEVICE
        assert pts.value is None and ids.value is None and n.value == 0
        assert lib.srl_lio_color_cloud_view(h, 0, 1, 1, C.byref(pts), None, C.byref(n), None) == SRL_ERR_BAD_ARG
        assert lib.srl_lio_color_cloud(h, 2, 1, None, None, 0, C.byref(n), None) == SRL_ERR_BAD_ARG
        assert lib.srl_lio_color_cloud(h, 0, 1, None, None, 0, None, None) == SRL_ERR_BAD_ARG
        assert lib.srl_lio_color_cloud(h, 0, 1, None, None, 3, C.byref(n), None) == SRL_ERR_BAD_ARG
        assert lib.srl_lio_color_cloud(h, 0, 1, None, None, -1, C.byref(n), None) == SRL_ERR_BAD_ARG

        # the schedule is pure host logic: the checker's known answers through the handle
        def round_(p):
            m = C.c_int()
            assert lib.srl_lio_color_topic_sizes(h, p, None, 0, C.byref(m)) == capi.SRL_OK          # the number alone: nothing carried over
            sizes = np.zeros(m.value, np.int32)
            assert lib.srl_lio_color_topic_sizes(h, p, capi._ptr(sizes), m.value, C.byref(m)) == capi.SRL_OK
            return list(sizes)

        def state():
            a, b = C.c_int(), C.c_int()
            assert lib.srl_lio_color_topic_state(h, C.byref(a), C.byref(b)) == capi.SRL_OK
            return a.value, b.value
        s = ck.TopicSchedule()
        for p in (0, 999, 1000, 1001, 43999, 44000, 44000, 66000, 5, 200000):
            assert round_(p) == s.round(p), p
            assert state() == (s.number_of_points_per_topic, s.sleep_time_after_pub), p
        assert state()[0] > 1000
        m = C.c_int()
        sizes = np.zeros(1, np.int32)
        keep = state()
        assert lib.srl_lio_color_topic_sizes(h, 10 ** 7, capi._ptr(sizes), 1, C.byref(m)) == SRL_ERR_BAD_ARG and m.value > 45 and state() == keep
        assert lib.srl_lio_color_topic_sizes(h, -1, capi._ptr(sizes), 1, C.byref(m)) == SRL_ERR_BAD_ARG
    finally:
        lib.srl_lio_destroy(h)
