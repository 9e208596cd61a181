"""The sequential restatement of the coloured-cloud loops (tests/cloud_export_checker.py) pinned to the reference's own pieces, bytewise.

pubColorPoints, threadPubColorPoints and saveColorPoints (src/lioOptimization.cpp:1210-1241, :1243-1344, :1386-1426) cannot be compiled
against the stand-ins of oracle/ (ROS publishers, pcl::toROSMsg, the PCD writer).  tests/cloud_export_ref_reader.cpp drives what can:
rgbPoint objects built by the reference's constructor and brought to the checker's states by the reference's updateRgb, read through
getPosition() / getRgb() and compared with N_rgb as the loops do; compiled here, into the test's temporary directory, against a temporary
include mirror of symlinks as oracle/Makefile's `refpath` target builds one and linked to oracle/_ref/libref_path.so.  Neither the
reader's binary nor anything of the reference is committed; the tests that need it skip where the reference tree or the library is absent.

The loops' index arithmetic -- `i = 0; i < size` (:1217, :1275), `i = size - 1; i > 0; i--` (:1398), the topic counter and its growth
(:1295-1342) -- is restated by hand in the reader and in the checker alike: two restatements by hand agree, no more.  The schedule's known
answers below are worked out from the lines themselves."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_export_checker as ck
import render_checker as rk
from oracle import pyref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_TSL = os.path.join(REF, "thirdLibrary", "tessil-src", "include")
REF_HDRS = ("cloudMap", "utility", "eskfEstimator", "state", "parameters", "lioOptimization", "cloudProcessing")      # oracle/Makefile: REF_HDRS

needs_reference = pytest.mark.skipif(
    not pr.available() or not os.path.exists(os.path.join(REF, "include", "lioOptimization.h")) or shutil.which("g++") is None,
    reason="needs oracle/_ref/libref_path.so, the reference tree and g++")


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cloud_export_ref_reader")
    inc = tmp / "include"
    inc.mkdir()
    for h in REF_HDRS:
        os.symlink(os.path.join(REF, "include", h + ".h"), inc / (h + ".h"))
    os.symlink(os.path.join(ROOT, "oracle", "ref_shim", "local", "imageProcessing.h"), inc / "imageProcessing.h")
    out = tmp / "libcloud_export_ref_reader.so"
    refdir = os.path.join(ROOT, "oracle", "_ref")
    cmd = ["g++", "-std=c++14", "-O1", "-fPIC", "-w", "-ffp-contract=off", "-shared", "-I" + os.path.join(ROOT, "oracle"), "-I" + str(inc),
           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + REF_TSL, "-o", str(out), os.path.join(ROOT, "tests", "cloud_export_ref_reader.cpp"),
           "-L" + refdir, "-l:libref_path.so", "-Wl,-rpath," + refdir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    pr.load()
    lib = C.CDLL(str(out))
    p = C.c_void_p
    lib.cer_cloud.argtypes = [C.c_int, p, p, p, C.c_int, C.c_int, C.c_int, p, p, p, p]
    lib.cer_cloud.restype = C.c_long
    return lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------ preconditions, from the checker alone
def test_preconditions_from_the_checker_alone():
    regs = ck.scene_registered()
    last = regs[-1]
    assert len(last) == 24388
    classes = [int((last.n_rgb == 0).sum()), int((last.n_rgb == 1).sum()), int((last.n_rgb == 2).sum()), int((last.n_rgb >= 3).sum())]
    print("registered points with N_rgb = 0, 1, 2, >= 3 after the last render:", classes)
    assert min(classes) >= 1000 and sum(classes) == len(last)
    for reg in regs:
        assert reg.rgb.min() >= 0 and reg.rgb.max() <= 255 and reg.n_rgb.min() >= 0      # the byte is the reference's double -> uint8_t there
    assert last.rgb.min() == 0 and last.rgb.max() == 255
    # since = 10.3 splits the observed times
    seen = sorted(set(float(t) for t in last.time))
    assert seen == [0.0, 10.0, 10.1, 10.3, 10.35, 10.6]
    _, _, tot = ck.scene_export(5, 1, False, 10.3)
    assert tot["stale"] > 0 and tot["published"] > 0 and tot["below_views"] > 0
    assert int((last.time[last.n_rgb >= 1] < 10.3).sum()) == tot["stale"]
    # the two orders and the skipped index 0
    rec_up, idx_up, _ = ck.pub_color_points(last, 0)
    rec_dn, idx_dn, _ = ck.save_color_points(last, 0)
    assert idx_up[0] == 0 and 0 not in idx_dn and (np.diff(idx_dn) < 0).all() and len(idx_dn) == len(idx_up) - 1
    assert rec_dn.tobytes() == rec_up[:0:-1].tobytes()
    # a map never rendered: all black at minimum_views 0, nothing at 1
    rec, _, tot = ck.pub_color_points(ck.never_rendered(), 0)
    assert len(rec) == len(last) and not rec["r"].any() and not rec["g"].any() and not rec["b"].any() and (rec["a"] == 255).all()
    assert ck.pub_color_points(ck.never_rendered(), 1)[2]["below_views"] == len(last)


def test_export_is_the_three_loops():
    """the range-and-order form the device call takes gives the loops' records"""
    last = ck.scene_registered()[-1]
    for mv in (0, 3):
        a, b = ck.export(last, 0, -1, mv, False), ck.pub_color_points(last, mv)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2]
        a, b = ck.export(last, 1, -1, mv, True), ck.save_color_points(last, mv)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2]
        tot = a[2]
        assert tot["scanned"] == tot["published"] + tot["below_views"] + tot["stale"] == len(last) - 1


# ------------------------------------------------------------------------------------------------ the schedule's known answers
def test_schedule_known_answers():
    for p, want in ((0, [0]), (999, [999]), (1000, [1000, 0]), (1001, [1000, 1])):
        s = ck.TopicSchedule()
        assert s.round(p) == want and (s.number_of_points_per_topic, s.sleep_time_after_pub) == (1000, 10)
    s = ck.TopicSchedule()
    assert s.round(44000) == [1000] * 44 + [0]                              # 45 topics: growth
    assert (s.number_of_points_per_topic, s.sleep_time_after_pub) == (1500, 15)
    assert s.round(44000) == [1500] * 29 + [500]                            # the second round uses the grown size: 30 topics, no growth
    assert (s.number_of_points_per_topic, s.sleep_time_after_pub) == (1500, 15)
    assert s.round(66000) == [1500] * 44 + [0]                              # 45 again
    assert (s.number_of_points_per_topic, s.sleep_time_after_pub) == (2250, 22)      # 15 * 1.5 = 22.5, truncated
    s = ck.TopicSchedule()
    assert s.round(43999) == [1000] * 43 + [999]                            # 44 topics: no growth
    assert (s.number_of_points_per_topic, s.sleep_time_after_pub) == (1000, 10)


# ------------------------------------------------------------------------------------------------ against the reference's pieces
@needs_reference
def test_the_loops_equal_the_reference_after_every_render(reader):
    counts, obs = ck.scene_observations()
    regs = ck.scene_registered()
    xyz = regs[0].xyz
    n = len(xyz)
    assert counts.shape == (len(rk.RENDERS), n)
    compared = 0
    for k, reg in enumerate(regs):
        start = np.zeros(n + 1, np.int64)
        np.cumsum(counts[k], out=start[1:])
        flat = np.concatenate([o[:counts[k, i]] for i, o in enumerate(obs)] + [np.zeros((0, 5))]).reshape(-1, 5)
        flat = np.ascontiguousarray(flat)
        assert len(flat) == start[-1]
        for mv in ck.MINIMUM_VIEWS:
            for which in (ck.PUB, ck.THREAD_PUB, ck.SAVE):
                rec = np.zeros(n, ck.CLOUD_DTYPE); idx = np.zeros(n, np.int32); topics = np.zeros(n // 7 + 2, np.int32); n_topics = np.zeros(1, np.int32)
                m = reader.cer_cloud(n, _vp(xyz), _vp(start), _vp(flat), which, mv, 7 if which == ck.THREAD_PUB else 0, _vp(rec), _vp(idx), _vp(topics), _vp(n_topics))
                if which == ck.SAVE:
                    w_rec, w_idx, w_tot = ck.save_color_points(reg, mv)
                else:
                    w_rec, w_idx, w_tot = ck.pub_color_points(reg, mv)
                assert m == len(w_rec) == w_tot["published"], (k, mv, which)
                assert rec[:m].tobytes() == w_rec.tobytes(), (k, mv, which)    # records and order, bytewise
                assert np.array_equal(idx[:m], w_idx), (k, mv, which)
                if which == ck.THREAD_PUB:
                    s = ck.TopicSchedule()
                    s.number_of_points_per_topic = 7
                    assert list(topics[:n_topics[0]]) == s.round(m), (k, mv)
                compared += m
    assert compared > 500000
