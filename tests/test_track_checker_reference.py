"""The sequential restatement of the tracker's point-set update (tests/track_checker.py) pinned to the reference's own pieces, bit for bit.

opticalFlowTracker::updateAndAppendTrackPoints itself cannot be compiled against the stand-ins of oracle/ (it needs OpenCV's Point2f and
the include mirror shadows the vision stage).  tests/track_ref_reader.cpp drives what can: cloudFrame::project3dPointInThisImage, the
reference's own Hash_map_2d<int, float> holding the occupancy mask and Eigen's norm(), with the loops' remaining statements restated
line by line between them and the map walked in the caller's order; compiled here, into the test's temporary directory, against a
temporary include mirror of symlinks as oracle/Makefile's `refpath` target builds one and linked to oracle/_ref/libref_path.so.  Neither
the reader's binary nor anything of the reference is committed; the tests skip where the reference tree or the library is absent.

Tracked points behind the camera are left out of the comparison: there the reference forms its error from the previous element's pixel
(the stated departure), and so are positions the map does not hold and duplicates, which a std::map cannot hold.  Each compared set loses
at most 5 % of its tracked points that way.  The reference does not name what lies behind its break: the checker's `cut` is compared as
`not reached`.  A repeated candidate is walked again by the reference: it is found in the map if its first occurrence was added and is
otherwise refused for the same reason -- which the test asserts before it compares it as `already tracked`."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import select_checker as sk
import track_checker as tk
from oracle import pyref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_TSL = os.path.join(REF, "thirdLibrary", "tessil-src", "include")
REF_HDRS = ("cloudMap", "utility", "eskfEstimator", "state", "parameters", "lioOptimization", "cloudProcessing")      # oracle/Makefile: REF_HDRS

pytestmark = pytest.mark.skipif(
    not pr.available() or not os.path.exists(os.path.join(REF, "include", "lioOptimization.h")) or shutil.which("g++") is None,
    reason="needs oracle/_ref/libref_path.so, the reference tree and g++")


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("track_ref_reader")
    inc = tmp / "include"
    inc.mkdir()
    for h in REF_HDRS:
        os.symlink(os.path.join(REF, "include", h + ".h"), inc / (h + ".h"))
    os.symlink(os.path.join(ROOT, "oracle", "ref_shim", "local", "imageProcessing.h"), inc / "imageProcessing.h")
    out = tmp / "libtrack_ref_reader.so"
    refdir = os.path.join(ROOT, "oracle", "_ref")
    cmd = ["g++", "-std=c++14", "-O1", "-fPIC", "-w", "-ffp-contract=off", "-shared", "-I" + os.path.join(ROOT, "oracle"), "-I" + str(inc),
           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + REF_TSL, "-o", str(out), os.path.join(ROOT, "tests", "track_ref_reader.cpp"),
           "-L" + refdir, "-l:libref_path.so", "-Wl,-rpath," + refdir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    pr.load()
    lib = C.CDLL(str(out))
    p = C.c_void_p
    lib.trr_update.argtypes = [p, C.c_int, C.c_int, C.c_double, C.c_uint, C.c_int, p, p, p, p, p, p, p, C.c_int, p, p, p, p]
    lib.trr_update.restype = C.c_int
    return lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _compare(reader, case):
    name, k, margin, tracked, cand, md, maximum = case
    pos = tk.pool_positions()
    cam, rows, cols, _ = sk.scene_camera(k, margin)
    # what the reference's map cannot hold, or walks differently: left out
    first = tk.track_update_sequential(pos, cam, rows, cols, tracked, cand, md, maximum)
    left_out = np.isin(first[1], (tk.BEHIND, tk.UNKNOWN, tk.DUPLICATE))
    behind = int((first[1] == tk.BEHIND).sum())
    assert behind <= 0.05 * max(len(tracked), 1), (name, behind, len(tracked))
    tracked = tracked[~left_out]
    cand = cand[(cand >= 0) & (cand < len(pos))]
    want = tk.track_update_sequential(pos, cam, rows, cols, tracked, cand, md, maximum)
    n, nc = len(tracked), len(cand)
    cam12 = np.array(list(cam.q) + list(cam.t) + [cam.fx, cam.fy, cam.cx, cam.cy, cam.fov_margin])
    xyz_t = np.ascontiguousarray(pos[tracked["pool"]], np.float32).reshape(n, 3)
    xyz_c = np.ascontiguousarray(pos[cand], np.float32).reshape(nc, 3)
    uv_t = np.ascontiguousarray(np.stack([tracked["u"], tracked["v"]], 1), np.float32).reshape(n, 2)
    id_t, count_t, id_c = np.ascontiguousarray(tracked["pool"]), np.ascontiguousarray(tracked["flagged"]), np.ascontiguousarray(cand, np.int32)
    state_t = np.zeros(n, np.uint8); count_out = np.zeros(n, np.int32); error = np.zeros(n)
    state_c = np.zeros(nc, np.uint8); uv_c = np.zeros((nc, 2), np.float32)
    size = reader.trr_update(_vp(cam12), rows, cols, md, maximum, n, _vp(id_t), _vp(xyz_t), _vp(uv_t), _vp(count_t), _vp(state_t), _vp(count_out), _vp(error),
                             nc, _vp(id_c), _vp(xyz_c), _vp(state_c), _vp(uv_c))
    rec, t_out, c_out, tot, _ = want
    # the first loop: kept / kept flagged / erased, the counts behind it
    assert state_t.tobytes() == t_out.tobytes(), (name, np.flatnonzero(state_t != t_out)[:8])
    kept = state_t != 2
    assert np.array_equal(count_out[kept], rec["flagged"][:tot["kept"]]) and (count_out[~kept] == 0).all()
    # the second: a repeat behaves as its first occurrence did
    seen, got_c = {}, state_c.copy()
    for j, p in enumerate(int(c) for c in cand):
        if p in seen and got_c[j] != tk.NOT_REACHED:
            assert state_c[j] == (tk.ALREADY_TRACKED if state_c[seen[p]] in (tk.ADDED, tk.ALREADY_TRACKED) else state_c[seen[p]]), (name, j)
            got_c[j] = tk.ALREADY_TRACKED
        seen.setdefault(p, j)
    want_c = np.where(c_out == tk.CUT, tk.NOT_REACHED, c_out).astype(np.uint8)
    assert got_c.tobytes() == want_c.tobytes(), (name, np.flatnonzero(got_c != want_c)[:8])
    added = state_c == tk.ADDED
    assert size == len(rec) == tot["kept"] + tot["added"] and np.array_equal(cand[added], rec["pool"][tot["kept"]:])
    assert uv_c[added].tobytes() == np.stack([rec["u"], rec["v"]], 1)[tot["kept"]:].tobytes()        # the two casts to float
    return want, error


def test_the_sequence_equals_the_reference(reader):
    compared = 0
    repeats = 0
    for case, result in zip(tk.cases(), tk.case_results()):
        behind = int((result[1] == tk.BEHIND).sum())
        if case[6] < 0 or behind > 0.05 * max(len(case[3]), 1):             # the reference's maximum is unsigned; the stated departure
            continue
        want, _ = _compare(reader, case)
        repeats += len(case[4]) - len(set(case[4].tolist()))
        compared += 1
    assert compared >= 20 and repeats > 100


def test_the_error_is_eigens_norm(reader):
    case = {c[0]: c for c in tk.cases()}["track2"]
    want, error = _compare(reader, case)
    pos = tk.pool_positions()
    cam, rows, cols, _ = sk.scene_camera(case[1], case[2])
    for t, e in zip(case[3], error):
        p32 = pos[int(t["pool"])]
        _, u_d, v_d = cam.project((float(p32[0]), float(p32[1]), float(p32[2])), rows, cols)
        du, dv = u_d - float(t["u"]), v_d - float(t["v"])
        assert np.float64(np.sqrt(np.float64(du * du + dv * dv))).tobytes() == np.float64(e).tobytes()
