"""Builds and drives tests/flow_ref_reader.cpp: the reference's src/lkpyramid.cpp compiled where it lies against the stand-in of
tests/stub_opencv_lk (its own LK statements and Scharr derivative; pyrDown, copyMakeBorder, cvRound and cvFloor are the stand-in's),
into a scratch directory.  Neither the binary nor anything of the reference is committed.  Used by
tests/test_flow_checker_reference.py and tests/golden/make_golden_flow.py."""
import ctypes as C
import os
import shutil
import subprocess
import zlib

import numpy as np

import flow_checker as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


def available():
    return os.path.exists(os.path.join(REF, "src", "lkpyramid.cpp")) and os.path.exists(os.path.join(REF, "include", "lkpyramid.h")) and shutil.which("g++") is not None


def build(tmp):
    """compiles the reader into the directory `tmp`; returns the loaded library"""
    os.makedirs(str(tmp), exist_ok=True)
    out = os.path.join(str(tmp), "libflow_ref_reader.so")
    cmd = ["g++", "-std=c++14", "-O2", "-fPIC", "-w", "-ffp-contract=off", "-msse2", "-shared", "-I" + os.path.join(ROOT, "tests", "stub_opencv_lk"),
           "-I" + os.path.join(REF, "include"), "-o", out, os.path.join(ROOT, "tests", "flow_ref_reader.cpp"), os.path.join(REF, "src", "lkpyramid.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(out)
    p = C.c_void_p
    lib.frr_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.frr_create.restype = p
    lib.frr_destroy.argtypes = [p]
    lib.frr_destroy.restype = None
    lib.frr_max_level.argtypes = [p]
    lib.frr_criteria.argtypes = [p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    lib.frr_criteria.restype = None
    lib.frr_track.argtypes = [p, p, C.c_int, C.c_int, p, C.c_int, p, p]
    lib.frr_level.argtypes = [p, C.c_int, p, p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Tracker:
    """the reference's LKOpticalFlowKernel with opticalFlowTracker's constructor arguments"""

    def __init__(self, lib, opts=None):
        o = opts or fc.Opts()
        self.lib = lib
        self.h = lib.frr_create(o.win, o.max_level, o.max_count, o.epsilon, o.min_eig_threshold)

    def close(self):
        if self.h:
            self.lib.frr_destroy(self.h)
        self.h = None

    def criteria(self):
        c, e = C.c_int(), C.c_double()
        self.lib.frr_criteria(self.h, C.byref(c), C.byref(e))
        return c.value, e.value

    def track_image(self, gray, prev_xy):
        """(next_xy, status, trackImage's return value, L, padded images, padded derivatives of the image given)"""
        g = np.ascontiguousarray(gray, dtype=np.uint8)
        pts = np.ascontiguousarray(prev_xy, dtype=np.float32).reshape(-1, 2)
        n = len(pts)
        nxt, status = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        got = self.lib.frr_track(self.h, _vp(g), g.shape[0], g.shape[1], _vp(pts), n, _vp(nxt), _vp(status))
        L = self.lib.frr_max_level(self.h)
        images, derivs = [], []
        rows, cols = g.shape
        for level in range(L + 1):
            img = np.zeros((rows + 2 * fc.WIN, cols + 2 * fc.WIN), np.uint8)
            der = np.zeros((rows + 2 * fc.WIN, cols + 2 * fc.WIN, 2), np.int16)
            r, c = C.c_int(), C.c_int()
            assert self.lib.frr_level(self.h, level, _vp(img), _vp(der), C.byref(r), C.byref(c)) == 0 and (r.value, c.value) == (rows, cols)
            images.append(img)
            derivs.append(der)
            rows, cols = (rows + 1) // 2, (cols + 1) // 2
        return nxt, status, got, L, images, derivs


def run_scene(lib, name):
    imgs, pts, opts = fc.scene(name)
    tr = Tracker(lib, opts)
    try:
        return [tr.track_image(im, pts) for im in imgs]
    finally:
        tr.close()


def golden_pack(lib):
    """what tests/golden/golden_flow.npz holds: per scene L, per call the CRC-32 of every padded level and derivative and, for the
    tracking calls, next_xy as raw float bits and the status"""
    out = {}
    for name in fc.SCENES:
        calls = run_scene(lib, name)
        out[f"{name}/L"] = np.int32(calls[-1][3])
        for k, (nxt, status, got, L, images, derivs) in enumerate(calls):
            out[f"{name}/image_crc{k}"] = np.array([zlib.crc32(a.tobytes()) for a in images], dtype=np.uint32)
            out[f"{name}/deriv_crc{k}"] = np.array([zlib.crc32(a.tobytes()) for a in derivs], dtype=np.uint32)
            if k:
                out[f"{name}/next{k}"] = nxt.view(np.uint32)
                out[f"{name}/status{k}"] = status
    return out
