"""Builds and drives tests/pc2_ref_reader.cpp: the reference's cloudProcessing::process with its three PointCloud2 handlers, compiled where
they lie.

Used by tests/test_pc2_checker_reference.py, tests/golden/make_golden_pc2.py and tools/pc2_decode_time.py.
The reader is the reference's own translation unit src/cloudProcessing.cpp -- its loops, its std::sort with time_list* (from
oracle/_ref/libref_path.so), its point3D -- driven by a test-owned message stand-in (tests/stub_pc2) and a test-owned pcl::fromROSMsg
(tests/pc2_ref_reader.cpp).  Nothing compiled is kept: the caller names the directory, a temporary one.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import livox_reader as lr

ROOT, REF, REF_TSL, REF_HDRS, REF_LIB = lr.ROOT, lr.REF, lr.REF_TSL, lr.REF_HDRS, lr.REF_LIB
GOLDEN_FULL_RECORDS = lr.GOLDEN_FULL_RECORDS          # golden_pc2.npz keeps a message's records as they are up to this many; beyond, their SHA-256
available, records_of, digest = lr.available, lr.records_of, lr.digest


def build(tmp):
    """compile the reader into the directory tmp and load it"""
    inc = os.path.join(str(tmp), "include")
    os.makedirs(inc)
    for h in REF_HDRS:
        os.symlink(os.path.join(REF, "include", h + ".h"), os.path.join(inc, h + ".h"))
    os.symlink(os.path.join(ROOT, "oracle", "ref_shim", "local", "imageProcessing.h"), os.path.join(inc, "imageProcessing.h"))
    out = os.path.join(str(tmp), "libpc2_ref_reader.so")
    refdir = os.path.dirname(REF_LIB)
    # flags of oracle/Makefile's REFFLAGS; tests/stub_pc2 ahead of tests/stub_livox (its CustomMsg lets livoxHandler compile) ahead of
    # oracle/ref_shim; -Bsymbolic: see pc2_ref_reader.cpp
    cmd = ["g++", "-std=c++14", "-O3", "-fPIC", "-w", "-ffp-contract=off", "-shared", "-I" + os.path.join(ROOT, "tests", "stub_pc2"),
           "-I" + os.path.join(ROOT, "tests", "stub_livox"), "-I" + os.path.join(ROOT, "oracle"), "-I" + inc, "-I" + os.path.join(ROOT, "oracle", "ref_shim"),
           "-I" + REF_TSL, "-o", out, os.path.join(ROOT, "tests", "pc2_ref_reader.cpp"), os.path.join(REF, "src", "cloudProcessing.cpp"),
           "-L" + refdir, "-l:libref_path.so", "-Wl,-rpath," + refdir, "-Wl,-Bsymbolic"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(out)
    p = C.c_void_p
    lib.pcr_new.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]
    lib.pcr_new.restype = p
    lib.pcr_free.argtypes = [p]
    lib.pcr_free.restype = None
    lib.pcr_feed.argtypes = [p, C.c_int, p, C.c_size_t, p, C.c_double, p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.pcr_feed.restype = C.c_int
    return lib


def layout_words(layout):
    return np.array([layout.width, layout.height, layout.point_step, layout.row_step, layout.off_x, layout.off_y, layout.off_z, layout.off_time,
                     layout.off_ring], dtype=np.int32)


class Decoder:
    """one cloudProcessing object of the reference, fed message by message"""

    def __init__(self, lib, lidar_type, n_scans, scan_rate, unit, blind, pfn):
        self.lib, self.lidar_type = lib, int(lidar_type)
        self.h = lib.pcr_new(int(lidar_type), int(n_scans), int(scan_rate), int(unit), float(blind), int(pfn))

    def feed(self, data, layout, stamp):
        """-> (rows (k, 9): raw_point, point, relative_time, timestamp, alpha_time of the points this message queued, last_end_time, given)"""
        d = np.ascontiguousarray(data, dtype=np.uint8)
        w = layout_words(layout)
        cap = max(int(layout.width) * int(layout.height), 1)
        out = np.zeros((cap, 9))
        last, given = C.c_double(), C.c_int()
        k = self.lib.pcr_feed(self.h, self.lidar_type, d.ctypes.data_as(C.c_void_p), d.nbytes, w.ctypes.data_as(C.c_void_p), float(stamp),
                              out.ctypes.data_as(C.c_void_p), cap, C.byref(last), C.byref(given))
        assert 0 <= k <= cap
        return out[:k].copy(), last.value, given.value

    def close(self):
        if self.h:
            self.lib.pcr_free(self.h)
            self.h = None


def run(lib, case):
    """every message of a case through one decoder -> list of (rows, last_end_time, given)"""
    dec = Decoder(lib, case["lidar_type"], case["n_scans"], case["scan_rate"], case["unit"], case["blind"], case["pfn"])
    try:
        return [dec.feed(m["data"], m["layout"], m["stamp"]) for m in case["msgs"]]
    finally:
        dec.close()
