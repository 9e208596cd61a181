"""Builds and drives tests/livox_ref_reader.cpp: the reference's cloudProcessing::livoxHandler, compiled where it lies.

Used by tests/test_livox_checker_reference.py and tests/golden/make_golden_livox.py.  The reader is the reference's own translation
unit src/cloudProcessing.cpp -- its loop, its std::sort with time_list (from oracle/_ref/libref_path.so), its point3D -- driven by a
test-owned message stand-in (tests/stub_livox).  Nothing compiled is kept: the caller names the directory, a temporary one.
"""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_TSL = os.path.join(REF, "thirdLibrary", "tessil-src", "include")
REF_HDRS = ("cloudMap", "utility", "eskfEstimator", "state", "parameters", "lioOptimization", "cloudProcessing")      # oracle/Makefile: REF_HDRS
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libref_path.so")

# golden_livox.npz keeps the records of a case as they are up to this many; beyond, their SHA-256 (no committed file above 1 MiB)
GOLDEN_FULL_RECORDS = 2048


def available():
    return os.path.exists(os.path.join(REF, "src", "cloudProcessing.cpp")) and os.path.exists(REF_LIB) and shutil.which("g++") is not None


def build(tmp):
    """compile the reader into the directory tmp and load it"""
    inc = os.path.join(str(tmp), "include")
    os.makedirs(inc)
    for h in REF_HDRS:
        os.symlink(os.path.join(REF, "include", h + ".h"), os.path.join(inc, h + ".h"))
    os.symlink(os.path.join(ROOT, "oracle", "ref_shim", "local", "imageProcessing.h"), os.path.join(inc, "imageProcessing.h"))
    out = os.path.join(str(tmp), "liblivox_ref_reader.so")
    refdir = os.path.dirname(REF_LIB)
    # flags of oracle/Makefile's REFFLAGS; tests/stub_livox ahead of oracle/ref_shim; -Bsymbolic: see livox_ref_reader.cpp
    cmd = ["g++", "-std=c++14", "-O3", "-fPIC", "-w", "-ffp-contract=off", "-shared", "-I" + os.path.join(ROOT, "tests", "stub_livox"),
           "-I" + os.path.join(ROOT, "oracle"), "-I" + inc, "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + REF_TSL, "-o", out,
           os.path.join(ROOT, "tests", "livox_ref_reader.cpp"), os.path.join(REF, "src", "cloudProcessing.cpp"),
           "-L" + refdir, "-l:libref_path.so", "-Wl,-rpath," + refdir, "-Wl,-Bsymbolic"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(out)
    p = C.c_void_p
    lib.lrr_livox.argtypes = [p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, p, C.c_int, C.POINTER(C.c_double)]
    lib.lrr_livox.restype = C.c_int
    return lib


def run(lib, case):
    """-> (rows (k, 9): raw_point, point, relative_time, timestamp, alpha_time of the queued points, last_end_time)"""
    pts = case["points"]
    cap = max(len(pts), 1)
    out = np.zeros((cap, 9))
    last = C.c_double()
    k = lib.lrr_livox(pts.ctypes.data_as(C.c_void_p), len(pts), case["stamp"], case["n_scans"], case["unit"], case["blind"], case["pfn"],
                      out.ctypes.data_as(C.c_void_p), cap, C.byref(last))
    assert 0 <= k <= cap
    return out[:k].copy(), last.value


def records_of(rows):
    """the five doubles per point the device queue holds: raw_point, relative_time, timestamp"""
    return np.ascontiguousarray(np.concatenate([rows[:, 0:3], rows[:, 6:8]], axis=1))


def digest(records):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(records, dtype=np.float64).tobytes()).digest(), dtype=np.uint8).copy()
