"""The sequential restatement of the colour half of addPointsToMap (tests/color_checker.py) and the recorded results of
tests/golden/golden_color_map.npz, pinned to the reference's own translation units bit for bit.

oracle/_ref/libref_path.so runs the node's addPointsToMap (ref_node_add_points_to_map), which fills lio.color_voxel_map,
img_pro->map_tracker->rgb_points_vec, hashmap_3d_points and voxels_recent_visited_temp (to_rendering = false: the list accumulates); the
harness exports none of them.  tests/color_ref_reader.cpp reads them through ref_node_lio_ptr(): compiled here, into the test's
temporary directory, against a temporary include mirror of symlinks as oracle/Makefile's `refpath` target builds one (the shim's
imageProcessing.h shadowing the real one) and linked to libref_path.so.  Neither the reader's binary nor anything of the reference is
committed; the tests skip where the reference tree or the library is absent.

What the harness fixes: the colour options come from the parameter server when the node is constructed (pyref.set_params),
time_last_process = 0 and time_sweep_end = 1 + (LiDAR voxels before the call).  The branch |time_sweep_end - time_last_process| <= 1e-5
can therefore NOT be reached through the harness (1 + V is never 0): only the restatement covers it (and the device test compares the
device with the restatement there).  Equal consecutive times can: a batch inserted with the LiDAR min_num_points = 3 adds no LiDAR voxel.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import color_checker as cc
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
    tmp = tmp_path_factory.mktemp("color_ref_reader")
    inc = tmp / "include"
    inc.mkdir()
    for h in REF_HDRS:
        os.symlink(os.path.join(REF, "include", h + ".h"), inc / (h + ".h"))
    os.symlink(os.path.join(ROOT, "oracle", "ref_shim", "local", "imageProcessing.h"), inc / "imageProcessing.h")
    out = tmp / "libcolor_ref_reader.so"
    refdir = os.path.join(ROOT, "oracle", "_ref")
    cmd = ["g++", "-std=c++14", "-O1", "-fPIC", "-w", "-shared", "-I" + os.path.join(ROOT, "oracle"), "-I" + str(inc),
           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + REF_TSL, "-o", str(out), os.path.join(ROOT, "tests", "color_ref_reader.cpp"),
           "-L" + refdir, "-l:libref_path.so", "-Wl,-rpath," + refdir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    pr.load()                                   # the library the reader reads
    lib = C.CDLL(str(out))
    p = C.c_void_p
    lib.crr_sizes.argtypes = [p, p]
    lib.crr_map.argtypes = [p, p, p, p, p]
    lib.crr_registered.argtypes = [p, C.c_double, p, p, p]
    lib.crr_grid.argtypes = [p, p, p, C.c_int64]; lib.crr_grid.restype = C.c_int64
    lib.crr_visited.argtypes = [p, p, C.c_int64]; lib.crr_visited.restype = C.c_int64
    pr.load().ref_node_lio_ptr.argtypes = [p]; pr.load().ref_node_lio_ptr.restype = p
    return lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class RefColour:
    """a reference node with the given colour options, and what the reader sees in it"""

    def __init__(self, reader, opt):
        pr.set_params(num={"map_options/size_voxel_map": opt[0], "map_options/max_num_points_in_voxel": opt[1],
                           "map_options/min_distance_points": opt[2], "map_options/add_point_step": opt[3]})
        self.node = pr.Node(True)
        self.reader, self.opt = reader, opt
        self.lio = C.c_void_p(self.node.lib.ref_node_lio_ptr(self.node.h))

    def close(self):
        self.node.close()
        pr.set_params()

    def lidar_voxels(self):
        return int(self.node.lib.ref_node_map_num_voxels(self.node.h))

    def insert(self, pts, min_num_points=0):
        """returns the time_sweep_end the harness gives this batch"""
        t = 1.0 + self.lidar_voxels()
        self.node.add_points_to_map(pts, voxel_size=1.0, cap=20, min_dist=0.1, min_num_points=min_num_points)
        return t

    def sizes(self):
        out = np.zeros(4, np.int64)
        self.reader.crr_sizes(self.lio, _vp(out))
        return tuple(int(v) for v in out)

    def map_dict(self):
        V, P, _, _ = self.sizes()
        keys = np.zeros((V, 3), np.int16); counts = np.zeros(V, np.int32); times = np.zeros(V); xyz = np.zeros((P, 3), np.float32)
        self.reader.crr_map(self.lio, _vp(keys), _vp(counts), _vp(times), _vp(xyz))
        first = np.concatenate([[0], np.cumsum(counts)])
        return {tuple(int(c) for c in keys[v]): (times[v], _bits(xyz[first[v]: first[v + 1]]).tobytes()) for v in range(V)}

    def registered(self):
        R = self.sizes()[2]
        xyz = np.zeros((R, 3), np.float32); keys = np.zeros((R, 3), np.int16); slot = np.zeros(R, np.int32)
        self.reader.crr_registered(self.lio, float(self.opt[0]), _vp(xyz), _vp(keys), _vp(slot))
        return xyz, keys, slot

    def grid(self):
        G = self.sizes()[3]
        cells = np.zeros((G, 3), np.int64); index = np.zeros(G, np.int32)
        assert self.reader.crr_grid(self.lio, _vp(cells), _vp(index), G) == G
        return {tuple(int(c) for c in cells[i]): int(index[i]) for i in range(G)}

    def visited(self):
        n = self.reader.crr_visited(self.lio, None, 0)
        out = np.zeros((n, 3), np.int32)
        assert self.reader.crr_visited(self.lio, _vp(out), n) == n
        return out


def _equal(ref, chk, visited_all):
    """the reference's containers against the restatement's, bit for bit and in order where the reference has an order"""
    assert ref.sizes() == (len(chk.voxels), chk.num_points, len(chk.registered), len(chk.grid))
    keys, counts, times, xyz, _ = chk.map_arrays()
    first = np.concatenate([[0], np.cumsum(counts)])
    mine = {tuple(int(c) for c in keys[v]): (times[v], _bits(xyz[first[v]: first[v + 1]]).tobytes()) for v in range(len(keys))}
    theirs = ref.map_dict()
    assert mine.keys() == theirs.keys()
    for k in mine:
        assert mine[k] == theirs[k], k                       # last_visited_time and the points in slot order
    rx, rk, rs = ref.registered()
    wx, wk, ws = chk.registered_arrays()
    assert np.array_equal(_bits(rx), _bits(wx)) and np.array_equal(rk, wk) and np.array_equal(rs, ws)      # rgb_points_vec in order
    assert ref.grid() == chk.grid                            # every cell, and which registered point holds it
    assert np.array_equal(ref.visited(), visited_all)


@pytest.mark.parametrize("o", range(len(cc.OPTION_SETS)))
def test_restatement_and_golden_equal_the_reference(reader, o):
    opt = cc.OPTION_SETS[o]
    golden = np.load(os.path.join(ROOT, "tests", "golden", "golden_color_map.npz"), allow_pickle=False)
    ref, chk = RefColour(reader, opt), cc.ColorChecker(*opt)
    gold = cc.ColorChecker(*opt)           # driven with the golden file's times: the decisions do not depend on the times' values
    try:
        visited_all = []
        t_gold = 1.0
        for j in range(3):
            pts = cc.scene_batch(j)
            t = ref.insert(pts)
            assert j == 0 or t > 1.0
            outcome, stored, visited = chk.insert(pts, t, 0.0)
            visited_all.append(visited)
            _equal(ref, chk, np.concatenate(visited_all))
            # the recorded results are these decisions
            g_outcome, g_stored, g_visited = gold.insert(pts, t_gold, 0.0)
            t_gold += 1.0 + j
            assert np.array_equal(outcome, g_outcome) and g_stored.tobytes() == stored.tobytes() and np.array_equal(visited, g_visited)
            assert np.array_equal(outcome, golden[f"o{o}_b{j}_outcome"])
            assert np.array_equal(visited.astype(np.int16), golden[f"o{o}_b{j}_visited"])
            assert np.array_equal(stored["batch_index"], golden[f"o{o}_b{j}_batch_index"])
            assert np.array_equal(stored["point_index"], golden[f"o{o}_b{j}_point_index"])
            assert np.array_equal(stored["slot"].astype(np.uint8), golden[f"o{o}_b{j}_slot"])
            assert np.array_equal(np.stack([stored["kx"], stored["ky"], stored["kz"]], 1), golden[f"o{o}_b{j}_keys"])
        V, P, R, G = ref.sizes()
        assert (P, V, R, G) == tuple(int(v) for v in golden[f"o{o}_sizes"])        # (the order of srl_color_map_size)
        # a test that never reaches a branch proves nothing
        assert min(chk.n_refused_full, chk.n_stored_not_registered, chk.n_created, chk.n_retouched) > 0
        if opt[2] == 0.01:                 # the alias box sits one wrap of the 0.01 m grid away (655.36 m)
            assert min(chk.n_stored_not_registered_other_voxel, chk.n_registered_after_unstored) > 0
    finally:
        ref.close()


def test_equal_sweep_times_suppress_retouched_voxels_as_in_the_reference(reader):
    opt = cc.OPTION_SETS[0]
    ref, chk = RefColour(reader, opt), cc.ColorChecker(*opt)
    try:
        visited_all, times = [], []
        base = cc.scene_batch(0)
        ref.insert(base)                                      # a LiDAR map to append to; its colour insertion is part of the run
        t0 = 1.0
        visited_all.append(chk.insert(base, t0, 0.0)[2])
        suppressed = 0
        for j in range(1, 4):
            pts = cc.scene_batch(j)[:5000]
            t = ref.insert(pts, min_num_points=3)             # adds no LiDAR voxel: the next batch gets the same time_sweep_end
            times.append(t)
            before = {k for k, v in chk.voxels.items() if abs(v.last_visited_time - t) <= 1e-5}
            _, _, visited = chk.insert(pts, t, 0.0)
            touched = {tuple(int(c) for c in k) for k in cc.short_keys(pts.astype(np.float32), opt[0])}
            suppressed += len(before & touched)
            visited_all.append(visited)
            _equal(ref, chk, np.concatenate(visited_all))
        assert times[0] == times[1] == times[2] and times[0] > 1.0
        assert suppressed > 0 and sum(len(v) for v in visited_all[1:]) > 0
    finally:
        ref.close()
