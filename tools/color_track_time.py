"""One srl_color_map_track_update at the shipped sizes: 300 tracked points, the candidates of an all-points selection on a 1280 x 1024
frame.  HIP events around the call (torch.cuda.Event on the context's device), after warm-up calls; host wall time beside them."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import sr_livo_amd as srl  # noqa: E402
from sr_livo_amd import capi  # noqa: E402

rng = np.random.default_rng(1)
n_pts = 1_200_000
# a slab in front of a camera at the origin looking along +z: x, y spread so that the 1280 x 1024 frame is covered
z = rng.uniform(8.0, 30.0, n_pts)
pts = np.stack([rng.uniform(-1.1, 1.1, n_pts) * z, rng.uniform(-0.9, 0.9, n_pts) * z, z], 1)
ctx = srl.Context(0)
ctx.color_map_create(capi.default_color_opts(size_voxel_map=0.1, max_num_points_in_voxel=50, min_distance_points=0.01, add_point_step=1))
for part in np.array_split(pts, 12):
    ctx.color_map_insert(part, 1.0, 0.0)
rows, cols = 1024, 1280
cam = capi.ColorCamera((C.c_double * 4)(1, 0, 0, 0), (C.c_double * 3)(0, 0, 0), 640.0, 640.0, 640.0, 512.0, 0.005)
sel, stot = ctx.color_map_select(cam, rows, cols, None, capi.default_color_select_opts(use_all_points=1))
print("map points", ctx.color_map_size(), "selection", stot.as_tuple())
cand = np.ascontiguousarray(sel["pool"])
rec, _, _, tot = ctx.color_map_track_update(cam, rows, cols, np.zeros(0, capi.COLOR_TRACK_POINT_DTYPE), cand)
tracked = rec.copy()
tracked["u"] += rng.normal(0, 4.0, len(tracked)).astype(np.float32)
print("fill", tot.as_tuple(), "tracked", len(tracked), "candidates", len(cand))
o = capi.default_color_track_opts()
out = np.zeros(len(tracked) + 300, capi.COLOR_TRACK_POINT_DTYPE)
t = capi.ColorTrackTotals()


def call():
    return ctx.lib.srl_color_map_track_update(ctx.h, C.byref(cam), rows, cols, capi._ptr(tracked), len(tracked), capi._ptr(cand), len(cand), C.byref(o),
                                              capi._ptr(out), len(out), None, None, C.byref(t))


def select():
    return ctx.color_map_select(cam, rows, cols, None, capi.default_color_select_opts(use_all_points=1), totals_only=True)


for name, fn in (("track_update", call), ("select_all_points", select)):
    for _ in range(20):
        fn()
    ev, wall = [], []
    for _ in range(200):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - w0) * 1e6)
        ev.append(a.elapsed_time(b) * 1e3)
    ev, wall = np.array(ev), np.array(wall)
    print("%s: HIP events median %.1f us (p10 %.1f, p90 %.1f); host wall median %.1f us; n = %d" % (name, np.median(ev), np.percentile(ev, 10),
                                                                                               np.percentile(ev, 90), np.median(wall), len(ev)))
print("last totals", t.as_tuple())
ctx.close()
