"""Time the selection of colour-map points for projection (srl_color_map_select: rgbMapTracker::selectPointsForProjection,
rgbMapTracker.cpp:45-152) on the street scene of tools/color_map_probe.py: frames of 24k / 64k / 256k points inserted into a growing
map; after every insertion a LIST-mode call over the voxels that insertion visited (minimum_dis 10, skip_step 1, a 1280 x 1024 frame, a
camera that rides with the sensor: refreshPointsForProjection), and on the grown map ALL-points calls (every registered point into
about 10^4 cells: the contended case).  Host clock around the call (it ends in a synchronisation), records included; median over the
frames after the first, and over the all-points repeats after the first.  For kernel times run under rocprofv3 --kernel-trace --stats,
one leg at a time (COLOR_LEGS=l: the list-mode calls only, COLOR_LEGS=a: the all-points calls only), so that the k_select_* rows of the
statistics belong to one mode.
There is no CPU figure from the reference: selectPointsForProjection cannot be compiled against the stand-in headers.  Prints one JSON
line per frame size."""
import ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sr_livo_amd as srl
from sr_livo_amd import capi
SIZES = [int(a) for a in sys.argv[1:]] or [24_000, 64_000, 256_000]
FRAMES = int(os.environ.get("COLOR_FRAMES", "8"))
REPEATS = int(os.environ.get("COLOR_REPEATS", "6"))
LEGS = os.environ.get("COLOR_LEGS", "la")
ROWS, COLS = 1024, 1280


def frame(n, f):
    """tools/color_map_probe.py's street scene: a sensor that moves 1 m per frame along x: ground, two walls, clutter"""
    rng = np.random.default_rng(9400 + f)
    g, w = n // 2, n // 4
    ground = np.stack([rng.uniform(-40, 40, g) + f, rng.uniform(-40, 40, g), -1.7 + 0.02 * rng.standard_normal(g)], 1)
    walls = np.stack([rng.uniform(-40, 40, w) + f, rng.choice([-8.0, 8.0], w) + 0.02 * rng.standard_normal(w), rng.uniform(-1.7, 4.0, w)], 1)
    clutter = np.stack([rng.uniform(-40, 40, n - g - w) + f, rng.uniform(-8, 8, n - g - w), rng.uniform(-1.7, 1.0, n - g - w)], 1)
    pts = np.concatenate([ground, walls, clutter])
    return np.ascontiguousarray(pts[rng.permutation(n)])


def camera(f):
    """looks along +x from the sensor's position, z forward / x right / y down: q_world_camera = (0.5, -0.5, 0.5, -0.5)"""
    return capi.ColorCamera((C.c_double * 4)(0.5, -0.5, 0.5, -0.5), (C.c_double * 3)(float(f), 0.0, 0.0), 600.0, 600.0, COLS / 2.0, ROWS / 2.0, 0.005)


OUT = np.zeros(1 << 18, dtype=capi.COLOR_SELECTED_DTYPE)                 # the image has 13 000 cells at minimum_dis 10: ONE call gives totals and records


def select(ctx, cam, voxels, opts, want_records=True):
    """one srl_color_map_select call; returns (seconds, totals)"""
    tot = capi.ColorSelectTotals()
    v = None if voxels is None else np.ascontiguousarray(voxels, dtype=np.int32)
    t0 = time.perf_counter()
    rc = ctx.lib.srl_color_map_select(ctx.h, C.byref(cam), ROWS, COLS, capi._ptr(v), 0 if v is None else len(v), C.byref(opts),
                                      capi._ptr(OUT) if want_records else None, len(OUT) if want_records else 0, C.byref(tot))
    t1 = time.perf_counter()
    assert rc == capi.SRL_OK, rc
    return t1 - t0, tot


NAMES = ("candidates", "visited", "far", "near", "behind", "outside", "selected", "unknown")
for n in SIZES:
    ctx = srl.Context(0)
    ctx.color_map_create()
    t_list, rows = [], []
    in_list, use_all = capi.default_color_select_opts(), capi.default_color_select_opts(use_all_points=1)
    for f in range(FRAMES):
        visited = ctx.color_map_insert(frame(n, f), 1.0 + f, 0.0, want_outcome=False, want_stored=False)[2]
        if "l" not in LEGS:
            continue
        dt, tot = select(ctx, camera(f), visited, in_list)
        t_list.append(dt)
        rows.append(dict(pool_points=ctx.color_map_size()[0], listed_voxels=len(visited), selected=tot.selected, select_us=round(dt * 1e6)))
    t_all, t_tot = [], []
    for r in range(REPEATS if "a" in LEGS else 0):
        dt, tot_all = select(ctx, camera(FRAMES - 1), None, use_all)
        t_all.append(dt)
        t_tot.append(select(ctx, camera(FRAMES - 1), None, use_all, want_records=False)[0])
    res = dict(points=n, frames=FRAMES, image=[ROWS, COLS], legs=LEGS, registered=ctx.color_map_size()[2])
    if "l" in LEGS:
        res.update(list_call_us=round(float(np.median(t_list[1:])) * 1e6, 1), per_frame=rows, last_list_totals=dict(zip(NAMES, tot.as_tuple())))
    if "a" in LEGS:
        res.update(all_points_call_us=round(float(np.median(t_all[1:])) * 1e6, 1), all_points_totals_only_us=round(float(np.median(t_tot[1:])) * 1e6, 1),
                   all_points_us=[round(t * 1e6) for t in t_all], all_points_totals=dict(zip(NAMES, tot_all.as_tuple())))
    ctx.close()
    print(json.dumps(res), flush=True)
