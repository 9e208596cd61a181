"""Time the rendering of an image into the colour map (srl_color_image_upload + srl_color_map_render: rgbMapTracker::
renderPointsInRecentVoxel, rgbMapTracker.cpp:176-237) on the street scene of tools/color_map_probe.py: frames of 24k / 64k / 256k points
inserted into a growing map, and after every insertion a 1280 x 1024 image rendered into the voxels that insertion visited, from a
camera that rides with the sensor.  Host clock around the two calls (the render ends in a synchronisation), median over the frames
after the first; per frame the pool size the pass sweeps and the points of the listed voxels, and the bytes the sweep moves at least
(24 B pool record + 4 B mark word per pool point; 40 B read + 40 B written per point that changes) -- how far k_render_points is from a
streaming read, and what share of the pool a render touches (a per-voxel chain through the pool would make the pass proportional to
that share).  For kernel times run under rocprofv3 --kernel-trace --stats.  There is no CPU baseline from the reference itself: its loop
cannot see a pixel under the stand-in cv::Mat of oracle/ref_shim.  Prints one JSON line per frame size."""
import ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sr_livo_amd as srl
from sr_livo_amd import capi
SIZES = [int(a) for a in sys.argv[1:]] or [24_000, 64_000, 256_000]
FRAMES = int(os.environ.get("COLOR_FRAMES", "8"))
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


rng = np.random.default_rng(1)
images = [rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8) for _ in range(2)]
for n in SIZES:
    ctx = srl.Context(0)
    ctx.color_map_create()
    t_up, t_render, rows = [], [], []
    for f in range(FRAMES):
        visited = ctx.color_map_insert(frame(n, f), 1.0 + f, 0.0, want_outcome=False, want_stored=False)[2]
        t0 = time.perf_counter()
        ctx.color_image_upload(images[f % 2])
        t1 = time.perf_counter()
        tot = ctx.color_map_render(camera(f), visited, 100.0 + 0.1 * f)
        t2 = time.perf_counter()
        t_up.append(t1 - t0); t_render.append(t2 - t1)
        pool = ctx.color_map_size()[0]
        changed = tot.first + tot.updated
        rows.append(dict(pool_points=pool, listed_voxels=len(visited), listed_points=tot.listed, changed=changed, render_us=round((t2 - t1) * 1e6),
                         sweep_bytes_min=28 * pool + 80 * changed))
    res = dict(points=n, frames=FRAMES, image=[ROWS, COLS], upload_us=round(float(np.median(t_up[1:])) * 1e6, 1),
               render_call_us=round(float(np.median(t_render[1:])) * 1e6, 1), per_frame=rows,
               state_bytes_per_point=40, last_totals=dict(zip(("listed", "behind", "outside", "gated", "first", "updated", "unknown"), tot.as_tuple())))
    ctx.close()
    print(json.dumps(res), flush=True)
