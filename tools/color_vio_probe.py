"""Time one call of the camera ESIKF's measurement pass (srl_color_map_vio_rows: the per-point loops of imageProcessing::vioEsikf and
vioPhotometric) on the street scene of tools/color_map_probe.py: one frame of 256k points in the map, rendered three times from a
1280 x 1024 image so that its points have three views, the tracked list taken from an all-points selection at minimum_dis 10 and cut or
cycled to n entries (default 300 and 4096), seeded matches and velocities.  Host clock around the call (it ends in a synchronisation),
sums only and with rows and outcomes; median and 10th / 90th percentile over VIO_REPEATS calls after VIO_WARMUP.  For the kernel's own
time run under rocprofv3 --kernel-trace --stats in a run of its own (k_vio_rows).  Prints one JSON line per n and mode."""
import ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sr_livo_amd as srl
from sr_livo_amd import capi
SIZES = [int(a) for a in sys.argv[1:]] or [300, 4096]
REPEATS = int(os.environ.get("VIO_REPEATS", "20000"))      # 20 000 calls of 35 ... 115 us: a window of 0.7 ... 2.3 s per figure
WARMUP = int(os.environ.get("VIO_WARMUP", "200"))
ROWS, COLS, N_MAP = 1024, 1280, 256_000


def frame(n, f):
    """tools/color_map_probe.py's street scene: ground, two walls, clutter"""
    rng = np.random.default_rng(9400 + f)
    g, w = n // 2, n // 4
    ground = np.stack([rng.uniform(-40, 40, g) + f, rng.uniform(-40, 40, g), -1.7 + 0.02 * rng.standard_normal(g)], 1)
    walls = np.stack([rng.uniform(-40, 40, w) + f, rng.choice([-8.0, 8.0], w) + 0.02 * rng.standard_normal(w), rng.uniform(-1.7, 4.0, w)], 1)
    clutter = np.stack([rng.uniform(-40, 40, n - g - w) + f, rng.uniform(-8, 8, n - g - w), rng.uniform(-1.7, 1.0, n - g - w)], 1)
    pts = np.concatenate([ground, walls, clutter])
    return np.ascontiguousarray(pts[rng.permutation(n)])


ctx = srl.Context(0)
ctx.color_map_create()
visited = ctx.color_map_insert(frame(N_MAP, 0), 1.0, 0.0, want_outcome=False, want_stored=False)[2]
cam = capi.ColorCamera((C.c_double * 4)(0.5, -0.5, 0.5, -0.5), (C.c_double * 3)(0.0, 0.0, 0.0), 600.0, 600.0, COLS / 2.0, ROWS / 2.0, 0.005)
rng = np.random.default_rng(77)
ctx.color_image_upload(rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8))
for k in range(3):
    ctx.color_map_render(cam, visited, 2.0 + 0.1 * k)
rec, _ = ctx.color_map_select(cam, ROWS, COLS, None, capi.default_color_select_opts(use_all_points=1))
R = (C.c_double * 9)(0.0, 0.0, 1.0, -1.0, 0.0, 0.0, 0.0, -1.0, 0.0)
for n in SIZES:
    idx = np.arange(n) % len(rec)
    pts = np.zeros(n, capi.COLOR_VIO_POINT_DTYPE)
    pts["pool"] = rec["pool"][idx]
    pts["vel_u"], pts["vel_v"] = rng.uniform(-20, 20, n).astype(np.float32), rng.uniform(-20, 20, n).astype(np.float32)
    pts["match_u"], pts["match_v"] = rec["u"][idx] + rng.uniform(-1.5, 1.5, n), rec["v"][idx] + rng.uniform(-1.5, 1.5, n)
    rows, outcome = np.zeros((n, 24)), np.zeros(n, np.uint8)
    for mode, name in ((capi.SRL_VIO_REPROJECTION, "reprojection"), (capi.SRL_VIO_PHOTOMETRIC, "photometric")):
        args = capi.ColorVioArgs(cam, 0.0125, R, mode, 1, 1)
        res = dict(n=n, mode=name, selected=len(rec), repeats=REPEATS)
        windows = {}
        for label, r, o in (("sums_only", None, None), ("with_rows_and_outcomes", rows, outcome)):
            sums = capi.ColorVioSums()
            t = []
            for k in range(WARMUP + REPEATS):
                t0 = time.perf_counter()
                rc = ctx.lib.srl_color_map_vio_rows(ctx.h, C.byref(args), capi._ptr(pts), n, C.byref(sums), capi._ptr(r), capi._ptr(o))
                t.append(time.perf_counter() - t0)
                assert rc == capi.SRL_OK, rc
            us = np.array(t[WARMUP:]) * 1e6
            windows[label] = round(float(us.sum()) * 1e-6, 2)
            res[label + "_us"] = dict(median=round(float(np.median(us)), 1), p10=round(float(np.percentile(us, 10)), 1), p90=round(float(np.percentile(us, 90)), 1))
        res["window_s"] = windows
        res["counts"] = dict(zip(("used", "few_views", "behind", "outside", "unknown"), sums.counts()))
        print(json.dumps(res), flush=True)
ctx.close()
