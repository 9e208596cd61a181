"""srl_image_prepare at the shipped 1280 x 1024 (T = 64, tiles of 20 x 16): 200 calls behind 20 warm-up calls.

  whole call     HIP events (torch.cuda.Event on the context's device) and the host clock around the synchronous call: staging copy,
                 upload, the three kernels, the hand-over to the colour map, the wait.
  kernels alone  not taken here: run this script under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/image_prep_time.py`
                 in a run of its own and read k_prep_pixel / k_prep_tiles / k_prep_apply from the statistics (tracing slows the host, so
                 the whole-call figures of such a run are not the ones to quote).
  beside it      the two uploads the call replaces, on the entry points that were there before it: srl_color_image_upload of the
                 equalised BGR image plus srl_flow_track_image of the equalised gray image with n = 0 points, i.e. the gray upload
                 with the pyramid the prepared path also builds (srl_flow_track_prepared with n = 0 is timed for that share).
Algorithmic bytes of one prepared image = raw read (3) + maps (6) + undist, gray, Y, CrCb written (7) and gray, Y, CrCb read again (4) +
the two results (4) = 24 bytes per pixel, beside the look-up tables (2 T T 256 bytes written, read from L2)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import sr_livo_amd as srl  # noqa: E402
from sr_livo_amd import capi  # noqa: E402

ROWS, COLS = 1024, 1280
WARMUP, CALLS = 20, 200
HBM_PEAK = 8.0e12                   # bytes/s (specification; about 6.3e12 is achievable with a plain copy)

rng = np.random.default_rng(7)
yy, xx = np.mgrid[0:ROWS, 0:COLS]
raw = np.stack([xx * 255 // (COLS - 1), yy * 255 // (ROWS - 1), (xx + yy) * 255 // (ROWS + COLS - 2)], axis=-1) + rng.integers(-12, 13, size=(ROWS, COLS, 3))
raw = np.ascontiguousarray(np.clip(raw, 0, 255).astype(np.uint8))
opts = capi.default_image_prep_opts(rows=ROWS, cols=COLS, fx=863.4, fy=863.4, cx=640.6, cy=518.3, dist=[-0.1080, 0.1050, -1.2872e-4, 5.7923e-5, -0.0222])
none = np.zeros((0, 2), np.float32)


def timed(name, fn):
    for _ in range(WARMUP):
        fn()
    ev, wall = [], []
    for _ in range(CALLS):
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
    print("%-58s HIP events median %8.1f us (p10 %8.1f, p90 %8.1f); host wall median %8.1f us; calls = %d" % (
        name, np.median(ev), np.percentile(ev, 10), np.percentile(ev, 90), np.median(wall), len(ev)))
    return float(np.median(ev)), float(np.median(wall))


# the prepared path: one context with a colour map (the hand-over is part of the call) and a tracker
a = srl.Context(0)
a.color_map_create()
prep = srl.ImagePrep(a, opts)
flow_a = srl.Flow(a)
info = prep.prepare(raw)
assert info.installed_color == 1 and (info.tiles, info.tile_w, info.tile_h) == (64, 20, 16)
gray_eq, bgr_eq = prep.download(capi.SRL_PREP_GRAY_EQ), prep.download(capi.SRL_PREP_BGR_EQ)
prepare = timed("srl_image_prepare %d x %d (whole call)" % (COLS, ROWS), lambda: prep.prepare(raw))
prepared_pyramid = timed("srl_flow_track_prepared, n = 0 (the pyramid alone)", lambda: flow_a.track_prepared(none))

# what it replaces: the two uploads of the images a caller prepared on the host, on a context of their own
b = srl.Context(0)
b.color_map_create()
flow_b = srl.Flow(b)


def upload_bgr():
    b.color_image_upload(bgr_eq)
    torch.cuda.synchronize()          # the call returns behind its staging copy: wait for the DMA as the prepared call does


bgr_up = timed("srl_color_image_upload + wait", upload_bgr)
gray_up = timed("srl_flow_track_image, n = 0 (gray upload + the pyramid)", lambda: flow_b.track_image(gray_eq, none))

npix = ROWS * COLS
bytes_alg = 24 * npix
print("algorithmic bytes per image: %d (24 per pixel); look-up tables %d" % (bytes_alg, 2 * info.tiles * info.tiles * 256))
print("whole call: %.1f us by events = %.1f GB/s of algorithmic bytes = %.2f %% of the HBM peak (%.1f TB/s); the call is bound by the upload and "
      "the launches, not by HBM" % (prepare[0], bytes_alg / prepare[0] * 1e-3, 100 * bytes_alg / (prepare[0] * 1e-6) / HBM_PEAK, HBM_PEAK * 1e-12))
old = bgr_up[0] + gray_up[0]
new = prepare[0] + prepared_pyramid[0]
print("the two uploads it replaces (with the pyramid): %.1f us; the prepared path (prepare + pyramid): %.1f us -> the prepared path is %s by %.1f us" % (
    old, new, "BELOW" if new < old else "ABOVE", abs(old - new)))
print("srl_image_prepare alone against the two uploads with the pyramid: %.1f us vs %.1f us" % (prepare[0], old))
a.close()
b.close()
