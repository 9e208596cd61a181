"""Time one srl_color_map_export_cloud (the coloured cloud of pubColorPoints / threadPubColorPoints / saveColorPoints) against the path it
replaces -- srl_color_registered_rgb + srl_color_registered_download + a NumPy filter and pack on the host -- on colour maps of about
25 k, 250 k and 1.2 M registered points, at pub_point_minimum_views 1 and 3.  Both paths run in the same process, alternated, each into
buffers allocated once; host clock around the calls (both end in a synchronisation), median of REPS after two warm-ups; for kernel times
run it under rocprofv3 --kernel-trace --stats.  The maps are 0.05-m lattices (every point registers) rendered from four poses, so that
N_rgb runs from 0 to 4.  Prints one JSON line per case, with the bytes each path moves over PCIe."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sr_livo_amd as srl  # noqa: E402
from sr_livo_amd import capi  # noqa: E402

SHAPES = {25_000: (29, 29, 30), 250_000: (63, 63, 63), 1_200_000: (106, 106, 107)}
SIZES = [int(a) for a in sys.argv[1:]] or sorted(SHAPES)
REPS = int(os.environ.get("CLOUD_REPS", "9"))
WARMUPS = 2
ROWS, COLS = 480, 640


def lattice(nx, ny, nz, x0):
    g = np.mgrid[0:nx, 0:ny, 0:nz].reshape(3, -1).T.astype(np.float64)
    return g * 0.05 + np.array([x0 + 0.025, 0.025 - ny * 0.025, 0.025 - nz * 0.025])


def camera(yaw, pitch, t):
    """z forward, x right, y down; looking along world +x turned by yaw about z and pitched down"""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    fwd = np.array([cy * cp, sy * cp, -sp]); right = np.array([sy, -cy, 0.0]); down = np.cross(fwd, right)
    m = np.stack([right, down, fwd], 1)
    w = np.sqrt(1.0 + m[0, 0] + m[1, 1] + m[2, 2]) / 2.0
    q = (w, (m[2, 1] - m[1, 2]) / (4 * w), (m[0, 2] - m[2, 0]) / (4 * w), (m[1, 0] - m[0, 1]) / (4 * w))
    f = 0.36 * COLS
    return capi.ColorCamera((C.c_double * 4)(*q), (C.c_double * 3)(*t), f, f, COLS / 2.0, ROWS / 2.0, 0.005)


for N in SIZES:
    nx, ny, nz = SHAPES[N]
    ctx = srl.Context(0)
    ctx.color_map_create()
    visited = []
    step = max(1, 1_000_000 // (ny * nz))
    for x in range(0, nx, step):
        visited.append(ctx.color_map_insert(lattice(min(step, nx - x), ny, nz, x * 0.05), 1.0, 0.0, want_outcome=False, want_stored=False)[2])
    voxels = np.concatenate(visited)
    size = ctx.color_map_size()[2]
    rng = np.random.default_rng(5)
    ctx.color_image_upload(rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8))
    span = nx * 0.05
    for k, (yaw, pitch, t) in enumerate(((0.0, 0.3, (-0.6 * span, 0.0, 0.3 * span)), (0.3, 0.3, (-0.3 * span, -0.5 * span, 0.3 * span)),
                                         (-0.3, 0.3, (-0.3 * span, 0.5 * span, 0.3 * span)), (0.0, 0.6, (0.1 * span, 0.0, 0.6 * span)))):
        ctx.color_map_render(camera(yaw, pitch, t), voxels, 10.0 + 0.1 * k)
    lib, h = ctx.lib, ctx.h
    out = np.zeros(size, capi.COLOR_CLOUD_DTYPE)
    stored = np.zeros(size, capi.COLOR_STORED_DTYPE)
    rgb = np.zeros((size, 3), np.int16)
    n_rgb = np.zeros(size, np.int16)
    packed = np.zeros(size, capi.COLOR_CLOUD_DTYPE)
    for mv in (1, 3):
        o = capi.default_color_cloud_opts(minimum_views=mv)
        tot = capi.ColorCloudTotals()
        t_new, t_old, t_old_device, kept = [], [], [], 0
        for _ in range(WARMUPS + REPS):
            t0 = time.perf_counter()
            rc = lib.srl_color_map_export_cloud(h, 0, -1, C.byref(o), capi._ptr(out), None, size, C.byref(tot))
            t1 = time.perf_counter()
            assert rc == capi.SRL_OK
            t_new.append(t1 - t0)
            t0 = time.perf_counter()
            rc1 = lib.srl_color_registered_rgb(h, 0, size, capi._ptr(rgb), capi._ptr(n_rgb), None, None, None)
            rc2 = lib.srl_color_registered_download(h, 0, size, capi._ptr(stored))
            t1 = time.perf_counter()
            keep = np.flatnonzero(n_rgb >= mv)
            kept = len(keep)
            p = packed[:kept]
            p["x"], p["y"], p["z"] = stored["x"][keep], stored["y"][keep], stored["z"][keep]
            p["b"], p["g"], p["r"], p["a"] = rgb[keep, 0], rgb[keep, 1], rgb[keep, 2], 255
            t2 = time.perf_counter()
            assert rc1 == capi.SRL_OK and rc2 == capi.SRL_OK
            t_old.append(t2 - t0)
            t_old_device.append(t1 - t0)
        assert kept == tot.published and packed[:kept].tobytes() == out[:kept].tobytes()
        print(json.dumps(dict(registered=size, minimum_views=mv, published=int(tot.published),
                              export_us_median=round(float(np.median(t_new[WARMUPS:])) * 1e6, 1), export_us_min=round(float(np.min(t_new[WARMUPS:])) * 1e6, 1),
                              replaced_us_median=round(float(np.median(t_old[WARMUPS:])) * 1e6, 1), replaced_us_min=round(float(np.min(t_old[WARMUPS:])) * 1e6, 1),
                              replaced_two_calls_us_median=round(float(np.median(t_old_device[WARMUPS:])) * 1e6, 1),
                              export_pcie_bytes=int(tot.published) * 16 + 64, replaced_pcie_bytes=size * (40 + 24))), flush=True)
    ctx.close()
