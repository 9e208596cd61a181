"""Wall time per srl_pc2_decode (csrc/srl_pc2.hip), upload included, on two messages a user would feed -- an Ouster OS-128 sweep (128 rings x
1 024 columns = 131 072 points, the driver's 48-byte points, one t per column) and a VLP-16 sweep (16 x 1 800 = 28 800 points, 22-byte
points, per-point time) -- and, beside it, the reference's own handler on the same messages on one host core (tests/pc2_reader.py: the
reference's src/cloudProcessing.cpp compiled where it lies).  Also the yaw branch (the VLP-16 message with its times zeroed) and its host
atan2 pass alone.  Medians of --calls calls after --warmup calls; a decode is synchronous (it ends in a stream synchronise), so a host
clock around the call is the call.  The queue is emptied between calls, outside the clock.

    python tools/pc2_decode_time.py --device      [--out FILE]     needs a GPU
    python tools/pc2_decode_time.py --reference   [--out FILE]     needs the reference tree and oracle/_ref/libref_path.so; no GPU"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sr_livo_amd as srl  # noqa: E402
from sr_livo_amd import capi  # noqa: E402

STAMP = 1000.25


def ouster_message():
    rng = np.random.default_rng(1)
    rings, cols = 128, 1024
    p = np.zeros(rings * cols, dtype=capi.PC2_POINT_DTYPES[capi.LIDAR_OUST])
    col, ring = np.arange(rings * cols) // rings, np.arange(rings * cols) % rings
    az, el = 2 * np.pi * col / cols, np.deg2rad(-22.5 + 45.0 * ring / (rings - 1))
    r = 2.0 + 40.0 * rng.random(rings * cols)
    p["x"], p["y"], p["z"] = r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)
    p["time"] = (col + 1) * (100_000_000 // cols)                           # nanoseconds, one per column
    p["ring"] = ring
    return capi.pc2_message(p, capi.LIDAR_OUST, height=rings)               # (the driver's cloud is organised: 128 rows)


def vlp16_message(with_time=True):
    rng = np.random.default_rng(2)
    rings, cols = 16, 1800
    p = np.zeros(rings * cols, dtype=capi.PC2_POINT_DTYPES[capi.LIDAR_VELO])
    col, ring = np.arange(rings * cols) // rings, np.arange(rings * cols) % rings
    az, el = -2 * np.pi * col / cols, np.deg2rad(-15.0 + 2.0 * ring)
    r = 2.0 + 40.0 * rng.random(rings * cols)
    p["x"], p["y"], p["z"] = r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)
    if with_time:
        p["time"] = (col * 55.296e-6 + ring * 2.304e-6 + 1e-6).astype(np.float32)       # seconds: firing sequence and laser within it
    p["ring"] = ring
    return capi.pc2_message(p, capi.LIDAR_VELO)


PLAN = (("ouster_131072", ouster_message, dict(lidar_type=capi.LIDAR_OUST, n_scans=128, scan_rate=10, point_filter_num=3, time_unit=3, blind=0.5)),
        ("vlp16_28800", vlp16_message, dict(lidar_type=capi.LIDAR_VELO, n_scans=16, scan_rate=10, point_filter_num=3, time_unit=0, blind=0.5)),
        ("vlp16_28800_yaw", lambda: vlp16_message(False), dict(lidar_type=capi.LIDAR_VELO, n_scans=16, scan_rate=10, point_filter_num=3, time_unit=0, blind=0.5)))


def _median_ms(fn, between, calls, warmup):
    ts = []
    for k in range(warmup + calls):
        between()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= warmup:
            ts.append((t1 - t0) * 1e3)
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), calls=calls)


def device(calls, warmup):
    ctx = srl.Context(0)
    out = {}
    try:
        for name, make, kw in PLAN:
            data, lay = make()
            o = srl.pc2_opts(kw["lidar_type"], **{k: v for k, v in kw.items() if k != "lidar_type"})
            rep = {}
            ctx.pc2_decode(data, lay, STAMP, -1.0, o)
            out[name] = _median_ms(lambda: rep.update(ctx.pc2_decode(data, lay, STAMP, -1.0, o)), ctx.points_clear, calls, warmup)
            out[name].update(points=rep["points"], appended=rep["appended"], given=rep["given_offset_time"], bytes=int(data.nbytes))
            if name.endswith("_yaw"):
                out[name + "_host_atan2_alone"] = _median_ms(lambda: srl.pc2_yaw_angles(data, lay), lambda: None, calls, warmup)
    finally:
        ctx.close()
    return out


def reference(calls, warmup):
    import pc2_reader as pr
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = pr.build(tmp)
        for name, make, kw in PLAN:
            data, lay = make()
            box = {}

            def fresh():                                                     # a new cloudProcessing object: last_end_time = -1 again
                if "d" in box:
                    box["d"].close()
                box["d"] = pr.Decoder(lib, kw["lidar_type"], kw["n_scans"], kw["scan_rate"], kw["time_unit"], kw["blind"], kw["point_filter_num"])
            rep = {}
            out[name] = _median_ms(lambda: rep.update(rows=box["d"].feed(data, lay, STAMP)[0]), fresh, calls, warmup)
            out[name].update(appended=len(rep["rows"]), note="includes the test's own copy of the fields into the point structs (the stand-in for pcl::fromROSMsg) and of the queue out")
            box["d"].close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {}
    if a.device:
        res["device"] = device(a.calls, a.warmup)
    if a.reference:
        res["reference_one_host_core"] = reference(a.calls, a.warmup)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
