"""Time one call of the optical flow (srl_flow_track_image: LKOpticalFlowKernel::trackImage on the device) at the size the camera stage
runs it: a 640 x 512 gray image and 300 points (maximum_tracked_points), alternating between two views of a seeded texture one pixel
and a bit apart so that every call tracks.  Host clock around the call, which ends in a synchronisation; no device events.  Two figures,
each over FLOW_REPEATS calls after FLOW_WARMUP: the pyramid alone (n = 0: upload, four levels, four derivatives, swap) and the full
call (n = 300).  Median and 10th / 90th percentile, and the length of each timed window.  For the kernels' own times run under
rocprofv3 --kernel-trace --stats in a run of its own (k_flow_level0, k_flow_down, k_flow_scharr, k_flow_track).  One JSON line.

    python tools/flow_time.py                 on the GPU
    python tools/flow_time.py --reference     for scale, on one CPU core where the reference tree is present: the reference's own
                                              trackImage compiled against tests/stub_opencv_lk (tests/flow_reader.py) -- a figure of
                                              the STAND-IN OpenCV's pyrDown and copyMakeBorder and of a serial parallel_for_, not of OpenCV"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flow_checker as fc  # noqa: E402

ROWS, COLS, N = 512, 640, 300
REPEATS = int(os.environ.get("FLOW_REPEATS", "20000"))      # 20 000 calls of 55 ... 145 us: windows of 1.1 and 2.9 s
WARMUP = int(os.environ.get("FLOW_WARMUP", "200"))


def inputs():
    tex = fc.texture(640, ROWS, COLS)
    imgs = [fc.crop(tex, ROWS, COLS, 0, 0), fc.crop(tex, ROWS, COLS, 1, 1, sub=(1, 2))]
    return imgs, fc.grid_points(300, ROWS, COLS, N)


def stats(seconds):
    us = np.array(seconds) * 1e6
    return dict(median_us=round(float(np.median(us)), 1), p10_us=round(float(np.percentile(us, 10)), 1), p90_us=round(float(np.percentile(us, 90)), 1),
                window_s=round(float(us.sum()) * 1e-6, 2), calls=len(us))


def timed(call, imgs, pts, repeats, warmup):
    t, tracked = [], 0
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        tracked = call(imgs[k & 1], pts)
        t.append(time.perf_counter() - t0)
    return stats(t[warmup:]), tracked


def main():
    imgs, pts = inputs()
    none = pts[:0]
    if "--reference" in sys.argv[1:]:
        import tempfile

        import flow_reader as fr
        if hasattr(os, "sched_setaffinity"):
            os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
        with tempfile.TemporaryDirectory() as tmp:
            tr = fr.Tracker(fr.build(os.path.join(tmp, "reader")))
            g = [np.ascontiguousarray(i) for i in imgs]
            nxt, st = np.zeros((N, 2), np.float32), np.zeros(N, np.uint8)

            def call(im, p):
                return tr.lib.frr_track(tr.h, fr._vp(im), ROWS, COLS, fr._vp(p), len(p), fr._vp(nxt), fr._vp(st))
            reps, warm = min(REPEATS, 300), 20
            pyramid, _ = timed(call, g, none, reps, warm)
            full, tracked = timed(call, g, pts, reps, warm)
            tr.close()
        print(json.dumps(dict(what="reference trackImage on one CPU core, stand-in OpenCV", rows=ROWS, cols=COLS, n=N, tracked=tracked, pyramid_only=pyramid, full_call=full)))
        return
    import sr_livo_amd as srl
    ctx = srl.Context(0)                  # raises without a GPU: there is nothing to time on a CPU
    flow = srl.Flow(ctx)
    C, capi = srl.capi.C, srl.capi
    nxt, st, nt = np.zeros((N, 2), np.float32), np.zeros(N, np.uint8), C.c_int()

    def call(im, p):
        n = len(p)
        rc = ctx.lib.srl_flow_track_image(ctx.h, capi._ptr(im), ROWS, COLS, COLS, capi._ptr(p) if n else None, n, capi._ptr(nxt) if n else None,
                                          capi._ptr(st) if n else None, C.byref(nt))
        assert rc == 0, rc
        return nt.value
    call(imgs[1], pts)
    pyramid, _ = timed(call, imgs, none, REPEATS, WARMUP)
    full, tracked = timed(call, imgs, pts, REPEATS, WARMUP)
    # what was timed is what the checker computes
    want = fc.Tracker()
    want.track_image(imgs[(WARMUP + REPEATS - 2) & 1], pts)
    w_next, w_status, _ = want.track_image(imgs[(WARMUP + REPEATS - 1) & 1], pts)
    same = bool(nxt.view(np.uint32).tobytes() == w_next.view(np.uint32).tobytes() and st.tobytes() == w_status.tobytes())
    print(json.dumps(dict(what="srl_flow_track_image", rows=ROWS, cols=COLS, n=N, levels=flow.levels() + 1, tracked=tracked, equals_checker=same,
                          pyramid_only=pyramid, full_call=full)))
    flow.close()
    ctx.close()
    assert same


if __name__ == "__main__":
    main()
