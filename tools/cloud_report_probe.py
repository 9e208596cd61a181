"""Time what the insertion report costs: srl_frame_commit (synchronous, num_added given) against srl_frame_commit_report with outcome and
cloud downloaded, and against the plain commit with the 24 B / point world_out download (what a node pays today to rebuild cloud_world on
the host), on frames of the given sizes committed into the same ~200k-point map.  Host clock around the call (every form ends in a
synchronisation), median of REPS calls after two warm-ups, the forms alternated inside every repetition, each call on a freshly uploaded
copy of the map and a freshly uploaded frame; for kernel times run it under rocprofv3 --kernel-trace --stats.  --plain-only times the
plain forms alone (a build without the report calls).  Prints one JSON line per size."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sr_livo_amd as srl
from sr_livo_amd import synth
PLAIN_ONLY = "--plain-only" in sys.argv[1:]
SIZES = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [24_000, 65_536, 262_144]
REPS = int(os.environ.get("CLOUD_REPS", "9"))
TAG = os.environ.get("CLOUD_TAG", "")
KW = dict(voxel_size=0.5, cap=20, min_dist=0.1, min_num_points=0)
pts, L = synth.map_candidates(7, 200_000)
ctx = srl.Context(0)
ctx.map_insert(pts, **KW)
base = ctx.map_download()
for n in SIZES:
    sw = synth.make_sweep(11, n, L)
    raw = np.ascontiguousarray(sw["raw"])
    q, t = sw["q_pred"], sw["t_pred"]
    world = srl.PinnedArray((n, 3))                          # page-locked: the download's fastest path
    wbuf = world.array
    forms = {"plain": lambda: ctx.frame_commit(q, t, want_world=False, want_added=True, **KW),
             "plain_world_out": lambda: ctx.frame_commit(q, t, want_world=True, want_added=True, world_out=wbuf, **KW)}
    if not PLAIN_ONLY:
        # the C call on caller-owned arrays, as the other two forms (Context.frame_commit_report allocates its outputs per call)
        import ctypes as C
        from sr_livo_amd.capi import _dptr, _f64, _ptr
        outcome, cloud = np.zeros(n, np.uint8), np.zeros((n, 4), np.float32)
        m, added = C.c_int(), C.c_int()
        qa, ta, Ra, tia = _f64(q), _f64(t), _f64(np.eye(3)).ravel(), _f64(np.zeros(3))

        def report():
            rc = ctx.lib.srl_frame_commit_report(ctx.h, _dptr(qa), _dptr(ta), _dptr(Ra), _dptr(tia), KW["voxel_size"], 20, KW["min_dist"], 0, None,
                                                 _ptr(outcome), _ptr(cloud), C.byref(m), C.byref(added))
            assert rc == 0, rc
            return outcome, cloud[: m.value], added.value
        forms["report"] = report
    times = {k: [] for k in forms}
    info = {}
    for rep in range(REPS + 2):
        for name, call in forms.items():
            ctx.map_upload(*base)
            ctx.frame_upload(raw)
            ctx.map_size()                                   # everything above has landed
            t0 = time.perf_counter()
            out = call()
            dt = time.perf_counter() - t0
            if rep >= 2:
                times[name].append(dt)
            if name == "report":
                info = dict(num_cloud=len(out[1]), num_added=out[2], cloud_bytes=16 * len(out[1]), outcome_bytes=n)
            elif name == "plain":
                info.setdefault("num_added_plain", out[1])
    row = dict(tag=TAG, points=n, world_out_bytes=24 * n, **info)
    for name, ts in times.items():
        row[name + "_us_median"] = round(float(np.median(ts)) * 1e6, 1)
        row[name + "_us_min"] = round(float(np.min(ts)) * 1e6, 1)
        row[name + "_us_max"] = round(float(np.max(ts)) * 1e6, 1)
    print(json.dumps(row), flush=True)
    world.close()
ctx.close()
