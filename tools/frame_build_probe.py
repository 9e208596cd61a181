"""Time the sub-sample step of buildFrame (lioOptimization.cpp:838-846) both ways, through the C-ABI calls the host mirror makes:

  host   srl_frame_undistort with both n-point downloads, subSampleFrame's grouping over the n points on the host (srl_grid_sampling:
         the same std::tr1::unordered_map walk), srl_frame_take of the kept list after the second shuffle
  device srl_frame_undistort with no downloads, srl_frame_subsample, srl_frame_take_subsampled with the m-point index, raw and imu
         downloads

Synthetic Livox-like sweeps of a box room 4-30 m away, 0.1 m voxels.  Host clock around each form (every call ends in a synchronisation),
median of REPS; the two permutations are drawn before the clock starts (the shuffles are the caller's in both forms).  SRL_FRAME_TIMING
is set, so srl_frame_subsample also prints its own stages on stderr (enqueue / wait for the device chain / host replay).
Prints one JSON line per size."""
import json, os, sys, time
os.environ.setdefault("SRL_FRAME_TIMING", "1")
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sr_livo_amd as srl
from sr_livo_amd import capi

SIZES = [int(a) for a in sys.argv[1:]] or [24_000, 65_536, 262_144]
REPS = int(os.environ.get("FRAME_BUILD_REPS", "9"))
VOXEL = 0.1


def room(rng, n):
    d = rng.normal(size=(n, 3)); d[:, 2] *= 0.3
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * rng.uniform(4.0, 30.0, (n, 1))


st = np.zeros((2, 17)); st[:, 0] = [200.0, 200.1]; st[:, 10] = 1.0
ctx = srl.Context(0)
for n in SIZES:
    rng = np.random.default_rng(n)
    raw = room(rng, n)
    rel = np.sort(rng.uniform(0.0, 100.0, n))
    order = rng.permutation(n).astype(np.int32)
    m = len(srl.grid_sampling(raw[order], VOXEL))
    perm = rng.permutation(m).astype(np.int32)
    th, td, tg = [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        imu, corr = ctx.frame_undistort(raw, rel, st, 200.0, capi.MC_CONSTANT_VELOCITY)
        t1 = time.perf_counter()
        kept = order[srl.grid_sampling(raw[order], VOXEL)]
        t2 = time.perf_counter()
        ctx.frame_take(kept[perm])
        t3 = time.perf_counter()
        th.append(t3 - t0); tg.append(t2 - t1)
        t0 = time.perf_counter()
        ctx.frame_undistort(raw, rel, st, 200.0, capi.MC_CONSTANT_VELOCITY, want_outputs=False)
        ctx.frame_subsample(order, VOXEL)
        got = ctx.frame_take_subsampled(perm, want_index=True, want_raw=True, want_imu=True)
        td.append(time.perf_counter() - t0)
        assert np.array_equal(got["index"], kept[perm])
    us = lambda v: round(float(np.median(v)) * 1e6, 1)
    print(json.dumps(dict(points=n, voxels=m, host_form_us=us(th), host_grouping_us=us(tg), device_form_us=us(td),
                          order_used=ctx.frame_order_used())), flush=True)
ctx.close()
