"""Time the colour-map insertion (srl_color_map_insert: addPointToColorMap, lioOptimization.cpp:448-518) against what a caller had to do
without it, for frames of 24k / 64k / 256k points over a growing map.  Three legs, each on a context of its own, the same frames:
  a  srl_frame_commit alone (synchronous: num_added asked for) -- the baseline, no colour map
  b  the same commit + srl_color_map_insert on the world points the commit left in HBM, stored records and visited list returned
  c  the commit with world_out (n x 24 B across PCIe) + the reference's own addPointsToMap on one host core (oracle/_ref/libref_path.so,
     colour options 0.1 / 50 / 0.01 / 1).  That call ALSO does the reference's LiDAR insertion (addPointToMap): leg c is an upper bound of
     the colour loop's cost by that much.  Skipped where the library is absent.
Host clock around the calls (each ends in a synchronisation), median over the frames after the first; for kernel times run leg b under
rocprofv3 --kernel-trace --stats (COLOR_LEGS=b).  Prints one JSON line per frame size."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sr_livo_amd as srl
from sr_livo_amd import capi
from oracle import pyref as pr
SIZES = [int(a) for a in sys.argv[1:]] or [24_000, 64_000, 256_000]
FRAMES = int(os.environ.get("COLOR_FRAMES", "8"))
LEGS = os.environ.get("COLOR_LEGS", "abc")
KW = dict(voxel_size=1.0, cap=20, min_dist=0.1)
Q, T = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)


def frame(n, f):
    """a street scene seen from a sensor that moves 1 m per frame along x: ground, two walls, clutter"""
    rng = np.random.default_rng(9400 + f)
    g, w = n // 2, n // 4
    ground = np.stack([rng.uniform(-40, 40, g) + f, rng.uniform(-40, 40, g), -1.7 + 0.02 * rng.standard_normal(g)], 1)
    walls = np.stack([rng.uniform(-40, 40, w) + f, rng.choice([-8.0, 8.0], w) + 0.02 * rng.standard_normal(w), rng.uniform(-1.7, 4.0, w)], 1)
    clutter = np.stack([rng.uniform(-40, 40, n - g - w) + f, rng.uniform(-8, 8, n - g - w), rng.uniform(-1.7, 1.0, n - g - w)], 1)
    pts = np.concatenate([ground, walls, clutter])
    return np.ascontiguousarray(pts[rng.permutation(n)])


for n in SIZES:
    frames = [frame(n, f) for f in range(FRAMES)]
    res = dict(points=n, frames=FRAMES)
    if "a" in LEGS:
        ctx, t = srl.Context(0), []
        for f, raw in enumerate(frames):
            ctx.frame_upload(raw)
            t0 = time.perf_counter()
            ctx.frame_commit(Q, T, want_world=False, want_added=True, **KW)
            t.append(time.perf_counter() - t0)
        res["a_commit_us"] = round(float(np.median(t[1:])) * 1e6, 1)
        ctx.close()
    if "b" in LEGS:
        ctx, t, tc = srl.Context(0), [], []
        ctx.color_map_create()
        for f, raw in enumerate(frames):
            ctx.frame_upload(raw)
            t0 = time.perf_counter()
            ctx.frame_commit(Q, T, want_world=False, want_added=True, **KW)
            t1 = time.perf_counter()
            tot = ctx.color_map_insert(None, 1.0 + f, 0.0, n_frame=n, want_outcome=False)[3]
            t2 = time.perf_counter()
            t.append(t2 - t0); tc.append(t2 - t1)
        P, V, R, G = ctx.color_map_size()
        res.update(b_commit_colour_us=round(float(np.median(t[1:])) * 1e6, 1), b_colour_call_us=round(float(np.median(tc[1:])) * 1e6, 1),
                   b_colour_call_us_per_frame=[round(x * 1e6) for x in tc],      # (frames in which an array or a table grows stand out)
                   colour_points=P, colour_voxels=V, colour_registered=R, last_frame=dict(stored=tot.stored, created=tot.created,
                                                                                          registered=tot.registered, visited=tot.visited),
                   # records as laid out: 24 B per voxel, 24 B per stored point, 4 B per registered point; the two
                   # tables hold 16-B slots at a load <= 0.5 on top
                   record_bytes=24 * V + 24 * P + 4 * R, record_bytes_per_voxel=round((24 * V + 24 * P + 4 * R) / max(V, 1), 1),
                   slab_bytes_per_voxel_at_cap_50=16 + 50 * 12, rebuilds=ctx.color_map_rebuilds())
        ctx.close()
    if "c" in LEGS and pr.available():
        pr.set_params(num={"map_options/size_voxel_map": 0.1, "map_options/max_num_points_in_voxel": 50, "map_options/min_distance_points": 0.01,
                           "map_options/add_point_step": 1})
        node = pr.Node(True)
        ctx, t, th = srl.Context(0), [], []
        world = capi.PinnedArray((n, 3))
        for f, raw in enumerate(frames):
            ctx.frame_upload(raw)
            t0 = time.perf_counter()
            ctx.frame_commit(Q, T, want_world=True, want_added=True, world_out=world.array, **KW)
            t1 = time.perf_counter()
            node.add_points_to_map(world.array, **KW)
            t2 = time.perf_counter()
            t.append(t2 - t0); th.append(t2 - t1)
        res.update(c_commit_world_host_loop_us=round(float(np.median(t[1:])) * 1e6, 1), c_host_loop_us=round(float(np.median(th[1:])) * 1e6, 1))
        ctx.close(); world.close(); node.close(); pr.set_params()
    if "a_commit_us" in res:
        for k, leg in (("b_minus_a_us", "b_commit_colour_us"), ("c_minus_a_us", "c_commit_world_host_loop_us")):
            if leg in res:
                res[k] = round(res[leg] - res["a_commit_us"], 1)
    print(json.dumps(res), flush=True)
