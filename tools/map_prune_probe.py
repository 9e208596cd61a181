"""Time one srl_map_remove_far (removePointsFarFromLocation) on the 1M-point headline map and the 10M-point C4 map, removing ~0 %, ~1 %
and ~50 % of the voxels.  Host clock around the call (it ends in a synchronisation), median of REPS prunes, each on a freshly uploaded copy
of the built map; for kernel times run it under rocprofv3 --kernel-trace --stats.  Prints one JSON line per case."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sr_livo_amd as srl
from sr_livo_amd import synth
SIZES = [int(a) for a in sys.argv[1:]] or [1_000_000, 10_000_000]
REPS = int(os.environ.get("PRUNE_REPS", "9"))
SLAB = 256
for N in SIZES:
    pts, L = synth.map_candidates(7, N)
    ctx = srl.Context(0)
    ctx.map_insert(pts)
    keys, counts, xyz = ctx.map_download()
    V = len(counts)
    p0 = xyz[:, 0].astype(np.float64)
    loc = p0.mean(0) + np.array([0.1, -0.2, 0.05]) * L
    d = np.sqrt(((p0 - loc) ** 2).sum(1))
    for frac in (0.0, 0.01, 0.5):
        dist = float(d.max()) * 1.01 if frac == 0.0 else float(np.quantile(d, 1.0 - frac))
        times, removed = [], None
        for _ in range(REPS):
            ctx.map_upload(keys, counts, xyz)
            t0 = time.perf_counter()
            removed = ctx.map_remove_far(loc, dist)
            times.append(time.perf_counter() - t0)
        V_new = V - removed[0]
        # bytes the device moves (removed > 0): mark (one 64-B line per slab + the count line of erased ones, flags), scan, compaction
        # (survivors read + written to scratch, copied back), zeroed tail, table fill + rebuild (key / count lines of the survivors, 16-B slots)
        table_slots = 1 << int(np.ceil(np.log2(max(2048, 4 * (V + V // 2 + 4096)))))
        b_mark = V * 64 + removed[0] * 64 + V * 4
        b_compact = 4 * V_new * SLAB if removed[0] else 0
        b_tail = removed[0] * SLAB
        b_table = (table_slots * 16 + V_new * (64 + 16)) if removed[0] else 0
        print(json.dumps(dict(points=N, voxels=V, fraction=frac, voxels_removed=removed[0], points_removed=removed[1],
                              wall_us_median=round(float(np.median(times)) * 1e6, 1), wall_us_min=round(float(np.min(times)) * 1e6, 1),
                              bytes_mark=b_mark, bytes_compaction=b_compact, bytes_tail=b_tail, bytes_table=b_table, table_slots=table_slots)),
              flush=True)
    ctx.close()
