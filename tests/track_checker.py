"""Sequential restatement of opticalFlowTracker::updateAndAppendTrackPoints (src/opticalFlowTracker.cpp:13-102) on top of
tests/select_checker.py's map with pool positions and tests/render_checker.py's camera: the first loop over the tracked points (:22-61)
and the second over points_rgb_vec_for_projection (:63-99), one element after the other, Python floats (IEEE doubles) with an explicit
np.float32 where the reference holds a float, the occupancy mask (Hash_map_2d<int, float>, whose stored depth is never read) a Python
dict.  What the device call (srl_color_map_track_update) and the recorded golden file are compared with;
tests/test_track_checker_reference.py pins the pieces to the reference's own translation units.

The tracked set is a list in the caller's order where the reference holds a std::map keyed by pointer value: nothing the first loop
decides depends on the order (the occupied cells are a union), and the output keeps the input order.  Two stated departures, as the
device call makes them: a tracked point behind the camera -- whose error the reference forms from the previous element's pixel -- is
dropped with its flag 0, and a pool position the map does not hold, or one that occurred earlier in the list, is dropped (a std::map
holds neither).

The loop goes on behind its `break` with the adds switched off, only to name what it left: a candidate that would still have taken a
free cell is `cut`, every other one `not reached`.

Also the scenes of the tests: a fixed sequence of calls on select_checker's scene (CASES), built from the checker's own results.
"""
import functools
import math

import numpy as np

import select_checker as sk

F32 = np.float32
TRACK_POINT_DTYPE = np.dtype([("pool", "<i4"), ("u", "<f4"), ("v", "<f4"), ("flagged", "<i4")])
TOTALS = ("tracked_in", "kept", "flagged", "dropped", "behind", "unknown", "duplicate",
          "candidates", "already_tracked", "cand_unknown", "refused", "occupied", "added", "cut")
KEPT, KEPT_FLAGGED, DROPPED, BEHIND, UNKNOWN, DUPLICATE = range(6)
ADDED, ALREADY_TRACKED, CAND_UNKNOWN, REFUSED, OCCUPIED, CUT, NOT_REACHED = range(7)
# what the preconditions of the tests count, per call
CENSUS = ("kept_flagged", "second_strike", "beyond_twice", "kept_outside", "behind", "occupied_by_tracked", "occupied_by_candidate",
          "already_tracked", "readded")
MINI_DISTANCE, MAXIMUM_TRACKED_POINTS = 10.0, 300      # imageProcessing.cpp:161, opticalFlowTracker.cpp:10


@functools.lru_cache(maxsize=None)
def pool_positions(batches=3):
    """the stored FP32 position of every pool position of select_checker's scene, (P, 3) float32"""
    smap, _ = sk.scene_map(batches)
    out = np.zeros((len(smap.pool_of), 3), F32)
    for (key, slot), pool in smap.pool_of.items():
        out[pool] = smap.chk.voxels[key].points[slot]
    return out


def track_update_sequential(positions, camera, rows, cols, tracked, candidates, mini_distance=MINI_DISTANCE, maximum=MAXIMUM_TRACKED_POINTS):
    """the two loops.  Returns (records, tracked outcome, candidate outcome, totals dict, census dict)."""
    tracked = np.asarray(tracked, dtype=TRACK_POINT_DTYPE).reshape(-1)
    candidates = np.asarray(candidates, dtype=np.int64).reshape(-1)
    P = len(positions)
    tot = dict.fromkeys(TOTALS, 0)
    census = dict.fromkeys(CENSUS, 0)
    tot["tracked_in"], tot["candidates"] = len(tracked), len(candidates)
    t_out = np.zeros(len(tracked), np.uint8)
    c_out = np.zeros(len(candidates), np.uint8)
    max_err = 2.0 * cols / 320.0                                            # :18

    def position(pool):
        p32 = positions[pool]
        return (float(p32[0]), float(p32[1]), float(p32[2]))               # getPosition(): position.cast<double>()

    def cell_of(u_d, v_d):
        return (sk.cell_coordinate(u_d, mini_distance), sk.cell_coordinate(v_d, mini_distance))      # :29-30, :79-80

    # ---- the first loop (:22-61)
    last_pose = {}                          # map_rgb_points_in_last_image_pose: pool -> [u, v, is_out_lier_count], in the caller's order
    occupied = {}                           # map_2d_points_occupied: cell -> "T" or the candidate that inserted it
    met, dropped_here = set(), set()
    for i, t in enumerate(tracked):
        pool = int(t["pool"])
        if not 0 <= pool < P:
            t_out[i] = UNKNOWN
            continue
        if pool in met:
            t_out[i] = DUPLICATE
            continue
        met.add(pool)
        outcome, u_d, v_d = camera.project(position(pool), rows, cols)
        if outcome == 1:                    # behind the camera: u_d, v_d unwritten in the reference -- the stated departure
            t_out[i] = BEHIND
            census["behind"] += 1
            continue
        du, dv = u_d - float(t["u"]), v_d - float(t["v"])
        error = math.sqrt(du * du + dv * dv)                                # Eigen::Vector2d(...).norm()
        count = int(t["flagged"])
        if error > max_err:
            count += 1                                                      # is_out_lier_count++
            if count > 1 or error > max_err * 2:
                t_out[i] = DROPPED                                          # count = 0; erase
                dropped_here.add(pool)
                census["beyond_twice" if error > max_err * 2 else "second_strike"] += 1
                continue
            t_out[i] = KEPT_FLAGGED
            census["kept_flagged"] += 1
        else:
            count = 0
            t_out[i] = KEPT
        last_pose[pool] = (t["u"], t["v"], count)
        if outcome == 0:
            cell = cell_of(u_d, v_d)
            if cell not in occupied:
                occupied[cell] = "T"
        else:
            census["kept_outside"] += 1

    # ---- the second loop (:63-99); behind its break the adds are off
    records = [(pool, u, v, count) for pool, (u, v, count) in last_pose.items()]
    size = len(last_pose)
    in_map = set(last_pose)
    seen = set()
    broke = False
    for i, pool in enumerate(int(c) for c in candidates):
        if not 0 <= pool < P:
            c_out[i] = NOT_REACHED if broke else CAND_UNKNOWN
            continue
        if pool in in_map or pool in seen:  # found in the map (:69-73); a repeat is found there or refused as its first occurrence was
            c_out[i] = NOT_REACHED if broke else ALREADY_TRACKED
            census["already_tracked"] += 0 if broke else 1
            continue
        seen.add(pool)
        outcome, u_d, v_d = camera.project(position(pool), rows, cols)
        takes = False
        holder = None
        if outcome == 0:
            cell = cell_of(u_d, v_d)
            if cell not in occupied:
                occupied[cell] = i
                takes = True
            else:
                holder = occupied[cell]
        if broke:
            c_out[i] = CUT if takes else NOT_REACHED
            continue
        if takes:
            in_map.add(pool)
            records.append((pool, F32(u_d), F32(v_d), 0))                   # cv::Point2f(u_d, v_d)
            size += 1
            c_out[i] = ADDED
            census["readded"] += 1 if pool in dropped_here else 0
        elif outcome == 0:
            c_out[i] = OCCUPIED
            census["occupied_by_tracked" if holder == "T" else "occupied_by_candidate"] += 1
        else:
            c_out[i] = REFUSED
        if size >= maximum:                                                 # :94
            broke = True

    rec = np.zeros(len(records), TRACK_POINT_DTYPE)
    for k, r in enumerate(records):
        rec[k] = r
    for name, value in (("kept", KEPT), ("flagged", KEPT_FLAGGED), ("dropped", DROPPED), ("behind", BEHIND), ("unknown", UNKNOWN),
                        ("duplicate", DUPLICATE)):
        tot[name] = int((t_out == value).sum())
    tot["kept"] += tot["flagged"]                                           # kept = |T|, `flagged` of them
    for name, value in (("already_tracked", ALREADY_TRACKED), ("cand_unknown", CAND_UNKNOWN), ("refused", REFUSED), ("occupied", OCCUPIED),
                        ("added", ADDED), ("cut", CUT)):
        tot[name] = int((c_out == value).sum())
    return rec, t_out, c_out, tot, census


def totals_tuple(tot):
    return tuple(int(tot[name]) for name in TOTALS)


# ------------------------------------------------------------------------------------------------ the scenes
def perturbed(positions, camera, rows, cols, records, seed):
    """the tracked points as an optical flow would hand them back under `camera`: the new projection plus an offset that is small for
    most, between one and two allowed errors for some and beyond two for a few; flags as the records carry them"""
    rng = np.random.default_rng(seed)
    max_err = 2.0 * cols / 320.0
    out = np.array(records, dtype=TRACK_POINT_DTYPE)
    for k, t in enumerate(out):
        p32 = positions[int(t["pool"])]
        _, u_d, v_d = camera.project((float(p32[0]), float(p32[1]), float(p32[2])), rows, cols)
        kind, radius, angle = rng.random(), rng.random(), rng.random() * 2 * math.pi
        radius = radius * 0.8 * max_err if kind < 0.55 else ((1.1 + 0.8 * radius) * max_err if kind < 0.85 else (2.2 + 3 * radius) * max_err)
        out[k]["u"], out[k]["v"] = F32(u_d + radius * math.cos(angle)), F32(v_d + radius * math.sin(angle))
    return out


@functools.lru_cache(maxsize=None)
def registered_pools():
    """pool position of rgb_points_vec[i]"""
    smap, _ = sk.scene_map()
    return np.array([smap.pool_of[(r[3], r[4])] for r in smap.chk.registered], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    """the fixed sequence: [(name, render whose pose and image size are used, margin, tracked, candidates, mini_distance, maximum)].  Later
    cases are built from the checker's results for earlier ones."""
    pos = pool_positions()
    sel_a, sel_b = (r[0]["pool"].astype(np.int32) for r in sk.all_points_results(3))      # all-points selections at minimum_dis 10
    reg = registered_pools()
    none = np.zeros(0, TRACK_POINT_DTYPE)
    out = []

    def run(name, k, margin, tracked, cand, md=MINI_DISTANCE, maximum=MAXIMUM_TRACKED_POINTS):
        cam, rows, cols, _ = sk.scene_camera(k, margin)
        out.append((name, k, margin, np.array(tracked, dtype=TRACK_POINT_DTYPE), np.array(cand, dtype=np.int32), float(md), int(maximum)))
        return track_update_sequential(pos, cam, rows, cols, tracked, cand, md, maximum)

    def flow(k, margin, records, seed):
        cam, rows, cols, _ = sk.scene_camera(k, margin)
        return perturbed(pos, cam, rows, cols, records, seed)

    # a chain on the overview: the set is filled from nothing, then tracked three times (flags, second strikes, re-adds), then seen from
    # a pose that puts much of it outside the field of view, then from one that puts some of it behind the camera
    r = run("fill", 0, 0.005, none, sel_a)
    r = run("track1", 0, 0.005, flow(0, 0.005, r[0], 11), sel_a)
    track1 = r[0]
    r = run("track2", 0, 0.005, flow(0, 0.005, r[0], 12), sel_a)
    r = run("track3", 2, 0.005, flow(2, 0.005, r[0], 13), sel_a)
    r = run("wall", 3, 0.005, flow(3, 0.005, r[0], 14), sel_b)
    r = run("wide", 1, -0.4, flow(1, -0.4, r[0], 15), sel_b, 7.5)
    r = run("narrow", 1, 0.005, flow(1, 0.005, r[0], 16), reg[::5], 7.5)
    r = run("among", 4, 0.005, flow(4, 0.005, r[0], 17), reg[3::11])
    r = run("among_wide", 4, -0.4, flow(4, -0.4, track1, 18), sel_a, 0.4)
    # several thousand candidates: both all-points selections in a row (the second repeats points of the first), every one reached
    run("both", 0, 0.005, flow(0, 0.005, track1, 21), np.concatenate([sel_a, sel_b]), 10.0, 100000)
    # the sizes: n around a wave, candidate lists around a workgroup, the raw registered list (many points per cell)
    t1 = flow(1, -0.4, track1, 19)
    for n, nc, md in ((1, 255, 7.5), (63, 256, 10.0), (64, 257, 0.4), (65, 1, 10.0), (300, 0, 10.0), (0, 1, 10.0), (1, 0, 7.5), (0, 257, 0.4)):
        run("size_%d_%d" % (n, nc), 1, -0.4, t1[:n], reg[100:100 + nc], md, 100000)
    # budgets around the number of winners, on a dense list
    t2 = flow(0, 0.005, track1, 20)
    dense = reg[1000:3000]
    free = run("budget_more", 0, 0.005, t2, dense, 10.0, 100000)
    s0, winners = free[3]["kept"], free[3]["added"]
    run("budget_exact", 0, 0.005, t2, dense, 10.0, s0 + winners)
    run("budget_one_less", 0, 0.005, t2, dense, 10.0, s0 + winners - 1)
    run("budget_1", 0, 0.005, t2, dense, 10.0, s0 + 1)
    # a full set: the first processed candidate is added iff it wins
    first_win = int(np.flatnonzero(free[2] == ADDED)[3])
    first_lose = int(np.flatnonzero(free[2] == REFUSED)[0])
    for label, head in (("wins", first_win), ("loses", first_lose)):
        lst = np.concatenate([dense[head:head + 1], dense])                 # ... and occurs again further on
        run("full_equal_" + label, 0, 0.005, t2, lst, 10.0, s0)
        run("full_above_" + label, 0, 0.005, t2, lst, 10.0, s0 - 5)
    run("full_zero", 0, 0.005, t2, dense, 10.0, 0)
    run("full_negative", 0, 0.005, none, dense[::-1], 10.0, -3)
    # repeats, unknown positions and tracked duplicates
    odd = np.concatenate([dense[:300], [-1, len(pos), 2 ** 31 - 1, -2 ** 31], dense[:300][::-1], t2["pool"][:40]]).astype(np.int32)
    t3 = np.concatenate([t2[:50], t2[10:30], t2[:5]])
    t3["pool"][55] = -7
    t3["pool"][56] = len(pos)
    run("odd", 0, 0.005, t3, odd, 7.5, 330)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case_results():
    pos = pool_positions()
    out = []
    for name, k, margin, tracked, cand, md, maximum in cases():
        cam, rows, cols, _ = sk.scene_camera(k, margin)
        out.append(track_update_sequential(pos, cam, rows, cols, tracked, cand, md, maximum))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ the golden file's layout
def golden_pack():
    """arrays of tests/golden/golden_color_track.npz: per case the inputs' CRC-32 and the records, both outcome arrays and the totals"""
    import zlib
    out = {"names": np.array([c[0] for c in cases()])}
    for (name, _, _, tracked, cand, md, maximum), (rec, t_out, c_out, tot, _) in zip(cases(), case_results()):
        out[name + "_inputs"] = np.array([len(tracked), zlib.crc32(tracked.tobytes()), len(cand), zlib.crc32(cand.tobytes()), maximum], dtype=np.int64)
        out[name + "_records"] = rec.view(np.uint8).copy()
        out[name + "_tracked_outcome"] = t_out
        out[name + "_candidate_outcome"] = c_out
        out[name + "_totals"] = np.array(totals_tuple(tot), dtype=np.int64)
    return out


def golden_check(g, name, rec, t_out, c_out, tot):
    """a call's results against the golden arrays of that name: None, or what differs"""
    if tuple(int(v) for v in g[name + "_totals"]) != (totals_tuple(tot) if isinstance(tot, dict) else tuple(tot)):
        return "totals"
    if g[name + "_records"].tobytes() != rec.tobytes():
        return "records"
    if g[name + "_tracked_outcome"].tobytes() != np.asarray(t_out, np.uint8).tobytes():
        return "tracked outcome"
    if g[name + "_candidate_outcome"].tobytes() != np.asarray(c_out, np.uint8).tobytes():
        return "candidate outcome"
    return None
