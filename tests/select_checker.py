"""Sequential restatement of rgbMapTracker::selectPointsForProjection (src/rgbMapTracker.cpp:45-152) on top of tests/color_checker.py's
map and tests/render_checker.py's camera: the candidates (the last point of every listed voxel, or rgb_points_vec), the two depth tests,
project3dPointInThisImage through the same Camera.project, the cell key, and the mask of `float` depths held in a Python dict.  One
candidate after the other, Python floats (IEEE doubles) with an explicit np.float32 where the reference holds a float.  What the device
pass (srl_color_map_select) and the recorded golden file are compared with; tests/test_select_checker_reference.py pins the pieces to
the reference's own translation units bit for bit.

select_closed_form is the same selection as a function of ranks, the form the device evaluates: with M the smallest (float) depth of a
cell, its holder is the LAST candidate with depth < (double) M if there is one, otherwise the FIRST with (float) depth == M.

Also the scenes of the tests: render_checker's three batches with the pool position of every stored point (SelectMap), the list-mode
sequence over its poses (SEQUENCE), and two thin shells around a camera that exercise the float-depth rule (shell_scene).
"""
import functools
import math

import numpy as np

import color_checker as cc
import render_checker as rk

F32 = np.float32
TOTALS = ("candidates", "visited", "far", "near", "behind", "outside", "selected", "unknown")
SELECTED_DTYPE = np.dtype([("index", "<i4"), ("pool", "<i4"), ("point_index", "<i4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                           ("u", "<f4"), ("v", "<f4")])
MINIMUM_DEPTH, MAXIMUM_DEPTH = 0.1, 200.0             # rgbMapTracker.cpp:9-10


# ------------------------------------------------------------------------------------------------ the cell key
def std_round(x):
    """std::round: to the nearest integer, half-way cases away from zero (x - trunc(x) is exact)"""
    t = float(math.trunc(x))
    if abs(x - t) >= 0.5:
        t += math.copysign(1.0, x)
    return t


def cell_coordinate(u_f, minimum_dis):
    """int u = std::round(u_f / minimum_dis) * minimum_dis (:116): FP64 quotient, FP64 product, conversion by truncation"""
    return int(std_round(u_f / minimum_dis) * minimum_dis)


# ------------------------------------------------------------------------------------------------ the map with pool positions
class SelectMap:
    """a ColorChecker that also knows where the device's append-only pool holds every stored point: its rank among all stored points"""

    def __init__(self, *opt):
        self.chk = cc.ColorChecker(*opt)
        self.pool_of = {}                    # (voxel key, slot) -> pool position

    def insert(self, world_xyz, time_sweep_end, time_last_process=0.0):
        out = self.chk.insert(world_xyz, time_sweep_end, time_last_process)
        for r in out[1]:
            self.pool_of[((int(r["kx"]), int(r["ky"]), int(r["kz"])), int(r["slot"]))] = len(self.pool_of)
        return out

    def candidates(self, voxels_xyz, use_all_points):
        """points_for_projection (:72-89) as (x, y, z as np.float32, pool position, point_index), and the list entries without a voxel"""
        chk = self.chk
        out, unknown = [], 0
        entries = np.zeros((0, 3), np.int64) if voxels_xyz is None else np.asarray(voxels_xyz, dtype=np.int64).reshape(-1, 3)
        if (not use_all_points) and len(entries):
            for e in entries:
                key = (int(e[0]), int(e[1]), int(e[2]))
                vox = chk.voxels.get(key)
                if vox is None or not vox.points:          # map[voxel] creates an empty block: NumPoints() == 0
                    unknown += 1
                    continue
                slot = len(vox.points) - 1                 # points.back()
                out.append((vox.points[slot], self.pool_of[(key, slot)], vox.point_index[slot]))
        else:
            for idx, r in enumerate(chk.registered):
                out.append(((r[0], r[1], r[2]), self.pool_of[(r[3], r[4])], idx))
        return out, unknown


# ------------------------------------------------------------------------------------------------ the loop
def _visit(smap, camera, rows, cols, voxels_xyz, minimum_dis, skip_step, use_all_points, minimum_depth, maximum_depth):
    """the part of the loop in front of the mask: per accepted candidate (index, cell, depth, u_f, v_f, candidate), and the totals so far"""
    cand, unknown = smap.candidates(voxels_xyz, use_all_points)
    tot = dict.fromkeys(TOTALS, 0)
    tot["candidates"], tot["unknown"] = len(cand), unknown
    accepted = []
    for i in range(0, len(cand), skip_step):                               # :93
        tot["visited"] += 1
        p32 = cand[i][0]
        p = (float(p32[0]), float(p32[1]), float(p32[2]))                  # getPosition(): position.cast<double>()
        depth = camera.distance(p)                                         # (point_world - t_world_camera).norm()
        if depth > maximum_depth:
            tot["far"] += 1
            continue
        if depth < minimum_depth:
            tot["near"] += 1
            continue
        outcome, u_f, v_f = camera.project(p, rows, cols)
        if outcome:
            tot["behind" if outcome == 1 else "outside"] += 1
            continue
        cell = (cell_coordinate(u_f, minimum_dis), cell_coordinate(v_f, minimum_dis))
        accepted.append((i, cell, depth, u_f, v_f, cand[i]))
    return accepted, tot


def _records(holders, by_index):
    out = np.zeros(len(holders), SELECTED_DTYPE)
    for k, i in enumerate(sorted(holders)):                                # std::map<int, ...>: ascending in the index
        _, _, _, u_f, v_f, (p32, pool, pidx) = by_index[i]
        out[k] = (i, pool, pidx, p32[0], p32[1], p32[2], F32(u_f), F32(v_f))      # cv::Point2f(u_f, v_f)
    return out


def select_sequential(smap, camera, rows, cols, voxels_xyz=None, minimum_dis=10.0, skip_step=1, use_all_points=False,
                      minimum_depth=MINIMUM_DEPTH, maximum_depth=MAXIMUM_DEPTH):
    """the reference's loop, literally.  Returns (records, totals, cells): cells maps a key to its candidates [(index, depth)] in order."""
    accepted, tot = _visit(smap, camera, rows, cols, voxels_xyz, minimum_dis, skip_step, use_all_points, minimum_depth, maximum_depth)
    mask_index, mask_depth = {}, {}
    drawn = set()                                                          # the keys of map_idx_draw_center
    cells = {}
    for i, cell, depth, _, _, _ in accepted:
        cells.setdefault(cell, []).append((i, depth))
        if cell not in mask_depth or float(mask_depth[cell]) > depth:      # :119: the stored float, promoted
            if cell in mask_index:
                drawn.remove(mask_index[cell])
            mask_index[cell] = i
            mask_depth[cell] = F32(depth)
            drawn.add(i)
    tot["selected"] = len(drawn)
    return _records(drawn, {a[0]: a for a in accepted}), tot, cells


def closed_form_holder(cand):
    """holder of one cell from its candidates [(index, depth)] in index order"""
    M = min(F32(d) for _, d in cand)
    below = [i for i, d in cand if d < float(M)]
    if below:
        return below[-1]
    return next(i for i, d in cand if F32(d) == M)


def sequential_holder(cand):
    """the mask update of :119-138 over one cell"""
    holder, stored = None, None
    for i, d in cand:
        if stored is None or float(stored) > d:
            holder, stored = i, F32(d)
    return holder


def select_closed_form(smap, camera, rows, cols, voxels_xyz=None, minimum_dis=10.0, skip_step=1, use_all_points=False,
                       minimum_depth=MINIMUM_DEPTH, maximum_depth=MAXIMUM_DEPTH):
    accepted, tot = _visit(smap, camera, rows, cols, voxels_xyz, minimum_dis, skip_step, use_all_points, minimum_depth, maximum_depth)
    cells = {}
    for i, cell, depth, _, _, _ in accepted:
        cells.setdefault(cell, []).append((i, depth))
    holders = {closed_form_holder(c) for c in cells.values()}
    tot["selected"] = len(holders)
    return _records(holders, {a[0]: a for a in accepted}), tot, cells


def rule_census(cells):
    """how the float-depth rule shows in a selection: cells with several candidates; cells whose holder was set by a depth below the
    cell's float minimum and is not the candidate of smallest double depth; cells without such a depth, with several candidates at the
    float minimum, whose holder is not the candidate of smallest double depth"""
    several = below_not_nearest = tie_not_nearest = 0
    for cand in cells.values():
        if len(cand) < 2:
            continue
        several += 1
        holder = sequential_holder(cand)
        M = min(F32(d) for _, d in cand)
        dmin = min(d for _, d in cand)
        holder_depth = dict(cand)[holder]
        if any(d < float(M) for _, d in cand):
            below_not_nearest += 1 if holder_depth != dmin else 0
        elif sum(1 for _, d in cand if F32(d) == M) > 1:
            tie_not_nearest += 1 if holder_depth != dmin else 0
    return several, below_not_nearest, tie_not_nearest


def totals_tuple(tot):
    return tuple(int(tot[name]) for name in TOTALS)


# ------------------------------------------------------------------------------------------------ the scenes
PARAMETER_SETS = ((10.0, 1), (7.5, 2), (40.0, 3), (0.4, 1))               # minimum_dis, skip_step
MARGINS = (0.005, -0.4)                                                    # state.cpp:25; rgbMapTracker.cpp:157, :164
# list mode: every render of render_checker.RENDERS (its pose, its image size, its list with voxels named up to three times) x every
# parameter set x both margins
SEQUENCE = tuple((k, s, m) for k in range(len(rk.RENDERS)) for s in range(len(PARAMETER_SETS)) for m in range(len(MARGINS)))
EXTRA_BATCH_TIME = 6.0


@functools.lru_cache(maxsize=None)
def scene_map(batches=3):
    """render_checker's scene with pool positions; batches = 4 adds a further insertion (the first batch moved by 0.37 m)"""
    smap = SelectMap(*rk.OPT)
    visited = [smap.insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)[2] for j in range(3)]
    if batches == 4:
        visited.append(smap.insert(extra_batch(), EXTRA_BATCH_TIME, 0.0)[2])
    return smap, visited


def extra_batch():
    return cc.scene_batch(0) + np.array([0.37, -0.21, 0.013])


def scene_camera(k, margin):
    """the camera of render k with another margin, its image size, and the list of the render"""
    pose, which, _, lists = rk.RENDERS[k]
    cam = rk.scene_camera(rk.POSES[pose], which)
    cam.fov_margin = float(margin)
    rows, cols = rk.IMAGE_SIZES[which]
    return cam, rows, cols, lists


@functools.lru_cache(maxsize=None)
def sequence_results():
    """the checker's (records, totals, cells) for every entry of SEQUENCE"""
    smap, visited = scene_map()
    out = []
    for k, s, m in SEQUENCE:
        cam, rows, cols, lists = scene_camera(k, MARGINS[m])
        voxels = np.concatenate([visited[j] for j in lists])
        md, skip = PARAMETER_SETS[s]
        out.append(select_sequential(smap, cam, rows, cols, voxels, md, skip))
    return out


ALL_POINTS_CAMERAS = ((0, 0.005), (1, -0.4))                              # (render whose pose and image size are used, margin)


@functools.lru_cache(maxsize=None)
def all_points_results(batches):
    smap, _ = scene_map(batches)
    out = []
    for k, margin in ALL_POINTS_CAMERAS:
        cam, rows, cols, _ = scene_camera(k, margin)
        out.append(select_sequential(smap, cam, rows, cols, None, 10.0, 1, True))
    return out


# two thin shells around a camera at the origin: depths of neighbouring candidates differ by a few float ulps at most
SHELL_OPT = (0.1, 50, 0.001, 1)                                            # a 1 mm grid: nearly every point registers
SHELL_ROWS, SHELL_COLS, SHELL_F = 480, 640, 230.0


def shell_points():
    rng = np.random.default_rng(4242)
    n = 6000
    x = rng.uniform(-1, 1, n).astype(F32)
    y = rng.uniform(-1, 1, n).astype(F32)
    R = np.where(x < 0, 5.0, 5.3)
    z = np.sqrt(R * R - x.astype(np.float64) ** 2 - y.astype(np.float64) ** 2).astype(F32)
    nudge = rng.integers(0, 3, n)
    for _ in range(2):
        z = np.where(nudge > 0, np.nextafter(z, F32(np.inf)), z).astype(F32)
        nudge = nudge - 1
    return np.stack([x, y, z], 1).astype(np.float64)                       # exactly representable: the map's FP32 cast changes nothing


def shell_camera():
    return rk.Camera((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0), SHELL_F, SHELL_F, SHELL_COLS / 2.0, SHELL_ROWS / 2.0, 0.005)


@functools.lru_cache(maxsize=None)
def shell_scene():
    smap = SelectMap(*SHELL_OPT)
    smap.insert(shell_points(), 1.0, 0.0)
    return smap, select_sequential(smap, shell_camera(), SHELL_ROWS, SHELL_COLS, None, 10.0, 1, True)


# ------------------------------------------------------------------------------------------------ the golden file's layout
def golden_pack():
    """arrays of tests/golden/golden_color_select.npz: for every entry of SEQUENCE and of the all-points calls the totals and the records.
    pool, point_index and the position are functions of the index and the map (which golden_color_map.npz records), so the file holds
    index, u and v; at minimum_dis 0.4 nearly every candidate keeps a cell of its own and the records alone would pass the size limit of a
    committed file: there it holds the number of records and a CRC-32 of their bytes, as it does for every entry."""
    import zlib
    out = {"sequence": np.array(SEQUENCE, dtype=np.int32), "parameter_sets": np.array(PARAMETER_SETS), "margins": np.array(MARGINS)}
    calls = [("s%d" % n, r, PARAMETER_SETS[SEQUENCE[n][1]][0] >= 1.0) for n, r in enumerate(sequence_results())]
    calls += [("a%d_%d" % (b, n), r, True) for b in (3, 4) for n, r in enumerate(all_points_results(b))]
    calls.append(("shell", shell_scene()[1], True))
    for name, (rec, tot, _), whole in calls:
        out[name + "_totals"] = np.array(totals_tuple(tot), dtype=np.int64)
        out[name + "_crc"] = np.array([len(rec), zlib.crc32(rec.tobytes())], dtype=np.int64)
        if whole:
            out[name + "_index"] = rec["index"].copy()
            out[name + "_uv"] = np.stack([rec["u"], rec["v"]], 1)
    return out


def golden_check(g, name, rec, tot):
    """a selection against the golden arrays of that name: None, or what differs"""
    import zlib
    if tuple(int(v) for v in g[name + "_totals"]) != (totals_tuple(tot) if isinstance(tot, dict) else tuple(tot)):
        return "totals"
    if (len(rec), zlib.crc32(rec.tobytes())) != tuple(int(v) for v in g[name + "_crc"]):
        return "records (CRC)"
    if name + "_index" in g.files:
        if not np.array_equal(g[name + "_index"], rec["index"]):
            return "index"
        if g[name + "_uv"].tobytes() != np.stack([rec["u"], rec["v"]], 1).tobytes():
            return "u, v"
    return None
