"""Random scripts of passes, map edits, sweep changes and option changes for ONE live context, and their interpreter on the CPU oracle.

make_script(seed) draws the scene and 25 to 40 steps from np.random.default_rng(seed).  A step is a (kind, arguments) tuple of plain Python
values: print it, paste it, replay it.  run_on_oracle(script, oracle_lib, backend) keeps an oracle Map in step and returns the oracle's
build_plane_residuals result of every pass; the oracle restarts from nothing at every pass, so nothing is carried over on this side.
tests/test_gpu_pass_script.py feeds the same steps to device contexts; tests/test_pass_script_model.py shows, from this file and the oracle
alone, that the scripts can catch what they are for.  No device work happens here.

The scene: synth.map_candidates(seed, map_pts), shuffled once; the first 60 % are the starting map, the rest is dealt out by `insert` and
`commit` steps (points the map does not hold yet: they are stored, and they change what the keypoints see).

The steps:
  ("sweep",  seed, n, pattern, how)     synth.make_sweep; how: "upload", "swap" (prefetch from page-locked memory, then swap) or "again" (the
                                        current sweep uploaded once more: nothing changes but what the context remembers)
  ("opts",   K, max_res, thr, nb, frame_id, select_mode)    hold until the next opts step; min_number_neighbors = min(K, 20), so that a pass
                                        with K = 5 accepts keypoints at all (tests/test_gpu_option_envelope.py pairs them the same way)
  ("pass",   q, t, taps)                one srl_build_residuals at this pose
  ("insert", "held", a, b, centre, radius)      held-back candidates [a, b) within `radius` of `centre` (the sweep's reach)
  ("insert", "grow", a, b, centre, radius, total)   the same, padded with points of the starting map (refused: they are stored already) to
                                        `total` points -- more than the reserve: slab storage, records and table grow
  ("insert", "far", seed, at)           40 points in voxels nobody looks at
  ("prune",  location, distance)        srl_map_remove_far
  ("commit", a, b, centre, radius, q, t)    frame_upload + deferred frame_commit of those held-back candidates as a frame seen from (q, t)
  ("search", points)                    srl_search_neighbors on a few world points, under the current options
  ("end",    how)                       "solve_end" or "disarm"
"""
import functools

import numpy as np

from sr_livo_amd import synth

INT_MAX = 2**31 - 1
MAP_PTS = (3_000, 12_000, 40_000)
SWEEP_N = (1, 7, 63, 64, 65, 500, 1_500, 4_096)
PATTERNS = ("livox", "ouster16")
HOWS = ("upload", "swap", "again")
OPT_K = (5, 20, 32)
OPT_MAX_RES = (INT_MAX, 600, 37)
OPT_THR = (1, 5, 12, 20)                  # tests/test_gpu_option_envelope.py; 20: saturated voxels only, bounds left under 1 are far too tight
OPT_NB = (1, 2)
OPT_FRAME_ID = (5, 100)                   # 5: init mode (two layers, threshold 1 whatever the options say), 100: the options hold
OPT_SELECT = (0, 1, 2)
OPT_FIELDS = ("K", "max_res", "thr", "nb", "frame_id", "select_mode")
START_SHARE = 0.6
HELD_SHARE = 0.15                         # of the held-back candidates per insert
COMMIT_POINTS = 300
FAR_POINTS = 40
MIN_N_FOR_MAP_EDITS = 63                  # a map edit is asked to change the next pass's answer: not with 1 or 7 keypoints
VOXELS_UPPER = 3_000                      # no map of these scenes has more voxels (1 300 to 2 500)
EDIT_KINDS = ("sweep:upload", "sweep:swap", "sweep:again", "insert:held", "insert:grow", "insert:far", "prune", "commit", "opts", "search")

# The committed seeds: the first 12 run by default, SRL_FUZZ_CASES raises the number up to all 48.  Every one of them meets the conditions
# tests/test_pass_script_model.py asserts (each answer-changing edit changes the oracle's answer, no NaN planarity, no degenerate plane)
# and the conditions on the run tests/test_gpu_pass_script.py asserts (bounds live, armed launches fired).
SEEDS = (24, 37, 70, 80, 105, 162, 3, 7, 9, 13, 15, 18, 20, 21, 22, 27,
         31, 43, 46, 51, 52, 53, 58, 59, 60, 62, 67, 71, 74, 75, 76, 77,
         84, 90, 95, 106, 107, 117, 121, 122, 123, 133, 138, 141, 149, 154, 160, 161)


def committed_seeds(cases):
    return SEEDS[: max(1, min(int(cases), len(SEEDS)))]


# ------------------------------------------------------------------------------------------------ the scene and what steps stand for
@functools.lru_cache(maxsize=4)
def _scene_points(seed, map_pts):
    cands, L = synth.map_candidates(seed, map_pts)
    cands = cands[np.random.default_rng([seed, 60]).permutation(len(cands))]          # shuffled once
    return cands, L, int(START_SHARE * len(cands))


def scene_points(scene):
    """(start points, held-back points, L) of a script's scene"""
    cands, L, n0 = _scene_points(scene["seed"], scene["map_pts"])
    return cands[:n0], cands[n0:], L


@functools.lru_cache(maxsize=64)
def _sweep(seed, n, L, pattern):
    return synth.make_sweep(seed, n, L, pattern=pattern)


def sweep_of(scene, step):
    _, seed, n, pattern, _how = step
    return _sweep(seed, n, scene_points(scene)[2], pattern)


_start_maps = {}


def start_map(scene, po, backend):
    """the starting map as the oracle builds it, exported (keys, counts, xyz); built once per scene"""
    key = (scene["seed"], scene["map_pts"], backend)
    if key not in _start_maps:
        if len(_start_maps) >= 4:
            _start_maps.clear()
        m = po.Map(backend)
        m.add_points(scene_points(scene)[0])
        _start_maps[key] = m.export()
    return _start_maps[key]


def _within(points, centre, radius):
    return points[np.linalg.norm(points - np.asarray(centre), axis=1) <= radius]


def insert_points(scene, step):
    """the world points of an insert step"""
    start, held, _ = scene_points(scene)
    kind = step[1]
    if kind == "far":
        _, _, seed, at = step
        return np.asarray(at) + np.random.default_rng(seed).uniform(0.0, 3.0, (FAR_POINTS, 3))
    a, b, centre, radius = step[2:6]
    pts = _within(held[a:b], centre, radius)
    if kind == "grow":
        pts = np.concatenate([pts, np.resize(start, (max(step[6] - len(pts), 0), 3))])
    return pts


def commit_frame(scene, step):
    """(raw points in the lidar frame, q, t) of a commit step: held-back candidates as a frame seen from (q, t)"""
    _, a, b, centre, radius, q, t = step
    pts = _within(scene_points(scene)[1][a:b], centre, radius)[:COMMIT_POINTS]
    q = np.asarray(q); t = np.asarray(t)
    return (pts - t) @ synth.quat_to_rot(q), q, t


def opts_dict(step):
    return dict(zip(OPT_FIELDS, step[1:]))


def opt_kwargs(o):
    """keyword arguments of default_opts (the product's and the oracle's) for an options dictionary"""
    return dict(max_number_neighbors=o["K"], min_number_neighbors=min(o["K"], 20), max_num_residuals=o["max_res"],
                threshold_voxel_occupancy=o["thr"], voxel_neighborhood=o["nb"])


def effective(o):
    """what a pass's neighbour search depends on: (K, layers, threshold) -- two layers and threshold 1 in the init mode (optimize.cpp:21-23)"""
    return (o["K"], 2, 1) if o["frame_id"] < 20 else (o["K"], o["nb"], o["thr"])


# ------------------------------------------------------------------------------------------------ the generator
def _tup(a):
    return tuple(float(v) for v in np.asarray(a).ravel())


def _run_poses(rng, sw, count, jump_at):
    """poses of consecutive ESIKF iterations closing on the ground truth (tests/test_gpu_bound_culling.py: _poses), one far-off pose between"""
    out = []
    for k in range(count):
        a = 0.7 ** k
        q = synth.quat_mul(sw["q_gt"], synth.quat_from_rotvec(a * rng.normal(0, 0.004, 3)))
        t = sw["t_gt"] + a * (sw["t_pred"] - sw["t_gt"]) + rng.normal(0, 1e-4, 3)
        out.append((q, t))
    if jump_at is not None:
        phi = rng.uniform(0, 2 * np.pi)
        axis = rng.normal(size=3); axis *= 0.3 / np.linalg.norm(axis)
        out.insert(jump_at, (synth.quat_mul(sw["q_gt"], synth.quat_from_rotvec(axis)), sw["t_gt"] + np.array([1.5 * np.cos(phi), 1.5 * np.sin(phi), 0.2])))
    return out


def _draw_opts(rng, cur, force_select=None):
    """the options after an opts step.  Three times in four ONE of K, threshold, layers and frame_id changes and the other three stay (a
    threshold or layer count the init mode would ignore is not the one): the pass behind it meets what the pass before left for the old value,
    and only that value tells the two apart.  Otherwise all four are drawn anew.  Budget and selection path change with probability 0.3 each."""
    values = dict(zip(OPT_FIELDS, (OPT_K, OPT_MAX_RES, OPT_THR, OPT_NB, OPT_FRAME_ID, OPT_SELECT)))
    if cur is None:
        o = {f: int(rng.choice(v)) for f, v in values.items()}
    else:
        o = opts_dict(cur)
        if rng.random() < 0.75:
            fields = ["K", "frame_id"] + (["thr", "nb"] if o["frame_id"] >= 20 else [])
            f = str(rng.choice(fields))
            o[f] = int(rng.choice([v for v in values[f] if v != o[f]]))
        else:
            for f in ("K", "thr", "nb", "frame_id"):
                o[f] = int(rng.choice(values[f]))
        for f in ("max_res", "select_mode"):
            if rng.random() < 0.3:
                o[f] = int(rng.choice([v for v in values[f] if v != o[f]]))
    if force_select is not None:
        o["select_mode"] = force_select
    return ("opts",) + tuple(o[f] for f in OPT_FIELDS)


LIVE_EDITS = ("insert:held", "insert:grow", "prune", "commit", "opts")
MIN_LIVE_BLOCKS = 3                       # blocks that edit the map or the options under a sweep that stays: the bounds of the pass before are there


def _plan(rng):
    """the shape of a script, before anything is computed: per block the edit kinds in order, the new sweep's size, the run's length"""
    blocks = int(rng.integers(5, 8))
    quiet = int(rng.integers(1, blocks))              # the run of this block has its taps off and 4 096 keypoints: armed launches can fire
    plan, n_cur, sizes = [], 0, []
    for b in range(blocks):
        if b == 0:
            kinds = ["sweep:upload", "opts"]
        else:
            pool = [k for k in EDIT_KINDS if k != "search"]
            kinds = [str(k) for k in rng.choice(pool, size=int(rng.integers(1, 4)), replace=False)]
            if sum(k.startswith("sweep:") for k in kinds) > 1:            # one sweep step per block
                first = next(k for k in kinds if k.startswith("sweep:"))
                kinds = [k for k in kinds if not k.startswith("sweep:") or k == first]
            if b == quiet:
                kinds = [k for k in kinds if k != "sweep:again"]
                if not any(k.startswith("sweep:") for k in kinds):
                    kinds.append(str(rng.choice(["sweep:upload", "sweep:swap"])))
                if "opts" not in kinds:
                    kinds.append("opts")
                kinds = [kinds[i] for i in rng.permutation(len(kinds))]
        n_new = None
        if any(k in ("sweep:upload", "sweep:swap") for k in kinds):
            n_new = 4096 if b == quiet else int(rng.choice(SWEEP_N))
            sizes.append(n_new)
            n_cur = n_new
        if n_cur < MIN_N_FOR_MAP_EDITS:               # a map edit must change the next pass's answer: not asked of 1 or 7 keypoints
            kinds = [k for k in kinds if k.startswith("sweep:") or k == "opts"]
        run = int(rng.integers(2, 6))
        plan.append(dict(kinds=kinds, n_new=n_new, run=run, jump=bool(rng.random() < 0.3), search=bool(b != quiet and rng.random() < 0.35),
                         end=bool(rng.random() < 0.4), quiet=b == quiet))
    passes = sum(p["run"] + p["jump"] for p in plan)
    steps = passes + sum(len(p["kinds"]) + p["search"] + p["end"] for p in plan)
    stays = [p for p in plan[1:] if not any(k.startswith("sweep:") for k in p["kinds"])]
    live = sum(any(k in LIVE_EDITS for k in p["kinds"]) for p in stays)
    live_opts = sum("opts" in p["kinds"] for p in stays)
    shrunk = any(b < a for a, b in zip(sizes, sizes[1:]))
    grown = any(b > a for a, b in zip(sizes, sizes[1:]))
    if not (12 <= passes <= 20 and 25 <= steps <= 40 and live >= MIN_LIVE_BLOCKS and live_opts >= 1 and shrunk and grown):
        return None
    return plan


def _draw_steps(rng, scene):
    plan = _plan(rng)
    if plan is None:
        return None
    start, held, L = scene_points(scene)
    steps, sweep, n_cur, pose, opts = [], None, 0, None, None
    ptr, prunes, far, pruned_under = 0, 0, 0, None
    cap_ub = VOXELS_UPPER + VOXELS_UPPER // 2 + 4096  # an upper bound of the slab reserve (tests/test_gpu_neighbour_records.py has the arithmetic)
    slice_len = int(HELD_SHARE * len(held))
    for blk in plan:
        kinds = blk["kinds"]
        new_sweep = None
        for k in kinds:
            if k in ("sweep:upload", "sweep:swap"):
                new_sweep = ("sweep", int(rng.integers(1, 2**31 - 1)), blk["n_new"], str(rng.choice(PATTERNS)), k.split(":")[1])
        sw_block = sweep_of(scene, new_sweep) if new_sweep else sweep       # the sweep the passes of this block run on
        reach = float(np.max(np.linalg.norm(sw_block["raw"], axis=1))) + 1.0
        centre = _tup(sw_block["t_gt"])
        for k in kinds:
            if k in ("sweep:upload", "sweep:swap"):
                steps.append(new_sweep)
                sweep, n_cur, cur_step = sw_block, new_sweep[2], new_sweep
            elif k == "sweep:again":
                steps.append(cur_step[:4] + ("again",))
            elif k == "opts":
                opts = _draw_opts(rng, opts, force_select=0 if blk["quiet"] else None)
                steps.append(opts)
            elif k in ("insert:held", "insert:grow"):
                if ptr + slice_len > len(held):
                    return None
                step = ("insert", k.split(":")[1], ptr, ptr + slice_len, centre, reach)
                if k == "insert:grow":
                    step += (cap_ub + 64,)
                ptr += slice_len
                cap_ub = max(cap_ub, (VOXELS_UPPER + max(step[6] if k == "insert:grow" else 0, slice_len)) * 3 // 2 + 1)
                steps.append(step)
            elif k == "insert:far":
                steps.append(("insert", "far", int(rng.integers(1, 2**31 - 1)), (150.0 + 20.0 * far, -140.0, 40.0)))
                far += 1
            elif k == "prune":
                if prunes == 2:
                    return None
                prunes += 1
                # the median keypoint range: voxels inside the keypoints' reach go (a second prune under the same sweep cuts closer: the same
                # sphere again would remove nothing)
                again = pruned_under is sw_block
                pruned_under = sw_block
                steps.append(("prune", centre, float(np.median(np.linalg.norm(sw_block["raw"], axis=1))) * (0.7 if again else 1.0)))
            elif k == "commit":
                if ptr + 4 * COMMIT_POINTS > len(held):
                    return None
                steps.append(("commit", ptr, ptr + 4 * COMMIT_POINTS, centre, reach, _tup(sw_block["q_gt"]), _tup(sw_block["t_gt"])))
                ptr += 4 * COMMIT_POINTS
        poses = _run_poses(rng, sweep, blk["run"], int(rng.integers(1, blk["run"])) if blk["jump"] else None)
        search_at = int(rng.integers(1, len(poses))) if blk["search"] else None
        for i, (q, t) in enumerate(poses):
            if i == search_at:
                R = synth.quat_to_rot(pose[0] / np.linalg.norm(pose[0]))
                near = sweep["raw"][: min(4, n_cur)] @ R.T + pose[1]
                steps.append(("search", tuple(_tup(p) for p in np.concatenate([near, near[:1] + rng.normal(0, 0.5, (2, 3)), [[90.0, 90.0, 30.0]]]))))
            pose = (q, t)
            steps.append(("pass", _tup(q), _tup(t), False if blk["quiet"] else bool(rng.random() < 2 / 3)))
        if blk["quiet"]:
            # Behind the quiet run a launch may be left armed; nothing but an opts step -- host-only, it cancels nothing -- lies between it and
            # one more pass without taps: K or the threshold alone has changed, and only the launch's argument check can tell.  (Drawn from a
            # generator of its own.)
            side = np.random.default_rng([scene["seed"], 4096])
            o = opts_dict(opts)
            f = "thr" if o["frame_id"] >= 20 and side.random() < 0.5 else "K"
            o[f] = int(side.choice([v for v in dict(K=OPT_K, thr=OPT_THR)[f] if v != o[f]]))
            opts = ("opts",) + tuple(o[k] for k in OPT_FIELDS)
            q = synth.quat_mul(sweep["q_gt"], synth.quat_from_rotvec(side.normal(0, 0.0005, 3)))
            pose = (q, sweep["t_gt"] + side.normal(0, 1e-4, 3))
            steps += [opts, ("pass", _tup(pose[0]), _tup(pose[1]), False)]
        if blk["end"]:
            steps.append(("end", str(rng.choice(["solve_end", "disarm"]))))
    passes = sum(s[0] == "pass" for s in steps)
    return steps if len(steps) <= 40 and passes <= 20 else None


@functools.lru_cache(maxsize=128)
def _make_script(seed):
    rng = np.random.default_rng(seed)
    scene = dict(seed=int(seed), map_pts=int(rng.choice(MAP_PTS)), cull=int(rng.choice([1, 2])), armed=int(rng.choice([1, 2])))
    while True:                                        # (drawn again from the same generator until the script has the required shape)
        steps = _draw_steps(rng, scene)
        if steps is not None:
            return scene, tuple(steps)


def make_script(seed):
    scene, steps = _make_script(int(seed))
    return dict(scene=dict(scene), steps=list(steps))


def edit_kind(step):
    """the kind of edit a step is, as the scripts' rules count them (None for passes and `end`)"""
    if step[0] == "sweep":
        return "sweep:" + step[4]
    if step[0] == "insert":
        return "insert:" + step[1]
    return step[0] if step[0] in ("prune", "commit", "opts", "search") else None


def format_steps(steps, upto=None):
    """the steps, one per line with their index: what a failure message carries (paste a prefix into run_script(steps[:k]))"""
    return "\n".join(f"  [{i}] {s!r}," for i, s in enumerate(steps[: len(steps) if upto is None else upto + 1]))


# ------------------------------------------------------------------------------------------------ the interpreter on the oracle
MISTAKES = ("bounds_across_insert", "bounds_across_prune", "stale_sweep_tail", "stale_K", "stale_frame_id", "stale_threshold")


class OracleRun:
    """The oracle's side of a script, one step at a time.  `mistake`: one of MISTAKES -- the interpreter then makes that one mistake on purpose,
    the way a context with stale carried state would (tests/test_pass_script_model.py: the scripts must tell each of them from the truth)."""

    def __init__(self, scene, po, backend, mistake=None):
        from test_gpu_map_prune import _omap
        self.scene, self.po, self.backend, self.mistake = scene, po, backend, mistake
        self._omap = _omap
        self.map = _omap(po, backend, *start_map(scene, po, backend))
        self.sweep = self.raw = self.opts = None
        self.live = None                                # the options of the last pass, while what it learnt still holds: no sweep step, no map edit since
        self.stale_map = None                           # (mistake) the map before the last insert / prune, until the next pass
        self.reserve = None                             # the slab reserve as the device keeps it, modelled: _reserve_for
        self.grew = []                                  # per insert, in order: it grew the modelled reserve

    def fork(self):
        other = OracleRun.__new__(OracleRun)
        other.__dict__.update(self.__dict__)
        other.map = self._omap(self.po, self.backend, *self.map.export())
        other.grew = list(self.grew)
        return other

    def _map_edit(self, which=None):
        """a map edit voids what the last pass learnt -- unless the mistake is to keep it: then the map before the edit is what it was learnt on"""
        if self.mistake is not None and self.mistake == which and self.live is not None:
            if self.stale_map is None:
                self.stale_map = self._omap(self.po, self.backend, *self.map.export())
        else:
            self.live = self.stale_map = None

    def _reserve_for(self, n):
        """the device makes room for one new voxel per point of a batch beforehand; an upload reserves voxels * 3 / 2 + 4 096 slabs"""
        V = self.map.num_voxels()
        if self.reserve is None:
            self.reserve = V + V // 2 + 4096
        need = V + n
        grows = need > self.reserve
        if grows:
            self.reserve = max(need + need // 2, 1024)
        return grows

    def _pass(self, m, o, raw, q, t):
        return m.build_plane_residuals(self.po.default_opts(**opt_kwargs(o)), raw, np.asarray(q), np.asarray(t), self.sweep["t_last"], frame_id=o["frame_id"])

    def step(self, step, reference=None):
        """apply one step; returns the oracle's result for a pass, the exported map for a map edit, the search results for a search.
        reference: the true run's record of this step -- returned as it is where the mistake (if any) is not in play"""
        kind = step[0]
        if kind == "sweep":
            sw = sweep_of(self.scene, step)
            raw = sw["raw"]
            if self.mistake == "stale_sweep_tail" and step[4] != "again" and self.raw is not None and len(self.raw) > len(raw):
                raw = np.concatenate([raw, self.raw[len(raw):]])          # keypoints [n_new, n_old) of the sweep before still counted
            self.sweep, self.raw = sw, raw
            self.live = self.stale_map = None
        elif kind == "opts":
            self.opts = opts_dict(step)
        elif kind == "insert":
            self._map_edit("bounds_across_insert")
            pts = insert_points(self.scene, step)
            self.grew.append(self._reserve_for(len(pts)))
            self.map.add_points(pts)
            return self.map.export()
        elif kind == "prune":
            from test_gpu_map_prune import prune_keep
            self._map_edit("bounds_across_prune")
            k, c, x = self.map.export()
            keep = prune_keep(x, step[1], step[2])
            self.map = self._omap(self.po, self.backend, k[keep], c[keep], x[keep])
            return (k[keep], c[keep], x[keep]), (int((~keep).sum()), int(c[~keep].sum()))
        elif kind == "commit":
            self._map_edit()
            raw, q, t = commit_frame(self.scene, step)
            self._reserve_for(len(raw))
            self.map.add_points(self.po.transform_points(raw, q, t, backend=self.backend))
            return self.map.export()
        elif kind == "search":
            K, nb, thr = self.opts["K"], self.opts["nb"], self.opts["thr"]
            return [self.map.search_neighbors(np.asarray(p), nb=nb, K=K, thr=thr) for p in step[1]]
        elif kind == "pass":
            o, before = self.opts, self.live
            self.live = self.opts
            # What the pass before learnt holds under ITS K, layers and threshold only.  The mistake: one of them is not looked at, so a pass
            # whose options differ from the last pass's in that one alone is answered as if it had not changed.
            stale = {"stale_K": "K", "stale_frame_id": "frame_id", "stale_threshold": "thr"}.get(self.mistake)
            if stale and before is not None and effective(o) != effective(before) and effective(dict(o, **{stale: before[stale]})) == effective(before):
                o = dict(o, **{stale: before[stale]})
            elif self.stale_map is not None and (before is None or effective(o) != effective(before)):
                self.stale_map = None                     # other options: what was learnt is void whatever the map did
            if o is self.opts and self.stale_map is None and len(self.raw) == len(self.sweep["raw"]) and reference is not None:
                return reference
            res = self._pass(self.map, o, self.raw, step[1], step[2])
            if self.stale_map is not None:
                # keypoints whose home voxel holds what it held before the edit are answered from the map before the edit
                old = self._pass(self.stale_map, o, self.raw, step[1], step[2])
                before_c = {tuple(k): int(c) for k, c in zip(*(a.tolist() for a in self.stale_map.export()[:2]))}
                after_c = {tuple(k): int(c) for k, c in zip(*(a.tolist() for a in self.map.export()[:2]))}
                home = np.trunc(res["point_world"]).astype(np.int64)
                same = np.array([before_c.get(tuple(h), 0) == after_c.get(tuple(h), 0) for h in home.tolist()], bool)
                res["ids"][same] = old["ids"][same]
                res["status"][same] = old["status"][same]
                self.stale_map = None
            return res
        return None


def run_on_oracle(script, oracle_lib, backend, mistake=None, trace=None, reference=None):
    """the oracle's build_plane_residuals result of every pass of the script, in order.  trace: a list that receives the record of EVERY
    step (None for steps without one); reference: the trace of the true run, to save a variant run the passes its mistake does not touch"""
    run = OracleRun(script["scene"], oracle_lib, backend, mistake)
    out = []
    for i, step in enumerate(script["steps"]):
        rec = run.step(step, reference[i] if reference is not None else None)
        if trace is not None:
            trace.append(rec)
        if step[0] == "pass":
            out.append(rec)
    return out
