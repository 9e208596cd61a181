"""One live context under random scripts of passes, map edits, sweep changes and option changes (tests/pass_script.py).

Neighbourhood bounds, the prefilter threshold taken from them, the per-voxel neighbour records and armed launches are state that a map edit,
a sweep change or an option change must void or rebuild.  Each has its scenario file with a hand-written sequence; here the kinds of change
arrive in an order nobody wrote down.  Four runs of the same script, the device runs one after the other (a second live context on the
device keeps mode 1 from arming a launch at all):

  PLAIN    bound culling, neighbour records and armed launches off
  FAST     srl.Context(0) as shipped: neighbour records on, bound culling 1 or 2 and armed launches 1 or 2 as the script's scene says -- the
           identical calls as PLAIN and nothing else: no debug read sits between two steps
  WATCHED  FAST again, with bounds_download() before every pass and behind every edit.  srl_debug_bounds_download disarms, like most entry
           points: watching cancels the very launch that should meet a changed pass, so the guards come from this run and the answers
           from the one above
  ORACLE   pass_script.run_on_oracle: the CPU oracle, which starts from nothing at every pass

Every pass: FAST == PLAIN bit for bit (return code; num_residuals, sum_candidates, last_visited, success, nan_error, HtH, Hth, loss_sum; with
taps ids, status, candidate counts and every residual array); FAST against the oracle with test_gpu_parity.check_pass_against (ids and
status exact, counts equal, fields to TIGHT), no keypoint masked; without taps counts, HtH, Hth and loss_sum to TIGHT.  The product's
NormalEq has no num_ties; its num_fallback is not compared: how many keypoints leave the fast selection path may differ with the bounds
(DESIGN.md), the answer may not.  Every map edit: the three maps equal.  Every search: equal.  At the end the neighbour records equal the
brute-force model of tests/test_gpu_neighbour_records.py.

In FAST only an opts step (host-only) and prefetch + swap leave an armed launch alive; every script has, behind its run of passes without
taps on 4 096 keypoints, an opts step that changes K or the threshold alone and one more such pass: the launch armed under the old value
must be cancelled, not fired (fire_or_cancel's comparison of the arguments).

The run was not idle (WATCHED, and FAST's srl_get_arm_stats): bounds were there before at least a third of the passes -- each one looked at
--, gone behind every edit and sweep, and armed launches were fired.  tests/test_pass_script_model.py shows that the scripts would notice
stale state.  The interpreter sits between two passes, so FAST's armed launches wait longer than the shipped 150 us before the host gives
them up (set_arm_linger, as tests/test_gpu_option_envelope.py does); what a pass computes does not depend on it.

A failure -- an assertion, an error status inside a run, a guard -- names the seed, the step and the steps so far; paste them into
run_script(dict(scene=..., steps=[...]), oracle_lib, backend, guards=False).  Nothing is run again.  SRL_FUZZ_CASES raises the number of
scripts from 12 up to the 48 committed seeds.

That slab storage grew under a "grow" insert is not observed here: no entry point reports the reserve.  tests/test_pass_script_model.py
asserts it on a model of the reserve's arithmetic (pass_script.OracleRun._reserve_for).

Measured on an MI355X: the three device runs of a script take 0.03 to 0.1 s, a test 0.1 to 0.6 s with the oracle's run; the 12 default
scripts 3.8 s, all 48 14 s.

What the scripts notice was tried with builds that each drop or weaken one line, guards off (FAST != PLAIN or the oracle alone), over the 48
committed seeds / the first 12: an armed launch's signature without the threshold fails 11 / 2 (seeds 37, 105), without K 8 / 1 (seed 9); a
prune that leaves the bounds 11 / 3; bounds whose signature leaves out the threshold 7 / 1; insertions that leave the neighbour records
alone 41 / 10.  Bounds kept across an insertion change nothing -- more points only shorten a K-th distance, the stale bound stays an upper
bound -- so no test can hold that line.
"""
import os
import time

import numpy as np
import pytest

import pass_script as ps
import sr_livo_amd as srl
from sr_livo_amd import capi

from test_gpu_bound_culling import _same
from test_gpu_neighbour_records import _model
from test_gpu_parity import INT_MAX, TIGHT, check_pass_against, rel

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("SRL_FUZZ_CASES", "12"))
NEQ_FIELDS = ("num_residuals", "sum_candidates", "last_visited", "success", "nan_error", "loss_sum")
RESIDUAL_ARRAYS = ("normal", "a2D", "weight", "norm_offset", "distance", "jacobian")


class DeviceRun:
    """one context fed a script; records what every step returned.  fast: the carried state is on.  watch: bounds_download() before every pass
    and behind every edit -- srl_debug_bounds_download disarms, so a watched run is not the run whose answers are compared"""

    def __init__(self, scene, start_map, fast, watch=False):
        self.scene, self.fast, self.watch = scene, fast, watch
        self.ctx = ctx = srl.Context(0)
        self.pins = []
        if fast:
            ctx.set_bound_culling(scene["cull"])
            ctx.set_armed_launch(scene["armed"])
            ctx.set_arm_linger(host_linger_us=1e5, kernel_linger_us=2e5)
        else:
            ctx.set_bound_culling(0)
            ctx.set_neighbour_records(0)
            ctx.set_armed_launch(0)
        ctx.map_upload(*start_map)
        self.sweep = self.o = self.opts = None
        self.taps = False
        self.live_before = []           # (watch) per pass: bounds were there before it
        self.voided = []                # (watch) (step index, bounds left) directly behind every insert, prune, commit and sweep

    def close(self):
        self.ctx.close()
        for pin in self.pins:
            pin.close()

    def _bounds_left(self):
        return len(self.ctx.bounds_download())

    def step(self, i, step):
        ctx, kind = self.ctx, step[0]
        if kind == "sweep":
            self.sweep = sw = ps.sweep_of(self.scene, step)
            if step[4] == "swap":
                pin = srl.PinnedArray(sw["raw"].shape); pin.array[:] = sw["raw"]
                self.pins.append(pin)
                ctx.sweep_prefetch(pin.array); ctx.sweep_swap()
            else:
                ctx.sweep_upload(sw["raw"])
            rec = None
        elif kind == "opts":
            self.o = ps.opts_dict(step)
            self.opts = srl.default_opts(select_mode=self.o["select_mode"], **ps.opt_kwargs(self.o))
            return None
        elif kind == "pass":
            if self.watch:
                self.live_before.append(self._bounds_left() > 0)
            if self.taps != step[3]:
                ctx.set_taps(step[3]); self.taps = step[3]
            # nothing but this call between two passes without taps: a launch armed behind the one before is fired or cancelled HERE
            neq, rc = ctx.build_residuals(capi.make_frame(step[1], step[2], self.sweep["t_last"], frame_id=self.o["frame_id"]), self.opts)
            rec = dict(neq=neq, rc=rc)
            if step[3]:
                ids, status, ncand = ctx.fetch_neighbors(K=self.o["K"])
                rec.update(ids=ids, status=status, ncand=ncand, **ctx.fetch_residuals())
            return rec
        elif kind == "insert":
            rec = dict(added=ctx.map_insert(ps.insert_points(self.scene, step)))
        elif kind == "prune":
            rec = dict(removed=ctx.map_remove_far(step[1], step[2]))
        elif kind == "commit":
            raw, q, t = ps.commit_frame(self.scene, step)
            ctx.frame_upload(raw)
            world, _ = ctx.frame_commit(q, t, want_world=True, want_added=False)           # deferred: settled by whoever needs the map next
            rec = dict(world=world)
        elif kind == "search":
            ids, xyz, nf = ctx.search_neighbors(np.array(step[1]), nb=self.o["nb"], K=self.o["K"], thr=self.o["thr"])
            return dict(ids=ids, xyz=xyz, nf=nf)
        elif kind == "end":
            ctx.solve_end() if step[1] == "solve_end" else ctx.disarm()
            return None
        if self.watch:
            self.voided.append((i, self._bounds_left()))
        if kind in ("insert", "prune"):
            rec["map"] = ctx.map_download()
        return rec

    def run(self, steps):
        records, commit_at = [None] * len(steps), None
        for i, step in enumerate(steps):
            try:
                records[i] = self.step(i, step)
                if step[0] == "commit":
                    commit_at = i
                elif step[0] in ("insert", "prune"):
                    commit_at = None                                                         # this edit's map holds the commit's points too
                elif step[0] == "pass" and commit_at is not None:                            # the pass directly behind a commit has run
                    records[commit_at]["map"] = self.ctx.map_download()
                    commit_at = None
            except Exception as e:
                which = "WATCHED" if self.watch else "FAST" if self.fast else "PLAIN"
                raise AssertionError(_where(self.scene, steps, i, f"{which} run: {type(e).__name__}: {e}")) from e
        if commit_at is not None:                                                            # (a prefix that ends behind a commit)
            records[commit_at]["map"] = self.ctx.map_download()
        return records


def _where(scene, steps, i, what):
    return f"seed {scene['seed']}, step [{i}] {steps[i]!r}: {what}\nscene = {scene!r}\nsteps = [\n{ps.format_steps(steps, i)}\n]"


def _oracle_ref(o):
    ref = {f"x_one_{k}": v for k, v in o.items() if isinstance(v, np.ndarray)}
    ref.update(x_one_num_ties=o["neq"].num_ties, x_one_num_residuals=o["neq"].num_residuals, x_one_success=o["neq"].success, x_one_loss=o["neq"].loss_sum)
    return ref


def _check_pass(f, p, o, step, max_res):
    assert f["rc"] == p["rc"], ("return code", f["rc"], p["rc"])
    _same((f["neq"], f.get("ids")), (p["neq"], p.get("ids")), "FAST != PLAIN")
    for k in NEQ_FIELDS:
        assert getattr(f["neq"], k) == getattr(p["neq"], k), ("FAST != PLAIN", k, getattr(f["neq"], k), getattr(p["neq"], k))
    assert f["rc"] == 0 and o["neq"].nan_error == 0
    if step[3]:
        for k in ("ids", "status", "ncand") + RESIDUAL_ARRAYS:
            assert f[k].tobytes() == p[k].tobytes(), ("FAST != PLAIN", k, int(np.count_nonzero(f[k] != p[k])))
        check_pass_against(f, _oracle_ref(o), "x")
    else:                                                 # no taps: what the pass returns, against the oracle all the same
        assert f["neq"].num_residuals == o["neq"].num_residuals and f["neq"].success == o["neq"].success
        assert rel(np.array(f["neq"].HtH).reshape(6, 6), o["HtH"]) < TIGHT and rel(np.array(f["neq"].Hth), o["Hth"]) < TIGHT
        assert rel(f["neq"].loss_sum, o["neq"].loss_sum) < TIGHT
    assert f["neq"].last_visited == o["neq"].num_visited - 1
    if max_res == INT_MAX:
        assert f["neq"].sum_candidates == o["neq"].sum_candidates


def _check_map(f, p, want):
    for a, b in zip(f["map"], p["map"]):
        assert a.tobytes() == b.tobytes(), "maps of FAST and PLAIN differ"
    for a, b, name in zip(f["map"], want, ("keys", "counts", "xyz")):
        assert np.array_equal(a, b), f"the device map differs from the oracle's in {name}"


def run_script(script, oracle_lib, backend, guards=True):
    """PLAIN, FAST, a watched FAST run and ORACLE over a script (or a prefix of one: guards=False); returns the seconds the device runs took"""
    scene, steps = script["scene"], script["steps"]
    trace = []
    ps.run_on_oracle(script, oracle_lib, backend, trace=trace)
    start_map = ps.start_map(scene, oracle_lib, backend)
    t0 = time.perf_counter()
    runs = {}
    for name, fast, watch in (("plain", False, False), ("fast", True, False), ("watch", True, True)):      # one after the other: see the docstring
        run = DeviceRun(scene, start_map, fast, watch)
        try:
            runs[name] = (run, run.run(steps))
            if name == "fast":
                fired = run.ctx.arm_stats()["fired"]
                final_map = run.ctx.map_download()
                records = run.ctx.neighbour_records_download()
        finally:
            run.close()
    seconds = time.perf_counter() - t0
    (plain, rec_p), (fast, rec_f), (watch, rec_w) = runs["plain"], runs["fast"], runs["watch"]
    o = None
    for i, step in enumerate(steps):
        try:
            f, p, want = rec_f[i], rec_p[i], trace[i]
            if step[0] == "opts":
                o = ps.opts_dict(step)
            elif step[0] == "pass":
                _check_pass(f, p, want, step, o["max_res"])
            elif step[0] == "insert":
                assert f["added"] == p["added"]
                _check_map(f, p, want)
            elif step[0] == "prune":
                assert f["removed"] == p["removed"] == want[1]
                _check_map(f, p, want[0])
            elif step[0] == "commit":
                assert f["world"].tobytes() == p["world"].tobytes()
                raw, q, t = ps.commit_frame(scene, step)
                assert np.array_equal(f["world"], oracle_lib.transform_points(raw, q, t, backend=backend)), "the committed frame's world points"
                if "map" in f:                                # downloaded behind the pass that follows -- or left to the map edit in between
                    _check_map(f, p, want)
            elif step[0] == "search":
                for k in ("ids", "xyz", "nf"):
                    assert f[k].tobytes() == p[k].tobytes(), ("search: FAST != PLAIN", k)
                for q, r in enumerate(want):
                    assert f["nf"][q] == r["n"] and np.array_equal(f["ids"][q, : r["n"]], r["ids"]), ("search", q)
                    assert np.array_equal(f["xyz"][q, : r["n"]].astype(np.float64), r["xyz"]), ("search", q)
        except AssertionError as e:
            raise AssertionError(_where(scene, steps, i, e)) from e
    last = len(steps) - 1
    want = _model(final_map[0], final_map[1])
    assert np.array_equal(records, want), _where(scene, steps, last, f"at the end the neighbour records differ from the model at (voxel, word) {np.argwhere(records != want)[:6].tolist()}")
    for i, step in enumerate(steps):                      # the watched run computed the same (its armed launches aside, it IS the FAST run)
        if step[0] == "pass":
            assert rec_w[i]["rc"] == rec_f[i]["rc"] and np.array_equal(np.array(rec_w[i]["neq"].HtH), np.array(rec_f[i]["neq"].HtH)), _where(scene, steps, i, "the watched run differs")
    if guards:
        what = "the run did not exercise the carried state: "
        passes = [i for i, s in enumerate(steps) if s[0] == "pass"]
        assert len(watch.live_before) == len(passes) and 3 * sum(watch.live_before) >= len(passes), _where(scene, steps, last, what + f"bounds before the passes {watch.live_before}")
        edits = sum(s[0] in ("insert", "prune", "commit", "sweep") for s in steps)
        assert len(watch.voided) == edits, _where(scene, steps, last, what + "an edit went unwatched")
        for i, left in watch.voided:
            assert left == 0, _where(scene, steps, i, f"bounds of {left} keypoints left behind this step")
        assert fired > 0, _where(scene, steps, last, what + "no armed launch was fired")
    return seconds


@pytest.mark.parametrize("seed", ps.committed_seeds(CASES))
def test_a_random_script_on_one_live_context(oracle_lib, oracle_backend, seed):
    script = ps.make_script(seed)
    seconds = run_script(script, oracle_lib, oracle_backend)
    print(f"seed {seed}: {len(script['steps'])} steps, the three device runs took {seconds:.2f} s")
