"""The scripts of tests/pass_script.py can catch what they are for -- shown from the generator and the CPU oracle alone, for every committed
seed (the first 12, or as many as SRL_FUZZ_CASES asks for: the long form of tests/test_gpu_pass_script.py runs those).

  coverage     every step kind, every option value, both sweep directions; an edit is followed by a pass before the next edit of its kind
  edits count  the oracle pass behind every answer-changing edit (held-back and growing inserts, prunes, commits, new sweeps, options that
               change K, layers or threshold as the pass reads them) differs from the pass computed as if the edit had not happened -- in ids of
               a visited keypoint, status or num_residuals; the far cluster, `search` and a sweep uploaded again leave it as it was
  no excuses   no pass meets a NaN planarity, no accepted keypoint has a degenerate plane (eigen-gap below test_gpu_parity's limit): the
               device test skips nothing and masks nothing
  mistakes     six interpreters that each make one mistake stale carried state would make, and only where carried state could make it (the
               sweep stayed, a pass ran on it before, nothing else voided what that pass learnt): every one differs from the truth somewhere
"""
import os

import numpy as np
import pytest

import pass_script as ps
from test_gpu_parity import eigen_gap

CASES = int(os.environ.get("SRL_FUZZ_CASES", "12"))
SEEDS = ps.committed_seeds(CASES)
GAP_LIMIT = 1e-6          # tests/test_gpu_parity.py: well = ~(gap < 1e-6)
MUST_CHANGE = ("sweep:upload", "sweep:swap", "insert:held", "insert:grow", "prune", "commit")
MUST_NOT_CHANGE = ("sweep:again", "insert:far", "search")


def differs(a, b):
    """two passes give different answers: ids on a visited keypoint, status or num_residuals (over the keypoints both have)"""
    n = min(len(a["status"]), len(b["status"]))
    if int(a["neq"].num_residuals) != int(b["neq"].num_residuals) or not np.array_equal(a["status"][:n], b["status"][:n]):
        return True
    visited = a["status"][:n] != 3
    return a["ids"].shape[1] != b["ids"].shape[1] or not np.array_equal(a["ids"][:n][visited], b["ids"][:n][visited])


def gaps(ids, map_xyz):
    """eigen_gap of tests/test_gpu_parity.py, all rows at once -- and over the neighbours a row has where it has fewer than K (eigen_gap leaves
    those rows out)"""
    valid = (ids >= 0)[..., None]
    P = np.asarray(map_xyz, np.float64).reshape(-1, 3)[np.maximum(ids, 0)]
    E = (P - (P * valid).sum(1, keepdims=True) / valid.sum(1, keepdims=True)) * valid
    w = np.linalg.eigvalsh(np.einsum("nki,nkj->nij", E, E))
    return (w[:, 1] - w[:, 0]) / np.maximum(w[:, 2], 1e-300)


def analyse(script, po, backend):
    """the true run of a script on the oracle and, for every edit, the next pass computed as if that edit had not happened"""
    steps = script["steps"]
    run = ps.OracleRun(script["scene"], po, backend)
    trace, edits, min_gap, checked_gap = [], [], np.inf, False
    for i, step in enumerate(steps):
        kind = ps.edit_kind(step)
        if kind is not None and run.sweep is not None and run.opts is not None:
            j = next(k for k in range(i + 1, len(steps)) if steps[k][0] == "pass")
            if kind == "opts":
                new = ps.opts_dict(step)
                must = True if ps.effective(new) != ps.effective(run.opts) else (False if new["max_res"] == run.opts["max_res"] else None)
            else:
                must = kind in MUST_CHANGE
            alt = run.fork()
            for k in range(i + 1, j + 1):
                without = alt.step(steps[k])
            edits.append(dict(index=i, kind=kind, next_pass=j, must=must, without=without))
        rec = run.step(step)
        trace.append(rec)
        if step[0] == "pass":
            acc = rec["status"] == 2
            if acc.any():
                g = gaps(rec["ids"][acc], run.map.export()[2])
                if not checked_gap:                      # the batched restatement is test_gpu_parity.eigen_gap
                    theirs = eigen_gap(rec["ids"][acc][:50], run.map.export()[2])
                    assert np.allclose(g[:50][~np.isnan(theirs)], theirs[~np.isnan(theirs)], rtol=1e-9, atol=1e-12)
                    checked_gap = True
                min_gap = min(min_gap, float(g.min()))
    for e in edits:
        e["changed"] = differs(trace[e["next_pass"]], e.pop("without"))
    grows = [g for g, s in zip(run.grew, [s for s in steps if s[0] == "insert"]) if s[1] == "grow"]
    return dict(script=script, trace=trace, edits=edits, min_gap=min_gap, grows=grows)


@pytest.fixture(scope="module")
def runs(oracle_lib, oracle_backend):
    return {seed: analyse(ps.make_script(seed), oracle_lib, oracle_backend) for seed in SEEDS}


def test_scripts_are_replayable_values():
    for seed in SEEDS[:3]:
        a = ps.make_script(seed)
        scene, steps = ps._make_script.__wrapped__(seed)                               # drawn again, not remembered
        assert a == dict(scene=scene, steps=list(steps))
        assert eval(repr(a["steps"])) == a["steps"]                                   # plain tuples: print, paste, replay


def test_coverage():
    kinds, values, hows, total_passes, taps_on = {}, {f: set() for f in ps.OPT_FIELDS}, set(), 0, 0
    sizes, patterns, map_pts, culls, armeds, ends = set(), set(), set(), set(), set(), set()
    for seed in SEEDS:
        script = ps.make_script(seed)
        steps, scene = script["steps"], script["scene"]
        map_pts.add(scene["map_pts"]); culls.add(scene["cull"]); armeds.add(scene["armed"])
        passes = [s for s in steps if s[0] == "pass"]
        assert 25 <= len(steps) <= 40 and 12 <= len(passes) <= 20, seed
        assert steps[0][0] == "sweep" and steps[1][0] == "opts", seed
        total_passes += len(passes); taps_on += sum(s[3] for s in passes)
        news = [s[2] for s in steps if s[0] == "sweep" and s[4] != "again"]
        assert any(b < a for a, b in zip(news, news[1:])) and any(b > a for a, b in zip(news, news[1:])), (seed, "a shrink and a grow")
        waiting = set()                               # edit kinds not yet followed by a pass
        for s in steps:
            kind = ps.edit_kind(s)
            if s[0] == "pass":
                waiting.clear()
            elif kind is not None:
                assert kind not in waiting, (seed, kind, "twice without a pass between")
                waiting.add(kind)
                kinds[kind] = kinds.get(kind, 0) + 1
            if s[0] == "opts":
                for f, v in ps.opts_dict(s).items():
                    values[f].add(v)
            if s[0] == "sweep":
                sizes.add(s[2]); patterns.add(s[3]); hows.add(s[4])
            if s[0] == "end":
                ends.add(s[1])
        assert not waiting, (seed, "the script ends with a pass or an `end`")
        # a run that armed launches can fire in: 4 096 keypoints (sixteen-wave workgroups), the fast selection path, no taps, back to back
        quiet, best, n_cur, sel = 0, 0, 0, 0
        for s in steps:
            if s[0] == "sweep":
                n_cur = s[2]
            if s[0] == "opts":
                sel = s[6]
            quiet = quiet + 1 if (s[0] == "pass" and not s[3] and n_cur >= 2048 and sel == 0) else 0
            best = max(best, quiet)
        assert best >= 2, seed
    assert set(kinds) == set(ps.EDIT_KINDS) and min(kinds.values()) >= 2, kinds
    assert values == dict(K=set(ps.OPT_K), max_res=set(ps.OPT_MAX_RES), thr=set(ps.OPT_THR), nb=set(ps.OPT_NB), frame_id=set(ps.OPT_FRAME_ID),
                          select_mode=set(ps.OPT_SELECT)), values
    assert sizes == set(ps.SWEEP_N) and patterns == set(ps.PATTERNS) and hows == set(ps.HOWS) and ends == {"solve_end", "disarm"}
    assert map_pts == set(ps.MAP_PTS) and culls == {1, 2} and armeds == {1, 2}
    assert 0.45 < taps_on / total_passes < 0.75, taps_on / total_passes              # about two in three, the quiet runs taken off


def test_every_answer_changing_edit_changes_the_answer(runs):
    seen = {}
    for seed, r in runs.items():
        for e in r["edits"]:
            what = (seed, e["index"], r["script"]["steps"][e["index"]], "next pass", e["next_pass"])
            if e["must"] is True:
                assert e["changed"], ("the pass behind this edit is the pass without it", what)
            elif e["must"] is False:
                assert not e["changed"], ("this step must leave the answer alone", what)
            if e["must"] is not None:
                seen[e["kind"], e["must"]] = seen.get((e["kind"], e["must"]), 0) + 1
        assert all(r["grows"]), (seed, "a growing insert stayed within the modelled reserve", r["grows"])
    for kind in MUST_CHANGE + ("opts",):
        assert seen.get((kind, True), 0) >= 2, (kind, seen)
    for kind in MUST_NOT_CHANGE:
        assert seen.get((kind, False), 0) >= 2, (kind, seen)


def test_no_pass_meets_a_nan_planarity_or_a_degenerate_plane(runs):
    for seed, r in runs.items():
        for i, (step, rec) in enumerate(zip(r["script"]["steps"], r["trace"])):
            if step[0] == "pass":
                assert rec["neq"].nan_error == 0 and rec["rc"] == 0, (seed, i)
        assert r["min_gap"] >= GAP_LIMIT, (seed, r["min_gap"])


@pytest.mark.parametrize("mistake", ps.MISTAKES)
def test_one_mistake_variants_differ_from_the_truth(runs, oracle_lib, oracle_backend, mistake):
    caught = []
    for seed, r in runs.items():
        got = ps.run_on_oracle(r["script"], oracle_lib, oracle_backend, mistake=mistake, reference=r["trace"])
        want = [rec for step, rec in zip(r["script"]["steps"], r["trace"]) if step[0] == "pass"]
        assert len(got) == len(want)
        caught += [(seed, k) for k, (g, w) in enumerate(zip(got, want)) if g is not w and differs(g, w)]
    assert caught, f"no pass of any committed script tells `{mistake}` from the truth: the scripts are too tame"
