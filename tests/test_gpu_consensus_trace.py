"""Every hypothesis of the consensus estimators (srl_consensus_fundamental, srl_consensus_pnp) against the contract of include/srlivo_hip.h,
through the read-back of the last call (srl_debug_consensus_download): tests/test_gpu_consensus.py sees the winner alone, and on a scene
with one consensus dozens of hypotheses produce it.

1. The usable list is the ascending list of finite points, and EVERY hypothesis' sample is the contract's draw(seed, h, k, m) sequence
   mapped through it (tests/consensus_checker.py restates the generator from the header's text).
2. Hartley's normalisation is the checker's float64 centroid and sqrt 2 / mean distance.
3. EVERY valid slot's count is the number of ones of the checker's mask of that slot's model; every invalid slot holds -1 and zeros.
4. The winner is the first index of the maximum of the device's own counts, and the result record follows from it; on the scenes with
   one consensus several models share the maximum, and for two cases a later one of them sits in a lower thread of the pick kernel.
5. No solution is lost: a hypothesis sampled inside the truth inliers has a slot with the truth mask; the number of valid slots of a
   fundamental hypothesis is the number of real solutions of the checker's own 7-point solver; every pose fits its sample.
6. The scoring loops at the edges of their tiles (64 lanes, 256 threads, 1024-point chunks), and a workspace that an earlier, larger call
   or a call of the other model has used."""
import numpy as np
import pytest

import consensus_checker as ck
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
F_THR, P_THR = 1.0, 1.5
F_CONF, P_CONF = 0.997, 0.99            # the defaults of srl_consensus_opts_default


@pytest.fixture(scope="module")
def ctx():
    c = srl.Context(0)
    yield c
    c.close()


def _is_f(name):
    return name.startswith("f")


def _call(c, name, scene, **kw):
    """(mask (n,) uint8, ascending inlier list, result, read-back)"""
    if _is_f(name):
        mask, res = c.consensus_fundamental(scene[0], scene[1], **kw)
        idx = np.flatnonzero(mask).astype(np.int32)
    else:
        idx, res = c.consensus_pnp(scene[0], scene[1], ck.K, **kw)
        mask = np.zeros(len(scene[0]), np.uint8)
        mask[idx] = 1
    return mask, idx, res, c.debug_consensus_download()


def _error(name, scene, model):
    """(the checker's mask of a model, its error per point, threshold^2)"""
    if _is_f(name):
        err, t2 = ck.error_fundamental(model[:9], scene[0], scene[1]), F_THR * F_THR
        with np.errstate(invalid="ignore"):
            return err <= t2, err, t2
    (err, z), t2 = ck.error_pnp(model[:9], model[9:], ck.K, scene[0], scene[1]), P_THR * P_THR
    with np.errstate(invalid="ignore"):
        return (z > 0) & (err <= t2), err, t2


def _near_threshold(err, t2):
    """the points the allowance of tests/test_gpu_consensus.py's _self_consistent covers: within 4 ulp of threshold^2"""
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(np.abs(err - t2) <= 4 * np.spacing(t2))


def _check_call(name, scene, seed, H, out, rows=None):
    """items 1 to 4 for one call; rows: the contract's sample rows, where the caller has them already.  Returns the flat counts."""
    mask, idx, res, tr = out
    n, S, slots = len(scene[0]), (7 if _is_f(name) else 3), (3 if _is_f(name) else 4)
    assert (tr["model"], tr["hypotheses"], tr["n"], tr["slots"]) == (capi.SRL_CONSENSUS_FUNDAMENTAL if _is_f(name) else capi.SRL_CONSENSUS_PNP, H, n, slots)
    # 1. the usable list and every sample
    usable = ck.usable_points(scene[0], scene[1])
    assert tr["usable"].dtype == np.int32 and np.array_equal(tr["usable"], usable), name
    if rows is None:
        rows = np.array([ck.sample_indices(seed, h, usable, S) for h in range(H)])
    assert tr["samples"].shape == (H, 8) and np.array_equal(tr["samples"], rows[:H]), (name, np.flatnonzero((tr["samples"] != rows[:H]).any(axis=1))[:8])
    # 2. the normalisation: sums of n positive terms (pixels up to 640) in another order differ by n 2^-53 relative; the mean distance
    # inherits the centroid's error scaled by 640 / (mean distance) < 10: 1e-12 holds it for n <= 1025
    if _is_f(name):
        want = ck.hartley_values(scene[0], scene[1], usable)
        print(name, "normalisation: largest relative difference", np.abs(tr["norm"] / want - 1.0).max())
        assert (np.abs(tr["norm"] - want) <= 1e-12 * np.abs(want)).all(), (tr["norm"], want)
    else:
        assert (tr["norm"] == 0).all()
    # 3. the count of every slot
    counts, models = tr["counts"].reshape(-1), tr["models"].reshape(-1, 12)
    assert counts.shape == (H * slots,) and np.isfinite(models).all()
    none = counts < 0
    assert (counts[none] == -1).all() and (models[none] == 0).all(), name
    for m in np.flatnonzero(~none):
        want_mask, err, t2 = _error(name, scene, models[m])
        if int(want_mask.sum()) != counts[m]:
            near = _near_threshold(err, t2)
            print("count of model", m, "device", counts[m], "checker", int(want_mask.sum()), "points within 4 ulp of the threshold:", near, err[near])
            assert abs(int(want_mask.sum()) - int(counts[m])) <= min(len(near), 1), (name, m, counts[m], int(want_mask.sum()))
        if _is_f(name):
            assert (models[m, 9:] == 0).all()
    # 4. the winner: the first index of the maximum of the device's own counts, and the record
    assert res.models_valid == int((~none).sum()) and res.reserved == 0
    if none.all():
        assert (res.hypothesis, res.slot, res.inliers, res.confidence_reached) == (-1, -1, 0, 0) and not mask.any() and len(idx) == 0
        assert (res.model_array() == 0).all() and (res.sample_array() == -1).all()
        return counts
    win = int(np.argmax(counts))                                    # NumPy's argmax is the FIRST index of the maximum
    assert res.hypothesis * slots + res.slot == win and 0 <= res.slot < slots, (name, res.hypothesis, res.slot, win, counts[win])
    assert res.model_array().tobytes() == models[win].tobytes()
    assert np.array_equal(res.sample_array(), tr["samples"][win // slots])
    assert res.inliers == counts[win] == int(mask.sum())
    assert res.confidence_reached == ck.confidence_reached(res.inliers, n, S, H, F_CONF if _is_f(name) else P_CONF)
    want_mask, err, t2 = _error(name, scene, models[win])
    bad = np.flatnonzero(want_mask != (mask == 1))
    if len(bad):
        print("the winner's mask differs from the checker's at", bad, err[bad])
    assert len(bad) <= 1 and set(bad.tolist()) <= set(_near_threshold(err, t2).tolist()), (name, bad, err[bad])
    assert idx.dtype == np.int32 and np.array_equal(idx, np.flatnonzero(mask))
    return counts


# ------------------------------------------------------------------------------------------------ every hypothesis of the scenes
@pytest.mark.parametrize("seed", ck.TRACE_SEEDS)
@pytest.mark.parametrize("H", ck.TRACE_H)
@pytest.mark.parametrize("name", ck.TRACE_FUNDAMENTAL + ck.TRACE_PNP)
def test_every_hypothesis(ctx, name, H, seed):
    scene = ck.trace_scene(name)
    S, slots = (7, 3) if _is_f(name) else (3, 4)
    out = _call(ctx, name, scene, hypotheses=H, seed=seed)
    mask, idx, res, tr = out
    counts = _check_call(name, scene, seed, H, out, rows=ck.trace_samples(name, seed, H)[1])
    models = tr["models"]
    valid = (tr["counts"] >= 0).sum(axis=1)
    # the confidence flag takes both values: one hypothesis can never reach it on a scene with 35 % outliers, 512 do
    if name in ck.TRACE_EXACT and H == 1:
        assert res.confidence_reached == 0
    if name in ck.TRACE_EXACT and H == 512:
        assert res.confidence_reached == 1 and np.array_equal(mask, scene[2])
    # 5. no solution is lost
    if name in ck.TRACE_EXACT:
        complete = ck.trace_complete(name, seed, H)
        for h in complete:
            hit = [s for s in range(slots) if tr["counts"][h, s] >= 0 and np.array_equal(_error(name, scene, models[h, s])[0], scene[2] == 1)]
            assert hit, (name, seed, h, tr["samples"][h], tr["counts"][h])
        if len(complete) >= 2:                                      # the tie rule is exercised: several models share the maximum
            assert int((counts == counts.max()).sum()) >= 2 and counts.max() == int(scene[2].sum())
    if (name, seed, H) in ck.TRACE_TIE_CASES:
        top = np.flatnonzero(counts == counts.max())
        print(name, "maximal models", top[:12], "their threads in the pick kernel", top[:12] % 256)
        assert (top[1:] % 256 < top[0] % 256).any(), top
    if _is_f(name):
        ref = ck.trace_seven_point(name, seed, H)
        excused = [h for h in range(H) if ref[h][1]]
        assert len(excused) <= 0.02 * H, (name, seed, H, excused)
        wrong = [(h, int(valid[h]), ref[h][0]) for h in range(H) if not ref[h][1] and valid[h] != ref[h][0]]
        assert not wrong, (name, seed, wrong[:8])
    else:
        for h, s in zip(*np.nonzero(tr["counts"] >= 0)):
            pick = tr["samples"][h, :3]
            fit = ck.p3p_residual(models[h, s, :9], models[h, s, 9:], ck.K, scene[0][pick], scene[1][pick])
            assert fit <= 1e-6, (name, seed, h, s, fit)


# ------------------------------------------------------------------------------------------------ 6. tile edges and a used workspace
def _tiled(name, n):
    """the first n points of jittered copies of a 256-point scene, as tests/test_gpu_consensus.py builds its point-limit case"""
    rng = np.random.default_rng(3)
    rep = 5
    jig = rng.uniform(-0.2, 0.2, (256 * rep, 2)).astype(np.float32)
    a, b, _ = ck.scene_fundamental(41, 256, 64) if _is_f(name) else ck.scene_pnp(42, 256, 64)
    return np.tile(a, (rep, 1))[:n].copy(), (np.tile(b, (rep, 1)) + jig)[:n].copy(), None


@pytest.mark.parametrize("n", [8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
@pytest.mark.parametrize("name", ["f_tiled", "p_tiled"])
def test_the_edges_of_the_scoring_loops(ctx, name, n):
    scene = _tiled(name, n)
    counts = _check_call(name, scene, 0, 8, _call(ctx, name, scene, hypotheses=8, seed=0))
    print(name, n, "counts", counts)
    assert (counts >= 0).any()


def _same(a, b):
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and bytes(a[2]) == bytes(b[2])
    assert sorted(a[3]) == sorted(b[3])
    for k, v in a[3].items():
        assert (v.tobytes() == b[3][k].tobytes() and v.shape == b[3][k].shape) if isinstance(v, np.ndarray) else v == b[3][k], k


STALE = {
    "fewer_hypotheses_f": (("f120", dict(hypotheses=512, seed=0)), ("f120", dict(hypotheses=8, seed=0))),
    "fewer_hypotheses_p": (("p120", dict(hypotheses=512, seed=0)), ("p120", dict(hypotheses=8, seed=0))),
    "the_other_model": (("f120", dict(hypotheses=512, seed=1)), ("p60", dict(hypotheses=64, seed=1))),
    "the_other_model_back": (("p120", dict(hypotheses=512, seed=1)), ("f60", dict(hypotheses=64, seed=1))),
    "fewer_points_f": (("f_tiled1025", dict(hypotheses=64, seed=2)), ("f_tiled8", dict(hypotheses=64, seed=2))),
    "fewer_points_p": (("p_tiled1025", dict(hypotheses=64, seed=2)), ("p_tiled8", dict(hypotheses=64, seed=2))),
}


def _stale_scene(name):
    if "_tiled" in name:
        return _tiled(name, int(name.split("_tiled")[1]))
    if name.endswith("60"):
        a, b, truth = ck.trace_scene(name[0] + "120")
        return a[:60], b[:60], truth[:60]
    return ck.trace_scene(name)


@pytest.mark.parametrize("case", sorted(STALE))
def test_a_call_ignores_what_the_workspace_held(case):
    """the workspace is shared by both models and never cleared: the second call on a used context is, byte for byte, the same call on
    a fresh one -- result, mask, list and every hypothesis of the read-back"""
    (first, kw1), (second, kw2) = STALE[case]
    used, fresh = srl.Context(0), srl.Context(0)
    try:
        with pytest.raises(srl.SrlError) as e:                      # no call yet: nothing to read back
            fresh.debug_consensus_download()
        assert e.value.status == capi.SRL_ERR_NO_MAP
        _call(used, first, _stale_scene(first), **kw1)
        scene = _stale_scene(second)
        a, b = _call(used, second, scene, **kw2), _call(fresh, second, scene, **kw2)
        _same(a, b)
        _check_call(second, scene, kw2["seed"], kw2["hypotheses"], a)
        # a call too small to run on the device leaves the read-back of the call before it
        tiny = used.consensus_fundamental(scene[0][:3], scene[1][:3]) if _is_f(second) else used.consensus_pnp(scene[0][:3], scene[1][:3], ck.K)
        assert tiny[1].models_valid == 0
        again = used.debug_consensus_download()
        assert all((v.tobytes() == again[k].tobytes()) if isinstance(v, np.ndarray) else v == again[k] for k, v in a[3].items())
    finally:
        used.close()
        fresh.close()


def test_the_read_back_refuses_too_little_room(ctx):
    import ctypes as C
    scene = ck.trace_scene("f120")
    ctx.consensus_fundamental(scene[0], scene[1], hypotheses=22)
    info = capi.DebugConsensusInfo()
    usable, samples, models, counts = np.full(120, 7, np.int32), np.full((22, 8), 7, np.int32), np.full(22 * 3 * 12, 7.0), np.full(22 * 3, 7, np.int32)
    args = lambda **kw: [kw.get(k, v) for k, v in (("info", C.byref(info)), ("usable", capi._ptr(usable)), ("pc", 120), ("samples", capi._ptr(samples)),      # noqa: E731
                                                    ("models", capi._ptr(models)), ("counts", capi._ptr(counts)), ("hc", 22))]
    for kw in (dict(pc=119), dict(hc=21), dict(info=None), dict(usable=None), dict(samples=None), dict(models=None), dict(counts=None)):
        assert ctx.lib.srl_debug_consensus_download(ctx.h, *args(**kw)) == capi.SRL_ERR_BAD_ARG, kw
        assert (usable == 7).all() and (samples == 7).all() and (models == 7).all() and (counts == 7).all()
    assert ctx.lib.srl_debug_consensus_download(ctx.h, *args()) == capi.SRL_OK          # exactly enough room
    assert (info.hypotheses, info.n, info.slots, info.usable) == (22, 120, 3, 120) and np.array_equal(usable, np.arange(120))
    assert np.array_equal(samples, ck.trace_samples("f120", 0, 22)[1])
