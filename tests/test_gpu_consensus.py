"""The consensus estimators of the camera tracker on the device (srl_consensus_fundamental, srl_consensus_pnp) by their properties, against
the independent restatement of tests/consensus_checker.py -- there is no OpenCV to compare with, and the contract claims none.

1. On scenes whose consensus is unique (validated on the CPU by tests/test_consensus_checker.py) the mask is the ground truth.
2. On EVERY scene the returned mask is, bit for bit, `error(model) <= threshold^2` as the checker evaluates it in float64 from the returned
   model: the device's scoring is the documented operation order and nothing else.
3. The model fits its own sample, is a fundamental matrix (rank 2, unit norm) or a rotation, and the sample is 7 or 3 distinct indices.
4. Same inputs, same bytes; another seed, another winning hypothesis with the same mask.
5. Edges: too few points, every sample degenerate, NaN coordinates, one hypothesis, the point limit, more than one rank.
6. The loop of imageProcessing::process through the host mirror with the device estimators in place of the all-ones stand-ins."""
import ctypes as C

import numpy as np
import pytest

import consensus_checker as ck
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
F_THR, P_THR = 1.0, 1.5


@pytest.fixture(scope="module")
def ctx():
    c = srl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes():
    s = {}
    for name, (seed, n, n_out, noise) in ck.FUNDAMENTAL_SCENES.items():
        s[name] = ck.scene_fundamental(seed, n, n_out, noise)
    for name, (seed, n, n_out, noise) in ck.PNP_SCENES.items():
        s[name] = ck.scene_pnp(seed, n, n_out, noise)
    s["f_planar"] = ck.scene_fundamental(14, 120, 42, 0.0, planar=True)
    s["p_planar"] = ck.scene_pnp(24, 120, 48, 0.0, planar=True)
    a, b, X, uv = ck.scene_all_outliers(31, 90)
    s["f_random"], s["p_random"] = (a, b, None), (X, uv, None)
    return s


def _is_f(name):
    return name.startswith("f")


def _run(ctx, name, scene, **kw):
    """(mask (n,) uint8, ascending inlier list, result)"""
    if _is_f(name):
        mask, res = ctx.consensus_fundamental(scene[0], scene[1], **kw)
        return mask, np.flatnonzero(mask).astype(np.int32), res
    idx, res = ctx.consensus_pnp(scene[0], scene[1], ck.K, **kw)
    mask = np.zeros(len(scene[0]), np.uint8)
    mask[idx] = 1
    return mask, idx, res


def _self_consistent(name, scene, mask, res, Kc=ck.K):
    """the mask is error(model) <= threshold^2, bit for bit; a point within 4 ulp of the threshold may differ, one per scene at most"""
    model = res.model_array()
    if _is_f(name):
        err, t2 = ck.error_fundamental(model[:9], scene[0], scene[1]), F_THR * F_THR
        with np.errstate(invalid="ignore"):
            want = err <= t2
    else:
        (err, z), t2 = ck.error_pnp(model[:9], model[9:], Kc, scene[0], scene[1]), P_THR * P_THR
        with np.errstate(invalid="ignore"):
            want = (z > 0) & (err <= t2)
    if res.models_valid == 0:
        want = np.zeros(len(mask), bool)
    bad = np.flatnonzero(want != (mask == 1))
    near = [i for i in bad if abs(err[i] - t2) <= 4 * np.spacing(t2)]
    if len(bad):
        print("self-consistency: differing points", name, bad, err[bad], "within 4 ulp of the threshold:", near)
    assert len(near) == len(bad) and len(bad) <= 1, (name, bad[:8], err[bad][:8])
    assert int(mask.sum()) == res.inliers


# ------------------------------------------------------------------------------------------------ 1. the truth mask
@pytest.mark.parametrize("name", sorted(ck.FUNDAMENTAL_SCENES) + sorted(ck.PNP_SCENES))
def test_the_mask_is_the_ground_truth(ctx, scenes, name):
    scene = scenes[name]
    mask, idx, res = _run(ctx, name, scene)
    print(name, "inliers", res.inliers, "of", len(mask), "hypothesis", res.hypothesis, "slot", res.slot, "models_valid", res.models_valid)
    assert np.array_equal(mask, scene[2]), (name, np.flatnonzero(mask != scene[2]))
    assert np.array_equal(idx, np.flatnonzero(scene[2])) and idx.dtype == np.int32
    assert res.inliers == int(scene[2].sum()) and res.confidence_reached == 1 and res.models_valid > 0
    assert 0 <= res.hypothesis < (512 if _is_f(name) else 200) and 0 <= res.slot < (3 if _is_f(name) else 4) and res.reserved == 0


# ------------------------------------------------------------------------------------------------ 2. self-consistency, 3. the model and its sample
ALL_SCENES = sorted(ck.FUNDAMENTAL_SCENES) + sorted(ck.PNP_SCENES) + ["f_planar", "p_planar", "f_random", "p_random"]


@pytest.mark.parametrize("name", ALL_SCENES)
def test_the_mask_is_the_documented_error_of_the_returned_model(ctx, scenes, name):
    scene = scenes[name]
    mask, idx, res = _run(ctx, name, scene)
    _self_consistent(name, scene, mask, res)
    assert np.array_equal(idx, np.flatnonzero(mask))


@pytest.mark.parametrize("name", ALL_SCENES)
def test_the_model_fits_its_own_sample(ctx, scenes, name):
    scene = scenes[name]
    _, _, res = _run(ctx, name, scene)
    assert res.models_valid > 0
    model, sample = res.model_array(), res.sample_array()
    s = 7 if _is_f(name) else 3
    assert (sample[s:] == -1).all() and len(set(sample[:s].tolist())) == s and sample[:s].min() >= 0 and sample[:s].max() < len(scene[0])
    pick = sample[:s]
    if _is_f(name):
        F = model[:9].reshape(3, 3)
        assert (model[9:] == 0).all() and abs(np.linalg.det(F)) <= 1e-9 and abs(np.linalg.norm(F) - 1.0) <= 1e-12
        got = float(np.max(ck.error_fundamental(F, scene[0][pick], scene[1][pick])))
        sols = ck.seven_point(scene[0][pick], scene[1][pick])
        near = min(sols, key=lambda G: min(np.linalg.norm(G - F), np.linalg.norm(G + F)))
        floor = float(np.max(ck.error_fundamental(near, scene[0][pick], scene[1][pick])))
    else:
        R, t = model[:9].reshape(3, 3), model[9:]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0
        got = ck.p3p_residual(R, t, ck.K, scene[0][pick], scene[1][pick])
        R2, t2 = ck.refine_pose(R, t, ck.K, scene[0][pick], scene[1][pick])
        floor = ck.p3p_residual(R2, t2, ck.K, scene[0][pick], scene[1][pick])
    print(name, "sample", pick, "error on the sample", got, "px^2; the checker's own fit leaves", floor)
    assert got <= max(1e-6, 1e3 * floor), (name, got, floor, pick)


# ------------------------------------------------------------------------------------------------ 4. determinism and the seed
@pytest.mark.parametrize("name", ["f120", "p120"])
def test_same_call_same_bytes_and_another_seed_another_hypothesis(ctx, scenes, name):
    scene = scenes[name]
    a, b = _run(ctx, name, scene), _run(ctx, name, scene)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and bytes(a[2]) == bytes(b[2])
    c = _run(ctx, name, scene, seed=1)
    assert np.array_equal(c[0], a[0]) and c[2].inliers == a[2].inliers
    assert c[2].hypothesis != a[2].hypothesis and c[2].sample_array().tolist() != a[2].sample_array().tolist()
    assert bytes(_run(ctx, name, scene, seed=1)[2]) == bytes(c[2])


# ------------------------------------------------------------------------------------------------ 5. edges
def _empty(res):
    return (res.inliers, res.models_valid, res.confidence_reached, res.hypothesis, res.slot) == (0, 0, 0, -1, -1) and \
        (res.model_array() == 0).all() and (res.sample_array() == -1).all()


def test_too_few_points_is_an_empty_consensus(ctx, scenes):
    x1, x2, _ = scenes["f40"]
    X, uv, _ = scenes["p12"]
    for n in (0, 7):
        mask, res = ctx.consensus_fundamental(x1[:n], x2[:n])
        assert len(mask) == n and not mask.any() and _empty(res)
    for n in (0, 3):
        idx, res = ctx.consensus_pnp(X[:n], uv[:n], ck.K)
        assert len(idx) == 0 and _empty(res)
    # one more point and there is something to agree on
    mask, res = ctx.consensus_fundamental(x1[:8], x2[:8])
    assert res.models_valid > 0
    idx, res = ctx.consensus_pnp(X[:4], uv[:4], ck.K)
    assert res.models_valid > 0


def test_identical_points_give_no_model_and_no_nan(ctx):
    n = 70
    a = np.tile(np.float32([[100.5, 200.25]]), (n, 1))
    mask, res = ctx.consensus_fundamental(a, a + np.float32(3))
    assert not mask.any() and _empty(res) and np.isfinite(res.model_array()).all()
    X = np.tile(np.float32([[1, 2, 8]]), (n, 1))
    idx, res = ctx.consensus_pnp(X, a, ck.K)
    assert len(idx) == 0 and _empty(res) and np.isfinite(res.model_array()).all()


def test_nan_coordinates_are_never_inliers_and_never_sampled(ctx, scenes):
    x1, x2, truth = (v.copy() for v in scenes["f120"])
    hurt = np.flatnonzero(truth)[[0, 17, 40]]
    x1[hurt[0], 0] = np.nan
    x2[hurt[1], 1] = np.inf
    x1[hurt[2]] = np.nan; x2[hurt[2]] = np.nan
    want = truth.copy()
    want[hurt] = 0
    for seed in range(4):
        mask, res = ctx.consensus_fundamental(x1, x2, seed=seed)
        assert np.array_equal(mask, want) and not set(hurt.tolist()) & set(res.sample_array().tolist())
        _self_consistent("f120", (x1, x2), mask, res)
    X, uv, truth = (v.copy() for v in scenes["p120"])
    hurt = np.flatnonzero(truth)[[1, 20, 50]]
    X[hurt[0], 2] = np.nan
    uv[hurt[1], 0] = -np.inf
    X[hurt[2]] = np.nan
    want = truth.copy()
    want[hurt] = 0
    for seed in range(4):
        idx, res = ctx.consensus_pnp(X, uv, ck.K, seed=seed)
        assert np.array_equal(idx, np.flatnonzero(want)) and not set(hurt.tolist()) & set(res.sample_array().tolist())


def test_one_hypothesis(ctx, scenes):
    for name in ("f120", "p120"):
        mask, idx, res = _run(ctx, name, scenes[name], hypotheses=1)
        assert res.hypothesis in (0, -1) and res.models_valid <= (3 if _is_f(name) else 4)
        _self_consistent(name, scenes[name], mask, res)


def test_the_point_limit_runs_and_one_more_is_refused(ctx):
    n = capi.SRL_CONSENSUS_MAX_POINTS
    rng = np.random.default_rng(3)
    x1, x2, truth = ck.scene_fundamental(41, 256, 64)
    rep = n // 256
    jig = rng.uniform(-0.2, 0.2, (n, 2)).astype(np.float32)
    big = (np.tile(x1, (rep, 1)), np.tile(x2, (rep, 1)) + jig)        # sixteen jittered copies: 4096 points, four LDS chunks
    mask, res = ctx.consensus_fundamental(big[0], big[1], hypotheses=64)
    assert len(mask) == n and res.models_valid > 0
    _self_consistent("f4096", big, mask, res)
    X, uv, _ = ck.scene_pnp(42, 256, 64)
    bigp = (np.tile(X, (rep, 1)), np.tile(uv, (rep, 1)) + jig)
    idx, res = ctx.consensus_pnp(bigp[0], bigp[1], ck.K, hypotheses=65)
    pm = np.zeros(n, np.uint8)
    pm[idx] = 1
    _self_consistent("p4096", bigp, pm, res)
    assert (np.diff(idx) > 0).all()
    more = np.zeros((n + 1, 2), np.float32)
    with pytest.raises(srl.SrlError) as e:
        ctx.consensus_fundamental(more, more)
    assert e.value.status == capi.SRL_ERR_BAD_ARG


def test_refusals_with_a_context_and_more_than_one_rank(scenes):
    ctx = srl.Context(0)
    try:
        x1, x2, _ = scenes["f40"]
        X, uv, _ = scenes["p12"]
        for kw in (dict(hypotheses=0), dict(hypotheses=4097), dict(threshold=float("nan")), dict(threshold=0.0), dict(confidence=1.0)):
            with pytest.raises(srl.SrlError) as e:
                ctx.consensus_fundamental(x1, x2, **kw)
            assert e.value.status == capi.SRL_ERR_BAD_ARG
            with pytest.raises(srl.SrlError) as e:
                ctx.consensus_pnp(X, uv, ck.K, **kw)
            assert e.value.status == capi.SRL_ERR_BAD_ARG
        with pytest.raises(srl.SrlError) as e:
            ctx.consensus_pnp(X, uv, [400.0, 0.0, 320.0, 240.0])
        assert e.value.status == capi.SRL_ERR_BAD_ARG
        # each refusal on its own merits, with a live context, through the C-ABI itself: BAD_ARG, the result zeroed, the outputs untouched
        n = len(X)
        a, b = np.ascontiguousarray(x1[:n]), np.ascontiguousarray(x2[:n])
        Kc = np.ascontiguousarray(ck.K)
        zero = bytes(C.sizeof(capi.ConsensusResult))
        nan, inf = float("nan"), float("inf")

        def dirty():
            res = capi.ConsensusResult()
            C.memset(C.byref(res), 0xFF, C.sizeof(res))
            return res

        def fundamental(count=n, last=a, cur=b, out=True, want=capi.SRL_ERR_BAD_ARG, **kw):
            status, res = np.full(n, 7, np.uint8), dirty()
            o = capi.default_consensus_opts(capi.SRL_CONSENSUS_FUNDAMENTAL, **kw)
            rc = ctx.lib.srl_consensus_fundamental(ctx.h, capi._ptr(last), capi._ptr(cur), count, C.byref(o), capi._ptr(status) if out else None, C.byref(res))
            assert rc == want and bytes(res) == zero and (status == 7).all(), (count, kw)

        def pnp(count=n, pts=X, pix=uv, Kp=Kc, out=True, cnt=True, want=capi.SRL_ERR_BAD_ARG, **kw):
            idx, ni, res = np.full(n, 7, np.int32), C.c_int(-77), dirty()
            o = capi.default_consensus_opts(capi.SRL_CONSENSUS_PNP, **kw)
            rc = ctx.lib.srl_consensus_pnp(ctx.h, capi._ptr(pts), capi._ptr(pix), count, capi._dptr(Kp) if Kp is not None else None, C.byref(o),
                                           capi._ptr(idx) if out else None, C.byref(ni) if cnt else None, C.byref(res))
            assert rc == want and bytes(res) == zero and (idx == 7).all() and ni.value == -77, (count, kw)

        for count in (-1, capi.SRL_CONSENSUS_MAX_POINTS + 1):
            fundamental(count=count)
            pnp(count=count)
        fundamental(last=None); fundamental(cur=None); fundamental(out=False)
        pnp(pts=None); pnp(pix=None); pnp(out=False); pnp(cnt=False); pnp(Kp=None)
        for kw in (dict(hypotheses=0), dict(hypotheses=-5), dict(hypotheses=4097), dict(threshold=nan), dict(threshold=inf), dict(threshold=0.0),
                   dict(threshold=-1.0), dict(confidence=0.0), dict(confidence=1.0), dict(confidence=nan), dict(confidence=-0.5), dict(confidence=1.5)):
            fundamental(**kw)
            pnp(**kw)
        for k, v in ((0, nan), (1, inf), (2, nan), (3, -inf), (0, 0.0), (1, 0.0)):
            Kb = Kc.copy()
            Kb[k] = v
            pnp(Kp=Kb)
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])       # more than one rank
        fundamental(want=capi.SRL_ERR_UNSUPPORTED)
        pnp(want=capi.SRL_ERR_UNSUPPORTED)
        fundamental(hypotheses=0)                                                 # ... and a bad argument is still a bad argument
        for call in (lambda: ctx.consensus_fundamental(x1, x2), lambda: ctx.consensus_pnp(X, uv, ck.K)):
            with pytest.raises(srl.SrlError) as e:
                call()
            assert e.value.status == capi.SRL_ERR_UNSUPPORTED
        ctx.comm_set_host_callbacks(1, 0, None, None)
        assert np.array_equal(ctx.consensus_fundamental(x1, x2)[0], scenes["f40"][2])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 6. the loop of imageProcessing::process
def test_a_refused_opt_in_on_a_live_context_keeps_the_earlier_providers(ctx):
    """tests/test_consensus_abi.py's case with a context, where the refusal is the estimators' own (fx = 0, more than one rank)"""
    import gc
    rows, cols = 100, 100
    gray = np.zeros((rows, cols), np.uint8)
    rec = np.zeros(40, capi.COLOR_SELECTED_DTYPE)
    rec["pool"] = np.arange(40) * 3
    rec["u"], rec["v"], rec["z"] = 10 + np.arange(40), 20, 5.0
    calls = {"f": 0, "p": 0}

    def fundamental(last, cur, status):
        calls["f"] += 1
        status[:] = 1
        return 0

    def pnp(xyz, uv):
        calls["p"] += 1
        return 0, np.arange(len(uv))[2:]

    def flow(gray_, r, c, stride, prev, nxt, status):
        nxt[:] = prev
        return 0
    oft = srl.Oft(ctx)
    try:
        oft.set_flow_provider(flow)
        oft.set_fundamental_provider(fundamental)
        oft.set_pnp_provider(pnp)
        del fundamental, pnp
        oft.init(rec, gray, 1.0)
        with pytest.raises(srl.SrlError) as e:
            oft.use_device_consensus([0.0, 400.0, 320.0, 240.0])
        assert e.value.status == capi.SRL_ERR_BAD_ARG
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])
        try:
            with pytest.raises(srl.SrlError) as e:
                oft.use_device_consensus(ck.K)
            assert e.value.status == capi.SRL_ERR_UNSUPPORTED
        finally:
            ctx.comm_set_host_callbacks(1, 0, None, None)
        gc.collect()
        junk = [C.CFUNCTYPE(C.c_int)(lambda: 0) for _ in range(64)]
        assert oft.track_image(gray, 1.1, rows, cols) == 40 and calls == {"f": 1, "p": 0}
        assert oft.remove_outlier_using_ransac_pnp(1) is True and calls == {"f": 1, "p": 1} and oft.sizes() == (38, 38, 38, 0) and len(junk) == 64
        assert bytes(oft.last_consensus(0)) == bytes(C.sizeof(capi.ConsensusResult))      # no device call was made for this handle
    finally:
        oft.close()


def test_the_loop_of_process_with_the_device_estimators():
    """tests/test_gpu_color_track.py's loop with use_device_consensus instead of the all-ones stand-ins, and twenty tracked pixels put in
    the wrong place before the second image.  The image content moves by a pure (+3, +2) translation, which is degenerate for a
    fundamental matrix (every such correspondence is consistent with it), so what is asserted of that step is self-consistency and the
    bookkeeping; the PnP step then has to throw out what does not reproject."""
    import color_checker as cc
    import flow_checker as fc
    import render_checker as rk
    import select_checker as sk
    ctx = srl.Context(0)
    twin = srl.Context(0)                     # replays the mirror's two flow calls, to know what its fundamental step was given
    oft = None
    try:
        opt = rk.OPT
        ctx.color_map_create(capi.default_color_opts(size_voxel_map=opt[0], max_num_points_in_voxel=opt[1], min_distance_points=opt[2], add_point_step=opt[3]))
        for j in range(3):
            ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)
        c, rows, cols, _ = sk.scene_camera(0, 0.005)
        cam = capi.ColorCamera((C.c_double * 4)(*c.q), (C.c_double * 3)(*c.t), c.fx, c.fy, c.cx, c.cy, c.fov_margin)
        Kc = np.array([c.fx, c.fy, c.cx, c.cy])
        sel, sel_tot = ctx.color_map_select(cam, rows, cols, None, capi.default_color_select_opts(use_all_points=1))
        assert sel_tot.selected > 1000
        tex = fc.texture(77, rows, cols)
        gray0, gray1 = fc.crop(tex, rows, cols, 0, 0), fc.crop(tex, rows, cols, -2, -3)       # the content moves by (+3, +2) pixels
        oft = srl.Oft(ctx)
        first = sel[:300].copy()
        oft.init(first, gray0, 10.0)
        with pytest.raises(srl.SrlError) as e:                                                # nothing installed yet: refused as ever
            oft.track_image(gray1, 10.1, rows, cols)
        assert e.value.status == capi.SRL_ERR_BAD_ARG
        # an opt-in the estimators would refuse installs nothing: the rules are theirs (intrinsics, options, one rank)
        for bad, kw in (([0.0, c.fy, c.cx, c.cy], {}), ([c.fx, float("inf"), c.cx, c.cy], {}),
                        (Kc, dict(fundamental_opts=capi.default_consensus_opts(capi.SRL_CONSENSUS_FUNDAMENTAL, hypotheses=0))),
                        (Kc, dict(pnp_opts=capi.default_consensus_opts(capi.SRL_CONSENSUS_PNP, threshold=-1.0)))):
            with pytest.raises(srl.SrlError) as e:
                oft.use_device_consensus(bad, **kw)
            assert e.value.status == capi.SRL_ERR_BAD_ARG
            with pytest.raises(srl.SrlError) as e:
                oft.track_image(gray1, 10.1, rows, cols)
            assert e.value.status == capi.SRL_ERR_BAD_ARG
        oft.use_device_consensus(Kc)
        wrong = first.copy()
        hit = np.arange(20) * 13 + 5
        shift = np.where(wrong["u"][hit] < cols / 2, 24.0, -24.0).astype(np.float32)
        wrong["u"][hit] += shift
        wrong["v"][hit] += np.where(wrong["v"][hit] < rows / 2, 17.0, -17.0).astype(np.float32)
        oft.set_track_points(wrong)
        order = np.argsort(wrong["pool"])
        n_cur = oft.track_image(gray1, 10.1, rows, cols)                                      # no longer refuses
        # what the fundamental step saw: the flow of the pool-ordered points, reduced by its status
        flow = srl.Flow(twin)
        last = np.stack([wrong["u"][order], wrong["v"][order]], 1)
        flow.track_image(gray0, last)
        nxt, st, _ = flow.track_image(gray1, last)
        keep = st == 1
        f_in = (last[keep], nxt[keep])
        res_f = oft.last_consensus(0)
        assert res_f.models_valid > 0 and res_f.hypothesis >= 0
        # The device's mask never leaves the mirror, so self-consistency is asserted through what the mirror did with it: the checker's
        # mask of the returned model has the device's count, and the points it keeps are, pool for pool, the mirror's current map.
        mask = ck.mask_fundamental(res_f.model_array()[:9], f_in[0], f_in[1], F_THR)
        # res_f.inliers points enter the acceptance loop; those of them inside the 5 % margin make the current map
        u, v = f_in[1][mask == 1, 0].astype(np.float64), f_in[1][mask == 1, 1].astype(np.float64)
        inside = (u >= 0.05 * cols + 1) & (np.ceil(u) < (1 - 0.05) * cols) & (v >= 0.05 * rows + 1) & (np.ceil(v) < (1 - 0.05) * rows)
        cur = oft.pose_map(1)
        assert res_f.inliers == int(mask.sum()) and n_cur == int(inside.sum()) == len(cur)
        assert np.array_equal(cur["pool"], wrong["pool"][order][keep][mask == 1][inside])
        assert oft.sizes() == (300, n_cur, 300, 0) and n_cur >= 10
        # the PnP step on the current map: positions by pool, pixels as tracked
        by_pool = {int(r["pool"]): r for r in first}
        xyz = np.array([[by_pool[int(p)]["x"], by_pool[int(p)]["y"], by_pool[int(p)]["z"]] for p in cur["pool"]], np.float32)
        uv = np.stack([cur["u"], cur["v"]], 1)
        assert oft.remove_outlier_using_ransac_pnp(1) is True
        res_p = oft.last_consensus(1)
        pm = ck.mask_pnp(res_p.model_array(), Kc, xyz, uv, P_THR)      # likewise: held against the count, the rebuilt maps and the direct call
        after = oft.pose_map(0)
        assert int(pm.sum()) == res_p.inliers
        assert oft.sizes() == (res_p.inliers, res_p.inliers, res_p.inliers, 0)
        assert np.array_equal(after["pool"], cur["pool"][pm == 1]) and after.tobytes() == oft.pose_map(1).tobytes()
        print("loop: flow kept", int(keep.sum()), "fundamental", res_f.inliers, "current map", n_cur, "PnP", res_p.inliers,
              "wrongly placed points left:", len(set(after["pool"].tolist()) & set(wrong["pool"][hit].tolist())))
        # the direct call on the same lists is the same consensus
        idx, direct = ctx.consensus_pnp(xyz, uv, Kc)
        assert bytes(direct) == bytes(res_p) and np.array_equal(idx, np.flatnonzero(pm))
        # a provider set later replaces the device's estimator
        oft.set_pnp_provider(lambda a, b: (0, np.arange(len(b))))
        assert oft.remove_outlier_using_ransac_pnp(1) is True and bytes(oft.last_consensus(1)) == bytes(res_p)
    finally:
        if oft is not None:
            oft.close()
        twin.close()
        ctx.close()
