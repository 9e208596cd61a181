"""The three ways a sweep becomes current -- srl_sweep_upload, srl_sweep_swap behind srl_sweep_prefetch, and the selection of
srl_frame_select_keypoints -- alternated on ONE long-lived context, over sizes that straddle the 1 024-point minimum capacity of the
context's two sweep buffers and one growth of each: 1, 1 023, 1 025, 2 049, then 1 again (large first, small behind it: a large buffer
must leave nothing stale for a small sweep).  After every step the normal equations of one buildPlaneResiduals pass
(src/optimize.cpp:13-112, max_num_residuals = INT_MAX) must equal, bit for bit, those of a fresh context that only uploaded the same
points; with the taps on, the neighbour ids too.  Once with armed launches off, once with a launch armed behind every eligible pass
(the 2 049-point sweeps: a launch armed on one buffer is fired, kept across the swap or cancelled as the next sweep allows)."""
import numpy as np
import pytest

import sr_livo_amd as srl
from sr_livo_amd import capi, synth

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
SIZES = (1, 1023, 1025, 2049)
SELECT_VOXEL = 0.9


def _neq_tuple(neq):
    return (np.array(neq.HtH), np.array(neq.Hth), neq.loss_sum, neq.num_residuals, neq.sum_candidates, neq.last_visited, neq.num_fallback)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def scene():
    """a 20 000-point map, one pose, and disjoint point sets of every size cut from one 12 000-point sweep (`b`: a second set of the
    size); the reference of every set -- and of the selection out of the frame -- from a fresh context each, computed once"""
    cands, L = synth.map_candidates(4242, 20_000)
    sw = synth.make_sweep(4243, 12_000, L)
    frame = capi.make_frame(sw["q_pred"], sw["t_pred"], sw["t_last"])
    opts = srl.default_opts(max_num_residuals=INT_MAX)
    builder = srl.Context(0)
    builder.map_insert(cands)
    map_arrays = builder.map_download()
    builder.close()

    sets, off = {}, 0
    for tag in ("a", "b"):
        for n in SIZES:
            sets[(n, tag)] = sw["raw"][off:off + n].copy()
            off += n
    frame_raw = sw["raw"][off:off + 4000].copy()

    def fresh(points, taps=False):
        ctx = srl.Context(0)
        try:
            ctx.map_upload(*map_arrays)
            ctx.sweep_upload(points)
            ctx.set_taps(1 if taps else 0)
            neq, rc = ctx.build_residuals(frame, opts)
            assert rc == 0
            return _neq_tuple(neq), (ctx.fetch_neighbors(K=20) if taps else None)
        finally:
            ctx.close()

    ctx = srl.Context(0)
    ctx.frame_upload(frame_raw)
    sel_index = ctx.frame_select_keypoints(sw["q_pred"], sw["t_pred"], SELECT_VOXEL)
    ctx.close()
    assert 1 < len(sel_index) < len(frame_raw)
    sets["selection"] = frame_raw[sel_index].copy()

    ref = {k: fresh(p)[0] for k, p in sets.items()}
    tap_key = (1025, "b")
    ref_taps = fresh(sets[tap_key], taps=True)
    assert ref[(2049, "a")][3] > 1000 and ref[(1023, "a")][3] > 500                  # the scene does its job: most keypoints have a plane
    return dict(map=map_arrays, pose=(sw["q_pred"], sw["t_pred"]), frame=frame, opts=opts, sets=sets, frame_raw=frame_raw, sel_index=sel_index,
                ref=ref, tap_key=tap_key, ref_taps=ref_taps)


@pytest.mark.parametrize("arm_mode", [0, 2])
def test_every_way_a_sweep_becomes_current_equals_a_fresh_upload(scene, arm_mode):
    sc = scene
    sets, ref, frame, opts = sc["sets"], sc["ref"], sc["frame"], sc["opts"]
    ctx = srl.Context(0)
    try:
        ctx.map_upload(*sc["map"])
        ctx.set_armed_launch(arm_mode)

        def check(key, step):
            neq, rc = ctx.build_residuals(frame, opts)
            assert rc == 0, step
            assert ctx.sweep_shard() == (0, len(sets[key]), len(sets[key])), step
            assert _same(_neq_tuple(neq), ref[key]), (step, key)

        # upload, then a larger prefetch (the other buffer is made) and the swap; twice more, each buffer growing once
        ctx.sweep_upload(sets[(1, "a")]); check((1, "a"), "upload 1")
        ctx.sweep_prefetch(sets[(1023, "a")]); check((1, "a"), "prefetch 1023 leaves the current sweep alone")
        ctx.sweep_swap(); check((1023, "a"), "swap to 1023")
        ctx.sweep_prefetch(sets[(1025, "a")]); ctx.sweep_swap(); check((1025, "a"), "swap to 1025 (the first buffer grows)")
        ctx.sweep_prefetch(sets[(2049, "a")]); check((1025, "a"), "prefetch 2049"); ctx.sweep_swap(); check((2049, "a"), "swap to 2049 (the second buffer grows)")
        check((2049, "a"), "a second pass over 2049")
        # a smaller prefetch behind a large sweep, swapped in under whatever launch the pass before armed
        ctx.sweep_prefetch(sets[(1, "b")]); check((2049, "a"), "prefetch 1"); ctx.sweep_swap(); check((1, "b"), "swap to 1 (large, then small)")
        # a prefetch of the size armed on: the waiting launch may serve it from its alternate buffer
        ctx.sweep_prefetch(sets[(2049, "b")]); ctx.sweep_swap(); check((2049, "b"), "swap to 2049 again")
        ctx.sweep_prefetch(sets[(2049, "a")]); check((2049, "b"), "prefetch 2049 behind 2049"); ctx.sweep_swap(); check((2049, "a"), "swap 2049 -> 2049")
        # the selection of a frame becomes current behind a swap, then a plain upload
        ctx.frame_upload(sc["frame_raw"])
        index = ctx.frame_select_keypoints(*sc["pose"], SELECT_VOXEL)
        assert np.array_equal(index, sc["sel_index"])
        check("selection", "frame selection behind a swap")
        ctx.sweep_upload(sets[(1023, "b")]); check((1023, "b"), "upload behind a selection")
        # taps on for one step: the neighbour ids of the long-lived context are the fresh one's
        ctx.sweep_prefetch(sets[sc["tap_key"]]); ctx.sweep_swap()
        ctx.set_taps(1)
        neq, rc = ctx.build_residuals(frame, opts)
        got = ctx.fetch_neighbors(K=20)
        ctx.set_taps(0)
        assert rc == 0 and _same(_neq_tuple(neq), sc["ref_taps"][0])
        assert all(np.array_equal(g, r) for g, r in zip(got, sc["ref_taps"][1]))
        check(sc["tap_key"], "the same sweep without taps")
        # a prefetch that is not swapped, an upload in front of it, and the swap afterwards
        ctx.sweep_prefetch(sets[(2049, "b")])
        ctx.sweep_upload(sets[(1025, "a")]); check((1025, "a"), "upload with a prefetched sweep waiting")
        ctx.sweep_swap(); check((2049, "b"), "the swap of the prefetch issued before the upload")
        ctx.sweep_upload(sets[(1, "a")]); check((1, "a"), "upload 1 at the end")
        if arm_mode == 2:
            assert ctx.arm_stats()["armed"] > 0          # (whether one is fired depends on the host's pace between two calls: tests/test_gpu_armed.py)
    finally:
        ctx.close()
