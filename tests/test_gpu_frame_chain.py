"""The grid-sampling chain that srl_frame_select_keypoints and srl_frame_subsample share (one scratch table, one exchange block, one count
word), where the two callers meet: a rejected visit order under the host replay and the chain behind it, the callers alternating on one
context with tables of different sizes, and the sub-sample's kept list from the device's ranking against the host's replay of the same
sweep.  Everything is compared bit for bit with the host's subSampleFrame (srl.grid_sampling: a real std::tr1::unordered_map)."""
import numpy as np
import pytest

import sr_livo_amd as srl
from sr_livo_amd import capi, synth

from test_gpu_frame_subsample import BAD_ARG, NO_SWEEP, R_IL, T_IL, expected, points_of_keys, room, status_of, undistort

pytestmark = pytest.mark.gpu

Q = synth.quat_from_rotvec([0.03, -0.02, 0.4]) * 1.0003          # un-normalised: transformPoint uses q as is
T = np.array([3.0, -2.0, 0.5])


def subsample(ctx, raw, rng, size):
    """one sub-sample of `raw` in a random visit order -> (kept list in the container's order, what the host keeps)"""
    undistort(ctx, raw, rng, capi.MC_NONE)
    order = rng.permutation(len(raw)).astype(np.int32)
    m = ctx.frame_subsample(order, size)
    return ctx.frame_take_subsampled(None, m=m)["index"], expected(raw, order, size, None)


def select(ctx, oracle_lib, oracle_backend, raw, size):
    """one keypoint selection of `raw` under the pose (Q, T) -> (index list, what the host selects)"""
    ctx.frame_upload(raw)
    got = ctx.frame_select_keypoints(Q, T, size, R_IL, T_IL)
    world = oracle_lib.transform_points(raw, Q, T, R_IL, T_IL, backend=oracle_backend)
    return got, srl.grid_sampling(world, size)


def test_bad_visit_orders_under_the_host_replay(oracle_lib, oracle_backend):
    """mode 1: the count word -- and the bad-order mark in it -- is published by the scan's own last block, not by k_tr1_bucket"""
    rng = np.random.default_rng(21)
    n = 3_000
    raw = room(rng, n)
    ctx = srl.Context(0)
    try:
        ctx.set_frame_order_mode(1)
        bad_orders = []
        o = rng.permutation(n).astype(np.int32); o[17] = o[1234]; bad_orders.append(o)             # a duplicate
        o = rng.permutation(n).astype(np.int32); o[5] = n; bad_orders.append(o)                    # an entry equal to n
        o = rng.permutation(n).astype(np.int32); o[9] = -1; bad_orders.append(o)                   # an entry of -1
        for o in bad_orders:
            undistort(ctx, raw, rng, capi.MC_NONE)
            assert status_of(ctx.frame_subsample, o, 0.1) == BAD_ARG
            assert status_of(ctx.frame_take_subsampled, None, m=0) == NO_SWEEP
        got, want = subsample(ctx, raw, rng, 0.1)
        assert ctx.frame_order_used() == 2
        assert np.array_equal(got, want)
        # the bad-order mark did not survive into the next chain
        got, want = select(ctx, oracle_lib, oracle_backend, raw, 0.1)
        assert ctx.frame_order_used() == 2
        assert np.array_equal(got, want)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_the_two_callers_alternate_on_one_context(oracle_lib, oracle_backend, mode):
    """the table in use shrinks and grows between chains and the epochs of the two callers interleave"""
    rng = np.random.default_rng(22 + mode)
    ctx = srl.Context(0)
    try:
        ctx.set_frame_order_mode(mode)
        for caller, n, size in (("sub", 600, 0.2), ("select", 5_000, 0.5), ("sub", 600, 0.2), ("select", 300, 0.5)):
            if caller == "sub":
                got, want = subsample(ctx, room(rng, n), rng, size)
            else:
                got, want = select(ctx, oracle_lib, oracle_backend, rng.normal(size=(n, 3)) * np.array([25.0, 25.0, 4.0]), size)
            assert ctx.frame_order_used() == 1 + mode
            assert len(want) > 1 and np.array_equal(got, want), (caller, n)
    finally:
        ctx.close()


def test_sweep_indices_from_both_paths_of_the_subsample():
    """100 voxels whose keys collide in bucket 0 (x = 199 k: 199 buckets at the end), seven points each: the device's ranking gives up and
    the host orders what the device left (3), or the host orders what the scan handed over (2) -- sweep indices either way"""
    rng = np.random.default_rng(23)
    xs = rng.choice(np.arange(-160, 160), size=100, replace=False) * 199
    keys = np.column_stack([xs, np.zeros(100, int), np.zeros(100, int)])
    raw = np.repeat(points_of_keys(keys), 7, axis=0)
    order = rng.permutation(len(raw)).astype(np.int32)
    want = expected(raw, order, 1.0, None)
    assert len(raw) == 700 and len(want) == 100
    ctx = srl.Context(0)
    try:
        kept = {}
        for mode, used in ((0, 3), (1, 2)):
            ctx.set_frame_order_mode(mode)
            undistort(ctx, raw, rng, capi.MC_NONE)
            m = ctx.frame_subsample(order, 1.0)
            assert ctx.frame_order_used() == used
            kept[used] = ctx.frame_take_subsampled(None, m=m)["index"]
        assert np.array_equal(kept[3], kept[2])
        assert np.array_equal(kept[3], want)
    finally:
        ctx.close()
