"""The final reduction on the edges of its loops.

The finishing workgroup of a fused pass pulls the published rows in strides of NPART x INF = 256, takes its own row from LDS, switches
to two levels above 2 x SRL_FUSED_GROUP = 512 workgroups, and -- with a finite max_num_residuals -- cuts inside one workgroup's records
(srl_kernels.hip: finish_rows).  The other GPU tests reach 16, 128, 256, 274 and 547 workgroups and fixed budgets; the
cases here sit on the edges: 1, 2, 32, 33, 256, 257, 512, 513 and 769 workgroups, and budgets that end on the last accepted keypoint of
a workgroup, on the first of the next, and inside the finisher's own workgroup.

Scene: the ragged map (tests/ragged_scene.py) at threshold_voxel_occupancy = 5 -- about one keypoint in ten is NOT accepted, so
acceptance masks and records are not all-ones (the saturated maps accept every keypoint, which makes a cut trivial).  The budgets are
derived from the oracle's acceptance mask, and what they rest on is asserted from the oracle alone before any device call.
"""
import numpy as np
import pytest

import ragged_scene as rs
import sr_livo_amd as srl
from sr_livo_amd import capi, synth

from test_gpu_parity import INT_MAX, TIGHT, rel

pytestmark = pytest.mark.gpu

SEED, TARGET = 4242, 100_000
KW = dict(threshold_voxel_occupancy=5)
WPB = 16                                                              # waves per workgroup of the forced launch shape
NO_CUT_N = (32, 33, 1024, 1056, 8192, 8224, 16384, 16416, 24608)      # at 2 keypoints per wave: 1, 2, 32, 33, 256, 257, 512, 513, 769 workgroups
CUT_SHAPES = ((1056, 2), (8224, 2), (16384, 2), (8224, 3), (16416, 4))    # (n, keypoints per wave): 33, 257, 512, 172, 257 workgroups
INT_FIELDS = ("num_residuals", "success", "sum_candidates", "last_visited", "nan_error", "num_fallback")


@pytest.fixture(scope="module")
def scene(oracle_lib, oracle_backend):
    """ragged_scene(oracle_lib, oracle_backend, 4242, 100_000, n) for every n of this file: ONE map (it does not depend on n), one device
    context holding it, the sweep of n keypoints and the oracle's pass over it on first use"""
    sc = rs.ragged_scene(oracle_lib, oracle_backend, SEED, TARGET, max(NO_CUT_N))
    sweeps, passes = {max(NO_CUT_N): sc["sweep"]}, {}

    def sweep(n):
        if n not in sweeps:
            sweeps[n] = synth.make_sweep(SEED + 1, n, sc["L"])             # ragged_scene's sweep of n keypoints
        return sweeps[n]

    def oracle(n, max_res=INT_MAX):
        if (n, max_res) not in passes:
            sw = sweep(n)
            passes[n, max_res] = sc["map"].build_plane_residuals(oracle_lib.default_opts(max_num_residuals=max_res, **KW), sw["raw"], sw["q_pred"],
                                                                 sw["t_pred"], sw["t_last"], full=max_res == INT_MAX)
        return passes[n, max_res]

    ctx = srl.Context(0)
    ctx.map_upload(sc["keys"], sc["counts"], sc["xyz"])
    yield dict(ctx=ctx, sweep=sweep, oracle=oracle)
    ctx.close()


def _fused_unfused(ctx, f, opts):
    """the pass fused twice and through the reduce kernel once"""
    ctx.set_fused_reduce(1)
    a, rca = ctx.build_residuals(f, opts)
    a2, rca2 = ctx.build_residuals(f, opts)
    ctx.set_fused_reduce(0)
    b, rcb = ctx.build_residuals(f, opts)
    ctx.set_fused_reduce(1)
    assert rca == rca2 == rcb == 0
    return a, a2, b


def _check(a, a2, b, o, what):
    # fused twice: the same bits
    assert np.array_equal(np.array(a.HtH), np.array(a2.HtH)) and np.array_equal(np.array(a.Hth), np.array(a2.Hth)) and a.loss_sum == a2.loss_sum, what
    # fused against the reduce kernel: the summation order differs, nothing else
    assert rel(np.array(a.HtH), np.array(b.HtH)) < 1e-13 and rel(np.array(a.Hth), np.array(b.Hth)) < 1e-13 and rel(a.loss_sum, b.loss_sum) < 1e-13, what
    for k in INT_FIELDS:
        assert getattr(a, k) == getattr(a2, k) == getattr(b, k), (what, k)
    # both against the oracle
    for x in (a, b):
        assert x.num_residuals == o["neq"].num_residuals and x.last_visited == o["neq"].num_visited - 1, what
        assert x.success == o["neq"].success and x.nan_error == o["neq"].nan_error == 0, what
        assert rel(np.array(x.HtH).reshape(6, 6), o["HtH"]) < TIGHT and rel(np.array(x.Hth), o["Hth"]) < TIGHT, what
        assert rel(x.loss_sum, o["neq"].loss_sum) < TIGHT, what


@pytest.mark.parametrize("n", NO_CUT_N)
def test_no_cut_on_the_edges_of_the_row_loops(scene, n):
    """max_num_residuals = INT_MAX at 32 keypoints per workgroup: one workgroup (only the own row), two (the last one holds ONE keypoint
    and no residual), one stride of the part loop and one row more (32, 33), one stride of the poll loop and one row more (256, 257),
    the largest one-level grid and the smallest two-level one (512, 513), three groups (769)."""
    kpb = 2 * WPB
    o = scene["oracle"](n)
    acc = o["status"] == 2
    assert o["neq"].nan_error == 0 and 0 < acc.sum() < n
    if n == kpb + 1:
        assert acc[:kpb].sum() == 30 and acc[kpb:].sum() == 0             # the short last workgroup adds an all-zero row
    ctx, sw = scene["ctx"], scene["sweep"](n)
    ctx.sweep_upload(sw["raw"])
    ctx.set_launch_shape(2, WPB)
    f = capi.make_frame(sw["q_pred"], sw["t_pred"], sw["t_last"])
    a, a2, b = _fused_unfused(ctx, f, srl.default_opts(max_num_residuals=INT_MAX, **KW))
    assert a.num_residuals == int(acc.sum()) and a.last_visited == n - 1
    assert a.sum_candidates == o["neq"].sum_candidates                    # (behind a cut the device still counts every keypoint's candidates)
    _check(a, a2, b, o, n)


def _budgets(acc, kpb):
    """Budgets from the oracle's acceptance mask.  A(j) = accepted keypoints of workgroups 0..j: A(j) stops on the LAST accepted keypoint of
    workgroup j, A(j) + 1 on the FIRST of workgroup j + 1, for j = 0, 1 and last - 1 (the stop workgroup of A(last - 1) + 1 is the
    finisher's own); A(last) - 1 and A(last) = the total (the stop keypoint is the last accepted one); and 1.
    What the budgets rest on: every workgroup a budget names holds at least two accepted keypoints; the workgroups named through j = 0, 1
    also hold a keypoint that is NOT accepted (a fully accepted one: the next j is taken); last - 1 and last cannot move: one of the two
    holds a keypoint that is not accepted (at 1 056 keypoints in workgroups of 32 the last workgroup is fully accepted, the one before it
    holds 29; the last workgroups of the other four shapes hold 29 / 32, 30 / 32, 15 / 16 and 28 / 32)."""
    nb = (len(acc) + kpb - 1) // kpb
    per = np.array([int(acc[j * kpb:(j + 1) * kpb].sum()) for j in range(nb)])
    size = np.array([min(kpb, len(acc) - j * kpb) for j in range(nb)])
    mixed = (per >= 2) & (per < size)
    A = np.cumsum(per)
    assert mixed[0], "budget 1 stops in workgroup 0"
    assert per[-2] >= 2 and per[-1] >= 2 and (mixed[-2] or mixed[-1]), (per[-2:], size[-2:])
    out = [1, int(A[-1]) - 1, int(A[-1]), int(A[-2]), int(A[-2]) + 1]
    for j in (0, 1):
        while not (mixed[j] and mixed[j + 1]):                            # A(j) stops in workgroup j, A(j) + 1 in workgroup j + 1
            j += 1
            assert j + 2 < nb, "no pair of neighbouring workgroups with mixed acceptance"
        out += [int(A[j]), int(A[j]) + 1]
    return sorted(set(out)), int(A[-1])


@pytest.mark.parametrize("n,kpw", CUT_SHAPES)
def test_ordered_cut_on_the_edges_of_the_workgroups(scene, n, kpw):
    """A finite max_num_residuals, fused (<= 64 keypoints per workgroup, <= 512 workgroups) and through the reduce kernel: the same
    assertions as test_fused_ordered_cut_equals_the_two_kernel_path_and_the_oracle (tests/test_gpu_parity.py), for budgets on the edges of
    the workgroups."""
    o_all = scene["oracle"](n)
    assert o_all["neq"].nan_error == 0
    budgets, total = _budgets(o_all["status"] == 2, kpw * WPB)
    assert total == o_all["neq"].num_residuals
    ctx, sw = scene["ctx"], scene["sweep"](n)
    ctx.sweep_upload(sw["raw"])
    ctx.set_launch_shape(kpw, WPB)
    f = capi.make_frame(sw["q_pred"], sw["t_pred"], sw["t_last"])
    for max_res in budgets:
        a, a2, b = _fused_unfused(ctx, f, srl.default_opts(max_num_residuals=max_res, **KW))
        o = scene["oracle"](n, max_res)
        assert a.num_residuals == b.num_residuals == min(max_res, total), max_res
        _check(a, a2, b, o, (n, kpw, max_res))
