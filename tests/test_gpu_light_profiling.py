"""Light profiling (srl_set_profiling(ctx, 2)): which association launches are counted.  Every launch leaves an event pair in a ring
that is read lazily; with a period P > 1 (srl_set_profiling_period) only the launches numbered k with k mod P == 1 are timed (the one
before each leaves its end event as the timed one's start), and srl_timing_mark restarts the numbering at P - 2.  Armed launches are
counted once per pass, fired or launched, and the one left waiting -- cancelled by the read-out -- is not.  `sum_passes` follows `calls`.
(The wrap of the 512-entry ring: tests/test_gpu_parity.py::test_profiling_modes_report_consistent_kernel_times.)"""
import pytest

import sr_livo_amd as srl
from sr_livo_amd import capi, synth

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def pass_on():
    """a context with a 20 000-point map and a 2 049-keypoint sweep (a fused pass: one that can be armed); returns the call of one pass"""
    cands, L = synth.map_candidates(4242, 20_000)
    sw = synth.make_sweep(4243, 2049, L)
    ctx = srl.Context(0)
    ctx.map_insert(cands)
    ctx.sweep_upload(sw["raw"])
    frame = capi.make_frame(sw["q_pred"], sw["t_pred"], sw["t_last"])
    opts = srl.default_opts(max_num_residuals=INT_MAX)

    def one_pass():
        neq, rc = ctx.build_residuals(frame, opts)
        assert rc == 0 and neq.num_residuals > 1000
    one_pass()
    yield ctx, one_pass
    ctx.close()


def _timed(first, count, period):
    """launches numbered first ... first + count - 1 that are timed"""
    return sum(1 for k in range(first, first + count) if period == 1 or k % period == 1)


@pytest.mark.parametrize("N", [9, 11])
@pytest.mark.parametrize("period", [1, 2, 4])
def test_every_period_th_launch_is_counted(pass_on, period, N):
    ctx, one_pass = pass_on
    ctx.set_armed_launch(0)
    try:
        ctx.set_profiling_period(period)
        ctx.set_profiling(2)                       # (the sums and the numbering start here)
        for _ in range(N):
            one_pass()
        t = ctx.timing()
        assert t.calls == _timed(0, N, period) and t.sum_passes == t.calls, (t.calls, t.sum_passes)
        assert t.calls == {1: N, 2: N // 2, 4: (N + 2) // 4}[period]
        assert t.sum_assoc_ms > 0 and t.sum_keypoints == 2049 * t.calls
    finally:
        ctx.set_profiling(0)
        ctx.set_profiling_period(1)
        ctx.set_armed_launch(1)


@pytest.mark.parametrize("period", [2, 4])
def test_a_timing_mark_restarts_the_numbering_two_before_the_period(pass_on, period):
    M = 6
    ctx, one_pass = pass_on
    ctx.set_armed_launch(0)
    try:
        ctx.set_profiling_period(period)
        ctx.set_profiling(2)
        for _ in range(3):                         # launches before the mark: left out, whatever they were
            one_pass()
        ctx.timing_mark()
        for _ in range(M):
            one_pass()
        t = ctx.timing()
        assert t.calls == _timed(period - 2, M, period) and t.sum_passes == t.calls, (t.calls, t.sum_passes)
        assert t.calls == {2: 3, 4: 1}[period]
    finally:
        ctx.set_profiling(0)
        ctx.set_profiling_period(1)
        ctx.set_armed_launch(1)


@pytest.mark.parametrize("K", [9, 11])
def test_armed_launches_count_once_per_pass_and_the_one_left_waiting_does_not(pass_on, K):
    ctx, one_pass = pass_on
    ctx.set_armed_launch(2)
    try:
        ctx.set_profiling(2)
        s0 = ctx.arm_stats()
        for _ in range(K):
            one_pass()
        t = ctx.timing()                           # cancels the launch armed behind the last pass
        s1 = ctx.arm_stats()
        assert s1["armed"] - s0["armed"] == K and s1["cancelled"] - s0["cancelled"] >= 1
        assert t.calls == K and t.sum_passes == K, (t.calls, t.sum_passes, s0, s1)
    finally:
        ctx.set_profiling(0)
        ctx.set_armed_launch(1)
