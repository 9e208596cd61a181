"""The device point queue and srl_points_cut against the checker's queue (tests/livox_checker.py: PointQueue), step by step: several
messages with growth across two doublings of the queue's block, cuts before the front, inside, at an exact timestamp, beyond the back and
on the empty queue, a queue made unsorted by a late message (where the prefix rule differs from "everything below t"), clear -- and
srl_points_info against the checker after every step."""
import numpy as np
import pytest

import livox_cases as lc
import livox_checker as lk
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu

QUEUE_MIN_CAP = 4096          # csrc/srl_points.hip: the queue's first block


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _records(d):
    return np.ascontiguousarray(np.concatenate([d["raw"], d["relative_time"][:, None], d["timestamp"][:, None]], axis=1))


class Pair:
    """the device queue and the checker's, driven together and compared after every step"""

    def __init__(self, ctx, pfn=1, unit=2):
        self.ctx, self.q = ctx, lk.PointQueue()
        self.pfn, self.unit = pfn, unit
        self.opts = srl.livox_opts(n_scans=lc.N_SCANS, time_unit=unit, blind=0.5, point_filter_num=pfn)

    def feed(self, msg, stamp):
        r = self.ctx.livox_decode(msg, stamp, self.opts)
        w = lk.decode(msg, stamp, lc.N_SCANS, lk.time_unit_scale(self.unit), 0.5, self.pfn)
        assert r["appended"] == w["appended"]
        self.q.push(w["records"])
        self.same_info()
        return w

    def same_info(self):
        n, front, back = self.ctx.points_info()
        wn, wf, wb = self.q.info()
        assert n == wn and _same(front, wf) and _same(back, wb)

    def cut(self, t):
        count, front = self.ctx.points_cut(t)
        want = self.q.cut(t)
        assert count == len(want) and _same(front, self.q.info()[1])
        got = _records(self.ctx.points_cut_download())
        assert got.shape == want.shape and got.tobytes() == want.tobytes()
        self.same_info()
        return want

    def same_queue(self):
        got = _records(self.ctx.points_queue_download())
        assert got.shape == self.q.rec.shape and got.tobytes() == self.q.rec.tobytes()


@pytest.fixture()
def ctx():
    k = srl.Context(0)
    yield k
    k.close()


def test_growth_cuts_and_info_step_by_step(ctx):
    p = Pair(ctx)
    # microsecond offsets: message k spans [stamp, stamp + 0.1) s
    msgs = [lc.make_message(n, 900 + k, offset_step=100000 // n) for k, n in enumerate((1500, 3000, 2500, 6000, 5000))]
    total = 0
    for k, m in enumerate(msgs[:4]):
        total += p.feed(m, 100.0 + 0.1 * k)["appended"]
    assert total == 1499 + 2999 + 2499 + 5999 > 2 * QUEUE_MIN_CAP            # 4096 -> 8192 -> 16384: two doublings
    p.same_queue()
    assert len(p.cut(99.0)) == 0                                             # before the front
    p.same_queue()
    inside = p.cut(100.05)                                                   # inside the first message
    assert 0 < len(inside) < 1499
    t_exact = float(p.q.rec[300, 4])
    at = p.cut(t_exact)                                                      # at an exact timestamp: <, not <=
    assert len(at) == 300 and _same(p.q.info()[1], t_exact)
    assert len(p.cut(t_exact)) == 0
    p.same_queue()
    total += p.feed(msgs[4], 100.4)["appended"]                              # the tail no longer fits behind the head: a fresh block
    p.same_queue()
    rest = p.cut(1000.0)                                                     # beyond the back: everything
    assert len(rest) == p.ctx.points_cut_download()["timestamp"].size > 10000 and ctx.points_info()[0] == 0
    assert len(p.cut(1000.0)) == 0                                           # the empty queue: an empty cut, defined
    assert np.isnan(ctx.points_info()[1])
    p.feed(msgs[0], 101.0)
    ctx.points_clear()
    p.q.clear()
    p.same_info()
    p.feed(msgs[1], 102.0)
    p.same_queue()


def test_the_cut_is_a_prefix_of_an_unsorted_queue(ctx):
    p = Pair(ctx, pfn=3)
    a = p.feed(lc.make_message(400, 31, offset_step=250), 50.0)              # [50.0, 50.1)
    b = p.feed(lc.make_message(300, 32, offset_step=250), 49.95)             # a late message: starts BEFORE the back of the queue
    assert b["first_timestamp"] < a["last_timestamp"]
    t = 50.02
    below = int((p.q.rec[:, 4] < t).sum())
    got = p.cut(t)
    assert 0 < len(got) < below                                              # later elements would pass; the cut stops at the first that fails
    p.same_queue()
    # everything that is left in front of the late message fails t; the late message's points do not count
    assert len(p.cut(t)) == 0
    rest = p.cut(60.0)
    assert len(rest) == len(a["records"]) + len(b["records"]) - len(got)


def test_operations_without_a_queue_or_a_cut(ctx):
    for call in (ctx.points_info, ctx.points_clear, lambda: ctx.points_cut(1.0), ctx.points_queue_download, ctx.points_cut_download,
                 lambda: ctx.frame_point_times(np.zeros(0, np.int32))):
        with pytest.raises(srl.SrlError) as e:
            call()
        assert e.value.status == capi.SRL_ERR_NO_SWEEP
    with pytest.raises(srl.SrlError) as e:
        ctx.frame_undistort_cut(0.0, 0.1, True, np.zeros((2, 17)), capi.MC_NONE)
    assert e.value.status == capi.SRL_ERR_NO_SWEEP
    ctx.livox_decode(lc.make_message(20, 5), 10.0, srl.livox_opts(time_unit=2))
    with pytest.raises(srl.SrlError) as e:                                   # a queue, but no cut yet
        ctx.points_cut_download()
    assert e.value.status == capi.SRL_ERR_NO_SWEEP
    with pytest.raises(srl.SrlError) as e:
        ctx.points_cut(float("nan"))
    assert e.value.status == capi.SRL_ERR_BAD_ARG
    assert ctx.points_info()[0] == 19
