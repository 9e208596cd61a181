"""tests/shard_harness.py without a device: stub ranks drive the collectives, the script loop and the failure paths."""
import itertools
import threading
import time

import numpy as np

import shard_harness as sh


class StubRank:
    """a rank whose `reduce` step all-reduces a row of its own, and whose `gather` step all-gathers a word"""

    def __init__(self, rank, coll, rows=None, delay=0.0, fail_at=None):
        self.rank, self.coll, self.rows, self.delay, self.fail_at = rank, coll, rows, delay, fail_at
        self.closed = False
        self.steps = 0

    def step(self, kind, *a):
        self.steps += 1
        if self.fail_at is not None and self.steps - 1 == self.fail_at:
            raise ValueError(f"rank {self.rank} fails on purpose")
        if kind == "reduce":
            time.sleep(self.delay)                       # arrival order != rank order
            buf = np.array(self.rows[self.rank], dtype=np.float64)
            self.coll.allreduce(self.rank, buf)
            return buf
        if kind == "gather":
            return self.coll.allgather(self.rank, a[0])
        if kind == "echo":
            return a[0]
        raise KeyError(kind)

    def close(self):
        self.closed = True


# rows whose sum depends on the order: 1e16 + 1 + 1 - 1e16 = 0 from the left (each 1 is absorbed), 2 when the ones meet first
ROWS = [np.array([1e16, 0.1]), np.array([1.0, 0.2]), np.array([1.0, 0.3]), np.array([-1e16, 0.4])]


def _sum_in(order):
    total = 0.0
    for r in order:
        total = total + ROWS[r]
    return total


def test_the_allreduce_adds_the_rows_in_rank_order_whatever_the_arrival_order():
    G = len(ROWS)
    expect = _sum_in(range(G))
    # the rows are chosen so that another order gives other bits: that premise first
    others = {_sum_in(p).tobytes() for p in itertools.permutations(range(G))}
    assert len(others) > 1 and _sum_in((1, 2, 0, 3)).tobytes() != expect.tobytes()
    assert expect[0] == 0.0 and _sum_in((1, 2, 0, 3))[0] == 2.0
    for delays in ([0.0] * G, [0.15, 0.10, 0.05, 0.0], [0.0, 0.05, 0.10, 0.15], [0.05, 0.15, 0.0, 0.10]):
        ranks = [None] * G

        def make(rank, coll):
            ranks[rank] = StubRank(rank, coll, ROWS, delay=delays[rank])
            return ranks[rank]

        results, errors = sh.run(G, make, [("reduce",), ("reduce",)])
        assert errors == [None] * G
        for r in range(G):
            for i in range(2):
                assert results[r][i].tobytes() == expect.tobytes(), (delays, r, i)
            assert ranks[r].closed
    assert sh.rank_order_sum(ROWS).tobytes() == expect.tobytes()


def test_the_gather_returns_every_ranks_word_in_rank_order_on_every_rank():
    G = 3
    results, errors = sh.run(G, lambda rank, coll: StubRank(rank, coll), [("gather", lambda rank: 10 * rank + 7), ("gather", lambda rank: -rank), ("echo", 5)])
    assert errors == [None] * G
    for r in range(G):
        assert results[r] == [[7, 17, 27], [0, -1, -2], 5]


def test_a_raising_rank_ends_the_run_with_its_exception_and_releases_the_others():
    G = 3
    ranks = [None] * G

    def make(rank, coll):
        ranks[rank] = StubRank(rank, coll, [np.ones(2)] * G, fail_at=1 if rank == 1 else None)
        return ranks[rank]

    t0 = time.perf_counter()
    results, errors = sh.run(G, make, [("reduce",), ("reduce",), ("reduce",)], timeout=20.0)
    dt = time.perf_counter() - t0
    assert dt < 10.0, dt                                              # released by the abort, not by the barrier's time-out
    assert isinstance(errors[1], ValueError) and "on purpose" in str(errors[1])
    assert all(isinstance(errors[r], sh.RankFailed) for r in (0, 2))
    assert isinstance(sh.first_error(errors), ValueError)
    assert results[1][0] is not None                                  # (the others may still have been leaving step 0's second wait)
    for r in range(G):
        assert results[r][1] is None and results[r][2] is None
        assert ranks[r].closed
    assert threading.active_count() < 50


def test_a_rank_that_never_arrives_is_a_time_out_not_a_hang():
    class Absent(StubRank):
        def step(self, kind, *a):
            return None if self.rank == 0 else super().step(kind, *a)       # rank 0 skips the collective

    t0 = time.perf_counter()
    results, errors = sh.run(2, lambda rank, coll: Absent(rank, coll, [np.ones(1)] * 2), [("reduce",)], timeout=0.5)
    assert time.perf_counter() - t0 < 10.0
    assert errors[0] is None and isinstance(errors[1], sh.RankFailed)


def test_a_failure_inside_a_callback_is_kept_and_stops_the_rank():
    """the forms ctypes calls: they must not raise through the C frames; the error is kept and raised behind the step"""
    class ViaCallback(StubRank):
        def step(self, kind, *a):
            cb = self.coll.allreduce_cb(self.rank)
            buf = np.ones(2)
            if self.rank == 0:
                cb(np.ones(3) if kind == "bad" else buf)
            else:
                cb(buf)
            return buf

    results, errors = sh.run(2, lambda rank, coll: ViaCallback(rank, coll), [("ok",), ("bad",), ("ok",)], timeout=20.0)
    assert results[0][0].tolist() == [2.0, 2.0] and results[1][0].tolist() == [2.0, 2.0]
    assert errors[0] is not None or errors[1] is not None           # shapes that do not add up: whoever adds them fails
    assert results[0][2] is None and results[1][2] is None
