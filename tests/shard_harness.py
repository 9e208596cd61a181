"""G logical ranks on one device that stay alive over a SCRIPT (a plain helper module: no fixtures, no conftest).

_run_logical_shards of tests/test_gpu_parity.py runs one pass per context and sums the rows as they arrive.  Here every rank is a thread
with one context, host callbacks are the transport, and all ranks execute the same list of steps in the same order -- uploads,
prefetches, swaps, passes with or without taps, map edits, look-ups -- so that whatever a context carries from one pass to the next
(neighbourhood bounds, sweep slots, the replicated map) is exercised on a context with nranks > 1.

The all-reduce adds the ranks' rows IN RANK ORDER (total = 0.0; for r in range(G): total += row[r], float64): the same bytes on every
rank and run after run, and what the direct peer exchange documents ("adds the rows it received in rank order", include/srlivo_hip.h).

No rank can hang another: every barrier wait has a time-out, an exception in a rank (or inside one of its callbacks) aborts the barrier,
and nothing is asserted in here -- run() returns the per-rank, per-step results and the per-rank errors after every thread has been
joined and every rank object closed; the caller asserts.  A rank never skips a step: a rank without keypoints runs the pass like the
others (the collectives need it).

Ranks are objects with step(kind, *args) and close(): ContextRank drives a sr_livo_amd Context, tests/test_shard_harness_model.py drives
the same machinery with stubs and no device."""
import threading

import numpy as np

BARRIER_TIMEOUT_S = 60.0
MAX_LIVE_CONTEXTS = 8


class RankFailed(RuntimeError):
    """another rank failed (or the barrier timed out): this rank stops at its next step"""


class Collectives:
    """the in-process transport of one run: a rank-ordered all-reduce and an all-gather over a barrier with a time-out"""

    def __init__(self, G, timeout=BARRIER_TIMEOUT_S):
        self.G = G
        self.barrier = threading.Barrier(G, timeout=timeout)
        self.rows = [None] * G
        self.words = [0] * G
        self.errors = [None] * G

    def fail(self, rank, exc):
        if self.errors[rank] is None:
            self.errors[rank] = exc
        self.barrier.abort()

    @property
    def broken(self):
        return self.barrier.broken

    def _wait(self, rank):
        try:
            self.barrier.wait()
        except threading.BrokenBarrierError:
            raise RankFailed(f"rank {rank}: the barrier was aborted or timed out") from None

    def allreduce(self, rank, buf):
        """in place; float64.  Two waits: rows complete, rows read (nobody overwrites a row another rank still adds)."""
        self.rows[rank] = np.array(buf, dtype=np.float64, copy=True)
        self._wait(rank)
        total = 0.0
        for r in range(self.G):
            total = total + self.rows[r]
        self._wait(rank)
        buf[:] = total

    def allgather(self, rank, value):
        self.words[rank] = int(value)
        self._wait(rank)
        out = list(self.words)
        self._wait(rank)
        return out

    # the forms a ctypes callback can take: an exception must not travel through the C frames (ctypes would print and drop it)
    def allreduce_cb(self, rank):
        def cb(buf):
            try:
                self.allreduce(rank, buf)
            except BaseException as e:  # noqa: BLE001
                self.fail(rank, e)
        return cb

    def allgather_cb(self, rank):
        def cb(value):
            try:
                return self.allgather(rank, value)
            except BaseException as e:  # noqa: BLE001
                self.fail(rank, e)
                return [0] * self.G
        return cb


def run(G, make_rank, script, timeout=BARRIER_TIMEOUT_S):
    """G threads; make_rank(rank, coll) -> object with step(kind, *args) and close().  script: list of tuples (kind, *args); an argument
    that is callable is called with the rank (per-rank arguments).  Returns (results[rank][step], errors[rank]); a rank that failed has
    None from its failing step on.  Never raises for a rank's failure and never asserts."""
    assert 1 <= G <= MAX_LIVE_CONTEXTS
    coll = Collectives(G, timeout)
    results = [[None] * len(script) for _ in range(G)]

    def worker(rank):
        obj = None
        try:
            obj = make_rank(rank, coll)
            for i, step in enumerate(script):
                if coll.broken:
                    raise RankFailed(f"rank {rank}: stopped before step {i} ({step[0]})")
                args = [a(rank) if callable(a) else a for a in step[1:]]
                results[rank][i] = obj.step(step[0], *args)
                if coll.errors[rank] is not None:          # a callback of this rank failed inside the step
                    raise coll.errors[rank]
        except BaseException as e:  # noqa: BLE001
            coll.fail(rank, e)
        finally:
            if obj is not None:
                try:
                    obj.close()
                except BaseException as e:  # noqa: BLE001
                    coll.fail(rank, e)

    threads = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return results, list(coll.errors)


def first_error(errors):
    """the error that started it: the first that is not the echo another rank's failure leaves"""
    own = [e for e in errors if e is not None and not isinstance(e, RankFailed)]
    rest = [e for e in errors if e is not None]
    return own[0] if own else (rest[0] if rest else None)


# ------------------------------------------------------------------------------------------------ a rank on the device
def neq_record(neq):
    """the reduced record as comparable bytes and integers"""
    return dict(num_residuals=int(neq.num_residuals), success=int(neq.success), last_visited=int(neq.last_visited),
                sum_candidates=int(neq.sum_candidates), nan_error=int(neq.nan_error),
                HtH=np.array(neq.HtH, dtype=np.float64), Hth=np.array(neq.Hth, dtype=np.float64), loss_sum=np.float64(neq.loss_sum))


REDUCED_INTS = ("num_residuals", "success", "last_visited", "sum_candidates", "nan_error")
REDUCED_SUMS = ("HtH", "Hth", "loss_sum")


def same_bytes(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def records_equal(a, b):
    """bit for bit: the integers and the bytes of the sums"""
    return all(a[k] == b[k] for k in REDUCED_INTS) and all(same_bytes(a[k], b[k]) for k in REDUCED_SUMS)


def taps_equal(a, b):
    """ids, status, candidate counts and every array of fetch_residuals, bit for bit"""
    return all(same_bytes(a[k], b[k]) for k in a if k not in ("neq", "rc"))


class ContextRank:
    """one sr_livo_amd Context as rank `rank` of G over host callbacks (G == 1: no transport).  Armed launches are off: a waiting launch
    holds compute units that the other contexts of the process need."""

    def __init__(self, rank, G, coll, map_arrays, culling=1, ctx=None):
        """ctx: a context somebody else has created, attached and will close (the direct peer exchange's) -- its arm policy is left alone"""
        import sr_livo_amd as srl
        self.srl = srl
        self.rank, self.G = rank, G
        self._own = ctx is None
        self.ctx = srl.Context(0) if ctx is None else ctx
        if self._own:
            self.ctx.set_armed_launch(0)
        self.ctx.set_bound_culling(culling)
        if map_arrays is not None:
            self.ctx.map_upload(*map_arrays)
        if G > 1 and self._own:
            self.ctx.comm_set_host_callbacks(G, rank, coll.allreduce_cb(rank), coll.allgather_cb(rank))
        self._pins = []

    def close(self):
        for p in self._pins:
            p.close()
        self._pins = []
        if self._own:
            self.ctx.close()

    def step(self, kind, *a):
        return getattr(self, "do_" + kind)(*a)

    # ---- sweeps
    def do_upload(self, raw):
        self.ctx.sweep_upload(raw)
        return self.ctx.sweep_shard()

    def do_prefetch(self, raw):
        pin = self.srl.PinnedArray(raw.shape)
        pin.array[:] = raw
        self._pins.append(pin)
        self.ctx.sweep_prefetch(pin.array)

    def do_swap(self):
        self.ctx.sweep_swap()
        return self.ctx.sweep_shard()

    def do_shard(self):
        return self.ctx.sweep_shard()

    # ---- passes
    def do_pass(self, q, t, t_last, optkw, taps=False, frame_id=100):
        from sr_livo_amd import capi
        opts = self.srl.default_opts(**optkw)
        self.ctx.set_taps(bool(taps))
        neq, rc = self.ctx.build_residuals(capi.make_frame(q, t, t_last, frame_id=frame_id), opts)
        out = dict(neq=neq_record(neq), rc=int(rc))
        if taps:
            ids, status, ncand = self.ctx.fetch_neighbors(K=opts.max_number_neighbors)
            out.update(ids=ids.copy(), status=status.copy(), ncand=ncand.copy())
            out.update({k: v.copy() for k, v in self.ctx.fetch_residuals().items()})
            self.ctx.set_taps(False)
        return out

    # ---- the replicated map
    def do_map_upload(self, keys, counts, xyz):
        self.ctx.map_upload(keys, counts, xyz)

    def do_map_insert(self, pts):
        return self.ctx.map_insert(pts)

    def do_map_insert_report(self, pts, ref_z=0.0):
        return self.ctx.map_insert_report(pts, ref_z=ref_z)

    def do_map_remove_far(self, location, distance):
        return self.ctx.map_remove_far(location, distance)

    def do_map_probe_checksum(self, pts, stride=1):
        return self.ctx.map_probe_checksum(pts, stride=stride)

    def do_map_download(self):
        return self.ctx.map_download()

    def do_map_size(self):
        return self.ctx.map_size()

    def do_search_neighbors(self, pts, nb=1, thr=1):
        """(ids, xyz, num_found) with the entries behind num_found set to -1 / 0: the call leaves them as the caller's buffer had them"""
        ids, xyz, nf = self.ctx.search_neighbors(pts, nb=nb, thr=thr)
        unused = np.arange(ids.shape[1])[None, :] >= nf[:, None]
        ids[unused] = -1
        xyz[unused] = 0.0
        return ids, xyz, nf

    # ---- switches and reports
    def do_set_bound_culling(self, mode):
        self.ctx.set_bound_culling(mode)

    def do_comm_info(self):
        return self.ctx.comm_info()

    def do_arm_stats(self):
        return self.ctx.arm_stats()

    def do_peer_stats(self):
        return self.ctx.peer_stats()

    def do_blocks(self):
        """workgroups of the last pass's association launch (srl_debug_block_times reports the count): its launch shape"""
        import ctypes as C
        out = np.zeros((2048, 3))
        nb = C.c_int()
        self.ctx._chk(self.ctx.lib.srl_debug_block_times(self.ctx.h, out.ctypes.data_as(C.c_void_p), 2048, C.byref(nb)), "srl_debug_block_times")
        return nb.value

    def do_timing(self):
        t = self.ctx.timing()
        return {name: getattr(t, name) for name, _ in t._fields_}


def run_contexts(G, map_arrays, script, culling=1, timeout=BARRIER_TIMEOUT_S):
    """the script on G sharded contexts (G == 1: one unsharded context)"""
    return run(G, lambda rank, coll: ContextRank(rank, G, coll, map_arrays, culling), script, timeout)


def run_twins(G, map_arrays, script, culling=1, timeout=BARRIER_TIMEOUT_S):
    """the script on G UNSHARDED contexts side by side (no transport): per-rank arguments (callables of the rank) give each its own sweep"""
    return run(G, lambda rank, coll: ContextRank(rank, 1, coll, map_arrays, culling), script, timeout)


class LioRank:
    """one sr_livo_amd Lio (the host ESIKF on its own context) as rank `rank` of G over host callbacks: step `solve`"""

    def __init__(self, rank, G, coll, map_arrays, culling=1):
        import sr_livo_amd as srl
        self.srl = srl
        self.lio = srl.Lio(0)
        ctx = self.lio.ctx
        ctx.set_armed_launch(0)
        ctx.set_bound_culling(culling)
        ctx.map_upload(*map_arrays)
        if G > 1:
            ctx.comm_set_host_callbacks(G, rank, coll.allreduce_cb(rank), coll.allgather_cb(rank))

    def close(self):
        self.lio.close()

    def step(self, kind, *a):
        return getattr(self, "do_" + kind)(*a)

    def do_solve(self, eskf_state, eskf_cov, optkw, raw, state, t_last):
        self.lio.eskf_set_state(eskf_state)
        self.lio.eskf_set_cov(eskf_cov)
        r = self.lio.update_iekf(self.srl.default_opts(**optkw), raw, state, t_last)
        return dict(rc=int(r["rc"]), iters=int(r["iters"]), num_residuals=int(r["num_residuals"]), state=r["state"].copy(),
                    eskf_state=self.lio.eskf_get_state().copy(), cov=self.lio.eskf_get_cov().copy(), shard=self.lio.ctx.sweep_shard())


def rank_order_sum(rows):
    """what the harness's all-reduce gives for these rows (arrays or scalars), for a test that builds the expectation itself"""
    total = 0.0
    for row in rows:
        total = total + np.asarray(row, dtype=np.float64)
    return total
