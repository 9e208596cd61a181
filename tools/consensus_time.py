"""One srl_consensus_fundamental (H = 512) and one srl_consensus_pnp (H = 200) at the tracker's size, n = 300 points with a third of them
outliers.  HIP events around the synchronous call (torch.cuda.Event on the context's device), after warm-up calls; host wall time beside
them.  The scenes are those of tests/consensus_checker.py."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import consensus_checker as ck  # noqa: E402
import sr_livo_amd as srl  # noqa: E402
from sr_livo_amd import capi  # noqa: E402

n = 300
x1, x2, f_truth = ck.scene_fundamental(51, n, 100)
X, uv, p_truth = ck.scene_pnp(52, n, 100)
K = np.ascontiguousarray(ck.K)
ctx = srl.Context(0)
fo, po = capi.default_consensus_opts(capi.SRL_CONSENSUS_FUNDAMENTAL), capi.default_consensus_opts(capi.SRL_CONSENSUS_PNP)
mask, idx, cnt = np.zeros(n, np.uint8), np.zeros(n, np.int32), C.c_int()
res = capi.ConsensusResult()


def fundamental():
    return ctx.lib.srl_consensus_fundamental(ctx.h, capi._ptr(x1), capi._ptr(x2), n, C.byref(fo), capi._ptr(mask), C.byref(res))


def pnp():
    return ctx.lib.srl_consensus_pnp(ctx.h, capi._ptr(X), capi._ptr(uv), n, capi._dptr(K), C.byref(po), capi._ptr(idx), C.byref(cnt), C.byref(res))


for name, fn in (("fundamental n=300 H=512", fundamental), ("pnp n=300 H=200", pnp)):
    for _ in range(20):
        assert fn() == 0
    ev, wall = [], []
    for _ in range(200):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - w0) * 1e6)
        ev.append(a.elapsed_time(b) * 1e3)
    ev, wall = np.array(ev), np.array(wall)
    print("%s: HIP events median %.1f us (p10 %.1f, p90 %.1f); host wall median %.1f us; calls = %d; inliers %d, models_valid %d" % (
        name, np.median(ev), np.percentile(ev, 10), np.percentile(ev, 90), np.median(wall), len(ev), res.inliers, res.models_valid))
print("masks equal the truth:", bool(np.array_equal(mask, f_truth)), bool(np.array_equal(idx[:cnt.value], np.flatnonzero(p_truth))))
ctx.close()
