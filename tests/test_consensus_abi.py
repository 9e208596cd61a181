"""The C-ABI of the consensus estimators without a device (CPU): the symbols are declared and exported, the two structures agree between
include/srlivo_hip.h and the ctypes layer, the defaults are the reference's call-site arguments (512 hypotheses are ours), every refusal
made before a device is touched zeroes the result and leaves the outputs alone, and the host mirror's opt-in refuses on a handle
without a context and then still refuses to track without a provider, exactly as before."""
import ctypes as C
import os
import re

import numpy as np

import sr_livo_amd as srl
from sr_livo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRL_OK, SRL_ERR_NO_DEVICE, SRL_ERR_BAD_ARG = 0, -1, -3
SIZES = {"double": 8, "int32_t": 4, "uint32_t": 4}
NEW = ("srl_consensus_opts_default", "srl_consensus_fundamental", "srl_consensus_pnp", "srl_oft_use_device_consensus", "srl_oft_last_consensus",
       "srl_debug_consensus_download")


def _header_fields(name, header="srlivo_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            fields.append((m.group(1), SIZES[ctype] * int(m.group(2) or 1)))
    return fields


def test_symbols_are_declared_and_exported():
    declared, exported = srl.declared_symbols(), srl.library_symbols()
    for s in NEW:
        assert s in declared and s in exported, s


def test_structs_agree_with_the_header():
    for name, cls, size in (("srl_consensus_opts", capi.ConsensusOpts, 24), ("srl_consensus_result", capi.ConsensusResult, 152)):
        fields = _header_fields(name)
        assert [f for f, _ in fields] == [f for f, _ in cls._fields_], name
        assert [s for _, s in fields] == [C.sizeof(t) for _, t in cls._fields_], name
        assert sum(s for _, s in fields) == C.sizeof(cls) == size, name
    fields = _header_fields("srl_debug_consensus_info", "srlivo_hip_debug.h")
    assert [f for f, _ in fields] == [f for f, _ in capi.DebugConsensusInfo._fields_]
    assert [s for _, s in fields] == [C.sizeof(t) for _, t in capi.DebugConsensusInfo._fields_]
    assert sum(s for _, s in fields) == C.sizeof(capi.DebugConsensusInfo) == 72
    text = open(os.path.join(ROOT, "include", "srlivo_hip.h")).read()
    assert int(re.search(r"#define SRL_CONSENSUS_MAX_POINTS (\d+)", text).group(1)) == capi.SRL_CONSENSUS_MAX_POINTS == 4096
    assert int(re.search(r"#define SRL_CONSENSUS_MAX_HYPOTHESES (\d+)", text).group(1)) == capi.SRL_CONSENSUS_MAX_HYPOTHESES == 4096
    assert (capi.SRL_CONSENSUS_FUNDAMENTAL, capi.SRL_CONSENSUS_PNP) == (0, 1)


def test_defaults():
    f = capi.default_consensus_opts(capi.SRL_CONSENSUS_FUNDAMENTAL)
    p = capi.default_consensus_opts(capi.SRL_CONSENSUS_PNP)
    assert (f.threshold, f.confidence, f.hypotheses, f.seed) == (1.0, 0.997, 512, 0)
    assert (p.threshold, p.confidence, p.hypotheses, p.seed) == (1.5, 0.99, 200, 0)
    # the wrappers' keywords apply to a copy of given options too, and leave them as they were
    o = capi._consensus_opts(capi.SRL_CONSENSUS_PNP, p, dict(seed=5, hypotheses=64))
    assert (o.threshold, o.confidence, o.hypotheses, o.seed) == (1.5, 0.99, 64, 5) and (p.hypotheses, p.seed) == (200, 0)
    o = capi._consensus_opts(capi.SRL_CONSENSUS_FUNDAMENTAL, None, dict(threshold=2.0))
    assert (o.threshold, o.confidence, o.hypotheses, o.seed) == (2.0, 0.997, 512, 0)


def _dirty():
    res = capi.ConsensusResult()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    return res


def _opts(model, **kw):
    return capi.default_consensus_opts(model, **kw)


def test_every_refusal_on_a_null_context_zeroes_the_result_and_leaves_the_outputs():
    lib = srl.load_library()
    n = 16
    a, b = np.ones((n, 2), np.float32), np.ones((n, 2), np.float32)
    xyz = np.ones((n, 3), np.float32)
    K = np.array([400.0, 400.0, 320.0, 240.0])
    zero = bytes(C.sizeof(capi.ConsensusResult))
    nan, inf = float("nan"), float("inf")
    bad_opts = [dict(hypotheses=0), dict(hypotheses=-5), dict(hypotheses=4097), dict(threshold=nan), dict(threshold=inf), dict(threshold=0.0),
                dict(threshold=-1.0), dict(confidence=0.0), dict(confidence=1.0), dict(confidence=nan), dict(confidence=-0.5), dict(confidence=1.5)]
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    dptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731

    def fundamental(count=n, last=a, cur=b, out=True, **kw):
        status = np.full(n, 7, np.uint8)
        res = _dirty()
        o = _opts(capi.SRL_CONSENSUS_FUNDAMENTAL, **kw)
        rc = lib.srl_consensus_fundamental(None, ptr(last) if last is not None else None, ptr(cur) if cur is not None else None, count, C.byref(o),
                                           ptr(status) if out else None, C.byref(res))
        assert rc == SRL_ERR_BAD_ARG and bytes(res) == zero and (status == 7).all(), kw

    def pnp(count=n, pts=xyz, uv=a, Kc=K, out=True, cnt=True, **kw):
        idx = np.full(n, 7, np.int32)
        ni = C.c_int(-77)
        res = _dirty()
        o = _opts(capi.SRL_CONSENSUS_PNP, **kw)
        rc = lib.srl_consensus_pnp(None, ptr(pts) if pts is not None else None, ptr(uv) if uv is not None else None, count,
                                   dptr(Kc) if Kc is not None else None, C.byref(o), ptr(idx) if out else None, C.byref(ni) if cnt else None, C.byref(res))
        assert rc == SRL_ERR_BAD_ARG and bytes(res) == zero and (idx == 7).all() and ni.value == -77, kw

    fundamental()                                      # the NULL context alone
    pnp()
    for count in (-1, 4097):
        fundamental(count=count)
        pnp(count=count)
    fundamental(last=None); fundamental(cur=None); fundamental(out=False)
    pnp(pts=None); pnp(uv=None); pnp(out=False); pnp(cnt=False); pnp(Kc=None)
    for kw in bad_opts:
        fundamental(**kw)
        pnp(**kw)
    for k, v in ((0, nan), (1, inf), (2, nan), (3, -inf), (0, 0.0), (1, 0.0)):
        Kb = K.copy()
        Kb[k] = v
        pnp(Kc=Kb)
    # NULL options are the defaults and a NULL result is allowed: still refused for the context, nothing written
    status = np.full(n, 7, np.uint8)
    assert lib.srl_consensus_fundamental(None, ptr(a), ptr(b), n, None, ptr(status), None) == SRL_ERR_BAD_ARG and (status == 7).all()


def test_the_read_back_refuses_a_null_context_and_writes_nothing():
    lib = srl.load_library()
    info = capi.DebugConsensusInfo()
    C.memset(C.byref(info), 0xFF, C.sizeof(info))
    before = bytes(info)
    usable, samples, models, counts = np.full(16, 7, np.int32), np.full((4, 8), 7, np.int32), np.full(4 * 4 * 12, 7.0), np.full(4 * 4, 7, np.int32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = lib.srl_debug_consensus_download(None, C.byref(info), ptr(usable), 16, ptr(samples), ptr(models), ptr(counts), 4)
    assert rc == SRL_ERR_BAD_ARG and bytes(info) == before
    assert (usable == 7).all() and (samples == 7).all() and (models == 7).all() and (counts == 7).all()
    assert lib.srl_debug_consensus_download(None, None, None, 0, None, None, None, 0) == SRL_ERR_BAD_ARG


def test_a_refused_opt_in_leaves_the_providers_set_before_it_alive():
    """the refused call installs nothing, so the handle goes on calling the Python stand-ins set earlier: their ctypes thunks must
    outlive the refusal (the wrapper lets go of them only once the device estimators are in place)"""
    import gc
    rows, cols = 100, 100
    gray = np.zeros((rows, cols), np.uint8)
    rec = np.zeros(40, capi.COLOR_SELECTED_DTYPE)
    rec["pool"] = np.arange(40) * 3
    rec["u"], rec["v"] = 10 + np.arange(40), 20
    rec["z"] = 5.0
    calls = {"f": 0, "p": 0}

    def fundamental(last, cur, status):
        calls["f"] += 1
        status[:] = 1
        status[::4] = 0
        return 0

    def pnp(xyz, uv):
        calls["p"] += 1
        return 0, np.arange(len(uv))[1:]

    def flow(gray_, r, c, stride, prev, nxt, status):
        nxt[:] = prev
        return 0
    oft = srl.Oft(None)
    try:
        oft.set_flow_provider(flow)
        oft.set_fundamental_provider(fundamental)
        oft.set_pnp_provider(pnp)
        del fundamental, pnp
        oft.init(rec, gray, 1.0)
        for K in ([400.0, 400.0, 320.0, 240.0], [0.0, 400.0, 320.0, 240.0], [400.0, float("nan"), 320.0, 240.0]):
            try:
                oft.use_device_consensus(K)
                raise AssertionError("installed on a handle without a context")
            except srl.SrlError as e:
                assert e.status == SRL_ERR_NO_DEVICE
            assert "fundamental" in oft._keep and "pnp" in oft._keep
        gc.collect()
        junk = [C.CFUNCTYPE(C.c_int)(lambda: 0) for _ in range(64)]          # a freed thunk's memory would be handed out again here
        assert oft.track_image(gray, 1.1, rows, cols) == 30 and calls == {"f": 1, "p": 0}
        assert oft.remove_outlier_using_ransac_pnp(1) is True and calls == {"f": 1, "p": 1}
        assert oft.sizes() == (29, 29, 29, 0) and len(junk) == 64
    finally:
        oft.close()


def test_the_mirror_refuses_the_device_estimators_without_a_context_and_then_behaves_as_before():
    K = [400.0, 400.0, 320.0, 240.0]
    rows, cols = 48, 64
    gray = np.zeros((rows, cols), np.uint8)
    rec = np.zeros(40, capi.COLOR_SELECTED_DTYPE)
    rec["pool"] = np.arange(40) * 3
    rec["u"], rec["v"] = 10 + np.arange(40), 20
    oft = srl.Oft(None)
    try:
        try:
            oft.use_device_consensus(K)
            raise AssertionError("installed on a handle without a context")
        except srl.SrlError as e:
            assert e.status == SRL_ERR_NO_DEVICE
        res = oft.last_consensus(0)
        assert bytes(res) == bytes(C.sizeof(res)) and bytes(oft.last_consensus(1)) == bytes(C.sizeof(res))
        lib = srl.load_library()
        assert lib.srl_oft_use_device_consensus(None, None, None, None) == SRL_ERR_BAD_ARG
        assert lib.srl_oft_last_consensus(oft.h, 2, C.byref(res)) == SRL_ERR_BAD_ARG and lib.srl_oft_last_consensus(oft.h, 0, None) == SRL_ERR_BAD_ARG

        def flow(gray_, r, c, stride, prev, nxt, status):
            nxt[:] = prev
            return 0
        oft.set_flow_provider(flow)
        oft.init(rec, gray, 1.0)
        try:
            oft.track_image(gray, 1.1, rows, cols)
            raise AssertionError("tracked without a provider")
        except srl.SrlError as e:
            assert e.status == SRL_ERR_BAD_ARG
        # ... and the PnP step likewise, once a stand-in has let the tracking through
        oft.set_fundamental_provider(lambda last, cur, status: (status.__setitem__(slice(None), 1), 0)[1])
        assert oft.track_image(gray, 1.2, 100, 100) == 40
        try:
            oft.remove_outlier_using_ransac_pnp(1)
            raise AssertionError("PnP without a provider")
        except srl.SrlError as e:
            assert e.status == SRL_ERR_BAD_ARG
    finally:
        oft.close()
