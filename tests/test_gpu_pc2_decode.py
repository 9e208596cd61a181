"""srl_pc2_decode on the device against the independent checker (tests/pc2_checker.py) on every case of tests/pc2_cases.py -- report and
queue records bytewise, message by message with last_end_time carried by the caller as the node carries it -- against the reference's own
handlers through tests/golden/golden_pc2.npz on the pinned cases (in order where no two sort keys are equal, as a multiset on the named
tie cases with every point kept), and against itself: a second identical call sequence gives identical bytes.  The two refusals found on
the device (a ring >= n_scans, a NaN sort key) leave the queue as it was."""
import ctypes as C
import os

import numpy as np
import pytest

import pc2_cases as pc
import pc2_checker as pk
import pc2_reader as pr
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu

CASES = pc.all_cases()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_pc2.npz")


def _opts(c):
    return srl.pc2_opts(c["lidar_type"], n_scans=c["n_scans"], scan_rate=c["scan_rate"], point_filter_num=c["pfn"], time_unit=c["unit"], blind=c["blind"])


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _records(d):
    return np.ascontiguousarray(np.concatenate([d["raw"], d["relative_time"][:, None], d["timestamp"][:, None]], axis=1))


def _as_multiset(records):
    r = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 5)
    rows = sorted((float(row[3]), row.tobytes()) for row in r)
    return np.array([np.frombuffer(b, dtype=np.float64) for _, b in rows]).reshape(-1, 5)


def _decode_case(ctx, c):
    """every message of the case into an empty queue, last_end_time carried from report to report -> [(report, records)]"""
    out, last_end = [], -1.0
    o = _opts(c)
    for m in c["msgs"]:
        ctx.points_clear()
        r = ctx.pc2_decode(m["data"], m["layout"], m["stamp"], last_end, o)
        out.append((r, _records(ctx.points_queue_download())))
        if r["points"] > 0:
            last_end = r["last_end_time"]
    return out


@pytest.fixture(scope="module")
def ctx():
    k = srl.Context(0)
    m = pc.message(pc.VELO, pc.make_points(pc.VELO, 4, 1))
    k.pc2_decode(m["data"], m["layout"], m["stamp"], -1.0, srl.pc2_opts(pc.VELO, time_unit=0))      # the queue exists from the first decode on
    yield k
    k.close()


@pytest.fixture(scope="module")
def decoded(ctx):
    """every case decoded once, shared by the tests below"""
    return {c["name"]: _decode_case(ctx, c) for c in CASES}


@pytest.fixture(scope="module")
def checked():
    return {c["name"]: pk.decode_case(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_report_and_records_equal_the_checker_bytewise(decoded, checked, case):
    for k, ((r, rec), w) in enumerate(zip(decoded[case["name"]], checked[case["name"]])):
        assert w["status"] == "ok" and r["rc"] == capi.SRL_OK, k
        assert (r["points"], r["picked"], r["appended"]) == (w["points"], w["picked"], w["appended"]), k
        if w["points"] > 0:
            assert r["given_offset_time"] == w["given"], k
        assert _same(r["last_end_time"], w["last_end_time"]), k
        assert _same(r["first_timestamp"], w["first_timestamp"]) and _same(r["last_timestamp"], w["last_timestamp"]), k
        assert rec.shape == w["records"].shape and rec.tobytes() == w["records"].tobytes(), k


def test_pinned_cases_equal_the_reference_through_the_golden_file(decoded):
    g = np.load(GOLDEN)
    names = [str(n) for n in g["names"]]
    assert sorted(names) == sorted(c["name"] for c in pc.exact_cases() + pc.multiset_cases())
    full = in_order = 0
    for name in names:
        for k, (r, rec) in enumerate(decoded[name]):
            key = f"{name}/{k}"
            if name in pc.MULTISET_CASES:
                rec = _as_multiset(rec)                                      # among equal keys the reference's order is its library's own
            assert r["appended"] == int(g[key + "/count"]) == len(rec), key
            if r["points"] > 0:
                assert _same(r["last_end_time"], g[key + "/last_end_time"]) and r["given_offset_time"] == int(g[key + "/given"]), key
            if key + "/records" in g.files:
                assert rec.tobytes() == g[key + "/records"].tobytes(), key
                full += 1
            else:
                assert np.array_equal(pr.digest(rec), g[key + "/sha256"]) and rec[[0, -1]].tobytes() == g[key + "/ends"].tobytes(), key
        in_order += name not in pc.MULTISET_CASES
    assert in_order >= 24 and full >= 60


def test_a_second_identical_call_sequence_gives_identical_bytes(ctx, decoded):
    for name in ("velo_size_1025", "robo_size_131073", "oust_columns_pfn3", "yaw_16_rings_pfn3", "velo_overlap", "robo_both_words"):
        for (r1, rec1), (r2, rec2) in zip(decoded[name], _decode_case(ctx, pc.case_by_name(name))):
            assert rec1.tobytes() == rec2.tobytes() and all(_same(r1[k], r2[k]) for k in r1), name


@pytest.mark.parametrize("case", pc.refused_cases(), ids=[c["name"] for c in pc.refused_cases()])
def test_what_the_device_finds_is_refused_and_the_queue_is_unchanged(ctx, case):
    assert [w["status"] for w in pk.decode_case(case)] == ["refused"]
    keep = pc.case_by_name("oust_size_65")
    ctx.points_clear()
    ctx.pc2_decode(keep["msgs"][0]["data"], keep["msgs"][0]["layout"], keep["msgs"][0]["stamp"], -1.0, _opts(keep))
    before, info = _records(ctx.points_queue_download()), ctx.points_info()
    m = case["msgs"][0]
    r = ctx.pc2_decode(m["data"], m["layout"], m["stamp"], -1.0, _opts(case), ok=(capi.SRL_ERR_BAD_ARG,))
    assert r["rc"] == capi.SRL_ERR_BAD_ARG and (r["points"], r["appended"]) == (0, 0) and np.isnan(r["last_end_time"])
    assert ctx.points_info() == info and info[0] == 65
    assert _records(ctx.points_queue_download()).tobytes() == before.tobytes()
    # ... and the queue goes on as if the call had not been made
    ctx.pc2_decode(keep["msgs"][0]["data"], keep["msgs"][0]["layout"], keep["msgs"][0]["stamp"] + 1.0, -1.0, _opts(keep))
    after = _records(ctx.points_queue_download())
    assert len(after) == 130 and after[:65].tobytes() == before.tobytes() and after[65:, :4].tobytes() == before[:, :4].tobytes()


def test_refusals_with_a_device(ctx):
    lib = ctx.lib
    c = pc.case_by_name("yaw_single_ring_65")
    m = c["msgs"][0]
    ctx.points_clear()
    before = ctx.points_info()
    r = capi.Pc2Report()

    def rc(lay=m["layout"], data=m["data"], **kw):
        o = srl.pc2_opts(pc.VELO, **dict(dict(n_scans=16, scan_rate=10, time_unit=0), **kw))
        return lib.srl_pc2_decode(ctx.h, data.ctypes.data_as(C.c_void_p), data.nbytes, C.byref(lay), m["stamp"], -1.0, C.byref(o), C.byref(r))

    assert rc() == capi.SRL_OK and ctx.points_info()[0] == 65
    ctx.points_clear()
    assert rc(scan_rate=0) == rc(scan_rate=-10) == rc(n_scans=0) == capi.SRL_ERR_BAD_ARG         # the yaw branch needs both
    g = pc.case_by_name("velo_size_65")["msgs"][0]
    assert rc(lay=g["layout"], data=g["data"], scan_rate=0, n_scans=0) == capi.SRL_OK             # the given branch reads neither
    ctx.points_clear()
    big = np.zeros(4 * ((1 << 20) + 1), dtype=np.uint8)
    lay = capi.Pc2Layout(width=(1 << 20) + 1, height=1, point_step=4, row_step=4 * ((1 << 20) + 1), off_x=0, off_y=0, off_z=0, off_time=0, off_ring=0, is_bigendian=0)
    assert rc(lay=lay, data=big) == capi.SRL_ERR_UNSUPPORTED                                      # refused before the bytes are looked at
    assert ctx.points_info()[0] == before[0] == 0


def test_an_empty_message_and_a_fresh_context():
    k = srl.Context(0)
    try:
        with pytest.raises(srl.SrlError) as e:
            k.points_info()
        assert e.value.status == capi.SRL_ERR_NO_SWEEP                       # no queue before the first decode
        m = pc.message(pc.OUST, pc.make_points(pc.OUST, 0, 1))
        r = k.pc2_decode(m["data"], m["layout"], 5.0, -1.0, srl.pc2_opts(pc.OUST))
        assert (r["points"], r["picked"], r["appended"]) == (0, 0, 0) and np.isnan(r["last_end_time"]) and np.isnan(r["first_timestamp"])
        n, front, back = k.points_info()
        assert n == 0 and np.isnan(front) and np.isnan(back)
        c = pc.case_by_name("robo_size_1")
        r = k.pc2_decode(c["msgs"][0]["data"], c["msgs"][0]["layout"], c["msgs"][0]["stamp"], -1.0, _opts(c))
        assert (r["points"], r["appended"]) == (1, 1) and r["first_timestamp"] == r["last_timestamp"]
        assert k.points_info() == (1, r["first_timestamp"], r["last_timestamp"])
    finally:
        k.close()
