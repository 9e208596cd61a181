"""Livox CustomMsg messages for the tests of the decode, the point queue and the cut (csrc/srl_points.hip).

A case is a dict: name, points (the 20-byte CustomPoint records), stamp (header.stamp in seconds), n_scans, unit (0 s, 1 ms, 2 us, 3 ns),
blind, pfn (point_filter_num) and ties -- True where two VALID points share an offset_time.  Those are the cases whose order the reference's
std::sort does not define; TIE_CASES names them, and they are the only cases kept away from the comparison with the reference.
Sizes are the smallest at which the code can go wrong: around a wave (63-65), around a scan / radix tile (1023-1025), more than two
tiles (2049), and one message beyond the one-launch bound of the scan and the radix pass (131 073).
"""
import numpy as np

POINT_DTYPE = np.dtype([("offset_time", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("reflectivity", "u1"), ("tag", "u1"),
                        ("line", "u1"), ("pad", "u1")])
N_SCANS = 6
F32 = np.float32


def up(v):
    return np.nextafter(F32(v), F32(np.inf))


def down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def make_message(n, seed, offsets="shuffled", offset_step=977, offset_base=0):
    """n points that are all valid from index 1 on (line < N_SCANS, 1 < x < 60, tag 0, every point differs from the one before it by far
    more than 1e-7) with DISTINCT offsets: shuffled (the sort has work to do), ascending or descending."""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=POINT_DTYPE)
    p["x"] = (1.0 + 59.0 * rng.random(n)).astype(F32)
    p["y"] = (-20.0 + 40.0 * rng.random(n)).astype(F32)
    p["z"] = (-5.0 + 10.0 * rng.random(n)).astype(F32)
    # (two neighbours with the same float x, y and z: not with 24 random bits per axis and these seeds; the tests check the valid count)
    p["line"] = rng.integers(0, N_SCANS, n).astype(np.uint8)
    p["reflectivity"] = rng.integers(0, 256, n).astype(np.uint8)
    k = np.arange(n, dtype=np.uint64)
    if offsets == "shuffled":
        k = rng.permutation(n).astype(np.uint64)
    elif offsets == "descending":
        k = k[::-1].copy()
    p["offset_time"] = (np.uint64(offset_base) + k * np.uint64(offset_step)).astype(np.uint32)
    return p


def _case(name, points, stamp=1000.25, n_scans=N_SCANS, unit=3, blind=0.5, pfn=1, ties=False):
    return dict(name=name, points=np.ascontiguousarray(points, dtype=POINT_DTYPE), stamp=float(stamp), n_scans=int(n_scans), unit=int(unit),
                blind=float(blind), pfn=int(pfn), ties=bool(ties))


def _points(rows, offsets=None):
    """rows of (x, y, z, tag, line); offsets default to 100, 200, ... (distinct, ascending)"""
    p = np.zeros(len(rows), dtype=POINT_DTYPE)
    for i, r in enumerate(rows):
        p[i]["x"], p[i]["y"], p[i]["z"] = F32(r[0]), F32(r[1]), F32(r[2])
        p[i]["tag"], p[i]["line"] = r[3], r[4]
        p[i]["offset_time"] = 100 * (i + 1) if offsets is None else offsets[i]
    return p


def _sizes():
    out = []
    for n in (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049):
        out.append(_case(f"size_{n}", make_message(n, 100 + n)))
    out.append(_case("size_131073", make_message(131073, 7, offset_step=31), pfn=3))
    return out


def _filter_counts():
    # every point from index 1 on is valid: valid = n - 1, chosen = 0, 1 and pfn - 1 (mod pfn)
    out = []
    for pfn, valids in ((1, (40,)), (3, (30, 31, 32)), (4, (40, 41, 43))):
        for v in valids:
            out.append(_case(f"pfn{pfn}_valid{v}", make_message(v + 1, 500 + 10 * pfn + v), pfn=pfn))
    return out


def _validity():
    out = []
    filler = (10.0, 1.0, 1.0, 0, 0)
    # no valid point (every line is n_scans), exactly one
    out.append(_case("no_valid_point", _points([(5.0 + i, 1.0, 1.0, 0, N_SCANS) for i in range(40)])))
    rows = [(5.0 + i, 1.0, 1.0, 0, N_SCANS) for i in range(40)]
    rows[17] = (22.0, 1.0, 1.0, 0, 2)
    out.append(_case("one_valid_point", _points(rows)))
    # the previous MESSAGE point decides, whatever its own fate: duplicates in all axes, a difference in one axis alone, and differences
    # of exactly float(1e-7) (> 1e-7 as a double) and the float below it (< 1e-7)
    e, e_lo = F32(1e-7), down(1e-7)
    rows = [filler,
            (3.0, 0.0, 0.0, 0, 1), (3.0, 0.0, 0.0, 0, 1),                   # duplicate of a valid point
            (up(3.0), 0.0, 0.0, 0, 1), (up(3.0), e, 0.0, 0, 1), (up(3.0), e, e, 0, 1),      # x alone, y alone (exactly float(1e-7)), z alone
            (up(3.0), e, 0.0, 0, 1), (up(3.0), 0.0, 0.0, 0, 1),             # z, then y, back by float(1e-7)
            (up(3.0), e_lo, 0.0, 0, 1), (up(3.0), e_lo, e_lo, 0, 1),        # by the float just below 1e-7, y then z: duplicates
            (4.0, 2.0, 2.0, 0, N_SCANS), (4.0, 2.0, 2.0, 0, 1),             # duplicate of an INVALID point: still a duplicate
            (0.5, 2.0, 2.0, 0, 1), (4.0, 2.0, 2.0, 0, 1)]                   # ... and a valid point behind an invalid one
    out.append(_case("duplicates", _points(rows)))
    # x at and around 0.7 and 2.0, every tag pattern of the two masks (and bits outside them)
    rows = [filler]
    tags = list(range(16)) + [0x10, 0x20, 0x30, 0xF0, 0xFF]
    for k, xv in enumerate((down(0.7), F32(0.7), up(0.7), down(2.0), F32(2.0), up(2.0), F32(7.5))):
        for tg in tags:
            rows.append((xv, 0.25 * len(rows), -0.125 * k, tg, len(rows) % N_SCANS))
    out.append(_case("x_thresholds_and_tags", _points(rows), blind=0.01))
    # line = n_scans - 1 and n_scans (and beyond)
    rows = [filler] + [(5.0 + i, 0.5 * i, 1.0, 0, ln) for i, ln in enumerate((N_SCANS - 1, N_SCANS, N_SCANS + 1, 255, 0, N_SCANS - 1))]
    out.append(_case("line_edges", _points(rows)))
    # NaN in each coordinate, +-inf, magnitudes around 1e8; and the points BEHIND them (a NaN difference is not > 1e-7)
    nan, inf = F32(np.nan), F32(np.inf)
    rows = [filler,
            (nan, 1.0, 1.0, 0, 0), (5.0, 1.0, 1.0, 0, 0),                   # behind a NaN x: x differs by NaN, y and z by 0 -> a duplicate
            (5.5, nan, 1.0, 0, 0), (5.0, 2.0, 1.0, 0, 0), (5.5, 2.0, nan, 0, 0), (6.0, 2.0, 3.0, 0, 0),      # NaN in y / z: valid (x moved); the range test drops them
            (inf, 1.0, 1.0, 0, 0), (-inf, 1.0, 1.0, 0, 0), (5.0, inf, 1.0, 0, 0), (5.0, -inf, 1.0, 0, 0), (5.0, 1.0, -inf, 0, 0), (5.0, 1.0, inf, 0, 0),
            (7.0, 1.0, 1.0, 0, 0),
            (F32(1e8), 0.0, 0.0, 0, 0), (up(1e8), 0.0, 0.0, 0, 0), (down(1e8), 0.0, 0.0, 0, 0),
            (8.0, F32(-1e8), 0.0, 0, 0), (8.0, down(-1e8), 0.0, 0, 0), (8.0, 0.0, F32(1e8), 0, 0), (8.0, 0.0, up(1e8), 0, 0), (9.0, 0.0, 0.0, 0, 0)]
    out.append(_case("nan_inf_1e8", _points(rows)))
    # ranges at and around blind (1.5: exact in float and double, so is its square)
    rows = [filler, (1.5, 0.0, 0.0, 0, 0), (up(1.5), 0.0, 0.0, 0, 1), (down(1.5), 0.0, 0.0, 0, 2), (0.9, 1.2, 0.0, 0, 3), (0.9, up(1.2), 0.0, 0, 3),
            (0.9, 0.0, 1.2, 0, 4), (0.9, 0.0, down(1.2), 0, 4), (1.0, 1.0, 0.5, 0, 5), (1.0, up(1.0), 0.5, 0, 5), (0.75, -1.0, 0.9, 0, 0)]
    out.append(_case("blind_edges", _points(rows), blind=1.5))
    out.append(_case("blind_zero_and_negative", make_message(50, 77), blind=-2.0))
    return out


def _offsets():
    out = []
    # offset 0, descending input, offsets beyond 2^31 (distinct: compared with the reference)
    out.append(_case("descending", make_message(300, 21, offsets="descending")))
    out.append(_case("ascending_from_zero", make_message(70, 22, offsets="ascending", offset_base=0)))
    hi = make_message(1500, 23, offset_step=2861003)                        # 1499 * 2861003 = 4 288 643 497 > 2^32 - 2^23: every bit in use
    assert int(hi["offset_time"].max()) >= 2 ** 31 and len(np.unique(hi["offset_time"])) == len(hi)
    out.append(_case("offsets_beyond_2_31", hi, pfn=3))
    top = make_message(200, 24, offset_step=1, offset_base=2 ** 32 - 200)
    out.append(_case("offsets_at_the_top", top, unit=2))
    # ties: equal pairs, runs, everything equal -- the stable order is this library's own
    t = make_message(600, 25)
    t["offset_time"] = (t["offset_time"] // 1954) * 1954                    # pairs
    out.append(_case("ties_pairs", t, pfn=3, ties=True))
    t = make_message(1100, 26)
    t["offset_time"] = (np.arange(1100) // 37 * 1000)[np.random.default_rng(5).permutation(1100)]      # runs of 37, shuffled
    out.append(_case("ties_runs", t, pfn=4, ties=True))
    t = make_message(130, 27)
    t["offset_time"] = 0
    out.append(_case("ties_all_zero", t, pfn=3, ties=True))
    t = make_message(90, 28)
    t["offset_time"][40:] = 0xFFFFFFFF
    out.append(_case("ties_at_the_top", t, ties=True))
    return out


def _units():
    # 0 s, 1 ms, 2 us, 3 ns -- and an unknown unit (the reference's default branch: 1.f)
    return [_case(f"unit_{u}", make_message(120, 40 + u, offset_step=3 if u == 0 else 7919), unit=u, stamp=1.5e9 + 0.125 * u) for u in (0, 1, 2, 3, 9)]


DUPLICATES_VALID = (0, 1, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1)                # what the "duplicates" case is built to give, by message index

_CASES = None


def all_cases():
    """built once; nobody changes a case's arrays"""
    global _CASES
    if _CASES is None:
        _CASES = _sizes() + _filter_counts() + _validity() + _offsets() + _units()
        for c in _CASES:
            c["points"].setflags(write=False)
    return _CASES


TIE_CASES = ("ties_pairs", "ties_runs", "ties_all_zero", "ties_at_the_top")


# Messages without a valid point: cloudProcessing.cpp:183 reads .back() of an empty vector there -- there is no reference behaviour to
# record, and calling it is undefined.  The comparison with the reference asserts that these are exactly the cases without a valid point
# and leaves the call out; the library's answer for them (all counts 0, last_end_time NaN) is checked against the checker.
UNDEFINED_UPSTREAM = ("size_1", "no_valid_point")


def reference_cases():
    """what is compared with the reference: everything but the named tie cases"""
    return [c for c in all_cases() if c["name"] not in TIE_CASES]


def case_by_name(name):
    for c in all_cases():
        if c["name"] == name:
            return c
    raise KeyError(name)
