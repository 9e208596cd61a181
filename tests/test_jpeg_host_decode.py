"""The host half of the JPEG decode (sr_livo_amd/csrc/srl_jpeg_scan.cpp: srl_jpeg_parse, srl_jpeg_entropy_decode) through ctypes, no
device: the header record, the quantised coefficients and the tables equal tests/jpeg_checker.py's exactly on every committed stream,
and every refusal include/srlivo_hip.h lists answers with its status.  What a refusal leaves: *info untouched; coef and qt untouched
when the refusal is found before the scan's first bit.  A refusal INSIDE the scan leaves qt untouched and coef partly decoded -- the
coefficients are decoded in place (the caller's block may be the page-locked staging block) in one pass and without an allocation, so
there is nothing to restore them from; the header says so."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_checker as ck
from sr_livo_amd import capi

SRL_OK, SRL_ERR_BAD_ARG, SRL_ERR_UNSUPPORTED = 0, -3, -4
GOLDEN = jc.load_golden()
SENTINEL16 = 0x5A5A
C422 = [n for n in sorted(GOLDEN) if n.startswith("37x43_422_q")][0]      # whatever quality the fixture holds for that size and sampling
C420 = [n for n in sorted(GOLDEN) if n.startswith("37x43_420_q")][0]


def _parse(data):
    d = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    info = capi.JpegInfo()
    C.memset(C.byref(info), 0xA5, C.sizeof(info))
    before = bytes(info)
    rc = capi.load_library().srl_jpeg_parse(capi._ptr(d), len(data), C.byref(info))
    return rc, info, bytes(info) == before


def _decode(data, info, capacity=None):
    """status, coef, qt, coef untouched, qt untouched"""
    d = np.frombuffer(bytes(data), np.uint8)
    blocks = max(int(info.total_blocks), 1)
    coef = np.full((blocks, 64), SENTINEL16, np.int16)
    qt = np.full((3, 64), SENTINEL16, np.uint16)
    rc = capi.load_library().srl_jpeg_entropy_decode(capi._ptr(d), len(data), C.byref(info), capi._ptr(coef), blocks if capacity is None else capacity,
                                                     capi._ptr(qt))
    return rc, coef, qt, bool(np.all(coef == SENTINEL16)), bool(np.all(qt == SENTINEL16))


def _segments(data):
    """(marker, offset of its FF, offset behind the segment) up to and including SOS"""
    out, p = [], 2
    while True:
        m = data[p + 1]
        length = data[p + 2] * 256 + data[p + 3]
        out.append((m, p, p + 2 + length))
        p += 2 + length
        if m == 0xDA:
            return out


def _segment(data, marker, nth=0):
    return [s for s in _segments(data) if s[0] == marker][nth]


def _bits(s):
    """a bit string padded with ones to whole bytes, FF stuffed"""
    s += "1" * (-len(s) % 8)
    out = bytearray()
    for k in range(0, len(s), 8):
        out.append(int(s[k:k + 8], 2))
        if out[-1] == 0xFF:
            out.append(0)
    return bytes(out)


def _handmade(cols, rows, dc_symbol, ac_symbol, scan_bits, restart=0):
    """one gray component, a table of all 1, a DC and an AC table of ONE code each ("0")"""
    seg = lambda m, body: bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + body
    one_code = lambda tc, sym: seg(0xC4, bytes([tc << 4, 1] + [0] * 15 + [sym]))
    out = b"\xFF\xD8" + seg(0xDB, bytes([0] + [1] * 64)) + seg(0xC0, bytes([8, rows >> 8, rows & 255, cols >> 8, cols & 255, 1, 1, 0x11, 0]))
    out += one_code(0, dc_symbol) + one_code(1, ac_symbol)
    if restart:
        out += seg(0xDD, restart.to_bytes(2, "big"))
    return out + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + _bits(scan_bits) + b"\xFF\xD9"


def test_the_record_has_the_headers_layout():
    assert C.sizeof(capi.JpegInfo) == 14 * 4 + 5 * 8


def test_the_device_entry_points_refuse_a_null_context_before_anything_else():
    lib = capi.load_library()
    d = np.frombuffer(GOLDEN[C420][0], np.uint8)
    info, pinfo, out = capi.JpegInfo(), capi.ImagePrepInfo(), np.zeros(64, np.uint8)
    C.memset(C.byref(info), 0xFF, C.sizeof(info)); C.memset(C.byref(pinfo), 0xFF, C.sizeof(pinfo))
    assert lib.srl_jpeg_decode(None, capi._ptr(d), d.size, C.byref(info)) == SRL_ERR_BAD_ARG and bytes(info) == bytes(C.sizeof(info))
    assert lib.srl_image_prepare_jpeg(None, capi._ptr(d), d.size, C.byref(pinfo)) == SRL_ERR_BAD_ARG and pinfo.as_tuple() == (0,) * 8
    assert lib.srl_jpeg_download(None, capi._ptr(out), 3) == SRL_ERR_BAD_ARG
    assert lib.srl_jpeg_idct_blocks(None, capi._ptr(np.zeros(64, np.int16)), 1, capi._ptr(np.ones(64, np.uint16)), capi._ptr(out)) == SRL_ERR_BAD_ARG


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_parse_and_entropy_decode_equal_the_checker(name):
    data = GOLDEN[name][0]
    hdr = ck.parse(data)
    rc, info, _ = _parse(data)
    assert rc == SRL_OK
    nc = hdr["components"]
    assert (info.rows, info.cols, info.components) == (hdr["rows"], hdr["cols"], nc)
    assert list(info.h)[:nc] == hdr["h"] and list(info.v)[:nc] == hdr["v"] and list(info.h)[nc:] == [0] * (3 - nc)
    assert (info.mcus_per_row, info.mcus_per_col, info.restart_interval) == (hdr["mcus_per_row"], hdr["mcus_per_col"], hdr["restart"])
    assert list(info.blocks)[:nc] == hdr["blocks"] and info.total_blocks == hdr["total_blocks"] and info.scan_offset == hdr["scan_offset"]
    rc, coef, qt, _, _ = _decode(data, info)
    assert rc == SRL_OK
    want_coef, want_qt = ck.entropy_decode(data, hdr)
    assert np.array_equal(coef, want_coef)
    assert np.array_equal(qt[:nc], want_qt) and np.all(qt[nc:] == SENTINEL16)      # rows of absent components are left alone
    # the wrapper of the package gives the same
    c2, q2 = capi.jpeg_entropy_decode(data)
    assert np.array_equal(c2, want_coef) and np.array_equal(q2, want_qt)


def _edited(name, marker, at, value, nth=0):
    data = bytearray(GOLDEN[name][0])
    _, start, _ = _segment(data, marker, nth)
    data[start + at] = value
    return bytes(data)


def _unsupported_streams():
    base = C422
    out = {
        "arithmetic (SOF9)": _edited(base, 0xC0, 1, 0xC9),
        "extended sequential (SOF1)": _edited(base, 0xC0, 1, 0xC1),
        "progressive marker (SOF2)": _edited(base, 0xC0, 1, 0xC2),
        "12-bit": _edited(base, 0xC0, 4, 12),
        "4:4:0": _edited(base, 0xC0, 11, 0x12),
        "4:1:1": _edited(base, 0xC0, 11, 0x41),
        "chroma 2x1": _edited(base, 0xC0, 14, 0x21),
    }
    data = bytearray(GOLDEN[base][0])
    _, s, e = _segment(data, 0xC0)
    four = bytes([0xFF, 0xC0, 0, 8 + 12]) + bytes(data[s + 4:s + 9]) + bytes([4]) + bytes(data[s + 10:e]) + bytes([4, 0x11, 1])
    out["four components"] = bytes(data[:s]) + four + bytes(data[e:])
    _, s, e = _segment(data, 0xDA)
    out["a scan of one component of three (multi-scan)"] = bytes(data[:s]) + bytes([0xFF, 0xDA, 0, 8, 1, data[s + 5], data[s + 6], 0, 63, 0]) + bytes(data[e:])
    _, s, e = _segment(data, 0xDB)
    out["16-bit quantisation table"] = bytes(data[:s + 4]) + bytes([0x10 | data[s + 4]]) + bytes(data[s + 5:])
    return out


@pytest.mark.parametrize("what", sorted(_unsupported_streams()))
def test_unsupported_streams_are_refused_as_such_and_nothing_is_written(what):
    data = _unsupported_streams()[what]
    rc, info, untouched = _parse(data)
    assert rc == SRL_ERR_UNSUPPORTED and untouched, what
    good = capi.jpeg_parse(GOLDEN[C422][0])
    rc, _, _, coef_untouched, qt_untouched = _decode(data, good)
    assert rc == SRL_ERR_UNSUPPORTED and coef_untouched and qt_untouched, what
    with pytest.raises(ck.JpegRefused) as ei:
        ck.parse(data)
    assert ei.value.kind == "unsupported"


def test_pillows_progressive_file_is_unsupported():
    # (4:4:0 and 4:1:1 are made above by editing the sampling byte: Pillow's encoder writes neither)
    pytest.importorskip("PIL")
    data = jc.encode(jc.image(40, 48, 5), "420", progressive=True)
    rc, _, untouched = _parse(data)
    assert rc == SRL_ERR_UNSUPPORTED and untouched
    with pytest.raises(ck.JpegRefused) as ei:
        ck.parse(data)
    assert ei.value.kind == "unsupported"


def _without(data, marker):
    out, at = b"", 0
    for m, a, b in _segments(data):
        if m == marker:
            out, at = out + data[at:a], b
    return out + data[at:]


def _malformed_headers():
    name = C420
    base = GOLDEN[name][0]
    dht, sos = _segment(base, 0xC4), _segment(base, 0xDA)
    return {
        "no SOI": b"\xFF\xD9" + base[2:],
        "empty": b"",
        "a segment length beyond the buffer": base[:dht[1] + 2] + b"\xFF\xFF" + base[dht[1] + 4:],
        "the buffer ends inside a segment": base[:dht[1] + 20],
        "a segment length of one": base[:dht[1] + 2] + b"\x00\x01" + base[dht[1] + 4:],
        "an undefined Huffman table": _edited(name, 0xDA, 6, 0x33),
        "an undefined quantisation table": _edited(name, 0xC0, 12, 3),
        "no Huffman tables at all": _without(base, 0xC4),
        "no quantisation tables at all": _without(base, 0xDB),
        "Huffman counts that form no prefix code": _edited(name, 0xC4, 5, 3),
        "a spectral selection that is not sequential": base[:sos[2] - 2] + b"\x3E" + base[sos[2] - 1:],
        "EOI in front of the scan": base[:sos[1]] + b"\xFF\xD9",
        "SOS in front of SOF0": base[:2] + base[sos[1]:sos[2]] + base[2:],
        "a second SOF0": base[:sos[1]] + base[_segment(base, 0xC0)[1]:_segment(base, 0xC0)[2]] + base[sos[1]:],
        "zero columns": _edited(name, 0xC0, 8, 0),
    }


@pytest.mark.parametrize("what", sorted(_malformed_headers()))
def test_malformed_headers_are_bad_arguments_and_nothing_is_written(what):
    data = _malformed_headers()[what]
    rc, info, untouched = _parse(data)
    assert rc == SRL_ERR_BAD_ARG and untouched, what
    good = capi.jpeg_parse(GOLDEN[C420][0])
    if len(data):
        rc, _, _, coef_untouched, qt_untouched = _decode(data, good)
        assert rc == SRL_ERR_BAD_ARG and coef_untouched and qt_untouched, what


def test_null_arguments_a_foreign_record_and_a_small_capacity():
    lib = capi.load_library()
    data = GOLDEN["40x48_420_rrow"][0]
    d = np.frombuffer(data, np.uint8)
    info = capi.jpeg_parse(data)
    assert lib.srl_jpeg_parse(None, 10, C.byref(info)) == SRL_ERR_BAD_ARG and lib.srl_jpeg_parse(capi._ptr(d), len(data), None) == SRL_ERR_BAD_ARG
    rc, _, _, cu, qu = _decode(data, info, capacity=int(info.total_blocks) - 1)
    assert rc == SRL_ERR_BAD_ARG and cu and qu
    other = capi.jpeg_parse(GOLDEN["40x48_444_noise"][0])
    rc, _, _, cu, qu = _decode(data, other)
    assert rc == SRL_ERR_BAD_ARG and cu and qu
    coef = np.zeros((int(info.total_blocks), 64), np.int16)
    qt = np.zeros((3, 64), np.uint16)
    for args in ((None, len(data), C.byref(info), capi._ptr(coef), len(coef), capi._ptr(qt)), (capi._ptr(d), len(data), None, capi._ptr(coef), len(coef), capi._ptr(qt)),
                 (capi._ptr(d), len(data), C.byref(info), None, len(coef), capi._ptr(qt)), (capi._ptr(d), len(data), C.byref(info), capi._ptr(coef), len(coef), None)):
        assert lib.srl_jpeg_entropy_decode(*args) == SRL_ERR_BAD_ARG


def _scan_refusals():
    r1 = GOLDEN["37x43_420_r1"][0]
    off = ck.parse(r1)["scan_offset"]
    first = r1.index(b"\xFF\xD0", off)
    plain = GOLDEN[C420][0]
    poff = ck.parse(plain)["scan_offset"]
    return {
        "a code that is in no table": _handmade(8, 8, 0, 0x00, "1" * 24),
        "a run past coefficient 63": _handmade(8, 8, 0, 0xF1, "0" + "01" * 4 + "0"),
        "a ZRL that reaches coefficient 64": _handmade(8, 8, 0, 0xF0, "0" + "0" * 4),
        "a DC category above 15": _handmade(8, 8, 16, 0x00, "0" + "1" * 16 + "0"),
        "a DC value leaving int16_t": _handmade(16, 8, 15, 0x00, "0" + "1" * 15 + "0" + "0" + "1" * 15 + "0"),
        "a wrong restart marker": r1[:first + 1] + b"\xD1" + r1[first + 2:],
        "a missing restart marker": r1[:first] + r1[first + 2:],
        "a whole unread byte in front of a restart marker": r1[:first] + b"\x55" + r1[first:],
        "a restart marker where none is due": _handmade(16, 8, 0, 0x00, "")[:-2] + b"\xFF\xD0" + _bits("0000") + b"\xFF\xD9",
        "data ending before the last MCU": plain[:poff + (len(plain) - poff) // 2],
        "data ending at the scan's first byte": plain[:poff],
        "an unstuffed FF at the end of the buffer": plain[:poff + 5] + b"\xFF",
    }


@pytest.mark.parametrize("what", sorted(_scan_refusals()))
def test_refusals_inside_the_scan_are_bad_arguments_and_the_tables_stay(what):
    data = _scan_refusals()[what]
    rc, info, _ = _parse(data)
    assert rc == SRL_OK, what                              # the header is good
    rc, coef, qt, _, qt_untouched = _decode(data, info)
    assert rc == SRL_ERR_BAD_ARG and qt_untouched, what
    with pytest.raises(ck.JpegRefused) as ei:
        ck.entropy_decode(data)
    assert ei.value.kind == "malformed", what


def test_the_handmade_streams_decode_when_they_are_whole():
    # DC category 0 and EOB twice; then a DC of + 32767 in one block, the edge of int16_t
    for data, want in ((_handmade(16, 8, 0, 0x00, "0000"), [0, 0]), (_handmade(8, 8, 15, 0x00, "0" + "1" * 15 + "0"), [32767])):
        rc, info, _ = _parse(data)
        assert rc == SRL_OK
        rc, coef, qt, _, _ = _decode(data, info)
        assert rc == SRL_OK and list(coef[:, 0]) == want and np.all(coef[:, 1:] == 0) and np.all(qt[0] == 1)
        assert np.array_equal(coef, ck.entropy_decode(data)[0])


def test_fill_bytes_in_front_of_a_restart_marker_are_skipped():
    r2 = GOLDEN["37x43_422_r2"][0]
    off = ck.parse(r2)["scan_offset"]
    first = r2.index(b"\xFF\xD0", off)
    data = r2[:first] + b"\xFF\xFF\xFF" + r2[first:]
    rc, info, _ = _parse(data)
    rc, coef, qt, _, _ = _decode(data, info)
    assert rc == SRL_OK and np.array_equal(coef, ck.entropy_decode(r2)[0]) and np.array_equal(coef, ck.entropy_decode(data)[0])


def test_every_truncation_of_a_small_stream_is_refused():
    data = GOLDEN[[n for n in sorted(GOLDEN) if n.startswith("8x9_420")][0]][0]
    eoi = len(data) - 2
    hdr = ck.parse(data)
    ok_from = None
    for n in range(len(data)):
        rc, info, _ = _parse(data[:n])
        if rc == SRL_OK:
            rc = _decode(data[:n], info)[0]
        if rc == SRL_OK and ok_from is None:
            ok_from = n
        assert rc in (SRL_OK, SRL_ERR_BAD_ARG), n
        assert (rc == SRL_OK) == (ok_from is not None), n   # once enough bytes are there it stays decodable
    # everything in front of the last MCU's last byte is refused; the decode needs neither the padding's end nor EOI
    assert ok_from is not None and hdr["scan_offset"] < ok_from <= eoi
