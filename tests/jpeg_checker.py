"""An independent restatement of the baseline JPEG decode that include/srlivo_hip.h specifies (srl_jpeg_parse, srl_jpeg_entropy_decode,
srl_jpeg_decode): marker walk, Huffman decode, dequantisation and the 8 x 8 inverse DCT of jidctint.c, "fancy" triangle upsampling and the
16-bit fixed-point colour conversion -- Python integers and NumPy int64, no code shared with the library.  tests/test_jpeg_checker_reference.py
compares it bytewise with libjpeg-turbo's decode (through Pillow); the library's tests compare the library with it."""
import numpy as np


class JpegRefused(Exception):
    def __init__(self, kind, why):
        super().__init__(f"{kind}: {why}")
        self.kind = kind                                   # "unsupported" or "malformed"


def _zigzag():
    """natural position of zig-zag position k, from the walk itself (T.81 figure A.6)"""
    order, r, c, up = [], 0, 0, True
    for _ in range(64):
        order.append(8 * r + c)
        if up:
            if c == 7:
                r, up = r + 1, False
            elif r == 0:
                c, up = c + 1, False
            else:
                r, c = r - 1, c + 1
        else:
            if r == 7:
                c, up = c + 1, True
            elif c == 0:
                r, up = r + 1, True
            else:
                r, c = r + 1, c - 1
    return order


NATURAL = _zigzag()


def parse(data):
    """the header up to SOS as a dict; raises JpegRefused"""
    data = bytes(data)
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise JpegRefused("malformed", "no SOI")
    hdr = dict(qt={}, huff={}, restart=0, frame=None)
    p = 2
    while True:
        if p >= n or data[p] != 0xFF:
            raise JpegRefused("malformed", "no marker")
        while p < n and data[p] == 0xFF:
            p += 1
        if p >= n:
            raise JpegRefused("malformed", "the buffer ends in a marker")
        m = data[p]
        p += 1
        if m in (0x00, 0x01) or 0xD0 <= m <= 0xD9:
            raise JpegRefused("malformed", "a marker without a segment in front of the scan")
        if p + 2 > n:
            raise JpegRefused("malformed", "no segment length")
        length = data[p] * 256 + data[p + 1]
        if length < 2 or p + length > n:
            raise JpegRefused("malformed", "a segment beyond the buffer")
        seg = data[p + 2:p + length]
        p += length
        if m == 0xC0:
            if hdr["frame"] is not None or len(seg) < 6:
                raise JpegRefused("malformed", "SOF0")
            precision, rows, cols, nf = seg[0], seg[1] * 256 + seg[2], seg[3] * 256 + seg[4], seg[5]
            if nf == 0 or len(seg) != 6 + 3 * nf or cols == 0:
                raise JpegRefused("malformed", "SOF0")
            if precision != 8 or rows == 0 or nf not in (1, 3):
                raise JpegRefused("unsupported", "precision, DNL or component count")
            comps = [dict(id=seg[6 + 3 * c], h=seg[7 + 3 * c] >> 4, v=seg[7 + 3 * c] & 15, tq=seg[8 + 3 * c]) for c in range(nf)]
            for c in comps:
                if not (1 <= c["h"] <= 4 and 1 <= c["v"] <= 4 and c["tq"] <= 3):
                    raise JpegRefused("malformed", "component")
            if nf == 1:
                comps[0]["h"] = comps[0]["v"] = 1
            elif (comps[0]["h"], comps[0]["v"]) not in ((1, 1), (2, 1), (2, 2)) or any((c["h"], c["v"]) != (1, 1) for c in comps[1:]):
                raise JpegRefused("unsupported", "sampling")
            hdr["frame"] = dict(rows=rows, cols=cols, comps=comps)
        elif 0xC1 <= m <= 0xCF and m != 0xC4:
            raise JpegRefused("unsupported", "frame type %02X" % m)
        elif m == 0xC4:
            while seg:
                if len(seg) < 17:
                    raise JpegRefused("malformed", "DHT")
                tc, th, counts = seg[0] >> 4, seg[0] & 15, list(seg[1:17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or len(seg) < 17 + total:
                    raise JpegRefused("malformed", "DHT")
                codes, code, k = {}, 0, 0
                for length_bits in range(1, 17):
                    for _ in range(counts[length_bits - 1]):
                        if code >= 1 << length_bits:
                            raise JpegRefused("malformed", "no prefix code")
                        codes[(length_bits, code)] = seg[17 + k]
                        code, k = code + 1, k + 1
                    code <<= 1
                hdr["huff"][(tc, th)] = codes
                seg = seg[17 + total:]
        elif m == 0xDB:
            while seg:
                pq, tq = seg[0] >> 4, seg[0] & 15
                if pq > 1 or tq > 3:
                    raise JpegRefused("malformed", "DQT")
                if pq == 1:
                    raise JpegRefused("unsupported", "16-bit table")
                if len(seg) < 65:
                    raise JpegRefused("malformed", "DQT")
                table = [0] * 64
                for k in range(64):
                    table[NATURAL[k]] = seg[1 + k]
                hdr["qt"][tq] = table
                seg = seg[65:]
        elif m == 0xDD:
            if len(seg) != 2:
                raise JpegRefused("malformed", "DRI")
            hdr["restart"] = seg[0] * 256 + seg[1]
        elif m == 0xDA:
            f = hdr["frame"]
            if f is None or len(seg) < 1:
                raise JpegRefused("malformed", "SOS")
            ns = seg[0]
            if not 1 <= ns <= 4 or len(seg) != 4 + 2 * ns:
                raise JpegRefused("malformed", "SOS")
            if ns != len(f["comps"]):
                raise JpegRefused("unsupported", "more than one scan")
            for c, comp in enumerate(f["comps"]):
                if seg[1 + 2 * c] != comp["id"]:
                    raise JpegRefused("unsupported" if seg[1 + 2 * c] in [x["id"] for x in f["comps"]] else "malformed", "scan components")
                comp["td"], comp["ta"] = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
                if comp["td"] > 3 or comp["ta"] > 3 or (0, comp["td"]) not in hdr["huff"] or (1, comp["ta"]) not in hdr["huff"] or comp["tq"] not in hdr["qt"]:
                    raise JpegRefused("malformed", "an undefined table")
            if tuple(seg[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
                raise JpegRefused("malformed", "Ss Se Ah Al")
            hdr["scan_offset"] = p
            break
    f = hdr["frame"]
    h0, v0 = f["comps"][0]["h"], f["comps"][0]["v"]
    hdr.update(rows=f["rows"], cols=f["cols"], components=len(f["comps"]), h=[c["h"] for c in f["comps"]], v=[c["v"] for c in f["comps"]],
               mcus_per_row=-(-f["cols"] // (8 * h0)), mcus_per_col=-(-f["rows"] // (8 * v0)))
    hdr["blocks"] = [hdr["mcus_per_row"] * c["h"] * hdr["mcus_per_col"] * c["v"] for c in f["comps"]]
    hdr["total_blocks"] = sum(hdr["blocks"])
    return hdr


class _Bits:
    def __init__(self, data, p):
        self.data, self.p, self.cur, self.left = data, p, 0, 0

    def bit(self):
        if self.left == 0:
            d, p = self.data, self.p
            if p >= len(d):
                raise JpegRefused("malformed", "data ends before the last MCU")
            c = d[p]
            if c == 0xFF:
                if p + 1 >= len(d) or d[p + 1] != 0:
                    raise JpegRefused("malformed", "a marker inside an interval")
                p += 1
            self.p, self.cur, self.left = p + 1, c, 8
        self.left -= 1
        return (self.cur >> self.left) & 1

    def symbol(self, codes):
        code = 0
        for length in range(1, 17):
            code = 2 * code + self.bit()
            if (length, code) in codes:
                return codes[(length, code)]
        raise JpegRefused("malformed", "a code that is in no table")

    def value(self, s):
        raw = 0
        for _ in range(s):
            raw = 2 * raw + self.bit()
        return raw - (1 << s) + 1 if raw < 1 << (s - 1) else raw

    def restart(self, m):
        d = self.data
        self.left = 0
        if self.p >= len(d) or d[self.p] != 0xFF:
            raise JpegRefused("malformed", "restart marker")
        while self.p < len(d) and d[self.p] == 0xFF:
            self.p += 1
        if self.p >= len(d) or d[self.p] != 0xD0 + m:
            raise JpegRefused("malformed", "restart marker")
        self.p += 1


def entropy_decode(data, hdr=None):
    """(coef, qt): coef int16 (total_blocks, 64), natural order, the components' padded planes one after the other in block-raster order;
    qt uint16 (components, 64) natural order"""
    data = bytes(data)
    hdr = hdr or parse(data)
    comps = hdr["frame"]["comps"]
    coef = np.zeros((hdr["total_blocks"], 64), np.int16)
    base = np.concatenate([[0], np.cumsum(hdr["blocks"])])
    bits = _Bits(data, hdr["scan_offset"])
    pred = [0] * len(comps)
    ri = hdr["restart"]
    for mcu in range(hdr["mcus_per_row"] * hdr["mcus_per_col"]):
        mr, mc = divmod(mcu, hdr["mcus_per_row"])
        if ri and mcu and mcu % ri == 0:
            bits.restart((mcu // ri - 1) % 8)
            pred = [0] * len(comps)
        for c, comp in enumerate(comps):
            dc, ac = hdr["huff"][(0, comp["td"])], hdr["huff"][(1, comp["ta"])]
            wb = hdr["mcus_per_row"] * comp["h"]
            for y in range(comp["v"]):
                for x in range(comp["h"]):
                    blk = coef[base[c] + (mr * comp["v"] + y) * wb + mc * comp["h"] + x]
                    s = bits.symbol(dc)
                    if s > 15:
                        raise JpegRefused("malformed", "DC category")
                    pred[c] += bits.value(s) if s else 0
                    if not -32768 <= pred[c] <= 32767:
                        raise JpegRefused("malformed", "DC leaves int16")
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = bits.symbol(ac)
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            if k > 63:
                                raise JpegRefused("malformed", "a run past coefficient 63")
                            continue
                        k += r
                        if k > 63:
                            raise JpegRefused("malformed", "a run past coefficient 63")
                        blk[NATURAL[k]] = bits.value(s)
                        k += 1
    qt = np.array([hdr["qt"][comp["tq"]] for comp in comps], np.uint16)
    return coef, qt


def _pass(d, shift):
    """one 1-D pass of jidctint.c on the eight int64 arrays d[0] ... d[7]"""
    half = 1 << (shift - 1)
    z1 = (d[2] + d[6]) * 4433
    e2 = z1 - d[6] * 15137
    e3 = z1 + d[2] * 6270
    e0 = (d[0] + d[4]) * 8192
    e1 = (d[0] - d[4]) * 8192
    a, b, c, e = e0 + e3, e1 + e2, e1 - e2, e0 - e3      # tmp10, tmp11, tmp12, tmp13
    z1, z2, z3, z4 = d[7] + d[1], d[5] + d[3], d[7] + d[3], d[5] + d[1]
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = d[7] * 2446, d[5] * 16819, d[3] * 25172, d[1] * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + (z1 + z3), o1 + (z2 + z4), o2 + (z2 + z3), o3 + (z1 + z4)      # jidctint.c: tmp0 += z1 + z3; ...
    out = [a + o3, b + o2, c + o1, e + o0, e - o0, c - o1, b - o2, a - o3]
    return [(v + half) >> shift for v in out]


def idct_blocks(coef, qt):
    """coef (N, 64) integers and qt (64,), both natural order -> (N, 64) uint8 samples"""
    d = np.asarray(coef, np.int64).reshape(-1, 8, 8) * np.asarray(qt, np.int64).reshape(1, 8, 8)
    ws = np.stack(_pass([d[:, k, :] for k in range(8)], 11), axis=1)           # columns: along the row index
    res = np.stack(_pass([ws[:, :, k] for k in range(8)], 18), axis=2)         # rows: along the column index
    idx = res & 0x3FF
    out = np.where(idx < 128, idx + 128, np.where(idx < 512, 255, np.where(idx < 896, 0, idx - 896)))
    return out.astype(np.uint8).reshape(-1, 64)


def planes(hdr, coef, qt):
    """the component planes at their REAL sizes, int64"""
    rows, cols, hmax, vmax = hdr["rows"], hdr["cols"], hdr["h"][0], hdr["v"][0]
    out, at = [], 0
    for c in range(hdr["components"]):
        nb, wb = hdr["blocks"][c], hdr["mcus_per_row"] * hdr["h"][c]
        s = idct_blocks(coef[at:at + nb], qt[c]).reshape(nb // wb, wb, 8, 8).transpose(0, 2, 1, 3).reshape(nb // wb * 8, wb * 8)
        at += nb
        out.append(s[:-(-rows * hdr["v"][c] // vmax), :-(-cols * hdr["h"][c] // hmax)].astype(np.int64))
    return out


def _h2v1(C, cols):
    cw = C.shape[1]
    left, right = np.concatenate([C[:, :1], C[:, :-1]], 1), np.concatenate([C[:, 1:], C[:, -1:]], 1)
    out = np.empty((C.shape[0], 2 * cw), np.int64)
    out[:, 0::2] = (3 * C + left + 1) >> 2
    out[:, 1::2] = (3 * C + right + 2) >> 2
    out[:, 0], out[:, -1] = C[:, 0], C[:, -1]
    return out[:, :cols]


def _h2v2(C, rows, cols):
    ch, cw = C.shape
    y = np.arange(rows)
    near = y // 2
    far = np.clip(np.where(y % 2 == 0, near - 1, near + 1), 0, ch - 1)
    S = 3 * C[near] + C[far]
    left, right = np.concatenate([S[:, :1], S[:, :-1]], 1), np.concatenate([S[:, 1:], S[:, -1:]], 1)
    out = np.empty((rows, 2 * cw), np.int64)
    out[:, 0::2] = (3 * S + left + 8) >> 4
    out[:, 1::2] = (3 * S + right + 7) >> 4
    out[:, 0], out[:, -1] = (4 * S[:, 0] + 8) >> 4, (4 * S[:, -1] + 7) >> 4
    return out[:, :cols]


def color(hdr, P):
    """the planes of `planes` -> (rows, cols, 3) uint8, B G R"""
    rows, cols = hdr["rows"], hdr["cols"]
    Y = P[0]
    if hdr["components"] == 1:
        return np.repeat(Y.astype(np.uint8)[:, :, None], 3, axis=2)
    if (hdr["h"][0], hdr["v"][0]) == (1, 1):
        Cb, Cr = P[1], P[2]
    elif (hdr["h"][0], hdr["v"][0]) == (2, 1):
        Cb, Cr = _h2v1(P[1], cols), _h2v1(P[2], cols)
    else:
        Cb, Cr = _h2v2(P[1], rows, cols), _h2v2(P[2], rows, cols)
    fix = lambda x: int(x * 65536 + 0.5)
    R = Y + ((fix(1.40200) * (Cr - 128) + 32768) >> 16)
    B = Y + ((fix(1.77200) * (Cb - 128) + 32768) >> 16)
    G = Y + ((-fix(0.34414) * (Cb - 128) - fix(0.71414) * (Cr - 128) + 32768) >> 16)
    return np.clip(np.stack([B, G, R], axis=2), 0, 255).astype(np.uint8)


def decode(data):
    """(rows, cols, 3) uint8 B G R: the whole decode"""
    hdr = parse(data)
    coef, qt = entropy_decode(data, hdr)
    return color(hdr, planes(hdr, coef, qt))


def block_l1(coef, qt):
    """largest sum over one block of |coefficient| x table entry (what guards the device's 32-bit IDCT)"""
    return int(np.max(np.sum(np.abs(np.asarray(coef, np.int64).reshape(-1, 64)) * np.asarray(qt, np.int64).reshape(1, 64), axis=1)))
