// srl_jpeg_scan.cpp -- see srl_jpeg_scan.h.  Baseline JPEG (ITU-T T.81) as far as srlivo_hip.h accepts it: the marker walk up to SOS and the
// sequential Huffman decode of the one interleaved scan.  Every read is checked against the buffer's length first; nothing is allocated.
#include "srl_jpeg_scan.h"

#include <cstring>

namespace {

// zig-zag position -> natural (row-major) position (T.81 figure A.6)
const uint8_t k_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined;
    uint8_t vals[256];
    int32_t maxcode[17];      // largest code of each length, -1: none
    int32_t valoff[17];       // vals index of a code = code + valoff[length]
    uint16_t look[512];       // nine leading bits -> (length << 8) | symbol, 0: longer than nine bits or no code
};

struct Header {
    srl_jpeg_info info;
    int tq[3], td[3], ta[3];
    bool qt_defined[4];
    uint16_t qt[4][64];       // natural order
    Huff dc[4], ac[4];
};

// T.81 annex C; refuses counts that do not form a prefix code
bool huff_build(Huff &h, const uint8_t *counts /* [16] */, const uint8_t *symbols, int total) {
    std::memcpy(h.vals, symbols, (size_t)total);
    std::memset(h.look, 0, sizeof h.look);
    int32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        const int c = counts[len - 1];
        h.valoff[len] = k - code;
        if (code + c > (1 << len)) return false;
        if (len <= 9)
            for (int i = 0; i < c; i++) {
                const int first = (code + i) << (9 - len);
                for (int j = 0; j < (1 << (9 - len)); j++) h.look[first + j] = (uint16_t)((len << 8) | symbols[k + i]);
            }
        k += c;
        code += c;
        h.maxcode[len] = c ? code - 1 : -1;
        code <<= 1;
    }
    h.defined = true;
    return true;
}

int parse_header(const uint8_t *b, int64_t n, Header &H) {
    std::memset(&H.info, 0, sizeof H.info);
    for (int k = 0; k < 4; k++) { H.qt_defined[k] = false; H.dc[k].defined = false; H.ac[k].defined = false; }
    if (!b || n < 2 || b[0] != 0xFF || b[1] != 0xD8) return SRL_ERR_BAD_ARG;      // SOI
    int64_t p = 2;
    bool have_sof = false;
    int comp_id[3] = {0, 0, 0}, restart = 0;
    srl_jpeg_info &I = H.info;
    for (;;) {
        if (p >= n || b[p] != 0xFF) return SRL_ERR_BAD_ARG;
        while (p < n && b[p] == 0xFF) p++;                  // fill bytes
        if (p >= n) return SRL_ERR_BAD_ARG;
        const int m = b[p++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return SRL_ERR_BAD_ARG;      // no segment: stuffing, TEM, RSTn, SOI, EOI before a scan
        if (p + 2 > n) return SRL_ERR_BAD_ARG;
        const int64_t L = ((int64_t)b[p] << 8) | b[p + 1];
        if (L < 2 || p + L > n) return SRL_ERR_BAD_ARG;
        const uint8_t *s = b + p + 2;
        int64_t sl = L - 2;
        p += L;
        if (m == 0xC0) {                                     // SOF0
            if (have_sof || sl < 6) return SRL_ERR_BAD_ARG;
            const int precision = s[0], rows = (s[1] << 8) | s[2], cols = (s[3] << 8) | s[4], nf = s[5];
            if (nf == 0 || sl != 6 + 3 * (int64_t)nf || cols == 0) return SRL_ERR_BAD_ARG;
            if (precision != 8 || rows == 0 || (nf != 1 && nf != 3)) return SRL_ERR_UNSUPPORTED;
            for (int c = 0; c < nf; c++) {
                comp_id[c] = s[6 + 3 * c];
                I.h[c] = s[7 + 3 * c] >> 4; I.v[c] = s[7 + 3 * c] & 15; H.tq[c] = s[8 + 3 * c];
                if (I.h[c] < 1 || I.h[c] > 4 || I.v[c] < 1 || I.v[c] > 4 || H.tq[c] > 3) return SRL_ERR_BAD_ARG;
            }
            if (nf == 1) { I.h[0] = 1; I.v[0] = 1; }         // one component: the scan is not interleaved, the factors say nothing (T.81 A.2.2)
            else {
                const bool luma = (I.h[0] == 1 && I.v[0] == 1) || (I.h[0] == 2 && I.v[0] == 1) || (I.h[0] == 2 && I.v[0] == 2);
                if (!luma || I.h[1] != 1 || I.v[1] != 1 || I.h[2] != 1 || I.v[2] != 1) return SRL_ERR_UNSUPPORTED;
            }
            I.rows = rows; I.cols = cols; I.components = nf;
            I.mcus_per_row = (cols + 8 * I.h[0] - 1) / (8 * I.h[0]);
            I.mcus_per_col = (rows + 8 * I.v[0] - 1) / (8 * I.v[0]);
            I.total_blocks = 0;
            for (int c = 0; c < nf; c++) {
                I.blocks[c] = (int64_t)I.mcus_per_row * I.h[c] * I.mcus_per_col * I.v[c];
                I.total_blocks += I.blocks[c];
            }
            have_sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) {    // every other frame type; DAC: arithmetic coding
            return SRL_ERR_UNSUPPORTED;
        } else if (m == 0xC4) {                              // DHT
            while (sl > 0) {
                if (sl < 17) return SRL_ERR_BAD_ARG;
                const int tc = s[0] >> 4, th = s[0] & 15;
                int total = 0;
                for (int k = 0; k < 16; k++) total += s[1 + k];
                if (tc > 1 || th > 3 || total > 256 || sl < 17 + total) return SRL_ERR_BAD_ARG;
                if (!huff_build(tc ? H.ac[th] : H.dc[th], s + 1, s + 17, total)) return SRL_ERR_BAD_ARG;
                s += 17 + total; sl -= 17 + total;
            }
        } else if (m == 0xDB) {                              // DQT
            while (sl > 0) {
                const int pq = s[0] >> 4, tq = s[0] & 15;
                if (pq > 1 || tq > 3) return SRL_ERR_BAD_ARG;
                if (pq == 1) return SRL_ERR_UNSUPPORTED;     // 16-bit entries
                if (sl < 65) return SRL_ERR_BAD_ARG;
                for (int k = 0; k < 64; k++) H.qt[tq][k_natural[k]] = s[1 + k];
                H.qt_defined[tq] = true;
                s += 65; sl -= 65;
            }
        } else if (m == 0xDD) {                              // DRI
            if (sl != 2) return SRL_ERR_BAD_ARG;
            restart = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {                              // SOS
            if (!have_sof || sl < 1) return SRL_ERR_BAD_ARG;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != 4 + 2 * (int64_t)ns) return SRL_ERR_BAD_ARG;
            if (ns != I.components) return SRL_ERR_UNSUPPORTED;      // one scan holds every component
            for (int c = 0; c < ns; c++) {
                const int id = s[1 + 2 * c];
                if (id != comp_id[c]) {
                    for (int k = 0; k < ns; k++) if (id == comp_id[k]) return SRL_ERR_UNSUPPORTED;      // the frame's components in another order
                    return SRL_ERR_BAD_ARG;
                }
                H.td[c] = s[2 + 2 * c] >> 4; H.ta[c] = s[2 + 2 * c] & 15;
                if (H.td[c] > 3 || H.ta[c] > 3) return SRL_ERR_BAD_ARG;
                if (!H.dc[H.td[c]].defined || !H.ac[H.ta[c]].defined || !H.qt_defined[H.tq[c]]) return SRL_ERR_BAD_ARG;      // an undefined table
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return SRL_ERR_BAD_ARG;      // Ss, Se, Ah / Al of a sequential scan
            I.restart_interval = restart;
            I.scan_offset = p;
            return SRL_OK;
        }
        // APPn, COM and whatever else carries a length: skipped
    }
}

// the entropy-coded segment as a bit stream: byte stuffing removed, never past a marker, never past the buffer
struct Bits {
    const uint8_t *b;
    int64_t n, p;
    uint64_t acc;      // the next bits, from bit 63 down
    int cnt;
    void fill() {
        while (cnt <= 56 && p < n) {
            const unsigned c = b[p];
            if (c == 0xFF) {
                if (p + 1 >= n || b[p + 1] != 0) return;      // a marker, or the buffer ends inside one: no more bits
                p += 2;
            } else p++;
            acc |= (uint64_t)c << (56 - cnt);
            cnt += 8;
        }
    }
    void drop(int k) { acc <<= k; cnt -= k; }
    // one symbol, or -1: no such code, or the bits ran out
    int decode(const Huff &h) {
        if (cnt < 16) fill();
        const unsigned peek = (unsigned)(acc >> 48);       // zero bits behind the last real one
        const unsigned e = h.look[peek >> 7];
        if (e) {
            const int len = (int)(e >> 8);
            if (len > cnt) return -1;
            drop(len);
            return (int)(e & 255u);
        }
        for (int len = 10; len <= 16; len++) {
            const int32_t code = (int32_t)(peek >> (16 - len));
            if (code <= h.maxcode[len]) {
                if (len > cnt) return -1;
                drop(len);
                return h.vals[code + h.valoff[len]];
            }
        }
        return -1;
    }
    // s bits (1 ... 16) extended to a signed value (T.81 F.2.2.1); false: the bits ran out
    bool receive_extend(int s, int *v) {
        if (cnt < s) { fill(); if (cnt < s) return false; }
        const int raw = (int)(acc >> (64 - s));
        drop(s);
        *v = raw < (1 << (s - 1)) ? raw - (1 << s) + 1 : raw;
        return true;
    }
};

}  // namespace

extern "C" int srl_jpeg_parse(const uint8_t *bytes, int64_t n, srl_jpeg_info *info) {
    if (!info) return SRL_ERR_BAD_ARG;
    Header H;
    const int rc = parse_header(bytes, n, H);
    if (rc != SRL_OK) return rc;
    *info = H.info;
    return SRL_OK;
}

int srl_jpeg_entropy_decode_l1(const uint8_t *bytes, int64_t n, const srl_jpeg_info *info, int16_t *coef, int64_t capacity_blocks, uint16_t qt[3][64],
                               int64_t *max_block_l1) {
    if (!info || !coef || !qt) return SRL_ERR_BAD_ARG;
    Header H;
    { const int rc = parse_header(bytes, n, H); if (rc != SRL_OK) return rc; }
    const srl_jpeg_info &I = H.info;
    if (std::memcmp(&I, info, sizeof I) != 0) return SRL_ERR_BAD_ARG;      // not this stream's record
    if (capacity_blocks < I.total_blocks) return SRL_ERR_BAD_ARG;
    // ---- from here on the coefficients are written: a refusal below leaves them partly decoded (the tables are written last)
    std::memset(coef, 0, (size_t)I.total_blocks * 64 * sizeof(int16_t));
    int64_t base[3] = {0, 0, 0};
    int wb[3] = {0, 0, 0};
    for (int c = 0; c < I.components; c++) { base[c] = c ? base[c - 1] + I.blocks[c - 1] : 0; wb[c] = I.mcus_per_row * I.h[c]; }
    Bits B = {bytes, n, I.scan_offset, 0, 0};
    int pred[3] = {0, 0, 0};
    int64_t worst = 0;
    const int64_t mcus = (int64_t)I.mcus_per_row * I.mcus_per_col;
    int mr = 0, mc = 0;
    for (int64_t mcu = 0; mcu < mcus; mcu++) {
        if (I.restart_interval > 0 && mcu > 0 && mcu % I.restart_interval == 0) {
            // the interval's last byte holds fewer than eight padding bits; then fill bytes and RSTm, m counting modulo 8
            if (B.cnt >= 8) return SRL_ERR_BAD_ARG;
            B.acc = 0; B.cnt = 0;
            if (B.p >= n || bytes[B.p] != 0xFF) return SRL_ERR_BAD_ARG;
            while (B.p < n && bytes[B.p] == 0xFF) B.p++;
            if (B.p >= n || bytes[B.p] != 0xD0 + (int)((mcu / I.restart_interval - 1) & 7)) return SRL_ERR_BAD_ARG;
            B.p++;
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < I.components; c++) {
            const Huff &hd = H.dc[H.td[c]], &ha = H.ac[H.ta[c]];
            const uint16_t *q = H.qt[H.tq[c]];
            for (int y = 0; y < I.v[c]; y++)
                for (int x = 0; x < I.h[c]; x++) {
                    int16_t *blk = coef + (base[c] + (int64_t)(mr * I.v[c] + y) * wb[c] + (mc * I.h[c] + x)) * 64;
                    int s = B.decode(hd);
                    if (s < 0 || s > 15) return SRL_ERR_BAD_ARG;
                    int v = 0;
                    if (s && !B.receive_extend(s, &v)) return SRL_ERR_BAD_ARG;
                    pred[c] += v;
                    if (pred[c] < -32768 || pred[c] > 32767) return SRL_ERR_BAD_ARG;
                    blk[0] = (int16_t)pred[c];
                    int64_t l1 = (int64_t)(pred[c] < 0 ? -pred[c] : pred[c]) * q[0];
                    for (int k = 1; k < 64;) {
                        const int rs = B.decode(ha);
                        if (rs < 0) return SRL_ERR_BAD_ARG;
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;              // EOB
                            k += 16;                         // ZRL: sixteen zeros, and a coefficient must follow
                            if (k > 63) return SRL_ERR_BAD_ARG;
                            continue;
                        }
                        k += r;
                        if (k > 63) return SRL_ERR_BAD_ARG;
                        if (!B.receive_extend(s, &v)) return SRL_ERR_BAD_ARG;
                        const int at = k_natural[k];
                        blk[at] = (int16_t)v;
                        l1 += (int64_t)(v < 0 ? -v : v) * q[at];
                        k++;
                    }
                    if (l1 > worst) worst = l1;
                }
        }
        if (++mc == I.mcus_per_row) { mc = 0; mr++; }
    }
    for (int c = 0; c < I.components; c++) std::memcpy(qt[c], H.qt[H.tq[c]], 64 * sizeof(uint16_t));
    if (max_block_l1) *max_block_l1 = worst;
    return SRL_OK;
}

extern "C" int srl_jpeg_entropy_decode(const uint8_t *bytes, int64_t n, const srl_jpeg_info *info, int16_t *coef, int64_t capacity_blocks, uint16_t qt[3][64]) {
    return srl_jpeg_entropy_decode_l1(bytes, n, info, coef, capacity_blocks, qt, nullptr);
}

int64_t srl_jpeg_blocks_l1(const int16_t *coef, int64_t n_blocks, const uint16_t qt[64]) {
    int64_t worst = 0;
    for (int64_t b = 0; b < n_blocks; b++) {
        int64_t l1 = 0;
        for (int k = 0; k < 64; k++) { const int v = coef[b * 64 + k]; l1 += (int64_t)(v < 0 ? -v : v) * qt[k]; }
        if (l1 > worst) worst = l1;
    }
    return worst;
}
