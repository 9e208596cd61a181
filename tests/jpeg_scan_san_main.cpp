// tests/jpeg_scan_san_main.cpp -- a stand-alone program (its own main, never loaded into Python) that tests/test_jpeg_sanitizer.py compiles
// together with sr_livo_amd/csrc/srl_jpeg_scan.cpp under -fsanitize=address,undefined and runs: srl_jpeg_parse and srl_jpeg_entropy_decode
// over streams held in heap blocks of EXACTLY their size (one byte read beyond the last is a report), into coefficient blocks of exactly
// total_blocks x 64 values.  Whole streams are checked against the hash of the checker's decode; then every truncation of one stream
// (each length from 0 to n - 1) and single-byte corruptions of every header and table byte of another: each call must come back with a
// status, whatever it is handed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../sr_livo_amd/csrc/srl_jpeg_scan.h"
#include "jpeg_scan_san_streams.inc"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static unsigned long long fnv(unsigned long long h, const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

// parse and, where the header is good, decode: bytes[0, n) copied into a heap block of n bytes, the coefficients into one of exactly
// min(total_blocks, max_blocks) x 64 values.  Returns the status the stream ends with; *hash: of the outputs of a successful decode
static int run(const unsigned char *bytes, size_t n, int64_t max_blocks, unsigned long long *hash) {
    unsigned char *heap = static_cast<unsigned char *>(std::malloc(n ? n : 1));
    if (n) std::memcpy(heap, bytes, n);
    srl_jpeg_info info;
    int rc = srl_jpeg_parse(heap, (int64_t)n, &info);
    if (rc == SRL_OK) {
        CHECK(info.rows >= 1 && info.cols >= 1 && (info.components == 1 || info.components == 3) && info.total_blocks >= 1);
        CHECK(info.scan_offset > 0 && info.scan_offset <= (int64_t)n);
        const int64_t blocks = info.total_blocks < max_blocks ? info.total_blocks : max_blocks;
        int16_t *coef = static_cast<int16_t *>(std::malloc((size_t)blocks * 64 * sizeof(int16_t)));
        uint16_t(*qt)[64] = static_cast<uint16_t(*)[64]>(std::malloc(3 * 64 * sizeof(uint16_t)));
        int64_t l1 = -1;
        rc = srl_jpeg_entropy_decode_l1(heap, (int64_t)n, &info, coef, blocks, qt, &l1);
        if (rc == SRL_OK) {
            CHECK(blocks == info.total_blocks && l1 >= 0);
            if (info.components == 1) CHECK(l1 == srl_jpeg_blocks_l1(coef, blocks, qt[0]));
            if (hash) *hash = fnv(fnv(0xcbf29ce484222325ull, coef, (size_t)blocks * 128), qt, (size_t)info.components * 128);
        } else {
            CHECK(rc == SRL_ERR_BAD_ARG);
        }
        std::free(coef);
        std::free(qt);
    } else {
        CHECK(rc == SRL_ERR_BAD_ARG || rc == SRL_ERR_UNSUPPORTED);
    }
    std::free(heap);
    return rc;
}

int main() {
    const size_t count = sizeof k_streams / sizeof k_streams[0];
    // 1. whole streams
    for (size_t s = 0; s < count; s++) {
        unsigned long long h = 0;
        CHECK(run(k_streams[s].bytes, k_streams[s].n, 1 << 20, &h) == SRL_OK);
        if (h != k_streams[s].hash) { std::printf("FAILED: %s decodes to another hash\n", k_streams[s].name); failures++; }
        // the public entry point, and a capacity one block short
        unsigned char *heap = static_cast<unsigned char *>(std::malloc(k_streams[s].n));
        std::memcpy(heap, k_streams[s].bytes, k_streams[s].n);
        srl_jpeg_info info;
        CHECK(srl_jpeg_parse(heap, (int64_t)k_streams[s].n, &info) == SRL_OK);
        int16_t *coef = static_cast<int16_t *>(std::malloc((size_t)info.total_blocks * 128));
        uint16_t qt[3][64];
        CHECK(srl_jpeg_entropy_decode(heap, (int64_t)k_streams[s].n, &info, coef, info.total_blocks - 1, qt) == SRL_ERR_BAD_ARG);
        CHECK(srl_jpeg_entropy_decode(heap, (int64_t)k_streams[s].n, &info, coef, info.total_blocks, qt) == SRL_OK);
        std::free(coef);
        std::free(heap);
    }
    // 2. every truncation of every stream (the restart intervals of the last two included)
    long truncations = 0, refused = 0;
    for (size_t s = 0; s < count; s++)
        for (size_t n = 0; n < k_streams[s].n; n++) {
            const int rc = run(k_streams[s].bytes, n, 1 << 20, nullptr);
            truncations++;
            if (rc != SRL_OK) refused++;
            if (n + 2 < k_streams[s].n / 2) CHECK(rc != SRL_OK);      // half a stream never holds the last MCU
        }
    // 3. single-byte corruptions of the header and table segments (everything in front of the scan), four values per byte; the
    //    coefficient block is capped so that a corrupted size cannot ask for gigabytes (a larger total is refused for its capacity)
    long corruptions = 0;
    for (size_t s = 0; s < count; s++) {
        srl_jpeg_info info;
        CHECK(srl_jpeg_parse(k_streams[s].bytes, (int64_t)k_streams[s].n, &info) == SRL_OK);
        unsigned char *work = static_cast<unsigned char *>(std::malloc(k_streams[s].n));
        for (int64_t at = 0; at < info.scan_offset; at++) {
            const unsigned char flips[4] = {0xFF, 0x01, 0x80, 0x10};
            for (int f = 0; f < 4; f++) {
                std::memcpy(work, k_streams[s].bytes, k_streams[s].n);
                work[at] ^= flips[f];
                run(work, k_streams[s].n, 4096, nullptr);
                corruptions++;
            }
        }
        // ... and of the first bytes of the scan, where a flipped bit changes every code behind it
        for (int64_t at = info.scan_offset; at < info.scan_offset + 64 && at < (int64_t)k_streams[s].n; at++) {
            std::memcpy(work, k_streams[s].bytes, k_streams[s].n);
            work[at] ^= 0x5A;
            run(work, k_streams[s].n, 4096, nullptr);
            corruptions++;
        }
        std::free(work);
    }
    CHECK(refused > truncations / 2 && corruptions > 1000);
    if (failures) { std::printf("jpeg scan: %d FAILURES\n", failures); return 1; }
    std::printf("jpeg scan: ok (%zu streams, %ld truncations, %ld corruptions)\n", count, truncations, corruptions);
    return 0;
}
